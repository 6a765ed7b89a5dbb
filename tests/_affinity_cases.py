"""Inputs shared by tests/test_affinity.py (host path against the definition) and tests/test_gpu_affinity.py (device
against the host path): the Lennard-Jones energy map of a region of voxels and its Boltzmann sums (pw_affinity).  Every
comparison is of bytes.  numpy only and seeded; nothing here is taken from pywindow_amd/csrc/pw_affinity.hpp --
`reference` is the definition of include/pywindow_amd.h written directly: the energy by a loop over the atoms on voxel
arrays, the chunk tree by reshapes, the chunk sums added one after the other, pw_exp element by element through the
library's test entry on a host context (tests/_kde_cases.py: internal_exp)."""
import pathlib
import re

import numpy as np

import _kde_cases as K

ROOT = pathlib.Path(__file__).resolve().parents[1]
SENTINEL = 0xA5                                                      # every byte of an output nobody owns


def source_constant(name: str) -> int:
    text = (ROOT / "pywindow_amd" / "csrc" / "pw_affinity.hpp").read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


TILE = source_constant("AFF_TILE")                                   # the atoms the kernel stages at a time
CLAMPED = 1


class Case:
    """One job: atoms (n, 3) with rows (A, B), the grid (origin, spacing h, dims (nx, ny, nz)), the region's words
    (ny * nz uint64, word l * ny + j; None: every voxel), core2, cutoff2, betas and edges."""

    def __init__(self, name, dims, xyz=None, coef=None, words=None, origin=(0.0, 0.0, 0.0), h=1.0, core2=0.25,
                 cutoff2=0.0, betas=(0.4,), edges=()):
        self.name, self.dims = name, tuple(int(d) for d in dims)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = np.zeros((0, 2)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64).reshape(-1, 2)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        self.origin, self.h = np.asarray(origin, dtype=np.float64), float(h)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        self.edges = np.asarray(edges, dtype=np.float64).reshape(-1)
        assert len(self.xyz) == len(self.coef)
        assert self.words is None or len(self.words) == self.dims[1] * self.dims[2]


def region(c: Case) -> np.ndarray:
    """The voxels of the region as a bool array [l, j, i]: the bits < nx of the words, or every voxel."""
    nx, ny, nz = c.dims
    if c.words is None:
        return np.ones((nz, ny, nx), dtype=bool)
    return ((c.words.reshape(nz, ny, 1) >> np.arange(nx, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def energies_of(c: Case):
    """(U, blocked) of every voxel of the region in rank order, by the definition; U is 0 where blocked."""
    nx, ny, nz = c.dims
    x = (c.origin[0] + np.arange(nx).astype(np.float64) * c.h)[None, None, :]
    y = (c.origin[1] + np.arange(ny).astype(np.float64) * c.h)[None, :, None]
    z = (c.origin[2] + np.arange(nz).astype(np.float64) * c.h)[:, None, None]
    U = np.zeros((nz, ny, nx))
    blocked = np.zeros((nz, ny, nx), dtype=bool)
    with np.errstate(all="ignore"):
        for (X, Y, Z), (A, B) in zip(c.xyz, c.coef):
            dx, dy, dz = x - X, y - Y, z - Z
            r2 = (dx * dx + dy * dy) + dz * dz
            blocked |= r2 <= c.core2
            q = 1.0 / r2
            s = (q * q) * q
            u = s * (A * s - B)
            counts = np.ones_like(blocked) if c.cutoff2 == 0.0 else r2 <= c.cutoff2
            U = np.where(counts, U + u, U)
    keep = region(c)
    return np.where(blocked, 0.0, U)[keep], blocked[keep]


def chunk_total(terms: np.ndarray) -> np.float64:
    """The defined sum of the terms of the ranks 0 .. V - 1: the tree inside chunks of 64, then the chunks in order."""
    chunks = (len(terms) + 63) // 64
    slots = np.zeros(chunks * 64)
    slots[:len(terms)] = terms
    a = slots.reshape(chunks, 64)
    while chunks and a.shape[1] > 1:
        a = a.reshape(chunks, -1, 2)
        a = a[:, :, 0] + a[:, :, 1]
    total = np.float64(0.0)
    for v in a.reshape(-1):
        total = total + v
    return total


def reference(c: Case, host):
    """(an AFFINITY_OUT_DTYPE record, the L level rows, the E counts, the V energies) of the definition."""
    from pywindow_amd import _lib

    U, blocked = energies_of(c)
    live = ~blocked
    out = np.zeros((), dtype=_lib.AFFINITY_OUT_DTYPE)
    levels = np.zeros(len(c.betas), dtype=_lib.AFFINITY_LEVEL_DTYPE)
    out["n_voxels"], out["n_blocked"] = len(U), int(blocked.sum())
    flags = 0
    for b, beta in enumerate(c.betas):
        x = -(beta * U)
        if (x[live] > 700.0).any():
            flags |= CLAMPED
        w = K.internal_exp(host, np.where(x > 700.0, 700.0, x)) if len(U) else np.zeros(0)
        levels[b] = (chunk_total(np.where(live, w, 0.0)), chunk_total(np.where(live, w * U, 0.0)))
    out["flags"] = flags
    out["u_min"], out["min_voxel"] = np.inf, -1
    if live.any():
        m = U[live].min()
        rank = int(np.flatnonzero(live & (U == m))[0])
        l, j, i = (v[rank] for v in np.nonzero(region(c)))
        out["u_min"], out["min_voxel"] = U[rank], (i, j, l)
    hist = np.array([int((live & (U < e)).sum()) for e in c.edges], dtype=np.int64)
    return out, levels, hist, np.where(blocked, np.inf, U)


_cache = {}


def reference_cached(c: Case, host):
    """`reference`, computed once a case object and shared; the results are read-only."""
    if id(c) not in _cache:
        got = reference(c, host)
        for a in got[1:]:
            a.setflags(write=False)
        _cache[id(c)] = (c, got)                                     # (the case is kept: its id stays its own)
    return _cache[id(c)][1]


_lists = {}


def _once(f):
    """The list a function makes, made once and shared."""
    def g():
        if f.__name__ not in _lists:
            _lists[f.__name__] = f()
        return _lists[f.__name__]
    g.__name__ = f.__name__
    return g


def words_with(dims, count: int, seed: int, junk: bool = True) -> np.ndarray:
    """Words of a grid with exactly `count` voxels set, chosen at random, and (junk) every bit at i >= nx set too."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    ok = np.zeros(nx * ny * nz, dtype=bool)
    ok[rng.choice(nx * ny * nz, count, replace=False)] = True
    w = (ok.reshape(nz, ny, nx).astype(np.uint64) << np.arange(nx, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)
    if junk and nx < 64:
        w |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nx)
    return w


def shell_atoms(n: int, dims, h: float, seed: int):
    """n atoms scattered around the box of a grid at the origin, with coefficients of a few units: (xyz, coef)."""
    rng = np.random.default_rng(seed)
    size = h * (np.asarray(dims, dtype=np.float64) - 1.0)
    xyz = rng.uniform(-0.5, 1.5, (n, 3)) * size + rng.uniform(-0.2, 0.2, (n, 3))
    sigma, eps = rng.uniform(0.8, 1.6, n), rng.uniform(0.1, 1.0, n)
    return xyz, np.stack([4.0 * eps * sigma ** 12, 4.0 * eps * sigma ** 6], axis=1)


@_once
def cases():
    """The case list of the issue, small grids."""
    out = []
    dims = (13, 5, 4)
    atoms = shell_atoms(9, dims, 0.7, 1)
    for V in (0, 1, 63, 64, 65, 128, 129):
        out.append(Case(f"V={V}", dims, *atoms, words=words_with(dims, V, 10 + V), h=0.7, betas=(0.4, 1.0), edges=(-1.0, 0.0, 5.0)))
    far = shell_atoms(5, (64, 2, 2), 0.5, 2)
    for bit in (0, 63):
        w = np.zeros(4, dtype=np.uint64)
        w[2] = np.uint64(1) << np.uint64(bit)
        out.append(Case(f"bit-{bit}-alone", (64, 2, 2), *far, words=w, h=0.5, edges=(0.0,)))
    for nx in (5, 63, 64):
        d = (nx, 3, 2)
        out.append(Case(f"nx={nx}-junk-bits", d, *shell_atoms(6, d, 0.5, 3 + nx), words=np.full(6, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64),
                        h=0.5, edges=(-0.5, 0.5)))
    out.append(Case("no-mask-3x2x2", (3, 2, 2), *shell_atoms(4, (3, 2, 2), 1.0, 5), edges=(0.0,)))
    out.append(Case("no-mask-64x1x1", (64, 1, 1), *shell_atoms(4, (64, 1, 1), 0.3, 6), h=0.3, cutoff2=36.0))
    d = (9, 7, 3)
    out.append(Case("n=0", d, words=words_with(d, 100, 7), betas=(0.0, 0.7), edges=(-1.0, 0.0, 1.0)))
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append(Case(f"n={n}", d, *shell_atoms(n, d, 0.8, 20 + n), h=0.8, cutoff2=16.0 if n % 2 else 0.0, edges=(0.0,)))
    # an atom exactly on a voxel centre and voxels exactly at r2 == core2 (blocked); a voxel exactly at r2 == cutoff2
    # (counts) and the next one out (does not: its U is +0.0)
    out.append(Case("ties", (8, 1, 1), [[2.0, 0.0, 0.0]], [[3.0, 2.0]], core2=1.0, cutoff2=9.0, edges=(0.0,)))
    # two voxels tied for the minimum (the atom halfway between them, attraction only), and a clamped beta
    out.append(Case("tied-minimum", (6, 1, 1), [[2.5, 0.0, 0.0]], [[0.0, 1.0]], core2=0.01, betas=(1.0, 1e3)))
    out.append(Case("all-blocked", (4, 3, 2), [[1.0, 1.0, 0.0]], [[1.0, 1.0]], core2=1e6, edges=(0.0,)))
    d = (7, 6, 5)
    out.append(Case("L=8,E=16", d, *shell_atoms(12, d, 0.6, 8), words=words_with(d, 150, 9), h=0.6,
                    betas=np.linspace(0.0, 2.0, 8), edges=np.linspace(-3.0, 3.0, 16)))
    out.append(Case("L=1,E=0", d, *shell_atoms(12, d, 0.6, 8), words=words_with(d, 150, 9), h=0.6))
    return out


def with_edge_on_a_voxel(host):
    """The case L=1,E=0 again with three edges, the middle one the exact U of one of its voxels."""
    base = [c for c in cases() if c.name == "L=1,E=0"][0]
    if "edge" not in _lists:
        U = reference_cached(base, host)[3]
        value = np.sort(U[np.isfinite(U)])[40]
        _lists["edge"] = (Case("U-equals-an-edge", base.dims, base.xyz, base.coef, words=base.words, h=base.h,
                               edges=(value - 1.0, value, value + 1.0)), value)
    return _lists["edge"]


@_once
def big_cases():
    """5000 atoms; one 64^3 grid without a mask and 8 atoms (4096 chunks go through the reduce)."""
    d = (10, 8, 6)
    return [Case("n=5000", d, *shell_atoms(5000, d, 0.9, 30), h=0.9, cutoff2=25.0, edges=(0.0,)),
            Case("64^3", (64, 64, 64), *shell_atoms(8, (64, 64, 64), 0.25, 31), h=0.25, betas=(0.5, 1.0), edges=(-1.0, 0.0))]


@_once
def other_shapes():
    d = (11, 3, 9)
    return [Case("other-a", d, *shell_atoms(40, d, 0.5, 40), h=0.5, betas=(0.1, 0.2, 0.3), edges=(0.0, 1.0)),
            Case("other-b", (2, 2, 2), *shell_atoms(3, (2, 2, 2), 1.0, 41))]


@_once
def mixed_batch():
    """64 jobs of mixed grids, masks, atom counts, L and E; some share their atoms."""
    rng = np.random.default_rng(50)
    out, atoms = [], None
    for k in range(64):
        d = tuple(int(v) for v in rng.integers(1, 17, 3))
        if k == 7:
            d = (64, 9, 3)
        if atoms is None or k % 3:
            atoms = shell_atoms(int(rng.integers(0, 300)), (8, 8, 8), 0.6, 100 + k)
        total = d[0] * d[1] * d[2]
        words = None if k % 4 == 0 else words_with(d, int(rng.integers(0, total + 1)), 200 + k)
        out.append(Case(f"mixed-{k}", d, *atoms, words=words, h=0.6, cutoff2=(0.0, 9.0)[k % 2],
                        betas=rng.uniform(0.0, 1.5, int(rng.integers(1, 9))), edges=np.sort(rng.uniform(-2, 2, int(rng.integers(0, 17))))))
    return out


def pack(jobs, hole: int = 0, energies: bool = True):
    """(rec, xyz, coef, words, betas, edges, n_energies, n_levels, n_hist, n_out, V): the arrays of one call; `hole`
    rows and entries nobody owns before each job's outputs; atoms that two cases share (the same array) are shared."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.AFFINITY_JOB_DTYPE)
    xyz, coef, words, betas, edges, where, V = [np.zeros((0, 3))], [np.zeros((0, 2))], [np.zeros(0, np.uint64)], [], [], {}, []
    n_atoms = n_words = n_betas = n_edges = n_energies = n_levels = n_hist = n_out = 0
    for k, c in enumerate(jobs):
        key = (c.xyz.ctypes.data, c.coef.ctypes.data, len(c.xyz))     # (the same memory: the same atoms)
        if key not in where:
            where[key] = n_atoms
            xyz.append(c.xyz)
            coef.append(c.coef)
            n_atoms += len(c.xyz)
        count = int(region(c).sum())
        V.append(count)
        n_out += hole
        n_levels += hole
        n_hist += hole
        n_energies += hole if energies else 0
        a = where[key]
        rec[k] = (a, len(c.xyz), a, -1 if c.words is None else n_words, n_betas, len(c.betas), n_edges, len(c.edges),
                  n_levels, n_hist, n_energies if energies else -1, n_out, c.origin, c.h, c.core2, c.cutoff2, *c.dims, 0)
        if c.words is not None:
            words.append(c.words)
            n_words += len(c.words)
        betas.append(c.betas)
        edges.append(c.edges)
        n_betas += len(c.betas)
        n_edges += len(c.edges)
        n_out += 1
        n_levels += len(c.betas)
        n_hist += len(c.edges)
        n_energies += count if energies else 0
    return (rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(words), np.concatenate(betas + [np.zeros(0)]),
            np.concatenate(edges + [np.zeros(0)]), n_energies, n_levels, n_hist, n_out, V)


def blank(n_out, n_levels, n_hist, n_energies):
    """(out, levels, hist, energies) with every byte SENTINEL."""
    from pywindow_amd import _lib

    def filled(dtype, n):
        dtype = np.dtype(dtype)
        return np.frombuffer(bytes([SENTINEL]) * (dtype.itemsize * n), dtype=dtype).copy()

    return (filled(_lib.AFFINITY_OUT_DTYPE, n_out), filled(_lib.AFFINITY_LEVEL_DTYPE, n_levels), filled(np.int64, n_hist),
            filled(np.float64, n_energies))


def blank_of(packed):
    return blank(packed[9], packed[7], packed[8], packed[6])


def expected(jobs, host, hole: int = 0, energies: bool = True):
    """(out, levels, hist, energies) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    packed = pack(jobs, hole, energies)
    rec = packed[0]
    out, levels, hist, en = blank_of(packed)
    for k, c in enumerate(jobs):
        o, lv, h, e = reference_cached(c, host)
        out[int(rec["out"][k])] = o
        levels[int(rec["level_first"][k]):int(rec["level_first"][k]) + len(lv)] = lv
        hist[int(rec["hist_first"][k]):int(rec["hist_first"][k]) + len(h)] = h
        if energies:
            en[int(rec["energy_first"][k]):int(rec["energy_first"][k]) + len(e)] = e
    return out, levels, hist, en


def raw(ctx, packed, workspace_bytes=None, sizes=None):
    """pw_affinity through ctypes into SENTINEL-filled arrays -- through the library's test entry when
    `workspace_bytes` is given (0: the default budget).  `sizes`: other numbers of rows and entries of (xyz, coef,
    words, betas, edges, energies, levels, hist, out) to tell the entry, None for the true ones.
    Returns (rc, (out, levels, hist, energies))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, words, betas, edges, n_energies, n_levels, n_hist, n_out, _ = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.AFFINITY_JOB_DTYPE)
    out, levels, hist, en = blank(n_out, n_levels, n_hist, n_energies)
    told = [len(xyz), len(coef), len(words), len(betas), len(edges), n_energies, n_levels, n_hist, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], words.ctypes.data,
            told[2], betas.ctypes.data, told[3], edges.ctypes.data, told[4], en.ctypes.data, told[5], levels.ctypes.data,
            told[6], hist.ctypes.data, told[7], out.ctypes.data, told[8]]
    if workspace_bytes is None:
        rc = L.pw_affinity(*args)
    else:
        rc = L.pw_internal_affinity(*args, int(workspace_bytes), None)
    return rc, (out, levels, hist, en)


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: which array differs first, where, and the two values."""
    for name, g, w in zip(("out", "levels", "hist", "energies"), got, want):
        for k in range(len(w)):
            if g[k].tobytes() != w[k].tobytes():
                return name, k, g[k], w[k]
    return None


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = cases()[3]
    d = (9, 8, 7)
    other = Case("other", d, *shell_atoms(6, d, 0.5, 60), words=words_with(d, 90, 61), h=0.5, betas=(0.3, 0.6),
                 edges=(-1.0, 1.0))
    out = []

    def edit(fn, reason, sizes=None):
        packed = list(pack([good, other]))
        packed[0] = packed[0].copy()
        fn(packed)
        out.append((tuple(packed), sizes, reason))

    def field(name, value):
        def fn(p):
            p[0][name][1] = value
        return fn

    def entry(index, at, value):
        def fn(p):
            p[index] = p[index].copy()
            p[index].reshape(-1)[at(p)] = value
        return fn

    atom = lambda p: 3 * (int(p[0]["atom_first"][1]) + 2) + 1
    row = lambda p: 2 * (int(p[0]["coef_first"][1]) + 2)
    n_atoms, n_words = len(good.xyz) + len(other.xyz), len(good.words) + len(other.words)
    n_betas, n_edges = len(good.betas) + len(other.betas), len(good.edges) + len(other.edges)
    none = [None] * 9

    def told(q, v):
        return tuple(none[:q] + [v] + none[q + 1:])

    edit(entry(1, atom, np.nan), "a coordinate is not finite")
    edit(entry(1, atom, -np.inf), "a coordinate is not finite")
    edit(entry(2, row, np.nan), "a coefficient is not finite")
    edit(entry(2, row, -1.0), "a coefficient outside 0 .. 1e100")
    edit(entry(2, lambda p: row(p) + 1, 2e100), "a coefficient outside 0 .. 1e100")
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin or the spacing is not finite")
    edit(field("spacing", np.inf), "the origin or the spacing is not finite")
    edit(field("spacing", 0.0), "spacing <= 0")
    edit(field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(field("core2", np.nan), "core2 below 1e-6 or not finite")
    edit(field("cutoff2", 0.25), "cutoff2 is neither 0 nor above core2")
    edit(field("cutoff2", np.inf), "cutoff2 is neither 0 nor above core2")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("n", -1), "a negative count")
    edit(field("n_betas", 0), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(field("n_betas", 9), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(field("n_edges", -1), "n_edges outside 0 .. PW_AFF_MAX_EDGES")
    edit(field("n_edges", 17), "n_edges outside 0 .. PW_AFF_MAX_EDGES")
    edit(entry(4, lambda p: int(p[0]["beta_first"][1]) + 1, -0.5), "a beta is negative or not finite")
    edit(entry(4, lambda p: int(p[0]["beta_first"][1]), np.nan), "a beta is negative or not finite")
    edit(entry(5, lambda p: int(p[0]["edge_first"][1]) + 1, np.inf), "an edge is not finite")
    edit(entry(5, lambda p: int(p[0]["edge_first"][1]) + 1, -1.0), "the edges are not strictly ascending")
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", told(0, n_atoms - 1))
    edit(lambda p: None, "coefficients outside coef", told(1, n_atoms - 1))
    edit(lambda p: None, "the words are outside their array", told(2, n_words - 1))
    edit(field("word_first", -2), "the words are outside their array")
    edit(lambda p: None, "betas outside the array", told(3, n_betas - 1))
    edit(lambda p: None, "edges outside the array", told(4, n_edges - 1))
    edit(lambda p: None, "the energies are outside their array", told(5, 64 + 90 - 1))
    edit(field("energy_first", -2), "the energies are outside their array")
    edit(lambda p: None, "the rows are outside levels", told(6, n_betas - 1))
    edit(lambda p: None, "the counts are outside hist", told(7, n_edges - 1))
    edit(lambda p: None, "the row is outside out", told(8, 1))
    edit(field("out", -1), "the row is outside out")
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", len(good.betas) - 1), "shares rows of levels with an earlier job")
    edit(field("hist_first", len(good.edges) - 1), "shares counts of hist with an earlier job")
    edit(field("energy_first", 63), "shares energies with an earlier job")
    return out
