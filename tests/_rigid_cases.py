"""Inputs shared by tests/test_rigid.py (host path against the definition) and tests/test_gpu_rigid.py (device against
the host path): the orientation-averaged affinity of a region of voxels for a rigid linear guest (pw_rigid_affinity).
Every comparison is of bytes.  numpy only and seeded; nothing here is taken from pywindow_amd/csrc/pw_rigid.hpp --
`reference` is the definition of include/pywindow_amd.h written directly: the pose energies on (voxel, orientation)
arrays by a Python loop over the sites and the atoms, the fold over the orientations one column after the other, the
chunk tree by reshapes (tests/_affinity_cases.py: chunk_total), pw_exp element by element through the library's test
entry on a host context (tests/_kde_cases.py: internal_exp)."""
import numpy as np

import _affinity_cases as A
import _kde_cases as K

SENTINEL = A.SENTINEL
TILE = A.TILE
CLAMPED = A.CLAMPED
MAX_SITES, MAX_DIRS = 8, 1024


class Case:
    """One job: atoms (n, 3) with rows (A, B, C) per site (S, n, 3), the S offsets, the M directions (M, 3), the grid
    (origin, spacing h, dims (nx, ny, nz)), the region's words (None: every voxel), core2, cutoff2, the betas, charged
    and map_level."""

    def __init__(self, name, dims, xyz=None, coef=None, offsets=(0.0,), dirs=((0.0, 0.0, 1.0),), words=None,
                 origin=(0.0, 0.0, 0.0), h=1.0, core2=0.25, cutoff2=0.0, betas=(0.4,), charged=0, map_level=-1):
        self.name, self.dims = name, tuple(int(d) for d in dims)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        self.dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        S = len(self.offsets)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = (np.zeros((S, 0, 3)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64)).reshape(S, -1, 3)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        self.origin, self.h = np.asarray(origin, dtype=np.float64), float(h)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        self.charged, self.map_level = int(charged), int(map_level)
        assert self.coef.shape[1] == len(self.xyz)
        assert self.words is None or len(self.words) == self.dims[1] * self.dims[2]


region = A.region


def centres(c: Case):
    """(x, y, z) of the voxels of the region in rank order."""
    nx, ny, nz = c.dims
    l, j, i = np.nonzero(region(c))
    return (c.origin[0] + i.astype(np.float64) * c.h, c.origin[1] + j.astype(np.float64) * c.h,
            c.origin[2] + l.astype(np.float64) * c.h)


def pose_energies(c: Case, terms=None):
    """(U, blocked), both (V, M), by the definition; U is 0 where blocked.  `terms`: a list that receives every pair
    term array that was added."""
    x, y, z = centres(c)
    V, M = len(x), len(c.dirs)
    U = np.zeros((V, M))
    blocked = np.zeros((V, M), dtype=bool)
    with np.errstate(all="ignore"):
        for s, t in enumerate(c.offsets):
            px = x[:, None] + (t * c.dirs[:, 0])[None, :]
            py = y[:, None] + (t * c.dirs[:, 1])[None, :]
            pz = z[:, None] + (t * c.dirs[:, 2])[None, :]
            Us = np.zeros((V, M))
            for (X, Y, Z), (a, b, q) in zip(c.xyz, c.coef[s]):
                dx, dy, dz = px - X, py - Y, pz - Z
                r2 = (dx * dx + dy * dy) + dz * dz
                blocked |= r2 <= c.core2
                inv = 1.0 / r2
                s6 = (inv * inv) * inv
                u = s6 * (a * s6 - b)
                if c.charged:
                    u = u + q / np.sqrt(r2)
                counts = np.ones_like(blocked) if c.cutoff2 == 0.0 else r2 <= c.cutoff2
                if terms is not None:
                    terms.append(u[counts & ~blocked])
                Us = np.where(counts, Us + u, Us)
            U = Us if s == 0 else U + Us
    return np.where(blocked, 0.0, U), blocked


def reference(c: Case, host):
    """(a RIGID_OUT_DTYPE record, the L level rows, the (V, 2) map or None) of the definition."""
    from pywindow_amd import _lib

    U, blocked = pose_energies(c)
    live = ~blocked
    V, M = U.shape
    inv_M = np.float64(1.0) / np.float64(M)
    out = np.zeros((), dtype=_lib.RIGID_OUT_DTYPE)
    levels = np.zeros(len(c.betas), dtype=_lib.AFFINITY_LEVEL_DTYPE)
    out["n_voxels"], out["n_blocked_poses"], out["n_dead"] = V, int(blocked.sum()), int((~live.any(axis=1)).sum())
    umin_v = np.where(live, U, np.inf).min(axis=1) if V else np.zeros(0)
    flags, zmap = 0, None
    for b, beta in enumerate(c.betas):
        arg = -(beta * U)
        if (arg[live] > 700.0).any():
            flags |= CLAMPED
        w = K.internal_exp(host, np.where(arg > 700.0, 700.0, arg).reshape(-1)).reshape(V, M) if V else np.zeros((0, M))
        e = w * U
        zs, es = np.zeros(V), np.zeros(V)
        for o in range(M):
            zs = np.where(live[:, o], zs + w[:, o], zs)
            es = np.where(live[:, o], es + e[:, o], es)
        zbar, ebar = zs * inv_M, es * inv_M
        levels[b] = (A.chunk_total(zbar), A.chunk_total(ebar))
        if b == c.map_level:
            zmap = zbar
    out["flags"] = flags
    out["u_min"], out["min_voxel"], out["min_dir"] = np.inf, -1, -1
    if live.any():
        m = umin_v.min()
        rank = int(np.flatnonzero(umin_v == m)[0])
        l, j, i = (v[rank] for v in np.nonzero(region(c)))
        out["u_min"], out["min_voxel"] = m, (i, j, l)
        out["min_dir"] = int(np.flatnonzero(live[rank] & (U[rank] == m))[0])
    return out, levels, None if c.map_level < 0 else np.stack([zmap, umin_v], axis=1)


_cache = {}


def reference_cached(c: Case, host):
    """`reference`, computed once a case object and shared; the results are read-only."""
    if id(c) not in _cache:
        got = reference(c, host)
        for a in got[1:]:
            if a is not None:
                a.setflags(write=False)
        _cache[id(c)] = (c, got)                                     # (the case is kept: its id stays its own)
    return _cache[id(c)][1]


_lists = {}


def _once(f):
    """The list a function makes, made once and shared (a store of this module's own: the names repeat
    tests/_affinity_cases.py's)."""
    def g():
        if f.__name__ not in _lists:
            _lists[f.__name__] = f()
        return _lists[f.__name__]
    g.__name__ = f.__name__
    return g


words_with = A.words_with


def unit_dirs(M: int, seed: int) -> np.ndarray:
    """M random directions of length 1 up to rounding, every component within [-1, 1]."""
    v = np.random.default_rng(seed).normal(size=(M, 3))
    return np.clip(v / np.linalg.norm(v, axis=1)[:, None], -1.0, 1.0)


def guest_atoms(n: int, S: int, dims, h: float, seed: int):
    """n atoms around the box of a grid (tests/_affinity_cases.py: shell_atoms) with S rows (A, B, C) each: (xyz, coef)."""
    xyz, _ = A.shell_atoms(n, dims, h, seed)
    rng = np.random.default_rng(1000 + seed)
    sigma, eps = rng.uniform(0.6, 1.2, (S, n)), rng.uniform(0.1, 1.0, (S, n))
    return xyz, np.stack([4.0 * eps * sigma ** 12, 4.0 * eps * sigma ** 6, rng.uniform(-2.0, 2.0, (S, n))], axis=2)


def line(S: int, reach: float) -> np.ndarray:
    """S offsets spread over [-reach, reach] (one site: the centre)."""
    return np.zeros(1) if S == 1 else np.linspace(-reach, reach, S)


@_once
def cases():
    """The case list of the issue, small grids."""
    out = []
    dims = (13, 5, 4)
    atoms = guest_atoms(9, 2, dims, 0.7, 1)
    for q, V in enumerate((0, 1, 63, 64, 65, 129)):
        out.append(Case(f"V={V}", dims, *atoms, offsets=(-0.3, 0.3), dirs=unit_dirs(3, 10 + V), words=words_with(dims, V, 10 + V),
                        h=0.7, betas=(0.4, 1.0), charged=q % 2, map_level=(q + 1) % 3 - 1))
    far = guest_atoms(5, 1, (64, 2, 2), 0.5, 2)
    for bit in (0, 63):
        w = np.zeros(4, dtype=np.uint64)
        w[2] = np.uint64(1) << np.uint64(bit)
        out.append(Case(f"bit-{bit}-alone", (64, 2, 2), *far, dirs=unit_dirs(2, 3), words=w, h=0.5, map_level=0))
    for nx in (5, 64):
        d = (nx, 3, 2)
        out.append(Case(f"nx={nx}-junk-bits", d, *guest_atoms(6, 2, d, 0.5, 3 + nx), offsets=(-0.2, 0.25), dirs=unit_dirs(4, nx),
                        words=np.full(6, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), h=0.5, charged=1))
    out.append(Case("no-mask-3x2x2", (3, 2, 2), *guest_atoms(4, 3, (3, 2, 2), 1.0, 5), offsets=line(3, 0.4), dirs=unit_dirs(5, 6),
                    map_level=0))
    d = (4, 3, 2)
    for M in (1, 2, 63, 64, 65):
        out.append(Case(f"M={M}", d, *guest_atoms(5, 2, d, 0.9, 30 + M), offsets=(-0.35, 0.35), dirs=unit_dirs(M, 40 + M), h=0.9,
                        betas=(0.0, 0.8), charged=M % 2, map_level=1))
    out.append(Case("M=1024", (3, 1, 1), *guest_atoms(5, 3, (3, 1, 1), 0.9, 31), offsets=line(3, 0.4), dirs=unit_dirs(1024, 41),
                    h=0.9, charged=1, map_level=0))
    d = (6, 5, 2)
    for S in (1, 2, 3, 4, 5, 8):
        for charged in (0, 1):
            out.append(Case(f"S={S},charged={charged}", d, *guest_atoms(7, S, d, 0.8, 50 + S), offsets=line(S, 0.5),
                            dirs=unit_dirs(5, 60 + S), h=0.8, betas=(0.3, 0.9), charged=charged, map_level=charged))
    d = (9, 7, 3)
    out.append(Case("n=0", d, offsets=(-0.3, 0.3), dirs=unit_dirs(3, 7), words=words_with(d, 100, 7), betas=(0.0, 0.7), map_level=1))
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out.append(Case(f"n={n}", d, *guest_atoms(n, 2, d, 0.8, 20 + n), offsets=(-0.3, 0.3), dirs=unit_dirs(5, 70 + n),
                        words=words_with(d, 70, 8), h=0.8, cutoff2=16.0 if n % 2 else 0.0, charged=n % 2))
    out.append(Case(f"n={2 * TILE + 1},S=8", d, *guest_atoms(2 * TILE + 1, 8, d, 0.8, 21), offsets=line(8, 0.6), dirs=unit_dirs(3, 71),
                    words=words_with(d, 70, 8), h=0.8, charged=1))
    # charged with every C zero against the uncharged job: the same bytes (test_rigid.py checks that no term is -0.0)
    xyz, coef = guest_atoms(8, 3, (6, 5, 2), 0.8, 80)
    coef[:, :, 2] = 0.0
    for charged in (0, 1):
        out.append(Case(f"zero-charges,charged={charged}", (6, 5, 2), xyz, coef, offsets=line(3, 0.5), dirs=unit_dirs(6, 81), h=0.8,
                        betas=(0.5,), charged=charged, map_level=0))
    # the atom sits on voxel 2 and the second site one spacing along +x or -x.  Voxels 1, 2, 3: the centre within the
    # core (r2 == core2 at 1 and 3), DEAD.  Voxel 0: blocked along +x (the second site at r2 == core2), free along -x.
    # Voxel 4: along +x the second site exactly at r2 == cutoff2 (counts), along -x blocked with a free centre.
    # Voxel 5: along +x the second site is the next one out (does not count)
    out.append(Case("ties", (8, 1, 1), [[2.0, 0.0, 0.0]], [[[3.0, 2.0, 0.0]], [[5.0, 1.0, 0.0]]], offsets=(0.0, 1.0),
                    dirs=((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), core2=1.0, cutoff2=9.0, map_level=0))
    out.append(Case("all-dead", (4, 3, 2), [[1.0, 1.0, 0.0]], [[[1.0, 1.0, 0.5]]], dirs=unit_dirs(3, 9), core2=1e6, charged=1,
                    map_level=0))
    # a symmetric guest along d and along -d: equal pose energies, the lower o wins the tie
    xyz, coef = guest_atoms(6, 1, (5, 4, 1), 0.9, 90)
    d0 = unit_dirs(1, 91)[0]
    out.append(Case("tied-orientations", (5, 4, 1), xyz, np.concatenate([coef, coef]), offsets=(-0.4, 0.4), dirs=(d0, -d0), h=0.9,
                    core2=0.01, map_level=0))
    # two voxels tied for the minimum (the atom halfway between them, attraction only), and a clamped beta
    out.append(Case("tied-voxels", (6, 1, 1), [[2.5, 0.0, 0.0]], [[[0.0, 1.0, 0.0]]], dirs=((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)),
                    core2=0.01, betas=(1.0, 1e3)))
    d = (7, 6, 5)
    for L in (1, 8):
        out.append(Case(f"L={L}", d, *guest_atoms(12, 3, d, 0.6, 8), offsets=line(3, 0.3), dirs=unit_dirs(4, 92),
                        words=words_with(d, 150, 9), h=0.6, betas=np.linspace(0.0, 2.0, 8)[:L] if L > 1 else (0.4,),
                        charged=1, map_level=L - 1))
    return out


@_once
def grid_case():
    """One 64 x 64 x 4 grid without a mask, M = 8, S = 2, n = 8: 256 chunks go through the reduce."""
    d = (64, 64, 4)
    return [Case("64x64x4", d, *guest_atoms(8, 2, d, 0.25, 31), offsets=(-0.2, 0.2), dirs=unit_dirs(8, 32), h=0.25,
                 betas=(0.5, 1.0), map_level=1)]


@_once
def other_shapes():
    d = (11, 3, 9)
    return [Case("other-a", d, *guest_atoms(40, 3, d, 0.5, 40), offsets=line(3, 0.3), dirs=unit_dirs(7, 42), h=0.5,
                 betas=(0.1, 0.2, 0.3), charged=1, map_level=2),
            Case("other-b", (2, 2, 2), *guest_atoms(3, 1, (2, 2, 2), 1.0, 41))]


@_once
def mixed_batch():
    """64 jobs of mixed grids, masks, atom counts, sites, L and maps; some share their atoms, all share two direction sets."""
    rng = np.random.default_rng(50)
    sets = [unit_dirs(6, 51), unit_dirs(67, 52)]
    out, atoms, S = [], None, 1
    for k in range(64):
        d = tuple(int(v) for v in rng.integers(1, 13, 3))
        if k == 7:
            d = (64, 5, 2)
        if atoms is None or k % 3:
            S = int((1, 2, 3, 2, 5, 8)[k % 6])
            atoms = guest_atoms(int(rng.integers(0, 200)), S, (8, 8, 8), 0.6, 100 + k)
        total = d[0] * d[1] * d[2]
        words = None if k % 4 == 0 else words_with(d, int(rng.integers(0, total + 1)), 200 + k)
        L = int(rng.integers(1, 9))
        out.append(Case(f"mixed-{k}", d, *atoms, offsets=line(S, 0.4), dirs=sets[k % 5 == 0], words=words, h=0.6,
                        cutoff2=(0.0, 9.0)[k % 2], betas=rng.uniform(0.0, 1.5, L), charged=(k // 2) % 2,
                        map_level=int(rng.integers(-1, L))))
    return out


def pack(jobs, hole: int = 0, maps: bool = True):
    """(rec, xyz, coef, offsets, dirs, words, betas, n_maps, n_levels, n_out, V): the arrays of one call; `hole` rows
    and entries nobody owns before each job's outputs; atoms, coefficients and directions that two cases share (the same
    array) are shared.  maps=False: no job writes a map."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.RIGID_JOB_DTYPE)
    xyz, coef, offsets, dirs, words, betas = [np.zeros((0, 3))], [np.zeros((0, 3))], [], [np.zeros((0, 3))], [np.zeros(0, np.uint64)], []
    at_xyz, at_coef, at_dirs, V = {}, {}, {}, []
    n_atoms = n_rows = n_sites = n_dirs = n_words = n_betas = n_maps = n_levels = n_out = 0
    for k, c in enumerate(jobs):
        if c.xyz.ctypes.data not in at_xyz or at_xyz[c.xyz.ctypes.data][1] != len(c.xyz):   # (the same memory: the same atoms)
            at_xyz[c.xyz.ctypes.data] = (n_atoms, len(c.xyz))
            xyz.append(c.xyz)
            n_atoms += len(c.xyz)
        if c.coef.ctypes.data not in at_coef or at_coef[c.coef.ctypes.data][1] != c.coef.shape[:2]:
            at_coef[c.coef.ctypes.data] = (n_rows, c.coef.shape[:2])
            coef.append(c.coef.reshape(-1, 3))
            n_rows += c.coef.shape[0] * c.coef.shape[1]
        if c.dirs.ctypes.data not in at_dirs or at_dirs[c.dirs.ctypes.data][1] != len(c.dirs):
            at_dirs[c.dirs.ctypes.data] = (n_dirs, len(c.dirs))
            dirs.append(c.dirs)
            n_dirs += len(c.dirs)
        count = int(region(c).sum())
        V.append(count)
        level = c.map_level if maps else -1
        n_out += hole
        n_levels += hole
        n_maps += hole if level >= 0 else 0
        rec[k] = (at_xyz[c.xyz.ctypes.data][0], len(c.xyz), at_coef[c.coef.ctypes.data][0], -1 if c.words is None else n_words,
                  n_betas, len(c.betas), n_sites, len(c.offsets), at_dirs[c.dirs.ctypes.data][0], len(c.dirs), n_levels,
                  n_maps if level >= 0 else -1, n_out, c.origin, c.h, c.core2, c.cutoff2, *c.dims, c.charged, level, 0)
        if c.words is not None:
            words.append(c.words)
            n_words += len(c.words)
        offsets.append(c.offsets)
        betas.append(c.betas)
        n_sites += len(c.offsets)
        n_betas += len(c.betas)
        n_out += 1
        n_levels += len(c.betas)
        n_maps += 2 * count if level >= 0 else 0
    return (rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(offsets + [np.zeros(0)]), np.concatenate(dirs),
            np.concatenate(words), np.concatenate(betas + [np.zeros(0)]), n_maps, n_levels, n_out, V)


def blank(n_out, n_levels, n_maps):
    """(out, levels, maps) with every byte SENTINEL."""
    from pywindow_amd import _lib

    def filled(dtype, n):
        dtype = np.dtype(dtype)
        return np.frombuffer(bytes([SENTINEL]) * (dtype.itemsize * n), dtype=dtype).copy()

    return filled(_lib.RIGID_OUT_DTYPE, n_out), filled(_lib.AFFINITY_LEVEL_DTYPE, n_levels), filled(np.float64, n_maps)


def blank_of(packed):
    return blank(packed[9], packed[8], packed[7])


def expected(jobs, host, hole: int = 0, maps: bool = True):
    """(out, levels, maps) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    packed = pack(jobs, hole, maps)
    rec = packed[0]
    out, levels, mp = blank_of(packed)
    for k, c in enumerate(jobs):
        o, lv, m = reference_cached(c, host)
        out[int(rec["out"][k])] = o
        levels[int(rec["level_first"][k]):int(rec["level_first"][k]) + len(lv)] = lv
        if int(rec["map_level"][k]) >= 0:
            mp[int(rec["map_first"][k]):int(rec["map_first"][k]) + m.size] = m.reshape(-1)
    return out, levels, mp


def raw(ctx, packed, workspace_bytes=None, sizes=None):
    """pw_rigid_affinity through ctypes into SENTINEL-filled arrays -- through the library's test entry when
    `workspace_bytes` is given (0: the default budget).  `sizes`: other numbers of rows and entries of (xyz, coef,
    offsets, dirs, words, betas, maps, levels, out) to tell the entry, None for the true ones.
    Returns (rc, (out, levels, maps))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, offsets, dirs, words, betas, n_maps, n_levels, n_out, _ = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.RIGID_JOB_DTYPE)
    out, levels, mp = blank(n_out, n_levels, n_maps)
    told = [len(xyz), len(coef), len(offsets), len(dirs), len(words), len(betas), n_maps, n_levels, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], offsets.ctypes.data,
            told[2], dirs.ctypes.data, told[3], words.ctypes.data, told[4], betas.ctypes.data, told[5], mp.ctypes.data,
            told[6], levels.ctypes.data, told[7], out.ctypes.data, told[8]]
    if workspace_bytes is None:
        rc = L.pw_rigid_affinity(*args)
    else:
        rc = L.pw_internal_rigid_affinity(*args, int(workspace_bytes), None)
    return rc, (out, levels, mp)


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: which array differs first, where, and the two values."""
    for name, g, w in zip(("out", "levels", "maps"), got, want):
        for k in range(len(w)):
            if g[k].tobytes() != w[k].tobytes():
                return name, k, g[k], w[k]
    return None


def from_affinity(c) -> Case:
    """A job of tests/_affinity_cases.py as a rigid job: one site at the centre, one direction, not charged."""
    coef = np.concatenate([c.coef, np.zeros((len(c.coef), 1))], axis=1)[None]
    return Case(c.name, c.dims, c.xyz, coef, offsets=(0.0,), dirs=((0.3, -0.2, 0.9),), words=c.words, origin=c.origin, h=c.h,
                core2=c.core2, cutoff2=c.cutoff2, betas=c.betas)


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = cases()[3]
    d = (9, 8, 7)
    other = Case("other", d, *guest_atoms(6, 3, d, 0.5, 60), offsets=line(3, 0.4), dirs=unit_dirs(4, 62),
                 words=words_with(d, 90, 61), h=0.5, betas=(0.3, 0.6), charged=1, map_level=1)
    assert good.map_level >= 0 and int(region(good).sum()) == 64
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
    row = lambda p: 3 * (int(p[0]["coef_first"][1]) + 6 + 2)           # (site 1, atom 2)
    site = lambda p: int(p[0]["site_first"][1]) + 1
    comp = lambda p: 3 * (int(p[0]["dir_first"][1]) + 2) + 1
    n_atoms, n_rows = len(good.xyz) + len(other.xyz), good.coef.shape[0] * good.coef.shape[1] + 18
    n_sites, n_dirs = len(good.offsets) + 3, len(good.dirs) + 4
    n_words, n_betas = len(good.words) + len(other.words), len(good.betas) + len(other.betas)
    none = [None] * 9

    def told(q, v):
        return tuple(none[:q] + [v] + none[q + 1:])

    edit(field("n_sites", 0), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_sites", 9), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_dirs", 0), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(field("n_dirs", 1025), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(entry(3, site, np.inf), "an offset is not finite or beyond 16")
    edit(entry(3, site, np.nan), "an offset is not finite or beyond 16")
    edit(entry(3, site, -16.5), "an offset is not finite or beyond 16")
    edit(entry(4, comp, 1.5), "a direction's component is not finite or outside -1 .. 1")
    edit(entry(4, comp, np.nan), "a direction's component is not finite or outside -1 .. 1")
    edit(entry(2, row, -1.0), "a coefficient outside 0 .. 1e100")
    edit(entry(2, lambda p: row(p) + 1, 2e100), "a coefficient outside 0 .. 1e100")
    edit(entry(2, row, np.nan), "a coefficient is not finite")
    edit(entry(2, lambda p: row(p) + 2, -2e100), "a charge term is not finite or beyond 1e100")
    edit(entry(2, lambda p: row(p) + 2, np.inf), "a charge term is not finite or beyond 1e100")
    edit(field("charged", 2), "charged is neither 0 nor 1")
    edit(field("charged", -1), "charged is neither 0 nor 1")
    edit(field("map_level", 2), "map_level outside -1 .. n_betas - 1")
    edit(field("map_level", -2), "map_level outside -1 .. n_betas - 1")
    edit(field("map_first", -1), "map_level >= 0 with map_first < 0")
    edit(entry(1, atom, np.nan), "a coordinate is not finite")
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin or the spacing is not finite")
    edit(field("spacing", 0.0), "spacing <= 0")
    edit(field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(field("cutoff2", 0.25), "cutoff2 is neither 0 nor above core2")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("n", -1), "a negative count")
    edit(field("n_betas", 0), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(field("n_betas", 9), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(entry(6, lambda p: int(p[0]["beta_first"][1]) + 1, -0.5), "a beta is negative or not finite")
    # every span outside its array
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", told(0, n_atoms - 1))
    edit(field("coef_first", -1), "coefficients outside coef")
    edit(lambda p: None, "coefficients outside coef", told(1, n_rows - 1))
    edit(field("site_first", -1), "sites outside offsets")
    edit(lambda p: None, "sites outside offsets", told(2, n_sites - 1))
    edit(field("dir_first", -1), "directions outside dirs")
    edit(lambda p: None, "directions outside dirs", told(3, n_dirs - 1))
    edit(field("word_first", -2), "the words are outside their array")
    edit(lambda p: None, "the words are outside their array", told(4, n_words - 1))
    edit(field("beta_first", -1), "betas outside the array")
    edit(lambda p: None, "betas outside the array", told(5, n_betas - 1))
    edit(lambda p: None, "the maps are outside their array", told(6, 2 * (64 + 90) - 1))
    edit(field("level_first", -1), "the rows are outside levels")
    edit(lambda p: None, "the rows are outside levels", told(7, n_betas - 1))
    edit(lambda p: None, "the row is outside out", told(8, 1))
    edit(field("out", -1), "the row is outside out")
    # shared outputs
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", len(good.betas) - 1), "shares rows of levels with an earlier job")
    edit(field("map_first", 2 * 64 - 1), "shares maps with an earlier job")
    return out
