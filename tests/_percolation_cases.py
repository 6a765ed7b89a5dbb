"""Inputs shared by tests/test_percolation.py (host path against the definition) and tests/test_gpu_percolation.py
(device against the host path and against the definition): the energy levels at which the sub-level sets of a periodic
field connect (pw_percolation).  Every output is a comparison of doubles or an integer count: every comparison is of
bytes, no tolerance anywhere.  numpy only and seeded; nothing here is taken from pywindow_amd/csrc/pw_percolate.hpp --
the definition of include/pywindow_amd.h is written directly, and twice:

  `by_levels`   brute force: for each distinct finite value ascending, the components of U <= t with their wraps by
                _channels_cases.by_rolls; the first level per criterion, and the component, saddle and well at it.  Only
                affordable up to a few hundred voxels, or with few distinct values.
  `by_kruskal`  voxels added in the order of their values, ties together, to a union-find whose edges carry the crossing
                vector mod 2 (a voxel's parity offset to its root) and whose roots carry the winding subspace, the size,
                the first voxel and the well; a criterion's level is the first value after whose ties some root meets it.

The two must agree on every case that `by_levels` can afford."""
import ctypes
import functools

import numpy as np

import _channels_cases as CC

SENTINEL = CC.SENTINEL
INF = np.inf
UNIT = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0)


class Case:
    """One job: a field [l, j, i] of the caller's, or atoms (n, 3) with rows (A, B), core2 and cutoff2 on the grid
    (origin, step, dims = (nx, ny, nz)); `map`: whether the job asks for its map; `brute`: whether `by_levels` is
    affordable."""

    def __init__(self, name, field=None, dims=None, xyz=None, coef=None, core2=0.25, cutoff2=0.0, origin=(0.0, 0.0, 0.0),
                 step=UNIT, map=False, brute=None):
        self.name = name
        self.field = None if field is None else np.ascontiguousarray(field, dtype=np.float64)
        self.dims = tuple(int(d) for d in (dims if field is None else self.field.shape[::-1]))
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = np.zeros((0, 2)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64).reshape(-1, 2)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.origin, self.step = np.asarray(origin, dtype=np.float64), np.asarray(step, dtype=np.float64)
        self.map = bool(map)
        V = self.dims[0] * self.dims[1] * self.dims[2]
        few = self.field is not None and len(np.unique(self.field[np.isfinite(self.field)])) <= 4
        self.brute = (V <= 400 or (few and V <= 4096)) if brute is None else bool(brute)
        assert len(self.xyz) == len(self.coef)

    @property
    def voxels(self):
        return self.dims[0] * self.dims[1] * self.dims[2]


# ---- the field of the atoms, term by term in the order of the definition ------------------------------------------
def lj_field(c: Case) -> np.ndarray:
    """U [l, j, i] of the atoms of a case: pw_affinity.hpp's terms -- r2 = (dx*dx + dy*dy) + dz*dz, q = 1/r2,
    s = (q*q)*q, u = s*(A*s - B) -- added atom after atom where r2 <= cutoff2 (or there is no cutoff), +inf where some
    r2 <= core2.  Every operation is one IEEE operation of numpy, so the bits are the definition's."""
    nx, ny, nz = c.dims
    ax, bx, by, cx, cy, cz = c.step
    i = np.arange(nx).astype(np.float64)[None, None, :]
    j = np.arange(ny).astype(np.float64)[None, :, None]
    l = np.arange(nz).astype(np.float64)[:, None, None]
    z = c.origin[2] + l * cz
    y = (c.origin[1] + j * by) + l * cy
    x = ((c.origin[0] + i * ax) + j * bx) + l * cx
    U = np.zeros((nz, ny, nx))
    blocked = np.zeros((nz, ny, nx), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for (X, Y, Z), (A, B) in zip(c.xyz, c.coef):
            dx, dy, dz = x - X, y - Y, z - Z
            r2 = (dx * dx + dy * dy) + dz * dz
            blocked |= r2 <= c.core2
            q = 1.0 / r2
            s = (q * q) * q
            u = s * (A * s - B)
            counts = np.ones_like(blocked) if c.cutoff2 == 0.0 else r2 <= c.cutoff2
            U = np.where(counts, U + u, U)
    return np.where(blocked, INF, U)


# ---- the definition, twice -------------------------------------------------------------------------------------
def meets(wraps: int, c: int) -> bool:
    if c < 3:
        return CC.rank_of(wraps) >= c + 1
    return bool((int(wraps) >> (0, 1, 3)[c - 3]) & 1)


def never_row():
    return dict(level=INF, well=INF, first=-1, n_voxels=0, n_allowed=0, saddle=-1, well_rank=-1, wraps=0, rank=0, flags=1)


def by_levels(U: np.ndarray):
    """Six rows (dicts) by brute force over the levels."""
    flat = U.reshape(-1)
    finite = np.isfinite(U)
    rows = [None] * 6
    for t in np.unique(flat[finite.reshape(-1)]):                   # (ascending; the two zeros are one level)
        if all(r is not None for r in rows):
            break
        ok = finite & (U <= t)
        firsts, n_voxels, _, wraps, index = CC.by_rolls(ok)
        for c in range(6):
            if rows[c] is not None:
                continue
            ks = [k for k in range(len(firsts)) if meets(wraps[k], c)]
            if not ks:
                continue
            k = ks[0]                                                # (firsts ascend: the lowest first voxel)
            ranks = np.flatnonzero((index == k).reshape(-1))
            vals = flat[ranks]
            saddle = int(ranks[vals == t][0])
            well = int(ranks[vals == vals.min()][0])
            rows[c] = dict(level=flat[saddle], well=flat[well], first=int(firsts[k]), n_voxels=int(n_voxels[k]),
                           n_allowed=int(ok.sum()), saddle=saddle, well_rank=well, wraps=int(wraps[k]),
                           rank=CC.rank_of(wraps[k]), flags=0)
    return [never_row() if r is None else r for r in rows]


def _span(W: int, w: int) -> int:
    """The subspace (a bit per element of (Z/2)^3) spanned by the subspace W and the vector w."""
    out = W
    for e in range(8):
        if (W >> e) & 1:
            out |= 1 << (e ^ w)
    return out


def _wraps_of(W: int) -> int:
    wraps = 0
    for phi in range(1, 8):
        if any((W >> e) & 1 and bin(phi & e).count("1") % 2 for e in range(8)):
            wraps |= 1 << (phi - 1)
    return wraps


def by_kruskal(U: np.ndarray):
    """Six rows (dicts) by a union-find that carries cell offsets mod 2."""
    nz, ny, nx = U.shape
    n = (nx, ny, nz)
    stride = (1, nx, nx * ny)
    flat = U.reshape(-1)
    order = [int(v) for v in np.argsort(flat, kind="stable") if np.isfinite(flat[v])]
    parent, offset, W, size, first, well = {}, {}, {}, {}, {}, {}

    def find(v):
        path = []
        while parent[v] != v:
            path.append(v)
            v = parent[v]
        # compress: offsets to the root, from the node next to the root outwards
        acc = 0
        for u in reversed(path):
            acc ^= offset[u]
            offset[u] = acc
            parent[u] = v
        return v

    def union(a, b, d):
        ra, rb = find(a), find(b)
        w = offset[a] ^ offset[b] ^ d                                # (after find a node hangs on its root; a root's offset is 0)
        if ra == rb:
            if w:
                W[ra] = _span(W[ra], w)
            return
        if size[ra] < size[rb]:
            ra, rb = rb, ra
        parent[rb] = ra
        offset[rb] = w                                               # (offset of rb's root to ra's root)
        for e in range(8):
            if (W[rb] >> e) & 1:
                W[ra] = _span(W[ra], e)
        size[ra] += size[rb]
        first[ra] = min(first[ra], first[rb])
        well[ra] = min(well[ra], well[rb])

    rows = [None] * 6
    winding = set()
    at = n_allowed = 0
    while at < len(order) and any(r is None for r in rows):
        t = flat[order[at]]
        group = []
        while at < len(order) and flat[order[at]] == t:
            group.append(order[at])
            at += 1
        for v in group:
            parent[v], offset[v], W[v], size[v], first[v], well[v] = v, 0, 1, 1, v, (flat[v] + 0.0, v)
        n_allowed += len(group)
        for v in group:
            pos = (v % nx, (v // nx) % ny, v // (nx * ny))
            for k in range(3):
                for d in (1, -1):
                    p = pos[k] + d
                    cross = 0
                    if p == n[k]:
                        p, cross = 0, 1 << k
                    elif p < 0:
                        p, cross = n[k] - 1, 1 << k
                    u = v + (p - pos[k]) * stride[k]
                    if u in parent:
                        union(v, u, cross)
                        r = find(v)
                        if W[r] != 1:
                            winding.add(r)
        roots = sorted({find(r) for r in winding}, key=lambda r: first[r])
        winding = set(roots)
        for c in range(6):
            if rows[c] is not None:
                continue
            for r in roots:
                wraps = _wraps_of(W[r])
                if not meets(wraps, c):
                    continue
                saddle = min(v for v in group if find(v) == r)
                rows[c] = dict(level=flat[saddle], well=flat[well[r][1]], first=first[r], n_voxels=size[r], n_allowed=n_allowed,
                               saddle=saddle, well_rank=well[r][1], wraps=wraps, rank=CC.rank_of(wraps), flags=0)
                break
    return [never_row() if r is None else r for r in rows]


def reference_of_field(U: np.ndarray, brute: bool):
    """(a PERCOLATION_OUT_DTYPE record, six PERCOLATION_LEVEL_DTYPE rows) of the definition for the field U [l, j, i]."""
    from pywindow_amd import _lib

    nz, ny, nx = U.shape
    rows = by_kruskal(U)
    if brute:
        again = by_levels(U)
        for c, (a, b) in enumerate(zip(rows, again)):
            assert {k: (np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in a.items()} == \
                   {k: (np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in b.items()}, (c, a, b)

    def voxel(rank):
        return (-1, -1, -1) if rank < 0 else (rank % nx, (rank // nx) % ny, rank // (nx * ny))

    levels = np.zeros(6, dtype=_lib.PERCOLATION_LEVEL_DTYPE)
    for c, r in enumerate(rows):
        levels[c] = (r["level"], r["well"], r["first"], r["n_voxels"], r["n_allowed"], voxel(r["saddle"]), voxel(r["well_rank"]),
                     r["wraps"], r["rank"], r["flags"], 0)
    flat = U.reshape(-1)
    finite = np.isfinite(flat)
    out = np.zeros((), dtype=_lib.PERCOLATION_OUT_DTYPE)
    out["n_blocked"] = int((~finite).sum())
    if finite.any():
        low = int(np.flatnonzero(flat == flat[finite].min())[0])
        out["u_min"], out["u_min_voxel"] = flat[low], voxel(low)
    else:
        out["u_min"], out["u_min_voxel"] = INF, -1
    out["flags"] = rows[0]["flags"]
    return out, levels


_cache = {}


def field_of(c: Case) -> np.ndarray:
    return c.field if c.field is not None else lj_field(c)


def reference_cached(c: Case):
    """(out, levels, field) of a case, computed once a case object and shared; read-only."""
    if id(c) not in _cache:
        U = field_of(c)
        out, levels = reference_of_field(U, c.brute)
        levels.setflags(write=False)
        _cache[id(c)] = (c, (out, levels, U))
    return _cache[id(c)][1]


# ---- the cases -------------------------------------------------------------------------------------------------
def two_valued(ok: np.ndarray, low=-3.0, high=5.0) -> np.ndarray:
    return np.where(ok, low, high)


def _maze_words(name):
    c = next(c for c in CC.cases() if c.name == name)
    return CC.unpack_words(c.words, c.dims)


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernel and the host path can go wrong, as fields of the caller's."""
    out = []
    for name in ("channel-along-a", "channel-along-b", "channel-along-c", "staircase-110", "staircase-111", "slab",
                 "pocket-round-the-corner", "two-interleaved-channels"):
        out.append(Case(name, two_valued(_maze_words(name))))
    # the walls blocked instead of high: criteria that never hold (a 1-D channel: B_1 = B_2 = +inf, two axis levels +inf)
    out.append(Case("channel-along-a-walls-blocked", np.where(_maze_words("channel-along-a"), 1.5, INF)))
    out.append(Case("pocket-walls-blocked", np.where(_maze_words("pocket-round-the-corner"), 1.5, INF)))
    helix = _maze_words("double-helix")
    out.append(Case("double-helix", np.where(helix, -1.0, INF)))                         # the documented limit: never
    out.append(Case("double-helix-tiled-twice", np.where(np.concatenate([helix, helix], axis=2), -1.0, INF)))
    out.append(Case("double-helix-in-high-walls", two_valued(helix)))
    # a cubic maze: criteria that coincide
    g = np.arange(8)
    on = (g % 4) == 1
    a, b, c = on[None, None, :], on[None, :, None], on[:, None, None]
    out.append(Case("cubic-maze", np.where((a & b) | (a & c) | (b & c), -2.0, INF)))
    # random fields: integer-valued with many ties, and normal
    rng = np.random.default_rng(7)
    for dims in ((3, 4, 5), (1, 5, 6), (2, 2, 7), (6, 5, 4)):
        nx, ny, nz = dims
        out.append(Case(f"ties-{dims}", rng.integers(-3, 4, (nz, ny, nx)).astype(np.float64)))
        out.append(Case(f"normal-{dims}", rng.normal(size=(nz, ny, nx))))
        f = rng.integers(-2, 3, (nz, ny, nx)).astype(np.float64)
        f[rng.random((nz, ny, nx)) < 0.3] = INF
        out.append(Case(f"ties-blocked-{dims}", f))
    # word edges
    for nx in (1, 2, 63, 64):
        out.append(Case(f"nx={nx}", rng.integers(0, 3, (2, 3, nx)).astype(np.float64)))
    for ny, nz in ((1, 1), (63, 1), (64, 1), (6, 43), (7, 37)):
        f = rng.integers(0, 3, (nz, ny, 2)).astype(np.float64)
        f[rng.random((nz, ny, 2)) < 0.2] = INF
        out.append(Case(f"rows={ny}x{nz}", f))
    # other fields
    out.append(Case("all-blocked", np.full((3, 4, 5), INF)))
    f = np.full((3, 4, 5), INF)
    f[1, 2, 3] = -7.25
    out.append(Case("one-finite-voxel", f))
    out.append(Case("one-voxel", np.array([[[2.5]]])))
    out.append(Case("all-equal", np.full((3, 4, 5), 1.25)))
    # +0.0 against -0.0 at the saddle: a channel along a at -1 in walls at 3 with two gates at zero; the saddle is the gate
    # of the lower rank, and the level carries its bits
    f = np.full((4, 4, 6), 3.0)
    f[2, 1, :] = -1.0
    f[2, 1, 1] = -0.0
    f[2, 1, 4] = 0.0
    out.append(Case("minus-zero-saddle", f))
    f = np.full((4, 4, 6), 3.0)
    f[2, 1, :] = -1.0
    f[2, 1, 0] = 0.0
    f[2, 1, 3] = -0.0
    out.append(Case("plus-zero-before-minus-zero", f))
    tiny = np.nextafter(0.0, 1.0)
    f = rng.choice(np.array([tiny, -tiny, 3 * tiny, 1e-310, -1e-310, 1e308, -1e308, 1.7e308, 0.0]), (4, 5, 3))
    out.append(Case("denormals-and-huge", f))
    # a level reached only at the largest finite value
    f = np.full((4, 4, 5), INF)
    f[0, 3, :] = 2.0                                                 # a pocket above the channel's floor, below its gate
    f[0, 3, 2] = INF
    f[1, 1, :] = -1.0
    f[1, 1, 2] = 9.0                                                 # the channel's gate: the largest finite value
    out.append(Case("level-at-the-largest-finite-value", f))
    out.append(Case("with-map", next(c for c in out if c.name == "ties-(3, 4, 5)").field, map=True))
    return out


@functools.lru_cache(maxsize=None)
def big_cases():
    """One 64^3 with four distinct values: _channels_cases' bars (a network, a bar of its own, a pocket) at three
    levels, everything else blocked."""
    ok = CC.unpack_words(CC.big_cases()[0].words, (64, 64, 64))
    g = np.arange(64)
    f = np.where(ok, -4.0, INF)
    f[ok & (g[None, None, :] % 16 == 7)] = 1.0                       # gates in the bars along a
    f[ok & (g[None, :, None] % 16 == 9)] = 2.5                       # along b
    f[ok & (g[:, None, None] % 16 == 11)] = 6.0                      # along c
    return [Case("grid-64", f, brute=False)]


SKEW = (0.5, 0.125, 0.4375, -0.0625, 0.1875, 0.46875)


def _atoms(n, dims, step, seed):
    xyz, _ = CC.random_atoms(n, dims, seed, step)
    rng = np.random.default_rng(seed + 1)
    eps, sigma = rng.uniform(0.2, 1.0, n), rng.uniform(0.8, 1.3, n)
    return xyz, np.stack([4.0 * eps * sigma ** 12, 4.0 * eps * sigma ** 6], axis=1)


@functools.lru_cache(maxsize=None)
def atom_cases():
    """Jobs with atoms: the field kernel on an orthorhombic and a skewed cell, atom counts round the tile of the field
    kernel (PAS_FIELD_TILE = 128), with and without a cutoff, map on and off."""
    out = []
    h = 0.5
    for n in (0, 1, 128, 129):
        dims = (7, 6, 5)
        xyz, coef = _atoms(n, dims, (h, 0.0, h, 0.0, 0.0, h), 100 + n)
        out.append(Case(f"orthorhombic-n={n}", dims=dims, xyz=xyz, coef=coef, core2=0.09, cutoff2=0.0 if n % 2 else 6.25,
                        origin=(0.25, 0.25, 0.25), step=(h, 0.0, h, 0.0, 0.0, h), map=True))
    xyz, coef = _atoms(9, (9, 8, 7), SKEW, 77)
    out.append(Case("skewed-cell", dims=(9, 8, 7), xyz=xyz, coef=coef, core2=0.16, cutoff2=4.0, origin=(0.1, -0.2, 0.3), step=SKEW,
                    map=True))
    out.append(Case("skewed-cell-no-map", dims=(9, 8, 7), xyz=xyz, coef=coef, core2=0.16, cutoff2=4.0, origin=(0.1, -0.2, 0.3),
                    step=SKEW, map=False))
    xyz, coef = _atoms(70, (66 - 2, 3, 2), SKEW, 78)
    out.append(Case("skewed-two-chunks-a-row", dims=(64, 3, 2), xyz=xyz, coef=coef, core2=0.16, cutoff2=0.0, step=SKEW, map=True,
                    brute=False))
    return out


def mixed_batch():
    """A batch of mixed grids, fields and atoms."""
    return [c for q, c in enumerate(cases()) if q % 4 == 0] + list(atom_cases()) + big_cases()


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    rng = np.random.default_rng(5)
    return [Case("before-a", rng.normal(size=(40, 3, 50))), Case("before-b", rng.integers(0, 3, (2, 33, 9)).astype(np.float64))]


# ---- a call -------------------------------------------------------------------------------------------------------
def pack(jobs, hole: int = 0, reverse: bool = False):
    """The arguments of a call for a list of cases: (PERCOLATION_JOB_DTYPE array, xyz, coef, field, rows of out, rows of
    levels, entries of map).  A job's outputs come one job after the other (`reverse`: the last job's first), `hole`
    entries that nobody owns in front of each; atoms and fields that several jobs hold (the same case object) are stored
    once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.PERCOLATION_JOB_DTYPE)
    xyz, coef, field, where = [np.zeros((0, 3))], [np.zeros((0, 2))], [np.zeros(0)], {}
    atoms = entries = 0
    for c in jobs:
        if id(c) in where:
            continue
        if c.field is None:
            where[id(c)] = atoms
            xyz.append(c.xyz)
            coef.append(c.coef)
            atoms += len(c.xyz)
        else:
            where[id(c)] = entries
            field.append(c.field.reshape(-1))
            entries += c.voxels
    row = level = at = 0
    for k in (range(len(jobs) - 1, -1, -1) if reverse else range(len(jobs))):
        c = jobs[k]
        row, level = row + hole, level + hole
        at += hole if c.map else 0
        a = where[id(c)]
        rec[k] = (a if c.field is None else 0, len(c.xyz) if c.field is None else 0, a if c.field is None else 0,
                  -1 if c.field is None else a, at if c.map else -1, level, row, c.origin, c.step, c.core2, c.cutoff2, *c.dims, 0)
        row, level = row + 1, level + 6
        at += c.voxels if c.map else 0
    return rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(field), row, level, at


def blank(n_out: int, n_levels: int, n_map: int):
    """(levels, out, map) with every byte SENTINEL."""
    from pywindow_amd import _lib

    def filled(dtype, n):
        return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dtype).itemsize * n), dtype=dtype).copy()

    return filled(_lib.PERCOLATION_LEVEL_DTYPE, n_levels), filled(_lib.PERCOLATION_OUT_DTYPE, n_out), filled(np.float64, n_map)


def expected(jobs, hole: int = 0, reverse: bool = False):
    """(levels, out, map) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    rec = pack(jobs, hole, reverse)
    got = blank(*rec[4:7])
    for k, c in enumerate(jobs):
        o, rows, U = reference_cached(c)
        J = rec[0][k]
        got[0][int(J["level_first"]):int(J["level_first"]) + 6] = rows
        got[1][int(J["out"])] = o
        if c.map:
            got[2][int(J["map_first"]):int(J["map_first"]) + c.voxels] = U.reshape(-1)
    return got


def raw(ctx, packed, workspace_bytes=None, timed=False, sizes=None, diagnostics=None):
    """pw_percolation through ctypes into SENTINEL-filled arrays -- through the library's test entry when
    `workspace_bytes` is given (0: the default budget), `timed` or `diagnostics` (a list that receives (n_evaluations,
    n_fills)).  `sizes`: other numbers of rows and entries of (xyz, coef, field, map, levels, out) to tell the entry, None
    for the true ones.  Returns (rc, (levels, out, map)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, field, n_out, n_levels, n_map = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.PERCOLATION_JOB_DTYPE)
    got = blank(n_out, n_levels, n_map)
    told = [len(xyz), len(coef), len(field), n_map, n_levels, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], field.ctypes.data, told[2],
            got[2].ctypes.data, told[3], got[0].ctypes.data, told[4], got[1].ctypes.data, told[5]]
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None and not timed and diagnostics is None:
        rc = L.pw_percolation(*args)
    else:
        n_eval, n_fill = np.zeros(len(rec), dtype=np.int32), np.zeros(len(rec), dtype=np.int32)
        rc = L.pw_internal_percolation(*args, int(workspace_bytes or 0), ctypes.byref(ms) if timed else None, n_eval.ctypes.data,
                                       n_fill.ctypes.data)
        if diagnostics is not None:
            diagnostics.append((n_eval, n_fill))
    return (rc, got, ms.value) if timed else (rc, got)


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: the first entry that differs."""
    for what, g, w in zip(("levels", "out", "map"), got, want):
        for k in range(len(w)):
            if g[k].tobytes() != w[k].tobytes():
                return what, k, g[k], w[k]
    return None


def run_field(ctx, U):
    """(levels (6,), out record) of one field through Context.percolation."""
    from pywindow_amd import _lib

    nz, ny, nx = U.shape
    jobs = np.zeros(1, dtype=_lib.PERCOLATION_JOB_DTYPE)
    jobs[0] = (0, 0, 0, 0, -1, 0, 0, (0.0, 0.0, 0.0), UNIT, 0.25, 0.0, nx, ny, nz, 0)
    levels, out, _ = ctx.percolation(jobs, field=np.ascontiguousarray(U, dtype=np.float64).reshape(-1))
    return levels, out[0]


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = cases()[0]
    other = next(c for c in atom_cases() if c.name == "skewed-cell")   # atoms, with a map
    field2 = Case("field-with-map", next(c for c in cases() if c.name == "ties-(3, 4, 5)").field, map=True)
    out = []

    def edit(fn, reason, sizes=None, second=other):
        packed = list(pack([good, second]))
        fn(packed)
        out.append((tuple(packed), sizes, reason))

    def atom(values):
        def fn(p):
            p[1] = p[1].copy()
            p[1][int(p[0]["atom_first"][1]) + 2] = values
        return fn

    def row(values):
        def fn(p):
            p[2] = p[2].copy()
            p[2][int(p[0]["coef_first"][1]) + 1] = values
        return fn

    def field(name, value):
        def fn(p):
            p[0][name][1] = value
        return fn

    def step(q, value):
        def fn(p):
            p[0]["step"][1][q] = value
        return fn

    def value(v):
        def fn(p):
            p[3] = p[3].copy()
            p[3][int(p[0]["field_first"][1]) + 5] = v
        return fn

    n_atoms, V_good, V_other, V_f2 = len(other.xyz), good.voxels, other.voxels, field2.voxels
    edit(atom([0.0, np.nan, 0.0]), "a coordinate is not finite")
    edit(atom([np.inf, 0.0, 0.0]), "a coordinate is not finite")
    edit(row([np.nan, 1.0]), "a coefficient is not finite")
    edit(row([-1.0, 1.0]), "a coefficient outside 0 .. 1e100")
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin or a step is not finite")
    edit(step(3, np.inf), "the origin or a step is not finite")
    for q in (0, 2, 5):
        edit(step(q, 0.0), "ax, by or cz <= 0")
        edit(step(q, -0.5), "ax, by or cz <= 0")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(field("core2", np.nan), "core2 below 1e-6 or not finite")
    edit(field("cutoff2", 0.1), "cutoff2 is neither 0 nor above core2")
    edit(field("n", -1), "a negative count")
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", sizes=(n_atoms - 1, None, None, None, None, None))
    edit(lambda p: None, "coefficients outside coef", sizes=(None, n_atoms - 1, None, None, None, None))
    edit(field("field_first", -2), "the field is outside its array")
    edit(lambda p: None, "the field is outside its array", sizes=(None, None, V_good + V_f2 - 1, None, None, None), second=field2)
    edit(value(np.nan), "a field value is -inf or not a number", second=field2)
    edit(value(-np.inf), "a field value is -inf or not a number", second=field2)
    edit(field("map_first", -2), "the map is outside its array")
    edit(lambda p: None, "the map is outside its array", sizes=(None, None, None, V_other - 1, None, None))
    edit(lambda p: None, "the rows are outside levels", sizes=(None, None, None, None, 11, None))
    edit(field("level_first", -1), "the rows are outside levels")
    edit(lambda p: None, "the row is outside out", sizes=(None, None, None, None, None, 1))
    edit(field("out", -1), "the row is outside out")
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", 5), "shares rows of levels with an earlier job")

    def both_maps(p):
        p[0]["map_first"][0] = V_other - 1                          # job 0 gets a map that meets job 1's
        p[6] = V_other - 1 + V_good
    edit(both_maps, "shares entries of map with an earlier job")
    return out


# ---- the crystal cell of tests/golden/rebuild.npz ---------------------------------------------------------------
def cc3_cell():
    """(elements, coordinates, lattice) of the CC3 cell of the golden file."""
    return CC.crystal("cc3_cell")


# ---- checks that both the host and the device file run, on a context ----------------------------------------------
def check_against_channels(ctx, U):
    """Library against library: at each finite B_c, Context.channels with ready-made open words equal to allowed_{B_c}
    lists a component with the same first, n_voxels, wraps and rank that meets the criterion, and none before it does;
    with the words of the next lower distinct value no component meets the criterion."""
    from pywindow_amd import _lib

    nz, ny, nx = U.shape
    levels, _ = run_field(ctx, U)
    values = np.unique(U[np.isfinite(U)])

    def components(t):
        ok = np.isfinite(U) & (U <= t)
        job = np.zeros(1, dtype=_lib.CHANNELS_JOB_DTYPE)
        job[0] = (0, 0, 0, 0, -1, -1, 0, (0.0, 0.0, 0.0), UNIT, 0.0, nx, ny, nz, 254)
        out, comps, _, _ = ctx.channels(job, np.zeros((0, 3)), np.zeros(0), open_words=CC.pack_words(ok), open_first=[0])
        assert not out[0]["flags"]
        return comps[:int(out[0]["n_recorded"])]

    for c, row in enumerate(levels):
        if row["flags"]:
            top = components(values[-1]) if len(values) else []
            assert not any(meets(k["wraps"], c) for k in top), c
            continue
        comps = components(row["level"])
        hits = [k for k in comps if meets(k["wraps"], c)]
        assert hits and tuple(hits[0][["first", "n_voxels", "wraps", "rank"]]) == tuple(row[["first", "n_voxels", "wraps", "rank"]]), c
        lower = values[values < row["level"]]
        if len(lower):
            assert not any(meets(k["wraps"], c) for k in components(lower[-1])), c


def keys(levels):
    """The six levels as the integers that order as the doubles compare (pw_passage's key, written again)."""
    bits = np.ascontiguousarray(levels["level"], dtype=np.float64).view(np.uint64).copy()
    bits[bits == np.uint64(0x8000000000000000)] = 0
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(0x8000000000000000))
