"""Inputs shared by tests/test_rigid_cell.py (host path against the definition) and tests/test_gpu_rigid_cell.py (device
against the host path and the definition): the orientation-averaged Boltzmann factor of a rigid linear guest at every
voxel of a periodic cell (pw_rigid_cell).  Every comparison is of bytes.  numpy only and seeded; nothing here is taken
from pywindow_amd/csrc/pw_rigid_cell.hpp -- `reference` is the definition of include/pywindow_amd.h written directly:
every operation one IEEE operation of numpy, ALL atoms and no skip, the pose energies on (voxel, orientation) arrays by
a Python loop over the sites and the atoms, the fold over the orientations one column after the other, the chunk tree
spelled out (`chunk_total`), pw_exp element by element through the library's test entry on a host context
(tests/_kde_cases.py: internal_exp)."""
import numpy as np

import _kde_cases as K

SENTINEL = 0xA5
TILE = 128          # atoms staged at a time
NEAR_CAP = 2048     # indices of the near list of a group
CLAMPED = 1
INF = np.inf
SKEW = (0.5, 0.125, 0.4375, -0.0625, 0.1875, 0.46875)


def ortho(h):
    return (h, 0.0, h, 0.0, 0.0, h)


class Case:
    """One job: atoms (n, 3) with rows (A, B) per site (S, n, 2), the S offsets, the M directions (M, 3), the grid
    (origin, step, dims (nx, ny, nz)), core2, cutoff2, the betas and whether it asks for its maps."""

    def __init__(self, name, dims, xyz=None, coef=None, offsets=(0.0,), dirs=((0.0, 0.0, 1.0),), origin=(0.0, 0.0, 0.0),
                 step=ortho(1.0), core2=0.25, cutoff2=9.0, betas=(0.4,), map=True):
        self.name, self.dims = name, tuple(int(d) for d in dims)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        self.dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        S = len(self.offsets)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = (np.zeros((S, 0, 2)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64)).reshape(S, -1, 2)
        self.origin, self.step = np.asarray(origin, dtype=np.float64), np.asarray(step, dtype=np.float64)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        self.map = bool(map)
        assert self.coef.shape[1] == len(self.xyz)

    @property
    def voxels(self):
        return self.dims[0] * self.dims[1] * self.dims[2]


def centres(c: Case):
    """(x, y, z) of the voxels in rank order, in the association of the definition."""
    nx, ny, nz = c.dims
    ax, bx, by, cx, cy, cz = c.step
    l, j, i = (v.reshape(-1).astype(np.float64) for v in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"))
    z = c.origin[2] + l * cz
    y = (c.origin[1] + j * by) + l * cy
    x = ((c.origin[0] + i * ax) + j * bx) + l * cx
    return x, y, z


def pose_energies(c: Case):
    """(U, blocked), both (V, M), by the definition, over every atom; U is 0 where blocked."""
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
            for (X, Y, Z), (a, b) in zip(c.xyz, c.coef[s]):
                dx, dy, dz = px - X, py - Y, pz - Z
                r2 = (dx * dx + dy * dy) + dz * dz
                blocked |= r2 <= c.core2
                inv = 1.0 / r2
                s6 = (inv * inv) * inv
                u = s6 * (a * s6 - b)
                Us = np.where(r2 <= c.cutoff2, Us + u, Us)
            U = Us if s == 0 else U + Us
    return np.where(blocked, 0.0, U), blocked


def chunk_total(slots: np.ndarray) -> np.float64:
    """The sum of the slots by the definition: chunks of 64 ranks padded with +0.0, in a chunk for k = 1, 2, 4, 8, 16, 32
    slot[t] = slot[t] + slot[t + k] at every t that is a multiple of 2k, then the chunk sums in chunk order from +0.0."""
    chunks = -(-len(slots) // 64)
    a = np.zeros(chunks * 64)
    a[:len(slots)] = slots
    a = a.reshape(chunks, 64)
    k = 1
    while k < 64:
        for t in range(0, 64, 2 * k):
            a[:, t] = a[:, t] + a[:, t + k]
        k *= 2
    total = np.float64(0.0)
    for c in range(chunks):
        total = total + a[c, 0]
    return total


def reference(c: Case, host):
    """(a RIGID_OUT_DTYPE record, the L level rows, the (L + 1, V) planes zbar_0 .. zbar_{L-1}, umin_v) of the definition."""
    from pywindow_amd import _lib

    U, blocked = pose_energies(c)
    live = ~blocked
    V, M = U.shape
    nx, ny, _ = c.dims
    L = len(c.betas)
    inv_M = np.float64(1.0) / np.float64(M)
    out = np.zeros((), dtype=_lib.RIGID_OUT_DTYPE)
    levels = np.zeros(L, dtype=_lib.AFFINITY_LEVEL_DTYPE)
    planes = np.zeros((L + 1, V))
    out["n_voxels"], out["n_blocked_poses"], out["n_dead"] = V, int(blocked.sum()), int((~live.any(axis=1)).sum())
    umin_v = np.where(live, U, INF).min(axis=1)
    planes[L] = umin_v
    flags = 0
    for b, beta in enumerate(c.betas):
        arg = -(beta * U)
        if (arg[live] > 700.0).any():
            flags |= CLAMPED
        w = K.internal_exp(host, np.where(arg > 700.0, 700.0, arg).reshape(-1)).reshape(V, M)
        e = w * U
        zs, es = np.zeros(V), np.zeros(V)
        for o in range(M):
            zs = np.where(live[:, o], zs + w[:, o], zs)
            es = np.where(live[:, o], es + e[:, o], es)
        planes[b], ebar = zs * inv_M, es * inv_M
        levels[b] = (chunk_total(planes[b]), chunk_total(ebar))
    out["flags"] = flags
    out["u_min"], out["min_voxel"], out["min_dir"] = INF, -1, -1
    if live.any():
        m = umin_v.min()
        rank = int(np.flatnonzero(umin_v == m)[0])
        out["u_min"], out["min_voxel"] = m, (rank % nx, (rank // nx) % ny, rank // (nx * ny))
        out["min_dir"] = int(np.flatnonzero(live[rank] & (U[rank] == m))[0])
    return out, levels, planes


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
    def g():
        if f.__name__ not in _lists:
            _lists[f.__name__] = f()
        return _lists[f.__name__]
    g.__name__ = f.__name__
    return g


def dirs_of(M: int, seed: int) -> np.ndarray:
    """M random directions of length 1 up to rounding, every component within [-1, 1]."""
    v = np.random.default_rng(seed).normal(size=(M, 3))
    return np.clip(v / np.linalg.norm(v, axis=1)[:, None], -1.0, 1.0)


def line(S: int, reach: float) -> np.ndarray:
    return np.zeros(1) if S == 1 else np.linspace(-reach, reach, S)


def box_atoms(n: int, S: int, dims, step, seed: int, pad: float = 4.0, origin=(0.0, 0.0, 0.0)):
    """n atoms spread over the cell's bounding box and `pad` around it -- inside the grid, within the reach of some
    groups only, and beyond every reach -- with S rows (A, B) each: (xyz, coef (S, n, 2))."""
    rng = np.random.default_rng(seed)
    ax, bx, by, cx, cy, cz = step
    nx, ny, nz = dims
    corners = np.array([[i * nx * ax + j * ny * bx + l * nz * cx, j * ny * by + l * nz * cy, l * nz * cz]
                        for i in (0, 1) for j in (0, 1) for l in (0, 1)]) + np.asarray(origin)
    lo, hi = corners.min(axis=0) - pad, corners.max(axis=0) + pad
    xyz = rng.uniform(lo, hi, (n, 3))
    sigma, eps = rng.uniform(0.6, 1.2, (S, n)), rng.uniform(0.1, 1.0, (S, n))
    return xyz, np.stack([4.0 * eps * sigma ** 12, 4.0 * eps * sigma ** 6], axis=2)


def edge_case(name, cutoff2):
    """Exact arithmetic on an orthorhombic grid of unit steps (a 5 x 5 x 5 grid: the group of the voxels 0 .. 3 and the
    cut groups beside it), two sites at offsets 0 and 1, the directions +x and -z.  Atoms at r2 == 25 exactly from the
    second site of the pose +x of voxel (0, 0, 0) -- a corner of its group -- , of voxel (2, 1, 2) -- its middle -- and of
    voxel (3, 3, 3), straight out along x; `cutoff2` is 25, one ulp below or one ulp above.  An atom at r2 == core2
    exactly from the centre of voxel (4, 4, 0).  Twenty atoms far beyond every reach."""
    near = [[-2.0, 0.0, -4.0], [3.0, 4.0, 6.0], [9.0, 3.0, 3.0], [4.5, 4.0, 0.0]]
    far = np.random.default_rng(3).uniform(30.0, 40.0, (20, 3)) * np.random.default_rng(4).choice([-1.0, 1.0], (20, 3))
    xyz = np.concatenate([near, far])
    coef = np.zeros((2, len(xyz), 2))
    coef[0, :, 0], coef[0, :, 1] = 3.0, 2.0
    coef[1, :, 0], coef[1, :, 1] = 5.0, 1.0
    return Case(name, (5, 5, 5), xyz, coef, offsets=(0.0, 1.0), dirs=((1.0, 0.0, 0.0), (0.0, 0.0, -1.0)), core2=0.25, cutoff2=cutoff2,
                betas=(0.5, 1.0))


@_once
def cases():
    """The case list: the smallest shapes at which the kernel and the host path can go wrong."""
    out = []
    d = (7, 6, 5)
    # atom counts: none, one, the staging tile and one more; the skewed cell with all six steps non-zero
    for n in (0, 1, TILE, TILE + 1):
        out.append(Case(f"n={n}", d, *box_atoms(n, 2, d, SKEW, 10 + n, pad=2.0), offsets=(-0.3, 0.3), dirs=dirs_of(3, 20 + n),
                        origin=(0.1, -0.2, 0.3), step=SKEW, core2=0.04, cutoff2=4.0, betas=(0.4, 1.0)))
    # more survivors than the near list holds inside one group's reach: the pass loop runs (a small cell, a long cutoff)
    dd = (5, 4, 3)
    out.append(Case(f"n={NEAR_CAP + 150}", dd, *box_atoms(NEAR_CAP + 150, 1, dd, ortho(0.5), 31, pad=1.0), dirs=dirs_of(3, 32),
                    step=ortho(0.5), core2=0.0025, cutoff2=100.0))
    out.append(Case(f"n={2 * NEAR_CAP + 70},S=2", (2, 2, 1), *box_atoms(2 * NEAR_CAP + 70, 2, (2, 2, 1), ortho(0.5), 33, pad=1.0),
                    offsets=(-0.2, 0.2), dirs=dirs_of(2, 34), step=ortho(0.5), core2=0.0025, cutoff2=64.0))
    # orientations: 1, 2, 3 (the register pair has a tail), 64, and 1024 on one voxel
    d = (4, 3, 2)
    for M in (1, 2, 3, 64):
        out.append(Case(f"M={M}", d, *box_atoms(9, 2, d, ortho(0.9), 40 + M), offsets=(-0.35, 0.35), dirs=dirs_of(M, 50 + M),
                        step=ortho(0.9), betas=(0.0, 0.8)))
    out.append(Case("M=1024", (1, 1, 1), *box_atoms(7, 3, (1, 1, 1), ortho(0.9), 41), offsets=line(3, 0.4), dirs=dirs_of(1024, 51),
                    step=ortho(0.9)))
    # sites: 1, 2, 3, and the guarded instance at 4 and 8
    d = (6, 5, 2)
    for S in (1, 2, 3, 4, 8):
        out.append(Case(f"S={S}", d, *box_atoms(11, S, d, SKEW, 60 + S), offsets=line(S, 0.5), dirs=dirs_of(5, 70 + S), step=SKEW,
                        core2=0.04, cutoff2=6.25, betas=(0.3, 0.9)))
    out.append(Case(f"n={TILE + 1},S=8", (3, 3, 2), *box_atoms(TILE + 1, 8, (3, 3, 2), ortho(0.8), 61), offsets=line(8, 0.6),
                    dirs=dirs_of(3, 71), step=ortho(0.8), core2=0.01))
    # grid shapes: the word's edges along x, one row and a prime number of rows, V off the chunk and off the group
    for nx in (1, 2, 63, 64):
        dn = (nx, 3, 2)
        out.append(Case(f"nx={nx}", dn, *box_atoms(6, 1, dn, ortho(0.5), 80 + nx, pad=1.0), dirs=dirs_of(2, 90 + nx), step=ortho(0.5),
                        core2=0.01, cutoff2=4.0))
    out.append(Case("rows=1", (9, 1, 1), *box_atoms(5, 2, (9, 1, 1), SKEW, 85, pad=1.0), offsets=(-0.2, 0.2), dirs=dirs_of(3, 95),
                    step=SKEW, core2=0.01))
    out.append(Case("rows=prime", (3, 1, 37), *box_atoms(8, 1, (3, 1, 37), SKEW, 86, pad=1.0), dirs=dirs_of(2, 96), step=SKEW,
                    core2=0.01, cutoff2=4.0))
    out.append(Case("rows=prime-along-b", (2, 13, 1), *box_atoms(8, 3, (2, 13, 1), SKEW, 87, pad=1.0), offsets=line(3, 0.3),
                    dirs=dirs_of(3, 97), step=SKEW, core2=0.01, cutoff2=4.0))
    # the cutoff's edge and the core's edge
    out.append(edge_case("cutoff2=25", 25.0))
    out.append(edge_case("cutoff2=25-ulp", np.nextafter(25.0, 0.0)))
    out.append(edge_case("cutoff2=25+ulp", np.nextafter(25.0, 30.0)))
    # a site with A = B = 0 adds nothing and still blocks: the atom is at r2 == core2 exactly from the second site of the
    # pose +x of voxel (1, 0, 0), whose centre and other pose are free
    out.append(Case("zero-site-blocks", (3, 1, 1), [[2.5, 0.0, 0.0]], [[[3.0, 2.0]], [[0.0, 0.0]]], offsets=(0.0, 1.0),
                    dirs=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), core2=0.25, cutoff2=16.0))
    # directions that are no unit vectors: the reach has to take their norms as they are
    d = (6, 5, 4)
    out.append(Case("direction-norms", d, *box_atoms(60, 2, d, ortho(0.5), 100, pad=7.0), offsets=(-2.0, 1.5),
                    dirs=((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (1.0, 1.0, 1.0), (-1.0, 1.0, -1.0)), step=ortho(0.5), core2=0.01,
                    cutoff2=6.25))
    # degenerate outputs
    out.append(Case("all-dead", (4, 3, 2), [[1.0, 1.0, 0.0]], [[[1.0, 1.0]]], dirs=dirs_of(3, 9), core2=1e6, cutoff2=2e6))
    out.append(Case("one-live-pose", (1, 1, 1), [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [4.0, 4.0, 4.0]], np.full((2, 3, 2), 1.5),
                    offsets=(0.0, 1.0), dirs=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), core2=0.01, cutoff2=64.0))
    out.append(Case("tied-voxels-and-clamp", (6, 1, 1), [[2.5, 0.0, 0.0]], [[[0.0, 1.0]]], dirs=((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)),
                    core2=0.01, cutoff2=100.0, betas=(1.0, 1e3)))
    xyz, coef = box_atoms(6, 1, (5, 4, 1), ortho(0.9), 110)
    d0 = dirs_of(1, 111)[0]
    out.append(Case("tied-orientations", (5, 4, 1), xyz, np.concatenate([coef, coef]), offsets=(-0.4, 0.4), dirs=(d0, -d0),
                    step=ortho(0.9), core2=0.01))
    d = (7, 6, 5)
    for L in (1, 8):
        out.append(Case(f"L={L}", d, *box_atoms(12, 3, d, ortho(0.6), 8), offsets=line(3, 0.3), dirs=dirs_of(4, 92), step=ortho(0.6),
                        betas=np.linspace(0.0, 2.0, 8)[:L] if L > 1 else (0.4,)))
    out.append(Case("no-map", d, *box_atoms(12, 3, d, ortho(0.6), 8), offsets=line(3, 0.3), dirs=dirs_of(4, 92), step=ortho(0.6),
                    map=False))
    return out


@_once
def other_shapes():
    d = (11, 3, 9)
    return [Case("other-a", d, *box_atoms(40, 3, d, ortho(0.5), 40), offsets=line(3, 0.3), dirs=dirs_of(7, 42), step=ortho(0.5),
                 betas=(0.1, 0.2, 0.3)),
            Case("other-b", (2, 2, 2), *box_atoms(3, 1, (2, 2, 2), ortho(1.0), 41))]


@_once
def shared_batch():
    """Jobs that share their atoms, rows and directions: three grids on one set of atoms."""
    atoms = box_atoms(30, 2, (8, 8, 8), ortho(0.5), 120)
    dirs = dirs_of(5, 121)
    return [Case(f"shared-{q}", d, *atoms, offsets=(-0.3, 0.3), dirs=dirs, step=ortho(0.5), core2=0.01, cutoff2=4.0, betas=(0.2 + q,),
                 map=q != 1) for q, d in enumerate(((8, 8, 8), (5, 3, 2), (1, 9, 4)))]


def pack(jobs, hole: int = 0, reverse: bool = False):
    """(rec, xyz, coef, offsets, dirs, betas, n_maps, n_levels, n_out): the arrays of one call.  A job's outputs come one
    job after the other (`reverse`: the last job's first), `hole` rows and entries nobody owns in front of each; atoms,
    rows and directions that two cases share (the same array) are stored once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.RIGID_CELL_JOB_DTYPE)
    xyz, coef, offsets, dirs, betas = [np.zeros((0, 3))], [np.zeros((0, 2))], [], [np.zeros((0, 3))], []
    at_xyz, at_coef, at_dirs = {}, {}, {}
    n_atoms = n_rows = n_sites = n_dirs = n_betas = 0
    firsts = []
    for c in jobs:
        if c.xyz.ctypes.data not in at_xyz or at_xyz[c.xyz.ctypes.data][1] != len(c.xyz):   # (the same memory: the same atoms)
            at_xyz[c.xyz.ctypes.data] = (n_atoms, len(c.xyz))
            xyz.append(c.xyz)
            n_atoms += len(c.xyz)
        if c.coef.ctypes.data not in at_coef or at_coef[c.coef.ctypes.data][1] != c.coef.shape[:2]:
            at_coef[c.coef.ctypes.data] = (n_rows, c.coef.shape[:2])
            coef.append(c.coef.reshape(-1, 2))
            n_rows += c.coef.shape[0] * c.coef.shape[1]
        if c.dirs.ctypes.data not in at_dirs or at_dirs[c.dirs.ctypes.data][1] != len(c.dirs):
            at_dirs[c.dirs.ctypes.data] = (n_dirs, len(c.dirs))
            dirs.append(c.dirs)
            n_dirs += len(c.dirs)
        firsts.append((at_xyz[c.xyz.ctypes.data][0], at_coef[c.coef.ctypes.data][0], at_dirs[c.dirs.ctypes.data][0], n_betas, n_sites))
        offsets.append(c.offsets)
        betas.append(c.betas)
        n_sites += len(c.offsets)
        n_betas += len(c.betas)
    n_maps = n_levels = n_out = 0
    for k in (range(len(jobs) - 1, -1, -1) if reverse else range(len(jobs))):
        c = jobs[k]
        n_out, n_levels = n_out + hole, n_levels + hole
        n_maps += hole if c.map else 0
        a, r, dd, b, s = firsts[k]
        rec[k] = (a, len(c.xyz), r, b, len(c.betas), s, len(c.offsets), dd, len(c.dirs), n_levels, n_maps if c.map else -1, n_out,
                  c.origin, c.step, c.core2, c.cutoff2, *c.dims, 0)
        n_out += 1
        n_levels += len(c.betas)
        n_maps += (len(c.betas) + 1) * c.voxels if c.map else 0
    return (rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(offsets + [np.zeros(0)]), np.concatenate(dirs),
            np.concatenate(betas + [np.zeros(0)]), n_maps, n_levels, n_out)


def blank(n_out, n_levels, n_maps):
    """(out, levels, maps) with every byte SENTINEL."""
    from pywindow_amd import _lib

    def filled(dtype, n):
        dtype = np.dtype(dtype)
        return np.frombuffer(bytes([SENTINEL]) * (dtype.itemsize * n), dtype=dtype).copy()

    return filled(_lib.RIGID_OUT_DTYPE, n_out), filled(_lib.AFFINITY_LEVEL_DTYPE, n_levels), filled(np.float64, n_maps)


def expected(jobs, host, hole: int = 0, reverse: bool = False):
    """(out, levels, maps) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    packed = pack(jobs, hole, reverse)
    rec = packed[0]
    out, levels, mp = blank(packed[8], packed[7], packed[6])
    for k, c in enumerate(jobs):
        o, lv, planes = reference_cached(c, host)
        out[int(rec["out"][k])] = o
        levels[int(rec["level_first"][k]):int(rec["level_first"][k]) + len(lv)] = lv
        if c.map:
            mp[int(rec["map_first"][k]):int(rec["map_first"][k]) + planes.size] = planes.reshape(-1)
    return out, levels, mp


def raw(ctx, packed, workspace_bytes=None, sizes=None, diagnostics=None, skip=True):
    """pw_rigid_cell through ctypes into SENTINEL-filled arrays -- through the library's test entry when `workspace_bytes`
    is given (0: the default budget), with `diagnostics` (a list that receives (n_pairs, instances)) or with skip=False.
    `sizes`: other numbers of rows and entries of (xyz, coef, offsets, dirs, betas, maps, levels, out) to tell the entry,
    None for the true ones.  Returns (rc, (out, levels, maps))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, offsets, dirs, betas, n_maps, n_levels, n_out = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.RIGID_CELL_JOB_DTYPE)
    out, levels, mp = blank(n_out, n_levels, n_maps)
    told = [len(xyz), len(coef), len(offsets), len(dirs), len(betas), n_maps, n_levels, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], offsets.ctypes.data, told[2],
            dirs.ctypes.data, told[3], betas.ctypes.data, told[4], mp.ctypes.data, told[5], levels.ctypes.data, told[6],
            out.ctypes.data, told[7]]
    if workspace_bytes is None and diagnostics is None and skip:
        rc = L.pw_rigid_cell(*args)
    else:
        n_pairs, instances = np.zeros(len(rec), dtype=np.int64), np.zeros(1, dtype=np.int32)
        rc = L.pw_internal_rigid_cell(*args, int(workspace_bytes or 0), None, n_pairs.ctypes.data, 1 if skip else 0,
                                      instances.ctypes.data)
        if diagnostics is not None:
            diagnostics.append((n_pairs, int(instances[0])))
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


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = next(c for c in cases() if c.name == "M=2")
    other = next(c for c in cases() if c.name == "S=3")
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
    row = lambda p: 2 * (int(p[0]["coef_first"][1]) + len(other.xyz) + 2)      # (site 1, atom 2)
    site = lambda p: int(p[0]["site_first"][1]) + 1
    comp = lambda p: 3 * (int(p[0]["dir_first"][1]) + 2) + 1
    n_atoms = len(good.xyz) + len(other.xyz)
    n_rows = good.coef.shape[0] * good.coef.shape[1] + other.coef.shape[0] * other.coef.shape[1]
    n_sites, n_dirs, n_betas = len(good.offsets) + len(other.offsets), len(good.dirs) + len(other.dirs), len(good.betas) + len(other.betas)
    maps_good, maps_other = (len(good.betas) + 1) * good.voxels, (len(other.betas) + 1) * other.voxels
    none = [None] * 8

    def told(q, v):
        return tuple(none[:q] + [v] + none[q + 1:])

    edit(field("cutoff2", 0.0), "cutoff2 is 0")
    edit(field("cutoff2", 0.04), "cutoff2 is neither 0 nor above core2")
    edit(field("cutoff2", 0.03), "cutoff2 is neither 0 nor above core2")
    edit(field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(field("n_sites", 0), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_sites", 9), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_dirs", 0), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(field("n_dirs", 1025), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(entry(3, site, 16.5), "an offset is not finite or beyond 16")
    edit(entry(3, site, np.nan), "an offset is not finite or beyond 16")
    edit(entry(4, comp, 1.5), "a direction's component is not finite or outside -1 .. 1")
    edit(entry(4, comp, -np.inf), "a direction's component is not finite or outside -1 .. 1")
    edit(entry(2, row, -1.0), "a coefficient outside 0 .. 1e100")
    edit(entry(2, row, np.nan), "a coefficient is not finite")
    edit(entry(1, atom, np.nan), "a coordinate is not finite")
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin or a step is not finite")
    for q in (0, 2, 5):
        def step(p, q=q):
            p[0]["step"][1][q] = 0.0
        edit(step, "ax, by or cz <= 0")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("n", -1), "a negative count")
    edit(field("n_betas", 0), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(field("n_betas", 9), "n_betas outside 1 .. PW_AFF_MAX_LEVELS")
    edit(entry(5, lambda p: int(p[0]["beta_first"][1]) + 1, -0.5), "a beta is negative or not finite")
    # short arrays
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", told(0, n_atoms - 1))
    edit(lambda p: None, "coefficients outside coef", told(1, n_rows - 1))
    edit(lambda p: None, "sites outside offsets", told(2, n_sites - 1))
    edit(lambda p: None, "directions outside dirs", told(3, n_dirs - 1))
    edit(lambda p: None, "betas outside the array", told(4, n_betas - 1))
    edit(lambda p: None, "the maps are outside their array", told(5, maps_good + maps_other - 1))
    edit(field("map_first", -2), "the maps are outside their array")
    edit(lambda p: None, "the rows are outside levels", told(6, n_betas - 1))
    edit(lambda p: None, "the row is outside out", told(7, 1))
    # shared outputs: the later job is named
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", len(good.betas) - 1), "shares rows of levels with an earlier job")
    edit(field("map_first", maps_good - 1), "shares maps with an earlier job")
    return out


def as_percolation_case(c: Case):
    """The one-site, one-direction job of a case's atoms: (Case, the (A, B) rows (n, 2))."""
    one = Case(c.name + "-one-site", c.dims, c.xyz, c.coef[:1], offsets=(0.0,), dirs=((0.3, -0.2, 0.9),), origin=c.origin, step=c.step,
               core2=c.core2, cutoff2=c.cutoff2, betas=c.betas)
    return one, np.ascontiguousarray(c.coef[0])
