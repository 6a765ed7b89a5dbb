"""Inputs shared by tests/test_rigid_body.py (host path against the definition) and tests/test_gpu_rigid_body.py (device
against the host path): the pose-averaged affinity of a region of voxels for a rigid guest given as a pose table
(pw_rigid_body_affinity).  Every comparison is of bytes.  numpy only and seeded; nothing here is taken from
pywindow_amd/csrc/pw_rigid_body.hpp -- `reference` is tests/_rigid_cases.py's definition with the site position read from
the table: the pose energies on (voxel, pose) arrays by a Python loop over the sites and the atoms, the fold over the
poses one column after the other, the chunk tree by reshapes, pw_exp through the library's test entry on a host
context."""
import numpy as np

import _affinity_cases as A
import _kde_cases as K
import _rigid_cases as R
import _stat_edges as S

SENTINEL = R.SENTINEL
TILE = R.TILE
CLAMPED = R.CLAMPED
MAX_SITES, MAX_DIRS = R.MAX_SITES, R.MAX_DIRS


def pose_block() -> int:
    """The poses whose displacements the kernel holds in LDS at a time."""
    return S.constant("RIGID_BODY_POSE_BLOCK", "pw_rigid_body.hpp")


class Case:
    """One job: atoms (n, 3) with rows (A, B, C) per site (S, n, 3), the pose table (M, S, 3), the grid (origin, spacing
    h, dims (nx, ny, nz)), the region's words (None: every voxel), core2, cutoff2, the betas, charged and map_level."""

    def __init__(self, name, dims, xyz=None, coef=None, poses=(((0.0, 0.0, 0.0),),), words=None, origin=(0.0, 0.0, 0.0), h=1.0,
                 core2=0.25, cutoff2=0.0, betas=(0.4,), charged=0, map_level=-1):
        self.name, self.dims = name, tuple(int(d) for d in dims)
        self.poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert self.poses.ndim == 3 and self.poses.shape[2] == 3
        S_ = self.poses.shape[1]
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = (np.zeros((S_, 0, 3)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64)).reshape(S_, -1, 3)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        self.origin, self.h = np.asarray(origin, dtype=np.float64), float(h)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        self.charged, self.map_level = int(charged), int(map_level)
        assert self.coef.shape[1] == len(self.xyz)
        assert self.words is None or len(self.words) == self.dims[1] * self.dims[2]

    @property
    def M(self):
        return self.poses.shape[0]

    @property
    def S(self):
        return self.poses.shape[1]


region = A.region
centres = R.centres
words_with = A.words_with
guest_atoms = R.guest_atoms


def pose_energies(c: Case):
    """(U, blocked), both (V, M), by the definition; U is 0 where blocked."""
    x, y, z = centres(c)
    V, M = len(x), c.M
    U = np.zeros((V, M))
    blocked = np.zeros((V, M), dtype=bool)
    with np.errstate(all="ignore"):
        for s in range(c.S):
            px = x[:, None] + c.poses[None, :, s, 0]
            py = y[:, None] + c.poses[None, :, s, 1]
            pz = z[:, None] + c.poses[None, :, s, 2]
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
    def g(*args):
        if (f.__name__, args) not in _lists:
            _lists[(f.__name__, args)] = f(*args)
        return _lists[(f.__name__, args)]
    g.__name__ = f.__name__
    return g


def random_rotations(M: int, seed: int) -> np.ndarray:
    """M random proper rotations (M, 3, 3): the Q of a QR of normal matrices, a column flipped where det < 0."""
    q = np.linalg.qr(np.random.default_rng(seed).normal(size=(M, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def body(S_: int, reach: float, seed: int) -> np.ndarray:
    """S site positions (S, 3) within `reach` of the centre, not on a line for S >= 3."""
    return np.random.default_rng(3000 + seed).uniform(-reach, reach, (S_, 3)) / np.sqrt(3.0)


def table(S_: int, M: int, reach: float, seed: int) -> np.ndarray:
    """The pose table (M, S, 3) of a random body in M random rotations (what pywindow_amd.body_poses computes, here by
    its own sum)."""
    p, rot = body(S_, reach, seed), random_rotations(M, seed)
    return (rot[:, None, :, 0] * p[None, :, 0, None] + rot[:, None, :, 1] * p[None, :, 1, None]) + rot[:, None, :, 2] * p[None, :, 2, None]


def from_linear(c) -> Case:
    """A job of tests/_rigid_cases.py as a table: p[o, s] = t_s * d_o, one rounded product a component."""
    return Case(c.name, c.dims, c.xyz, c.coef, c.offsets[None, :, None] * c.dirs[:, None, :], words=c.words, origin=c.origin, h=c.h,
                core2=c.core2, cutoff2=c.cutoff2, betas=c.betas, charged=c.charged, map_level=c.map_level)


def from_affinity(c) -> Case:
    """A job of tests/_affinity_cases.py as a body job: one site at the centre, one pose, not charged."""
    coef = np.concatenate([c.coef, np.zeros((len(c.coef), 1))], axis=1)[None]
    return Case(c.name, c.dims, c.xyz, coef, np.zeros((1, 1, 3)), words=c.words, origin=c.origin, h=c.h, core2=c.core2,
                cutoff2=c.cutoff2, betas=c.betas)


@_once
def cases():
    """The case list of the issue, small grids."""
    out = []
    PB = pose_block()
    d = (6, 5, 2)
    for S_ in range(1, MAX_SITES + 1):                               # every unguarded instance and the guarded one with fewer than 8
        for charged in (0, 1):
            out.append(Case(f"S={S_},charged={charged}", d, *guest_atoms(7, S_, d, 0.8, 50 + S_), table(S_, 5, 0.5, 60 + S_), h=0.8,
                            betas=(0.3, 0.9), charged=charged, map_level=charged))
    d = (4, 3, 2)
    for M in (1, 2, 3, PB - 1, PB, PB + 1):                          # S = 3: an unguarded instance that evaluates two poses a pass
        out.append(Case(f"M={M}", d, *guest_atoms(5, 3, d, 0.9, 30 + M), table(3, M, 0.45, 40 + M), h=0.9, betas=(0.0, 0.8),
                        charged=M % 2, map_level=1))
    out.append(Case(f"M={PB + 1},S=6", d, *guest_atoms(5, 6, d, 0.9, 33), table(6, PB + 1, 0.45, 43), h=0.9, charged=1, map_level=0))
    out.append(Case(f"M={2 * PB + 1},S=7", (2, 2, 1), *guest_atoms(3, 7, (2, 2, 1), 0.9, 34), table(7, 2 * PB + 1, 0.45, 44), h=0.9))
    out.append(Case("M=1024,S=8", (1, 1, 1), [[0.9, 0.4, -0.7]], guest_atoms(1, 8, (1, 1, 1), 1.0, 35)[1], table(8, 1024, 0.4, 45),
                    charged=1, map_level=0))
    d = (9, 7, 3)
    out.append(Case("n=0", d, poses=table(3, 3, 0.4, 7), words=words_with(d, 100, 7), betas=(0.0, 0.7), map_level=1))
    for n in (1, TILE, TILE + 1):
        out.append(Case(f"n={n}", d, *guest_atoms(n, 4, d, 0.8, 20 + n), table(4, 5, 0.4, 70 + n), words=words_with(d, 70, 8), h=0.8,
                        cutoff2=16.0 if n % 2 else 0.0, charged=n % 2))
    # the atoms restaged pass by pass and the poses block by block, in the two-pose and in the one-pose instances
    out.append(Case(f"n={TILE + 1},M={PB + 2},S=3", (5, 3, 1), *guest_atoms(TILE + 1, 3, (5, 3, 1), 0.8, 22), table(3, PB + 2, 0.4, 72),
                    h=0.8, betas=(0.5, 1.0), map_level=1))
    out.append(Case(f"n={2 * TILE + 1},M={PB + 1},S=8", (3, 2, 1), *guest_atoms(2 * TILE + 1, 8, (3, 2, 1), 0.8, 21), table(8, PB + 1, 0.4, 71),
                    h=0.8, charged=1))
    dims = (13, 5, 4)
    atoms = guest_atoms(9, 5, dims, 0.7, 1)
    for q, V in enumerate((1, 64, 65)):
        out.append(Case(f"V={V},masked", dims, *atoms, table(5, 3, 0.35, 10 + V), words=words_with(dims, V, 10 + V), h=0.7,
                        betas=(0.4, 1.0), charged=q % 2, map_level=(q + 1) % 3 - 1))
    for dims in ((1, 1, 1), (8, 4, 2), (13, 5, 1)):
        V = dims[0] * dims[1] * dims[2]
        out.append(Case(f"V={V}", dims, *guest_atoms(6, 3, dims, 0.7, 2 + V), table(3, 4, 0.35, 12 + V), h=0.7, map_level=0))
    d = (7, 6, 5)
    for L in (1, 8):
        out.append(Case(f"L={L}", d, *guest_atoms(12, 5, d, 0.6, 8), table(5, 4, 0.3, 92), words=words_with(d, 150, 9), h=0.6,
                        betas=np.linspace(0.0, 2.0, 8)[:L] if L > 1 else (0.4,), charged=1, map_level=L - 1))
    # tests/_rigid_cases.py's edge cases as tables: a voxel whose poses are all blocked and one with exactly one live pose
    # ("ties"), every voxel dead, two poses tied for the minimum, two voxels tied for it and a clamped weight
    for name in ("ties", "all-dead", "tied-orientations", "tied-voxels"):
        out.append(from_linear([c for c in R.cases() if c.name == name][0]))
    # a body that is no line, the same rows twice: poses 1 and 3 tie with 0 and 2, the lower pose wins
    t = table(4, 2, 0.4, 93)
    out.append(Case("tied-poses", (5, 4, 1), *guest_atoms(6, 4, (5, 4, 1), 0.9, 90), np.concatenate([t, t]), h=0.9, core2=0.01,
                    map_level=0))
    return out


@_once
def grid_case():
    """One 64 x 64 x 4 grid without a mask, M = 8, S = 3, n = 8: 256 chunks go through the reduce."""
    d = (64, 64, 4)
    return [Case("64x64x4", d, *guest_atoms(8, 3, d, 0.25, 31), table(3, 8, 0.2, 32), h=0.25, betas=(0.5, 1.0), map_level=1)]


@_once
def other_shapes():
    d = (11, 3, 9)
    return [Case("other-a", d, *guest_atoms(40, 5, d, 0.5, 40), table(5, 7, 0.3, 42), h=0.5, betas=(0.1, 0.2, 0.3), charged=1,
                 map_level=2),
            Case("other-b", (2, 2, 2), *guest_atoms(3, 1, (2, 2, 2), 1.0, 41))]


@_once
def mixed_batch():
    """64 jobs of mixed grids, masks, atom counts, sites (every instance class, charged and not), L and maps; some share
    their atoms (every second job its predecessor's), jobs of the same S share one of two tables."""
    rng = np.random.default_rng(50)
    PB = pose_block()
    tables = {}
    out, atoms = [], None
    for k in range(64):
        d = tuple(int(v) for v in rng.integers(1, 10, 3))
        if k == 7:
            d = (64, 5, 2)
        S_ = int((3, 4, 5, 7, 1, 8, 2, 6)[(k // 2) % 8])
        if k % 2 == 0:
            atoms = guest_atoms(int(rng.integers(0, 160)), S_, (8, 8, 8), 0.6, 100 + k)
        M = PB + 3 if k % 5 == 0 else 6
        if (S_, M) not in tables:
            tables[(S_, M)] = table(S_, M, 0.4, 51 + S_ + M)
        total = d[0] * d[1] * d[2]
        words = None if k % 4 == 0 else words_with(d, int(rng.integers(0, total + 1)), 200 + k)
        L = int(rng.integers(1, 9))
        out.append(Case(f"mixed-{k}", d, *atoms, tables[(S_, M)], words=words, h=0.6, cutoff2=(0.0, 9.0)[k % 2],
                        betas=rng.uniform(0.0, 1.5, L), charged=(k // 16) % 2, map_level=int(rng.integers(-1, L))))
    return out


def body_class(S_, charged):
    """pw_rigid_body.hip: body_class."""
    return {3: 0, 4: 1, 5: 2, 7: 3}.get(int(S_), 4) * 2 + (1 if charged else 0)


def pack(jobs, hole: int = 0, maps: bool = True):
    """(rec, xyz, coef, poses, words, betas, n_maps, n_levels, n_out, V): the arrays of one call; `hole` rows and entries
    nobody owns before each job's outputs; atoms, coefficients and tables that two cases share (the same array) are
    shared.  maps=False: no job writes a map."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.RIGID_BODY_JOB_DTYPE)
    xyz, coef, poses, words, betas = [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros(0, np.uint64)], []
    at_xyz, at_coef, at_poses, V = {}, {}, {}, []
    n_atoms = n_rows = n_pose_rows = n_words = n_betas = n_maps = n_levels = n_out = 0
    for k, c in enumerate(jobs):
        if c.xyz.ctypes.data not in at_xyz or at_xyz[c.xyz.ctypes.data][1] != len(c.xyz):   # (the same memory: the same atoms)
            at_xyz[c.xyz.ctypes.data] = (n_atoms, len(c.xyz))
            xyz.append(c.xyz)
            n_atoms += len(c.xyz)
        if c.coef.ctypes.data not in at_coef or at_coef[c.coef.ctypes.data][1] != c.coef.shape[:2]:
            at_coef[c.coef.ctypes.data] = (n_rows, c.coef.shape[:2])
            coef.append(c.coef.reshape(-1, 3))
            n_rows += c.coef.shape[0] * c.coef.shape[1]
        if c.poses.ctypes.data not in at_poses or at_poses[c.poses.ctypes.data][1] != c.poses.shape[:2]:
            at_poses[c.poses.ctypes.data] = (n_pose_rows, c.poses.shape[:2])
            poses.append(c.poses.reshape(-1, 3))
            n_pose_rows += c.M * c.S
        count = int(region(c).sum())
        V.append(count)
        level = c.map_level if maps else -1
        n_out += hole
        n_levels += hole
        n_maps += hole if level >= 0 else 0
        rec[k] = (at_xyz[c.xyz.ctypes.data][0], len(c.xyz), at_coef[c.coef.ctypes.data][0], -1 if c.words is None else n_words,
                  n_betas, len(c.betas), at_poses[c.poses.ctypes.data][0], c.S, c.M, n_levels, n_maps if level >= 0 else -1, n_out,
                  c.origin, c.h, c.core2, c.cutoff2, *c.dims, c.charged, level, 0)
        if c.words is not None:
            words.append(c.words)
            n_words += len(c.words)
        betas.append(c.betas)
        n_betas += len(c.betas)
        n_out += 1
        n_levels += len(c.betas)
        n_maps += 2 * count if level >= 0 else 0
    return (rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(poses), np.concatenate(words),
            np.concatenate(betas + [np.zeros(0)]), n_maps, n_levels, n_out, V)


blank = R.blank


def blank_of(packed):
    return blank(packed[8], packed[7], packed[6])


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
    """pw_rigid_body_affinity through ctypes into SENTINEL-filled arrays -- through the library's test entry when
    `workspace_bytes` is given (0: the default budget).  `sizes`: other numbers of rows and entries of (xyz, coef, poses,
    words, betas, maps, levels, out) to tell the entry, None for the true ones.  Returns (rc, (out, levels, maps))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, poses, words, betas, n_maps, n_levels, n_out, _ = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.RIGID_BODY_JOB_DTYPE)
    out, levels, mp = blank(n_out, n_levels, n_maps)
    told = [len(xyz), len(coef), len(poses), len(words), len(betas), n_maps, n_levels, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], poses.ctypes.data, told[2],
            words.ctypes.data, told[3], betas.ctypes.data, told[4], mp.ctypes.data, told[5], levels.ctypes.data, told[6],
            out.ctypes.data, told[7]]
    if workspace_bytes is None:
        rc = L.pw_rigid_body_affinity(*args)
    else:
        rc = L.pw_internal_rigid_body_affinity(*args, int(workspace_bytes), None)
    return rc, (out, levels, mp)


same = R.same
first_difference = R.first_difference


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = [c for c in cases() if c.name == "V=64,masked"][0]
    d = (9, 8, 7)
    other = Case("other", d, *guest_atoms(6, 3, d, 0.5, 60), table(3, 4, 0.4, 62), words=words_with(d, 90, 61), h=0.5,
                 betas=(0.3, 0.6), charged=1, map_level=1)
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
    comp = lambda p: 3 * (int(p[0]["pose_first"][1]) + 2 * 3 + 1) + 2  # (pose 2, site 1, z)
    n_atoms, n_rows = len(good.xyz) + len(other.xyz), good.coef.shape[0] * good.coef.shape[1] + 18
    n_pose_rows = good.M * good.S + 4 * 3
    n_words, n_betas = len(good.words) + len(other.words), len(good.betas) + len(other.betas)
    none = [None] * 8

    def told(q, v):
        return tuple(none[:q] + [v] + none[q + 1:])

    edit(field("n_sites", 0), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_sites", 9), "n_sites outside 1 .. PW_RIGID_MAX_SITES")
    edit(field("n_dirs", 0), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(field("n_dirs", 1025), "n_dirs outside 1 .. PW_RIGID_MAX_DIRS")
    edit(entry(3, comp, np.inf), "a pose component is not finite or beyond 16")
    edit(entry(3, comp, np.nan), "a pose component is not finite or beyond 16")
    edit(entry(3, comp, -16.5), "a pose component is not finite or beyond 16")
    edit(entry(3, lambda p: 3 * int(p[0]["pose_first"][1]), 16.000001), "a pose component is not finite or beyond 16")
    edit(entry(3, lambda p: 3 * (int(p[0]["pose_first"][1]) + 12) - 1, -np.inf), "a pose component is not finite or beyond 16")
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
    edit(entry(5, lambda p: int(p[0]["beta_first"][1]) + 1, -0.5), "a beta is negative or not finite")
    # every span outside its array
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", told(0, n_atoms - 1))
    edit(field("coef_first", -1), "coefficients outside coef")
    edit(lambda p: None, "coefficients outside coef", told(1, n_rows - 1))
    edit(field("pose_first", -1), "poses outside their array")
    edit(lambda p: None, "poses outside their array", told(2, n_pose_rows - 1))
    edit(field("n_dirs", 5), "poses outside their array")            # (a pose more than the table holds)
    edit(field("word_first", -2), "the words are outside their array")
    edit(lambda p: None, "the words are outside their array", told(3, n_words - 1))
    edit(field("beta_first", -1), "betas outside the array")
    edit(lambda p: None, "betas outside the array", told(4, n_betas - 1))
    edit(lambda p: None, "the maps are outside their array", told(5, 2 * (64 + 90) - 1))
    edit(field("level_first", -1), "the rows are outside levels")
    edit(lambda p: None, "the rows are outside levels", told(6, n_betas - 1))
    edit(lambda p: None, "the row is outside out", told(7, 1))
    edit(field("out", -1), "the row is outside out")
    # shared outputs
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", len(good.betas) - 1), "shares rows of levels with an earlier job")
    edit(field("map_first", 2 * 64 - 1), "shares maps with an earlier job")
    return out
