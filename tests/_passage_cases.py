"""Inputs shared by tests/test_passage.py (host path against the definition) and tests/test_gpu_passage.py (device against
the host path and the definition): the barrier between a seed voxel and the faces of its box (pw_passage).  Every
comparison is of bytes.  numpy and heapq only and seeded; nothing here is taken from pywindow_amd/csrc/pw_passage.hpp --
`reference` is the definition of include/pywindow_amd.h by ANOTHER ALGORITHM than the library's bisection of flood
fills: a bottleneck Dijkstra from the seed, in which the key of a voxel is the largest U on the best path to it, over
the held voxels that are not blocked; B is the smallest key of a face voxel; the fills are plain breadth-first searches.
The Lennard-Jones map is tests/_affinity_cases.py's (a loop over the atoms on voxel arrays)."""
import heapq
from collections import deque

import numpy as np

import _affinity_cases as A

SENTINEL = 0xA5                                                      # every byte of an output nobody owns
SEED_CLOSED, NO_EXIT = 1, 2
INF = np.inf


class Case:
    """One job: the grid (dims (nx, ny, nz), origin, spacing h), the seed voxel (i, j, l), planes (m, 4) and either a
    field [l, j, i] or atoms (n, 3) with rows (A, B), core2 and cutoff2."""

    def __init__(self, name, dims, seed, field=None, xyz=None, coef=None, planes=None, origin=(0.0, 0.0, 0.0), h=1.0,
                 core2=0.25, cutoff2=0.0):
        self.name, self.dims, self.seed = name, tuple(int(d) for d in dims), tuple(int(s) for s in seed)
        nx, ny, nz = self.dims
        self.field = None if field is None else np.ascontiguousarray(field, dtype=np.float64).reshape(nz, ny, nx)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = np.zeros((0, 2)) if coef is None else np.ascontiguousarray(coef, dtype=np.float64).reshape(-1, 2)
        self.planes = np.zeros((0, 4)) if planes is None else np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        self.origin, self.h = np.asarray(origin, dtype=np.float64), float(h)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        assert len(self.xyz) == len(self.coef) and all(0 <= s < d for s, d in zip(self.seed, self.dims))

    @property
    def rows(self):
        return max(len(self.planes), 1)


def field_of(c: Case) -> np.ndarray:
    """U of every voxel, [l, j, i]: the caller's, or the Lennard-Jones energy by the definition (+inf where blocked)."""
    if c.field is not None:
        return c.field
    nx, ny, nz = c.dims
    U, blocked = A.energies_of(A.Case(c.name, c.dims, c.xyz, c.coef, origin=c.origin, h=c.h, core2=c.core2, cutoff2=c.cutoff2))
    return np.where(blocked, INF, U).reshape(nz, ny, nx)


def held_of(c: Case, k: int) -> np.ndarray:
    """held(v) of row k, [l, j, i]: every plane but plane k."""
    nx, ny, nz = c.dims
    x = (c.origin[0] + np.arange(nx).astype(np.float64) * c.h)[None, None, :]
    y = (c.origin[1] + np.arange(ny).astype(np.float64) * c.h)[None, :, None]
    z = (c.origin[2] + np.arange(nz).astype(np.float64) * c.h)[:, None, None]
    held = np.ones((nz, ny, nx), dtype=bool)
    for q, (a, b, cc, d) in enumerate(c.planes):
        if q != k:
            held &= ((a * x + b * y) + cc * z) <= d
    return held


def _neighbours(i, j, l, nx, ny, nz):
    if i > 0: yield i - 1, j, l
    if i + 1 < nx: yield i + 1, j, l
    if j > 0: yield i, j - 1, l
    if j + 1 < ny: yield i, j + 1, l
    if l > 0: yield i, j, l - 1
    if l + 1 < nz: yield i, j, l + 1


def _component(ok, seed, dims):
    """The 6-connected component of the bool array ok [l, j, i] that holds the seed (i, j, l), as a bool array."""
    nx, ny, nz = dims
    got = np.zeros_like(ok)
    i, j, l = seed
    if not ok[l, j, i]:
        return got
    got[l, j, i] = True
    todo = deque([seed])
    okl = ok.tolist()
    while todo:
        i, j, l = todo.popleft()
        for a, b, c in _neighbours(i, j, l, nx, ny, nz):
            if okl[c][b][a] and not got[c, b, a]:
                got[c, b, a] = True
                todo.append((a, b, c))
    return got


def reference_row(c: Case, k: int, U=None):
    """Row k of the job by the definition: a PASSAGE_OUT_DTYPE record."""
    from pywindow_amd import _lib

    nx, ny, nz = c.dims
    U = field_of(c) if U is None else U
    held = held_of(c, k)
    can = held & (U != INF)
    o = np.zeros((), dtype=_lib.PASSAGE_OUT_DTYPE)
    si, sj, sl = c.seed
    o["u_seed"] = U[sl, sj, si]
    o["saddle"] = o["well_voxel"] = -1
    if not can[sl, sj, si]:
        o["barrier"] = o["well"] = INF
        o["flags"] = SEED_CLOSED
        return o
    face = np.zeros((nz, ny, nx), dtype=bool)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = (True,) * 6
    # the bottleneck Dijkstra: voxels leave the heap in the order of the largest U on the best path to them
    Ul, canl, facel = U.tolist(), can.tolist(), face.tolist()
    done = np.zeros((nz, ny, nx), dtype=bool)
    heap = [(Ul[sl][sj][si], (sl * ny + sj) * nx + si)]
    B = None
    while heap:
        cost, rank = heapq.heappop(heap)
        i, row = rank % nx, rank // nx
        j, l = row % ny, row // ny
        if done[l, j, i]:
            continue
        done[l, j, i] = True
        if facel[l][j][i]:
            B = cost
            break
        for a, b, cc in _neighbours(i, j, l, nx, ny, nz):
            if canl[cc][b][a] and not done[cc, b, a]:
                heapq.heappush(heap, (max(cost, Ul[cc][b][a]), (cc * ny + b) * nx + a))
    if B is None:
        o["flags"] = NO_EXIT
        o["barrier"] = INF
        F = _component(can, c.seed, c.dims)
        o["n_basin"] = int(F.sum())
    else:
        F = _component(can & (U <= B), c.seed, c.dims)
        o["n_basin"] = int(_component(can & (U < B), c.seed, c.dims).sum())
        l, j, i = (v[0] for v in np.nonzero(F & (U == B)))
        o["saddle"] = (i, j, l)
        o["barrier"] = U[l, j, i]
    o["n_fill"] = int(F.sum())
    ranks = np.flatnonzero(F.reshape(-1))
    values = U.reshape(-1)[ranks]
    rank = int(ranks[np.flatnonzero(values == values.min())[0]])
    o["well"] = U.reshape(-1)[rank]
    o["well_voxel"] = (rank % nx, (rank // nx) % ny, rank // (nx * ny))
    return o


def reference(c: Case):
    from pywindow_amd import _lib

    U = field_of(c)
    out = np.zeros(c.rows, dtype=_lib.PASSAGE_OUT_DTYPE)
    for k in range(c.rows):
        out[k] = reference_row(c, k, U)
    return out


_cache = {}


def reference_cached(c: Case):
    """`reference`, computed once a case object and shared; the result is read-only."""
    if id(c) not in _cache:
        got = reference(c)
        got.setflags(write=False)
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


def corridor(name, values, seed_i, doors=(), **kw):
    """A line of voxels along x through the middle of a (len, 3, 3) grid whose other voxels are blocked: the only faces
    it reaches are its two ends -- and the `doors`, voxels (i, j, l) beside the line given the value 0."""
    f = np.full((3, 3, len(values)), INF)
    f[1, 1, :] = values
    for i, j, l in doors:
        f[l, j, i] = 0.0
    return Case(name, (len(values), 3, 3), (seed_i, 1, 1), field=f, **kw)


def random_field(dims, seed, lo=-1.0, hi=1.0, blocked=0.0):
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    f = rng.uniform(lo, hi, (nz, ny, nx))
    if blocked:
        f[rng.uniform(size=f.shape) < blocked] = INF
    return f


@_once
def field_cases():
    """The caller's fields of the issue: grids, values, blocked voxels."""
    x = 2.5
    up, down = np.nextafter(x, INF), np.nextafter(x, -INF)
    out = [
        Case("1x1x1", (1, 1, 1), (0, 0, 0), field=[3.0]),
        Case("64x1x1", (64, 1, 1), (31, 0, 0), field=random_field((64, 1, 1), 1)),
        Case("1x1x64", (1, 1, 64), (0, 0, 40), field=random_field((1, 1, 64), 2)),
        Case("3x17x16", (3, 17, 16), (1, 8, 8), field=random_field((3, 17, 16), 3, blocked=0.1)),
        corridor("single-ridge", [0, 1, 5, 0, 7, 2, 3], 3),
        corridor("two-equal-ridges", [0, 5, 1, 0, 1, 5, 0], 3),
        Case("constant", (6, 5, 4), (3, 2, 2), field=np.full((4, 5, 6), 2.5)),
        corridor("one-ulp-apart", [0, up, 1, down, 0, x, 0], 4),
        corridor("one-ulp-apart-mirrored", [0, x, 0, down, 1, up, 0], 2),
        corridor("sign-change-negative-B", [-1, 2, -3, -0.5, -2], 2),
        corridor("sign-change-positive-B", [-5, 1e-3, -3, 4, -1], 2),
        corridor("zeros-minus-first", [-1, -0.0, -2, 0.0, -1], 2),
        corridor("zeros-plus-first", [-1, 0.0, -2, -0.0, -1], 2),
        corridor("zero-wells-minus-first", [1, -0.0, 0.0, 1], 2),
        corridor("zero-wells-plus-first", [1, 0.0, -0.0, 1], 2),
        corridor("denormals", [-1, 1e-310, -1, 5e-324, -5e-324, -1], 2),
        corridor("1e300", [-1e300, 1e300, -1e300, 1e299, 0], 2),
        corridor("B-is-the-seed", [0, 1, 5, 2, 0], 2),
        corridor("B-is-the-largest", [7, 1, 7], 1),
        corridor("nearer-exit-higher", [6, 0, 1, 1, 1, 1, 2], 1),
        corridor("well-ties", [3, -4, 0, -4, 3], 2),
        corridor("seed-blocked", [0, 1, INF, 1, 0], 2),
    ]
    for nx in (5, 63, 64):
        out.append(Case(f"nx={nx}", (nx, 4, 3), (nx // 2, 2, 1), field=random_field((nx, 4, 3), 10 + nx, blocked=0.05)))
    shell = random_field((7, 7, 7), 4)
    shell[1:6, 1:6, 1:6] = INF
    shell[2:5, 2:5, 2:5] = random_field((3, 3, 3), 5)
    out.append(Case("closed-shell", (7, 7, 7), (3, 3, 3), field=shell))
    return out


def shell_atoms():
    """98 atoms on the voxel centres of the shell around the 3x3x3 interior of a 7x7x7 grid of spacing 1."""
    at = [(i, j, l) for l in range(1, 6) for j in range(1, 6) for i in range(1, 6) if not (2 <= i <= 4 and 2 <= j <= 4 and 2 <= l <= 4)]
    assert len(at) == 98
    rng = np.random.default_rng(6)
    sigma, eps = rng.uniform(0.8, 1.2, 98), rng.uniform(0.1, 1.0, 98)
    return np.array(at, dtype=np.float64), np.stack([4.0 * eps * sigma ** 12, 4.0 * eps * sigma ** 6], axis=1)


@_once
def plane_cases():
    far = [[0.0, 1.0, 0.0, 100.0], [0.0, 0.0, 1.0, 100.0]]
    left, right = [-1.0, 0.0, 0.0, -1.0], [1.0, 0.0, 0.0, 7.0]        # x >= 1 and x <= 7: the two ends of a line of 9
    line = [1, 2, 0, 0, 0, 5, 0, 3, 0.5]
    rng = np.random.default_rng(7)
    many = np.concatenate([rng.normal(size=(65, 3)), np.full((65, 1), 50.0)], axis=1)
    many[0], many[63], many[64] = [1, 0, 0, 4], [0, 1, 0, 3], [0, 0, 1, 2]
    d = (6, 5, 4)
    return [
        Case("m=0", d, (2, 2, 1), field=random_field(d, 20)),
        Case("m=1", d, (2, 2, 1), field=random_field(d, 20), planes=[[1, 0, 0, 3]]),
        # the plane `left` cuts off the low exit: the row that leaves it out and the rows that hold it differ; rows 2
        # and 3 hold both and have no exit
        corridor("m=4-low-exit-cut", line, 3, planes=[left, right] + far),
        Case("m=65", d, (2, 2, 1), field=random_field(d, 21), planes=many),
        # the seed is outside plane 0: row 0 leaves it out, row 1 holds it
        Case("seed-outside-a-plane", d, (4, 2, 1), field=random_field(d, 22), planes=[[1, 0, 0, 3], [0, 1, 0, 3]]),
        # voxel 7 of the line lies exactly on the plane x <= 7 and is held: the door beside it is the only exit of row 0
        corridor("voxel-on-a-plane", [INF, 1, 0, 0, 2, 0, 4, 3, 6], 3, doors=[(7, 0, 1)], planes=[far[0], right]),
        Case("planes-off-axis", (9, 8, 7), (4, 4, 3), field=random_field((9, 8, 7), 23), origin=(-1.0, -0.875, -0.75), h=0.25,
             planes=[[1, 1, 0, 0.5], [-1, 0.5, 0.25, 0.75], [0, -1, 1, 0.625]]),
    ]


@_once
def lj_cases():
    d = (9, 7, 5)
    out = []
    for n in (0, 1, 127, 128, 129, 257):
        xyz, coef = A.shell_atoms(n, d, 0.8, 30 + n)
        xyz[np.abs(xyz - 0.8 * np.array([4.0, 3.0, 2.0])).max(axis=1) <= 1.0] += 3.0   # (room round the seed)
        out.append(Case(f"n={n}", d, (4, 3, 2), xyz=xyz, coef=coef, h=0.8, cutoff2=16.0 if n % 2 else 0.0,
                        planes=[[1, 0, 0, 5.0], [0, 1, 0, 4.0]] if n in (128, 257) else None))
    # voxels exactly at r2 == core2 (blocked), one exactly at r2 == cutoff2 (counts: it is the seed, so its U is u_seed
    # and the barrier) and the next one out (does not)
    out.append(Case("ties", (8, 1, 1), (5, 0, 0), xyz=[[2.0, 0.0, 0.0]], coef=[[3.0, 2.0]], core2=1.0, cutoff2=9.0))
    xyz, coef = A.shell_atoms(20, d, 0.8, 40)
    out.append(Case("A=B=0", d, (4, 3, 2), xyz=xyz, coef=np.zeros_like(coef), h=0.8))
    out.append(Case("shell-of-98-atoms", (7, 7, 7), (3, 3, 3), xyz=shell_atoms()[0], coef=shell_atoms()[1], core2=0.25))
    return out


@_once
def big_cases():
    """One 64 x 64 x 64 grid: a bowl with noise, a tenth of it blocked."""
    g = np.arange(64) - 31.5
    r2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    f = np.cos(np.sqrt(r2) * 0.4) * 3.0 + random_field((64, 64, 64), 50)
    f[random_field((64, 64, 64), 51, 0.0, 1.0) < 0.1] = INF
    f[31, 31, 31] = 0.0
    return [Case("64^3", (64, 64, 64), (31, 31, 31), field=f, planes=[[1, 0, 0, 40.0], [0, 1, 0, 45.0]])]


def cases():
    return field_cases() + plane_cases() + lj_cases()


@_once
def other_shapes():
    return [Case("other-a", (11, 3, 9), (5, 1, 4), field=random_field((11, 3, 9), 60), planes=[[1, 0, 0, 8.0]]),
            Case("other-b", (2, 2, 2), (0, 1, 1), xyz=[[5.0, 5.0, 5.0]], coef=[[1.0, 1.0]])]


@_once
def mixed_batch():
    """64 jobs of mixed grids, fields and atoms, plane counts; some share their atoms and their planes."""
    rng = np.random.default_rng(70)
    out, atoms, planes = [], None, None
    for k in range(64):
        d = tuple(int(v) for v in rng.integers(1, 13, 3))
        if k == 7:
            d = (64, 5, 3)
        seed = tuple(int(v) // 2 for v in d)
        if k % 4 == 0:                                               # (jobs k and k + 2 share their atoms)
            atoms = A.shell_atoms(int(rng.integers(0, 200)), (8, 8, 8), 0.6, 100 + k)
        if planes is None or k % 4:
            m = int(rng.integers(0, 6))
            planes = np.concatenate([rng.normal(size=(m, 3)), rng.uniform(1.0, 6.0, (m, 1))], axis=1)
        if k % 2:
            out.append(Case(f"mixed-{k}", d, seed, field=random_field(d, 200 + k, blocked=0.1), planes=planes, h=0.6))
        else:
            out.append(Case(f"mixed-{k}", d, seed, xyz=atoms[0], coef=atoms[1], planes=planes, h=0.6, cutoff2=(0.0, 9.0)[k % 4 == 0]))
    return out


def pack(jobs, hole: int = 0, fields=None):
    """(rec, xyz, coef, planes, field, n_out): the arrays of one call; `hole` rows nobody owns before each job's rows;
    atoms and planes that two cases share (the same arrays) are shared.  `fields`: ready maps (flat, or None) to hand
    the jobs in place of their atoms."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.PASSAGE_JOB_DTYPE)
    xyz, coef, planes, field = [np.zeros((0, 3))], [np.zeros((0, 2))], [np.zeros((0, 4))], [np.zeros(0)]
    where, where_p = {}, {}
    n_atoms = n_planes = n_field = n_out = 0
    for k, c in enumerate(jobs):
        key = (c.xyz.ctypes.data, c.coef.ctypes.data, len(c.xyz))     # (the same memory: the same atoms)
        if key not in where:
            where[key] = n_atoms
            xyz.append(c.xyz)
            coef.append(c.coef)
            n_atoms += len(c.xyz)
        key_p = (c.planes.ctypes.data, len(c.planes))
        if key_p not in where_p:
            where_p[key_p] = n_planes
            planes.append(c.planes)
            n_planes += len(c.planes)
        f = c.field if fields is None or fields[k] is None else fields[k]
        n_out += hole
        a = where[key]
        rec[k] = (a, len(c.xyz), a, where_p[key_p], len(c.planes), -1 if f is None else n_field, n_out, c.origin, c.h,
                  c.core2, c.cutoff2, *c.dims, c.seed)
        if f is not None:
            field.append(np.asarray(f, dtype=np.float64).reshape(-1))
            n_field += field[-1].size
        n_out += c.rows
    return rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(planes), np.concatenate(field), n_out


def blank(n_out):
    """out with every byte SENTINEL."""
    from pywindow_amd import _lib

    return np.frombuffer(bytes([SENTINEL]) * (_lib.PASSAGE_OUT_DTYPE.itemsize * n_out), dtype=_lib.PASSAGE_OUT_DTYPE).copy()


def expected(jobs, hole: int = 0):
    """out in the layout of `pack`, SENTINEL bytes where nobody writes."""
    packed = pack(jobs, hole)
    out = blank(packed[5])
    for k, c in enumerate(jobs):
        first = int(packed[0]["out_first"][k])
        out[first:first + c.rows] = reference_cached(c)
    return out


def raw(ctx, packed, workspace_bytes=None, sizes=None, grids=0):
    """pw_passage through ctypes into a SENTINEL-filled array -- through the library's test entry when `workspace_bytes`
    is given (0: the default budget).  `sizes`: other numbers of rows and entries of (xyz, coef, planes, field, out) to
    tell the entry, None for the true ones.  `grids`: 3 for the kernel without its fourth bit grid (the test entry only).
    Returns (rc, out)."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, planes, field, n_out = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.PASSAGE_JOB_DTYPE)
    out = blank(n_out)
    told = [len(xyz), len(coef), len(planes), len(field), n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], planes.ctypes.data,
            told[2], field.ctypes.data, told[3], out.ctypes.data, told[4]]
    if workspace_bytes is None:
        rc = L.pw_passage(*args)
    else:
        rc = L.pw_internal_passage(*args, int(workspace_bytes), None, None, int(grids))
    return rc, out


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def first_difference(got, want):
    """For an assertion's message: the first row that differs and the two records."""
    for k in range(len(want)):
        if got[k].tobytes() != want[k].tobytes():
            return k, got[k], want[k]
    return None


def affinity_map(ctx, c: Case) -> np.ndarray:
    """The energy of every voxel of the case's box as pw_affinity returns it on the context (word_first = -1)."""
    from pywindow_amd import _lib

    nx, ny, nz = c.dims
    job = np.zeros(1, dtype=_lib.AFFINITY_JOB_DTYPE)
    job[0] = (0, len(c.xyz), 0, -1, 0, 1, 0, 0, 0, 0, 0, 0, c.origin, c.h, c.core2, c.cutoff2, nx, ny, nz, 0)
    return ctx.affinity(job, c.xyz, c.coef, [0.0], energies=np.zeros(nx * ny * nz))[3]


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = plane_cases()[1]
    xyz, coef = A.shell_atoms(6, (9, 8, 7), 0.5, 60)
    other_lj = Case("other", (9, 8, 7), (4, 4, 3), xyz=xyz, coef=coef, planes=[[1, 0, 0, 3.0], [0, 1, 0, 3.0]], h=0.5)
    other_field = Case("other", (5, 4, 3), (2, 2, 1), field=random_field((5, 4, 3), 61), planes=[[1, 0, 0, 3.0], [0, 1, 0, 3.0]])
    out = []

    def edit(other, fn, reason, sizes=None):
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

    none = [None] * 5

    def told(q, v):
        return tuple(none[:q] + [v] + none[q + 1:])

    atom = lambda p: 3 * (int(p[0]["atom_first"][1]) + 2) + 1
    row = lambda p: 2 * (int(p[0]["coef_first"][1]) + 2)
    plane = lambda p: 4 * (int(p[0]["plane_first"][1]) + 1) + 2
    value = lambda p: int(p[0]["field_first"][1]) + 17
    lj, fd = other_lj, other_field
    edit(lj, entry(1, atom, np.nan), "a coordinate is not finite")
    edit(lj, entry(1, atom, -INF), "a coordinate is not finite")
    edit(lj, entry(2, row, np.nan), "a coefficient is not finite")
    edit(lj, entry(2, row, -1.0), "a coefficient outside 0 .. 1e100")
    edit(lj, entry(2, lambda p: row(p) + 1, 2e100), "a coefficient outside 0 .. 1e100")
    edit(lj, field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(lj, field("core2", np.nan), "core2 below 1e-6 or not finite")
    edit(lj, field("cutoff2", 0.25), "cutoff2 is neither 0 nor above core2")
    edit(lj, field("cutoff2", INF), "cutoff2 is neither 0 nor above core2")
    edit(lj, field("atom_first", -1), "atoms outside xyz")
    edit(lj, lambda p: None, "atoms outside xyz", told(0, 5))
    edit(lj, lambda p: None, "coefficients outside coef", told(1, 5))
    for other in (lj, fd):
        edit(other, entry(3, plane, np.nan), "a plane is not finite")
        edit(other, entry(3, plane, INF), "a plane is not finite")
        edit(other, field("origin", [0.0, np.nan, 0.0]), "the origin or the spacing is not finite")
        edit(other, field("spacing", INF), "the origin or the spacing is not finite")
        edit(other, field("spacing", 0.0), "spacing <= 0")
        for name in ("nx", "ny", "nz"):
            edit(other, field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
            edit(other, field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(other, field("seed", [-1, 0, 0]), "the seed is outside the grid")
        edit(other, field("seed", [0, 0, other.dims[2]]), "the seed is outside the grid")
        edit(other, field("n", -1), "a negative count")
        edit(other, field("m", -1), "a negative count")
        edit(other, lambda p: None, "planes outside the array", told(2, 2))
        edit(other, field("plane_first", -1), "planes outside the array")
        edit(other, field("field_first", -2), "the field is outside its array")
        edit(other, lambda p: None, "the rows are outside out", told(4, 2))
        edit(other, field("out_first", -1), "the rows are outside out")
        edit(other, field("out_first", 0), "shares rows of out with an earlier job")
    edit(fd, entry(4, value, np.nan), "a field value is -inf or not a number")
    edit(fd, entry(4, value, -INF), "a field value is -inf or not a number")
    edit(fd, lambda p: None, "the field is outside its array", told(3, 6 * 5 * 4 + 5 * 4 * 3 - 1))
    edit(fd, field("field_first", 6 * 5 * 4 + 1), "the field is outside its array")
    return out
