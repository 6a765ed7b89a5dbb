"""Inputs shared by tests/test_cavity.py (host path against the definition) and tests/test_gpu_cavity.py (device against
the host path and against the definition): the cavity of a cage as a voxel flood fill (pw_cavity).  Every output is an
integer: every comparison is of bytes.  numpy only and seeded; nothing here is taken from
pywindow_amd/csrc/pw_cavity.hpp -- `reference` is the definition of include/pywindow_amd.h written directly: free and
open by its expressions on broadcast arrays, the fill as repeated 6-neighbour dilation of a bool array until it stops
changing."""
import ctypes
import functools

import numpy as np

SENTINEL = 0xA5                                                      # every byte of an output nobody owns


class Case:
    """One job: atoms (n, 3) with radii (n,), a probe, the grid (origin, spacing h, dims (nx, ny, nz)), planes (m, 4),
    the seed voxel and, optionally, ready-made open words (ny * nz uint64, word l * ny + j) in place of the atoms."""

    def __init__(self, name, dims, seed, xyz=None, radii=None, probe=0.0, origin=(0.0, 0.0, 0.0), h=1.0, planes=None,
                 words=None):
        self.name, self.dims, self.seed = name, tuple(int(d) for d in dims), tuple(int(s) for s in seed)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.radii = np.zeros(0) if radii is None else np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
        self.probe, self.h = float(probe), float(h)
        self.origin = np.asarray(origin, dtype=np.float64)
        self.planes = np.zeros((0, 4)) if planes is None else np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        assert len(self.xyz) == len(self.radii)
        assert self.words is None or len(self.words) == self.dims[1] * self.dims[2]


def open_voxels(c: Case) -> np.ndarray:
    """The open voxels of a case as a bool array [l, j, i]: by the definition, or from the bits < nx of its words."""
    nx, ny, nz = c.dims
    if c.words is not None:
        bits = (c.words.reshape(nz, ny, 1) >> np.arange(nx, dtype=np.uint64)) & np.uint64(1)
        return bits.astype(bool)
    x = (c.origin[0] + np.arange(nx).astype(np.float64) * c.h)[None, None, :]
    y = (c.origin[1] + np.arange(ny).astype(np.float64) * c.h)[None, :, None]
    z = (c.origin[2] + np.arange(nz).astype(np.float64) * c.h)[:, None, None]
    ok = np.ones((nz, ny, nx), dtype=bool)
    for (X, Y, Z), radius in zip(c.xyz, c.radii):
        dx, dy, dz = x - X, y - Y, z - Z
        ok &= (dx * dx + dy * dy) + dz * dz >= (radius + c.probe) * (radius + c.probe)
    for a, b, cc, d in c.planes:
        ok &= ((a * x + b * y) + cc * z) <= d
    return ok


def grow(fill: np.ndarray) -> np.ndarray:
    """A bool array with its six neighbours."""
    out = fill.copy()
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        out[tuple(hi)] |= fill[tuple(lo)]
        out[tuple(lo)] |= fill[tuple(hi)]
    return out


def component(ok: np.ndarray, seed) -> np.ndarray:
    """The 6-connected component of `ok` [l, j, i] that holds the voxel seed = (i, j, l); empty if that voxel is not set."""
    fill = np.zeros_like(ok)
    i, j, l = seed
    fill[l, j, i] = ok[l, j, i]
    while True:
        new = grow(fill) & ok
        if (new == fill).all():
            return fill
        fill = new


def reference(c: Case):
    """(a CAVITY_OUT_DTYPE record, the ny * nz mask words) of the definition."""
    from pywindow_amd import _lib

    nx, ny, nz = c.dims
    ok = open_voxels(c)
    cav = component(ok, c.seed)
    out = np.zeros((), dtype=_lib.CAVITY_OUT_DTYPE)
    l, j, i = (v.astype(np.int64) for v in np.nonzero(cav))
    out["n_voxels"], out["n_open"] = len(i), int(ok.sum())
    padded = np.zeros((nz + 2, ny + 2, nx + 2), dtype=bool)
    padded[1:-1, 1:-1, 1:-1] = cav
    inner = cav.copy()
    for dl, dj, di in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
        inner &= padded[1 + dl:nz + 1 + dl, 1 + dj:ny + 1 + dj, 1 + di:nx + 1 + di]
    out["n_surface"] = int((cav & ~inner).sum())
    out["n_face"] = int(((i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1) | (l == 0) | (l == nz - 1)).sum())
    out["first"] = [i.sum(), j.sum(), l.sum()]
    out["second"] = [(i * i).sum(), (j * j).sum(), (l * l).sum(), (i * j).sum(), (i * l).sum(), (j * l).sum()]
    out["box"] = [i.min(), i.max(), j.min(), j.max(), l.min(), l.max()] if len(i) else [-1] * 6
    out["flags"] = 0 if ok[c.seed[2], c.seed[1], c.seed[0]] else _lib.CAV_SEED_CLOSED
    words = (cav.astype(np.uint64) << np.arange(nx, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)
    return out, words


_cache = {}


def reference_cached(c: Case):
    """`reference`, computed once a case object and shared; the results are read-only."""
    if id(c) not in _cache:
        out, words = reference(c)
        words.setflags(write=False)
        _cache[id(c)] = (c, (out, words))                            # (the case is kept: its id stays its own)
    return _cache[id(c)][1]


def pack_words(ok: np.ndarray) -> np.ndarray:
    """The words of a bool array [l, j, i]."""
    nx = ok.shape[2]
    return (ok.astype(np.uint64) << np.arange(nx, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)


def random_atoms(n: int, dims, seed: int, h: float = 0.5, radius=(0.6, 1.4), hollow: float = 0.0):
    """n atoms scattered over the box of a grid at the origin, none within `hollow` of the box's middle."""
    rng = np.random.default_rng(seed)
    size = h * (np.asarray(dims, dtype=np.float64) - 1.0)
    xyz = rng.uniform(-0.1, 1.1, (4 * n + 8, 3)) * size
    xyz = xyz[np.linalg.norm(xyz - 0.5 * size, axis=1) >= hollow][:n]
    assert len(xyz) == n
    return xyz, rng.uniform(*radius, n)


def serpentine(nx: int, ny: int, nz: int):
    """(open [l, j, i], path length, voxels of the second component): a path one voxel wide that runs the length of the
    rows of even j in the planes of even l, reversing at alternate ends through one voxel of the rows between them and,
    at the end of a plane, through one voxel of the plane between two planes; j runs upwards in one plane and downwards
    in the next.  (Rows side by side are neighbours along their whole length, so every other row is the most a path one
    voxel wide can take.)  A second component of three voxels lies in a row the path only touches at its ends."""
    ok = np.zeros((nz, ny, nx), dtype=bool)
    end, length = 0, 0                                               # the path enters a run at x = end
    js = list(range(0, ny, 2))
    for l in range(0, nz, 2):
        for q, j in enumerate(js):
            ok[l, j, :] = True
            length += nx
            end = nx - 1 - end
            if q + 1 < len(js):
                ok[l, (j + js[q + 1]) // 2, end] = True
                length += 1
        if l + 2 < nz:
            ok[l + 1, js[-1], end] = True
            length += 1
        js.reverse()
    second = 0
    if nx >= 8 and ny >= 2 and nz >= 2:
        ok[1, 1, 3:6] = True
        second = 3
    return ok, length, second


def lattice_job(name, dims, n_atoms, seed, h=0.5, probe=0.0, planes=None):
    """Random atoms around a hollow middle in which the seed voxel lies."""
    xyz, radii = random_atoms(n_atoms, dims, seed, h, hollow=2.5 + probe)
    return Case(name, dims, tuple((d - 1) // 2 for d in dims), xyz, radii, probe, h=h, planes=planes)


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernel and the host path can go wrong."""
    out = []
    # a tie: voxels at integer coordinates, an atom of radius 5 at the origin -- (3, 4, 0) at distance exactly 5 is
    # free, (3, 3, 0) is not; then the plane x <= 3 exactly through voxel centres, which keeps them
    ball = dict(xyz=[[0.0, 0.0, 0.0]], radii=[5.0], origin=(-6.0, -6.0, -6.0), h=1.0)
    out.append(Case("tie", (13, 13, 13), (0, 0, 0), **ball))
    out.append(Case("tie-plane-through-centres", (13, 13, 13), (0, 0, 0), planes=[[1.0, 0.0, 0.0, 3.0]], **ball))
    out.append(Case("tie-probe", (13, 13, 13), (0, 0, 0), xyz=[[0.0, 0.0, 0.0]], radii=[3.75], probe=1.25,
                    origin=(-6.0, -6.0, -6.0)))
    out.append(Case("seed-closed", (13, 13, 13), (6, 6, 6), **ball))
    out.append(Case("seed-behind-a-plane", (13, 13, 13), (12, 0, 0), planes=[[1.0, 0.0, 0.0, 3.0]], **ball))
    # degenerate grids, without atoms (the whole grid is the cavity, n_face its shell) and cut in two by one
    for dims in ((1, 1, 1), (64, 1, 1), (1, 64, 1), (1, 1, 64), (2, 2, 2), (3, 3, 3), (64, 64, 1)):
        out.append(Case(f"no-atoms-{dims}", dims, (0, 0, 0)))
        middle = 0.5 * (np.asarray(dims, dtype=np.float64) - 1.0)
        out.append(Case(f"cut-in-two-{dims}", dims, (0, 0, 0), xyz=[middle + 0.25], radii=[0.8]))
    # word edges, as open words: a cavity in bit 0 alone and in bit 63 alone, a second component two bits away; nx = 63
    # and nx = 64 (and 5) with the bits beyond nx set in the words, which must be ignored
    for nx, bit in ((64, 0), (64, 63), (63, 0), (63, 62), (5, 4)):
        ok = np.zeros((3, 4, nx), dtype=bool)
        ok[:, :, bit] = True
        ok[1, 1:3, bit - 2 if bit >= 2 else bit + 2] = True
        words = pack_words(ok)
        if nx < 64:
            words = words | (np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nx))
        out.append(Case(f"word-edge-nx={nx}-bit={bit}", (nx, 4, 3), (bit, 0, 0), words=words))
    # a serpentine: the largest number of sweeps, row and plane neighbours crossed in both directions
    for dims in ((8, 8, 8), (64, 5, 3)):
        ok, length, second = serpentine(*dims)
        c = Case(f"serpentine-{dims}", dims, (0, 0, 0), words=pack_words(ok))
        got = reference_cached(c)[0]
        assert second == 3 and got["n_voxels"] == length and got["n_open"] == length + second, (dims, got, length)
        out.append(c)
        back = Case(f"serpentine-from-its-last-voxel-{dims}", dims, tuple(int(v[-1]) for v in np.nonzero(ok)[::-1]),
                    words=pack_words(ok))
        out.append(back)
    # rows: fewer than waves, around the wave, one past a multiple of the workgroup (257 is a prime above 64, so
    # ny * nz = 257 does not exist: 258 = 6 x 43 and 259 = 7 x 37 are the nearest, 513 = 19 x 27 is one past two blocks)
    for ny, nz in ((1, 1), (63, 1), (7, 9), (64, 1), (8, 8), (5, 13), (6, 43), (7, 37), (19, 27)):
        out.append(lattice_job(f"rows={ny}x{nz}", (37, ny, nz), 30, 1000 + 64 * ny + nz))
    out.append(lattice_job("planes-3", (23, 21, 19), 40, 5, planes=[[1.0, 0.2, 0.0, 9.0], [-1.0, 0.0, 0.3, -1.5], [0.0, 0.0, 1.0, 7.25]]))
    out.append(lattice_job("probe", (33, 31, 29), 60, 6, probe=0.7))
    return out


@functools.lru_cache(maxsize=None)
def big_cases():
    """More atoms than any staging could hold, many planes, and the largest grid."""
    rng = np.random.default_rng(77)
    normals = rng.normal(size=(200, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    middle = 0.5 * 0.5 * 15.0
    planes = np.concatenate([normals, (normals * middle).sum(axis=1)[:, None] + rng.uniform(1.0, 4.0, (200, 1))], axis=1)
    xyz, radii = random_atoms(5000, (16, 16, 16), 8, radius=(0.05, 0.3), hollow=1.0)
    return [Case("atoms-5000", (16, 16, 16), (7, 7, 7), xyz, radii),
            Case("planes-200", (16, 16, 16), (7, 7, 7), planes=planes, h=0.5),
            lattice_job("grid-64", (64, 64, 64), 300, 9),
            Case("grid-64-no-atoms", (64, 64, 64), (31, 31, 31))]


def mixed_batch():
    """64 jobs of mixed grid sizes, the largest grid among them."""
    small = [c for c in cases() if c.dims[1] * c.dims[2] <= 64]
    jobs = [big_cases()[2]]
    while len(jobs) < 64:
        jobs.append(small[(7 * len(jobs)) % len(small)] if len(jobs) % 5 else cases()[len(jobs) % len(cases())])
    return jobs


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    return [lattice_job("before-a", (50, 3, 40), 25, 31), lattice_job("before-b", (9, 33, 2), 10, 32)]


def pack(jobs, hole: int = 0, mask: bool = True):
    """The arguments of a call for a list of cases: (CAVITY_JOB_DTYPE array, xyz, radii, planes, rows of out, words of
    mask, open_words, open_first).  A job's row of the result and its mask words come one job after the other, `hole`
    entries that nobody owns in front of each; atoms and planes that several jobs hold (the same case object) are
    stored once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.CAVITY_JOB_DTYPE)
    open_first = np.full(len(jobs), -1, dtype=np.int64)
    xyz, radii, planes, words, where = [np.zeros((0, 3))], [np.zeros(0)], [np.zeros((0, 4))], [np.zeros(0, dtype=np.uint64)], {}
    atoms = cuts = row = at = n_words = 0
    for k, c in enumerate(jobs):
        if id(c) not in where:
            where[id(c)] = (atoms, cuts)
            xyz.append(c.xyz)
            radii.append(c.radii)
            planes.append(c.planes)
            atoms += len(c.xyz)
            cuts += len(c.planes)
        a, p = where[id(c)]
        row += hole
        at += hole if mask else 0
        rows = c.dims[1] * c.dims[2]
        rec[k] = (a, len(c.xyz), a, p, len(c.planes), at if mask else -1, row, c.origin, c.h, c.probe, *c.dims, c.seed)
        if c.words is not None:
            open_first[k] = n_words
            words.append(c.words)
            n_words += rows
        row += 1
        at += rows if mask else 0
    return (rec, np.concatenate(xyz), np.concatenate(radii), np.concatenate(planes), row, at, np.concatenate(words),
            open_first)


def blank(n_out: int, n_mask: int):
    """(out, mask) with every byte SENTINEL."""
    from pywindow_amd import _lib

    out = np.frombuffer(bytes([SENTINEL]) * (_lib.CAVITY_OUT_DTYPE.itemsize * n_out), dtype=_lib.CAVITY_OUT_DTYPE).copy()
    return out, np.frombuffer(bytes([SENTINEL]) * (8 * n_mask), dtype=np.uint64).copy()


def expected(jobs, hole: int = 0, mask: bool = True):
    """(out, mask) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    rec, *_, n_out, n_mask, _, _ = pack(jobs, hole, mask)
    out, words = blank(n_out, n_mask)
    for k, c in enumerate(jobs):
        o, w = reference_cached(c)
        out[int(rec["out"][k])] = o
        if mask:
            words[int(rec["mask_first"][k]):int(rec["mask_first"][k]) + len(w)] = w
    return out, words


def raw(ctx, packed, workspace_bytes=None, timed=False, sizes=None):
    """pw_cavity through ctypes into SENTINEL-filled arrays -- through the library's test entry when the jobs carry
    ready-made open words or `workspace_bytes` is given (0: the default budget).  `sizes`: other numbers of rows and
    entries of (xyz, radii, planes, out, mask) to tell the entry, None for the true ones.  Returns
    (rc, (out, mask)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, radii, planes, n_out, n_mask, words, open_first = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.CAVITY_JOB_DTYPE)
    out, mask = blank(n_out, n_mask)
    told = [len(xyz), len(radii), len(planes), n_out, n_mask]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], radii.ctypes.data, told[1], planes.ctypes.data,
            told[2], out.ctypes.data, told[3], mask.ctypes.data, told[4]]
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None and not (open_first >= 0).any() and not timed:
        rc = L.pw_cavity(*args)
    else:
        rc = L.pw_internal_cavity(*args, words.ctypes.data, open_first.ctypes.data, len(words), int(workspace_bytes or 0),
                                  ctypes.byref(ms) if timed else None)
    return (rc, (out, mask), ms.value) if timed else (rc, (out, mask))


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: the first row of out that differs."""
    for k in range(len(want[0])):
        if got[0][k].tobytes() != want[0][k].tobytes():
            return k, got[0][k], want[0][k]
    return "mask", int(np.flatnonzero(got[1] != want[1])[0]) if len(want[1]) else None


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = cases()[0]
    other = lattice_job("other", (9, 8, 7), 6, 41)
    out = []

    def edit(fn, reason, second=other, sizes=None):
        packed = list(pack([good, second]))
        fn(packed)
        out.append((tuple(packed), sizes, reason))

    def atom(values):
        def fn(p):
            p[1] = p[1].copy()
            p[1][int(p[0]["atom_first"][1]) + 2] = values
        return fn

    def field(name, value):
        def fn(p):
            p[0][name][1] = value
        return fn

    def entry(index, at, value):
        def fn(p):
            p[index] = p[index].copy()
            p[index].reshape(-1)[at(p)] = value
        return fn

    edit(atom([0.0, np.nan, 0.0]), "a coordinate is not finite")
    edit(atom([np.inf, 0.0, 0.0]), "a coordinate is not finite")
    edit(entry(2, lambda p: int(p[0]["radius_first"][1]) + 1, np.nan), "a radius is not finite")
    edit(entry(2, lambda p: int(p[0]["radius_first"][1]) + 1, -0.5), "a negative radius")
    with_planes = lattice_job("with-planes", (9, 8, 7), 6, 42, planes=[[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0]])
    edit(entry(3, lambda p: 4 * int(p[0]["plane_first"][1]) + 5, np.inf), "a plane is not finite", second=with_planes)
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin, the spacing or the probe is not finite")
    edit(field("probe", np.inf), "the origin, the spacing or the probe is not finite")
    edit(field("spacing", 0.0), "spacing <= 0")
    edit(field("spacing", -0.5), "spacing <= 0")
    edit(field("probe", -1.0), "a negative probe")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("seed", [9, 0, 0]), "the seed is outside the grid")
    edit(field("seed", [0, -1, 0]), "the seed is outside the grid")
    edit(field("seed", [0, 0, 7]), "the seed is outside the grid")
    edit(field("n", -1), "a negative count")
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", sizes=(len(good.xyz) + len(other.xyz) - 1, None, None, None, None))
    edit(lambda p: None, "radii outside the array", sizes=(None, len(good.xyz) + len(other.xyz) - 1, None, None, None))
    edit(lambda p: None, "planes outside the array", second=with_planes, sizes=(None, None, 1, None, None))
    edit(lambda p: None, "the row is outside out", sizes=(None, None, None, 1, None))
    edit(field("out", -1), "the row is outside out")
    edit(lambda p: None, "the words are outside mask", sizes=(None, None, None, None, 13 * 13 + 8 * 7 - 1))
    edit(field("mask_first", -2), "the words are outside mask")
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("mask_first", 13 * 13 - 1), "shares words of mask with an earlier job")
    edit(field("mask_first", 0), "shares words of mask with an earlier job")
    return out
