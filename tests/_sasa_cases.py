"""Inputs shared by tests/test_sasa.py (host path against the definition) and tests/test_gpu_sasa.py (device against the
host path and against the definition): the accessible surface of a cage by test points, split by a cavity's bit mask
(pw_sasa).  Every output is an integer: every comparison is of bytes.  numpy only and seeded; nothing here is taken from
pywindow_amd/csrc/pw_sasa.hpp -- `reference` is the definition of include/pywindow_amd.h written directly: the test
points and the exposure test by its expressions on arrays, over ALL other atoms (nothing is culled), the cell of a point
as the largest i whose voxel coordinate is <= the point's, found by comparing with every coordinate."""
import ctypes
import functools

import numpy as np

SENTINEL = 0xA5                                                      # every byte of an output nobody owns

AXES = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])


@functools.lru_cache(maxsize=None)
def spiral(P: int) -> np.ndarray:
    """The default directions (pywindow_amd.sphere_directions); one array a P, so that cases can share a call."""
    import pywindow_amd as pw

    u = pw.sphere_directions(P)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def random_directions(P: int, seed: int) -> np.ndarray:
    v = np.random.default_rng(seed).normal(size=(P, 3))
    v /= np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))[:, None]
    assert (np.abs(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) - 1.0) <= 1e-12).all()
    v.setflags(write=False)
    return v


class Case:
    """One job: atoms (n, 3) with radii (n,), a probe, the call's directions (P, 3) and, optionally, a grid: dims
    (nx, ny, nz), origin, spacing h and ny * nz uint64 words (word l * ny + j, bit i)."""

    def __init__(self, name, xyz, radii, directions, probe=0.0, dims=None, origin=(0.0, 0.0, 0.0), h=1.0, words=None):
        self.name = name
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.radii = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
        self.directions = directions
        self.probe, self.h = float(probe), float(h)
        self.dims = None if dims is None else tuple(int(d) for d in dims)
        self.origin = np.asarray(origin, dtype=np.float64)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        assert len(self.xyz) == len(self.radii) and directions.ndim == 2 and directions.shape[1] == 3
        assert (self.dims is None) == (self.words is None)
        assert self.words is None or len(self.words) == self.dims[1] * self.dims[2]


def cell(o: float, h: float, n: int, p: np.ndarray) -> np.ndarray:
    """The largest i in [0, n) with o + i * h <= p, -1 if there is none, for an array of p: every coordinate is compared."""
    coords = o + np.arange(n).astype(np.float64) * h
    below = coords[None, :] <= p[:, None]
    return np.where(below.any(axis=1), n - 1 - np.argmax(below[:, ::-1], axis=1), -1)


def reference(c: Case):
    """(a SASA_OUT_DTYPE record, exposed (n,) int32, inside (n,) int32) of the definition, without culling.  The points
    that an atom has buried are dropped from the work that follows -- a buried point stays buried -- but every atom is
    looked at for every point that is still exposed."""
    from pywindow_amd import _lib

    n, P = len(c.xyz), len(c.directions)
    R = c.radii + c.probe
    u = c.directions
    owner = np.repeat(np.arange(n), P)                               # the atom of every point still exposed
    which = np.tile(np.arange(P), n)
    p = [c.xyz[owner, a] + R[owner] * u[which, a] for a in range(3)]
    for j in range(n):
        dx, dy, dz = p[0] - c.xyz[j, 0], p[1] - c.xyz[j, 1], p[2] - c.xyz[j, 2]
        keep = ((dx * dx + dy * dy) + dz * dz >= R[j] * R[j]) | (owner == j)      # (excluded by index)
        if not keep.all():
            owner, which = owner[keep], which[keep]
            p = [v[keep] for v in p]
    exposed = np.bincount(owner, minlength=n).astype(np.int32)
    inside = np.zeros(n, dtype=np.int32)
    if c.dims is not None and len(owner):
        nx, ny, nz = c.dims
        i0, j0, l0 = (cell(c.origin[a], c.h, c.dims[a], p[a]) for a in range(3))
        bits = ((c.words.reshape(nz, ny, 1) >> np.arange(nx, dtype=np.uint64)) & np.uint64(1)).astype(bool)   # [l, j, i]
        hit = np.zeros(len(owner), dtype=bool)
        for dl in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    i, j, l = i0 + di, j0 + dj, l0 + dl
                    ok = (i >= 0) & (i < nx) & (j >= 0) & (j < ny) & (l >= 0) & (l < nz)
                    hit[ok] |= bits[l[ok], j[ok], i[ok]]
        inside = np.bincount(owner[hit], minlength=n).astype(np.int32)
    out = np.zeros((), dtype=_lib.SASA_OUT_DTYPE)
    out["exposed"], out["inside"] = int(exposed.sum()), int(inside.sum())
    out["flags"] = _lib.SASA_GRID if c.dims is not None else 0
    return out, exposed, inside


_cache = {}


def reference_cached(c: Case):
    """`reference`, computed once a case object and shared; the results are read-only."""
    if id(c) not in _cache:
        out, exposed, inside = reference(c)
        exposed.setflags(write=False)
        inside.setflags(write=False)
        _cache[id(c)] = (c, (out, exposed, inside))                  # (the case is kept: its id stays its own)
    return _cache[id(c)][1]


def random_atoms(n: int, side: float, seed: int, radius=(0.6, 1.4)):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, side, (n, 3)), rng.uniform(*radius, n)


def pack_words(ok: np.ndarray) -> np.ndarray:
    """The words of a bool array [l, j, i]."""
    nx = ok.shape[2]
    return (ok.astype(np.uint64) << np.arange(nx, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)


def voxels(dims, *set_voxels, garbage=False) -> np.ndarray:
    """The words of a grid with the voxels (i, j, l) set; garbage: every bit at i >= nx set as well."""
    nx, ny, nz = dims
    ok = np.zeros((nz, ny, nx), dtype=bool)
    for i, j, l in set_voxels:
        ok[l, j, i] = True
    words = pack_words(ok)
    if garbage and nx < 64:
        words = words | (np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nx))
    return words


def two_spheres(a: float, b: float, d: float, P: int):
    """(case, the exposed count of atom 0 by the analytic answer): atom 0 at the origin with reach a, atom 1 at
    (0, 0, d) with reach b, the default spiral.  The buried points of atom 0 are the k with z_k > c,
    c = (a^2 + d^2 - b^2) / (2 a d); no z_k may lie within 1e-9 of c, so that no rounding decides."""
    c = (a * a + d * d - b * b) / (2.0 * a * d)
    z = 1.0 - (2.0 * np.arange(P) + 1.0) / P
    assert np.abs(z - c).min() > 1e-9 and -1.0 < c < 1.0, (a, b, d, P)
    case = Case(f"two-spheres-a={a}-b={b}-d={d}-P={P}", [[0.0, 0.0, 0.0], [0.0, 0.0, d]], [a, b], spiral(P))
    return case, P - int((z > c).sum())


def one_atom_grid(name, X, dims, origin, h, set_voxels, garbage=False):
    """An atom of radius 1 at X with the six axis directions over a grid: the points are X +- e_a exactly."""
    return Case(name, [X], [1.0], AXES, dims=dims, origin=origin, h=h, words=voxels(dims, *set_voxels, garbage=garbage))


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernel and the host path can go wrong."""
    out = [Case("no-atoms", np.zeros((0, 3)), np.zeros(0), spiral(64)),
           Case("one-atom", [[0.25, -1.0, 3.0]], [1.5], spiral(64))]
    # tails of a wave of points
    for P in (1, 63, 64, 65, 129):
        xyz, radii = random_atoms(12, 4.0, 100 + P)
        out.append(Case(f"P={P}", xyz, radii, spiral(P), probe=0.3))
    # tails of a wave of candidate atoms, and atoms beyond one wave each
    for n in (2, 63, 64, 65, 130):
        xyz, radii = random_atoms(n, 1.6 * n ** (1.0 / 3.0), 200 + n)
        out.append(Case(f"n={n}", xyz, radii, spiral(65)))
    # equality, from values that are exact in binary: atom 0 at the origin with reach 1 and the point (1, 0, 0), atom 1
    # at (3, 0, 0) with reach 2, so dx^2 = 4 = R^2: exposed; with the next reach above 2 it is buried; then the same
    # reaches split between radius and probe
    pair = [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]
    out.append(Case("tie", pair, [1.0, 2.0], AXES))
    out.append(Case("tie-one-ulp-more", pair, [1.0, np.nextafter(2.0, 3.0)], AXES))
    out.append(Case("tie-probe", pair, [0.75, 1.75], AXES, probe=0.25))
    assert 1.75 + 2.0 ** -51 + 0.25 == np.nextafter(2.0, 3.0)        # (one ulp of 1.75 would be rounded away by the sum)
    out.append(Case("tie-probe-one-ulp-more", pair, [0.75, 1.75 + 2.0 ** -51], AXES, probe=0.25))
    # exclusion by index: two atoms at one position, equal and unequal radii; a zero radius; an atom inside another
    out.append(Case("same-position-equal", [[1.0, 2.0, 3.0]] * 2, [1.25, 1.25], spiral(65)))
    out.append(Case("same-position-unequal", [[1.0, 2.0, 3.0]] * 2, [1.0, 1.5], spiral(65)))
    out.append(Case("zero-radius", [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [9.0, 0.0, 0.0]], [0.0, 1.0, 0.0], spiral(65)))
    out.append(Case("inside-another", [[0.0, 0.0, 0.0], [0.25, 0.0, 0.25]], [2.0, 0.5], spiral(65)))
    # around the culling distance |X_i - X_j| = R_i + R_j: far outside it, just outside it (1e-7), at it and just
    # inside the margin (1e-9 and -1e-9), where the atom is looked at whatever the test then says
    for name, factor in (("far", 400.0), ("just-outside", 1.0 + 1e-7), ("touching", 1.0), ("in-the-margin", 1.0 + 1e-9),
                         ("overlapping-a-hair", 1.0 - 1e-9)):
        direction = np.array([2.0, -1.0, 2.0]) / 3.0
        out.append(Case(f"culling-{name}", [[0.5, 0.5, 0.5], np.array([0.5, 0.5, 0.5]) + 2.75 * factor * direction],
                        [1.5, 1.25], spiral(129)))
    # magnitudes at which nothing is culled: coordinates of the order 2^410, and radii of the order 2^-420
    out.append(Case("huge", np.array([[1.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.5]]) * 2.0 ** 410,
                    np.array([1.0, 1.5, 0.75]) * 2.0 ** 410, spiral(65)))
    out.append(Case("tiny", np.array([[1.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.5]]) * 2.0 ** -420,
                    np.array([1.0, 1.5, 0.75]) * 2.0 ** -420, spiral(65)))
    # two spheres on the z axis: the count of atom 0 is known analytically
    for args in ((1.5, 1.25, 2.0, 129), (1.0, 1.0, 1.0, 960), (2.0, 0.75, 2.25, 65)):
        out.append(two_spheres(*args)[0])
    # the grid.  Voxel coordinates 0, 0.5, 1, ...; the atom at (1, 1, 1) has the points (2, 1, 1), (0, 1, 1), ...
    g = dict(origin=(0.0, 0.0, 0.0), h=0.5)
    # (2, 1, 1) lies ON the coordinate of voxel 4 and belongs to the cell that starts there: its corners are 4, 5 x 2, 3
    # x 2, 3, so voxel (5, 2, 2) is a corner of it and voxel (3, 2, 2) is not
    out.append(one_atom_grid("on-a-coordinate-upper-corner", [1.0, 1.0, 1.0], (8, 8, 8), set_voxels=[(5, 2, 2)], **g))
    out.append(one_atom_grid("on-a-coordinate-not-the-cell-below", [1.0, 1.0, 1.0], (8, 8, 8), set_voxels=[(3, 2, 2)], **g))
    # left of voxel 0 (the origin at x = 0.25: the point (0, 1, 1) has i0 = -1 and the corner 0 alone), and the
    # voxel next to it, which is no corner
    out.append(one_atom_grid("left-of-voxel-0", [1.0, 1.0, 1.0], (8, 8, 8), (0.25, 0.0, 0.0), 0.5, [(0, 2, 2)]))
    out.append(one_atom_grid("left-of-voxel-0-next-voxel", [1.0, 1.0, 1.0], (8, 8, 8), (0.25, 0.0, 0.0), 0.5, [(1, 2, 2)]))
    # right of voxel nx - 1 (nx = 3: coordinates 0, 0.5, 1; the point (2, 1, 1) has i0 = 2 and the corner 2 alone)
    out.append(one_atom_grid("right-of-the-last-voxel", [1.0, 1.0, 1.0], (3, 8, 8), set_voxels=[(2, 2, 2)], **g))
    out.append(one_atom_grid("right-of-the-last-voxel-garbage-bits", [1.0, 1.0, 1.0], (3, 8, 8), set_voxels=[], garbage=True, **g))
    # a point whose whole cell lies outside the grid, far from it on every axis: by the definition i0 is -1 or n - 1 on
    # each axis, so the voxel at that corner of the grid decides (a cavity closed inside its box has none set there)
    out.append(one_atom_grid("far-from-the-grid-corner-voxel-set", [40.0, 40.0, 40.0], (4, 5, 6), set_voxels=[(3, 4, 5)], **g))
    out.append(one_atom_grid("far-from-the-grid-corner-voxel-clear", [40.0, 40.0, 40.0], (4, 5, 6),
                             set_voxels=[(i, j, l) for i in range(4) for j in range(5) for l in range(6) if (i, j, l) != (3, 4, 5)], **g))
    out.append(one_atom_grid("far-below-the-grid", [-40.0, -40.0, -40.0], (4, 5, 6), set_voxels=[(0, 0, 0)], **g))
    # nx = 1, ny = 1, nz = 1; nx = 64 with bit 63
    out.append(one_atom_grid("nx=1", [1.0, 1.0, 1.0], (1, 8, 8), (0.5, 0.0, 0.0), 0.5, [(0, 2, 2), (0, 4, 2)], garbage=True))
    out.append(one_atom_grid("ny=1-nz=1", [1.0, 1.0, 1.0], (8, 1, 1), (0.0, 1.0, 1.0), 0.5, [(4, 0, 0)], garbage=True))
    out.append(one_atom_grid("nx=64-bit-63", [31.0, 1.0, 1.0], (64, 8, 8), set_voxels=[(63, 2, 2)], **g))
    out.append(one_atom_grid("nx=64-bit-62-is-no-corner", [31.0, 1.0, 1.0], (64, 8, 8), set_voxels=[(62, 2, 2)], **g))
    # one set voxel that is exactly one corner of one point's cell: the atom off the coordinates, the point (1.6, 1.1,
    # 1.2) + e_x in the cell (5, 2, 2); voxel (6, 3, 3) is its far corner and a corner of no other point's cell
    out.append(one_atom_grid("one-corner-of-one-cell", [1.6, 1.1, 1.2], (8, 8, 8), set_voxels=[(6, 3, 3)], **g))
    # random atoms, random unit vectors that are no spiral, random words of an uneven grid with garbage beyond nx
    rng = np.random.default_rng(7)
    xyz, radii = random_atoms(40, 4.0, 8)
    dims = (7, 5, 6)
    words = rng.integers(0, 2 ** 63, dims[1] * dims[2], dtype=np.uint64) | np.uint64(1 << 63)
    out.append(Case("random-directions-and-words", xyz, radii, random_directions(129, 9), probe=0.2, dims=dims,
                    origin=(0.3, -0.1, 0.7), h=0.7, words=words))
    out.append(Case("random-directions-no-grid", xyz, radii, random_directions(129, 9), probe=0.2))
    # directions at the tolerance on |u|: |u|^2 = 1 +- 5e-10
    scaled = np.concatenate([spiral(64) * np.sqrt(1.0 + 5e-10), spiral(65) * np.sqrt(1.0 - 5e-10)])
    scaled.setflags(write=False)
    xyz, radii = random_atoms(30, 3.5, 10)
    out.append(Case("directions-at-the-tolerance", xyz, radii, scaled))
    # a grid of 64 x 64 rows (more than the kernel stages in LDS) around a shell of atoms, every other voxel set
    xyz, radii = random_atoms(50, 16.0, 11)
    pattern = np.random.default_rng(12).integers(0, 2 ** 63, 64 * 64, dtype=np.uint64)
    out.append(Case("grid-64x64-rows", xyz, radii, spiral(65), dims=(40, 64, 64), origin=(-1.0, -1.0, -1.0), h=0.28125, words=pattern))
    return out


@functools.lru_cache(maxsize=None)
def big_case():
    """5000 random atoms at P = 64: no capacity in n, and more near atoms than a wave's list holds."""
    xyz, radii = random_atoms(5000, 8.0, 13, radius=(0.3, 1.0))
    return Case("atoms-5000", xyz, radii, spiral(64))


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    xyz, radii = random_atoms(33, 5.0, 21)
    return [Case("before-a", xyz, radii, spiral(100), probe=1.0),
            Case("before-b", xyz[:7], radii[:7], spiral(100), dims=(3, 9, 2), h=2.0, words=np.arange(18, dtype=np.uint64))]


def by_directions(jobs):
    """The cases grouped into calls: the cases of a call share their directions (the same array object)."""
    groups = {}
    for c in jobs:
        groups.setdefault(id(c.directions), []).append(c)
    return list(groups.values())


def pack(jobs, hole: int = 0):
    """The arguments of a call for a list of cases that share their directions: (SASA_JOB_DTYPE array, xyz, radii,
    directions, words, entries of exposed / inside, rows of out).  A job's row of the result and its counts come one job
    after the other, `hole` entries that nobody owns in front of each; atoms and words that several jobs hold (the same
    case object) are stored once."""
    from pywindow_amd import _lib

    assert len({id(c.directions) for c in jobs}) <= 1
    rec = np.zeros(len(jobs), dtype=_lib.SASA_JOB_DTYPE)
    xyz, radii, words, where = [np.zeros((0, 3))], [np.zeros(0)], [np.zeros(0, dtype=np.uint64)], {}
    atoms = n_words = row = at = 0
    for k, c in enumerate(jobs):
        if id(c) not in where:
            where[id(c)] = (atoms, n_words if c.words is not None else -1)
            xyz.append(c.xyz)
            radii.append(c.radii)
            atoms += len(c.xyz)
            if c.words is not None:
                words.append(c.words)
                n_words += len(c.words)
        a, w = where[id(c)]
        row += hole
        at += hole
        rec[k] = (a, len(c.xyz), a, at, w, row, c.origin, c.h, c.probe, *(c.dims or (0, 0, 0)), 0)
        row += 1
        at += len(c.xyz)
    directions = np.ascontiguousarray(jobs[0].directions) if jobs else np.zeros((0, 3))
    return rec, np.concatenate(xyz), np.concatenate(radii), directions, np.concatenate(words), at, row


def blank(n_out: int, n_counts: int):
    """(out, exposed, inside) with every byte SENTINEL."""
    from pywindow_amd import _lib

    out = np.frombuffer(bytes([SENTINEL]) * (_lib.SASA_OUT_DTYPE.itemsize * n_out), dtype=_lib.SASA_OUT_DTYPE).copy()
    counts = np.frombuffer(bytes([SENTINEL]) * (4 * n_counts), dtype=np.int32)
    return out, counts.copy(), counts.copy()


def expected(jobs, hole: int = 0):
    """(out, exposed, inside) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    rec, *_, n_counts, n_out = pack(jobs, hole)
    out, exposed, inside = blank(n_out, n_counts)
    for k, c in enumerate(jobs):
        o, e, i = reference_cached(c)
        out[int(rec["out"][k])] = o
        first = int(rec["count_first"][k])
        exposed[first:first + len(e)] = e
        inside[first:first + len(i)] = i
    return out, exposed, inside


def raw(ctx, packed, hook=None, timed=False, sizes=None, null=()):
    """pw_sasa through ctypes into SENTINEL-filled arrays -- through the library's test entry when `hook` (a dict of
    list_capacity, lds_words, block_atoms) is given or the call is timed.  `sizes`: other numbers of rows and entries of
    (xyz, radii, directions, words, counts, out) to tell the entry, None for the true ones; `null`: the arrays, by name,
    to pass as null pointers.  Returns (rc, (out, exposed, inside)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, radii, directions, words, n_counts, n_out = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.SASA_JOB_DTYPE)
    out, exposed, inside = blank(n_out, n_counts)
    told = [len(xyz), len(radii), len(directions), len(words), n_counts, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v

    def ptr(name, array):
        return None if name in null else array.ctypes.data

    args = [ctx._h, rec.ctypes.data, len(rec), ptr("xyz", xyz), told[0], ptr("radii", radii), told[1],
            ptr("directions", directions), told[2], ptr("words", words), told[3], ptr("exposed", exposed),
            ptr("inside", inside), told[4], out.ctypes.data, told[5]]
    ms = ctypes.c_float(0.0)
    if hook is None and not timed:
        rc = L.pw_sasa(*args)
    else:
        hook = hook or {}
        rc = L.pw_internal_sasa(*args, int(hook.get("list_capacity", 0)), int(hook.get("lds_words", 0)),
                                int(hook.get("block_atoms", 0)), ctypes.byref(ms) if timed else None)
    return (rc, (out, exposed, inside), ms.value) if timed else (rc, (out, exposed, inside))


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: the first row of out, else the first count, that differs."""
    for k in range(len(want[0])):
        if got[0][k].tobytes() != want[0][k].tobytes():
            return "out", k, got[0][k], want[0][k]
    for name, g, w in (("exposed", got[1], want[1]), ("inside", got[2], want[2])):
        at = np.flatnonzero(g != w)
        if len(at):
            return name, int(at[0]), int(g[at[0]]), int(w[at[0]])
    return None


def bad_batches():
    """[(packed, sizes, null, reason)]: three jobs of which job 1 is refused.  The directions are read by the first job
    that has atoms: where they are what is wrong, job 0 has none."""
    xyz, radii = random_atoms(6, 3.0, 41)
    u = spiral(64)
    good = Case("good", xyz, radii, u)
    empty = Case("empty", np.zeros((0, 3)), np.zeros(0), u)
    other = Case("other", xyz[:5] + 0.5, radii[:5], u, probe=0.5)
    gridded = Case("gridded", xyz[:4] - 0.5, radii[:4], u, dims=(9, 8, 7), h=0.5, words=np.arange(56, dtype=np.uint64))
    third = Case("third", xyz[:3], radii[:3], u)
    out = []

    def edit(fn, reason, second=other, first=good, sizes=None, null=()):
        packed = list(pack([first, second, third]))
        fn(packed)
        out.append((tuple(packed), sizes, null, reason))

    def field(name, value):
        def fn(p):
            p[0][name][1] = value
        return fn

    def entry(index, at, value):
        def fn(p):
            p[index] = p[index].copy()
            p[index].reshape(-1)[at(p)] = value
        return fn

    def direction(row, value):
        def fn(p):
            p[3] = p[3].copy()
            p[3][row] = value
        return fn

    def more_directions(p):
        p[3] = np.concatenate([spiral(4096), spiral(1)])

    n_good, n_other, n_grid = len(good.xyz), len(other.xyz), len(gridded.xyz)
    edit(field("n", -1), "a negative count")
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", sizes=(n_good + n_other - 1,))
    edit(field("radius_first", -1), "radii outside the array")
    edit(lambda p: None, "radii outside the array", sizes=(None, n_good + n_other - 1))
    edit(field("count_first", -1), "the counts are outside exposed and inside")
    edit(lambda p: None, "the counts are outside exposed and inside", sizes=(None, None, None, None, n_good + n_other - 1))
    edit(field("out", -1), "the row is outside out")
    edit(lambda p: None, "the row is outside out", sizes=(None, None, None, None, None, 1))
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G", second=gridded)
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G", second=gridded)
    edit(field("word_first", -2), "the words are outside their array", second=gridded)
    edit(field("word_first", 1), "the words are outside their array", second=gridded)
    edit(lambda p: None, "the words are outside their array", second=gridded, sizes=(None, None, None, 55))
    edit(lambda p: None, "null array", second=gridded, null=("words",))
    edit(lambda p: None, "null array", first=empty, null=("xyz",))
    edit(lambda p: None, "null array", first=empty, null=("directions",))
    edit(lambda p: None, "null array", first=empty, null=("inside",))
    edit(field("probe", np.nan), "the probe is not finite")
    edit(field("probe", np.inf), "the probe is not finite")
    edit(field("probe", -1.0), "a negative probe")
    edit(field("origin", [0.0, np.nan, 0.0]), "the origin or the spacing is not finite", second=gridded)
    edit(field("spacing", np.inf), "the origin or the spacing is not finite", second=gridded)
    edit(field("spacing", 0.0), "spacing <= 0", second=gridded)
    edit(field("spacing", -0.5), "spacing <= 0", second=gridded)
    edit(entry(1, lambda p: 3 * (int(p[0]["atom_first"][1]) + 2) + 1, np.nan), "a coordinate is not finite")
    edit(entry(1, lambda p: 3 * (int(p[0]["atom_first"][1]) + 2), -np.inf), "a coordinate is not finite")
    edit(entry(2, lambda p: int(p[0]["radius_first"][1]) + 1, np.nan), "a radius is not finite")
    edit(entry(2, lambda p: int(p[0]["radius_first"][1]) + 1, -0.5), "a negative radius")
    edit(lambda p: None, "the number of directions is outside 1 .. PW_SASA_MAX_POINTS", first=empty, sizes=(None, None, 0))
    edit(more_directions, "the number of directions is outside 1 .. PW_SASA_MAX_POINTS", first=empty)
    edit(direction(3, [0.0, np.nan, 1.0]), "direction 3 is not finite", first=empty)
    edit(direction(63, u[63] * (1.0 + 1e-8)), "direction 63 is not a unit vector", first=empty)
    edit(direction(0, u[0] * (1.0 - 1e-8)), "direction 0 is not a unit vector", first=empty)
    edit(direction(5, [0.0, 0.0, 0.0]), "direction 5 is not a unit vector", first=empty)
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("count_first", n_good - 1), "shares entries of exposed and inside with an earlier job")
    edit(field("count_first", 0), "shares entries of exposed and inside with an earlier job")
    return out
