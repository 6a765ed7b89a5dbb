"""Inputs shared by tests/test_basins.py (host path against the definition) and tests/test_gpu_basins.py (device against
the host path and against the definition): the energy basins of a periodic field, the edges between them and their
Boltzmann sums (pw_basins).  Every comparison is of bytes.  numpy only and seeded; nothing here is taken from
pywindow_amd/csrc/pw_basins.hpp -- the definition of include/pywindow_amd.h is written directly:

  basins   the allowed voxels are visited in ascending (key, rank); each takes the label and the offset of its parent,
           which was visited before it (no pointer jumping); the parent is chosen by whole-array comparisons over the
           candidates in their order.
  edges    a Python dict from (a, b, d) to its faces.
  sums     an explicit 64-slot tree per row and group (halving the slots pairwise is the tree), the rows in order.

pw_exp comes through the library's instrumentation (pw_internal_exp on the host path), so the weights are the library's
bits and only the association is under test."""
import ctypes
import functools

import numpy as np

import _channels_cases as CC
import _kde_cases as K
import _percolation_cases as PC

SENTINEL = CC.SENTINEL
INF = np.inf
UNIT = PC.UNIT
MAX_OFFSET = 255
OVERFLOW, CLAMPED, RANGE = 1, 2, 4
NAMES = ("out", "basins", "edges", "labels", "map")


class Case(PC.Case):
    """PC.Case with the cap, the inverse temperatures, the capacities and whether the job asks for its labels."""

    def __init__(self, name, field=None, cap=INF, betas=(0.4,), b_cap=64, e_cap=256, labels=False, **kw):
        super().__init__(name, field, **kw)
        self.cap, self.betas, self.b_cap, self.e_cap, self.labels = float(cap), tuple(float(b) for b in betas), int(b_cap), int(e_cap), bool(labels)


# ---- the definition ----------------------------------------------------------------------------------------------
def key_of(U):
    """pw_passage's key, written again: integers that order as the doubles compare, the two zeros one key."""
    bits = np.ascontiguousarray(U, dtype=np.float64).view(np.uint64).copy()
    bits[bits == np.uint64(0x8000000000000000)] = 0
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(0x8000000000000000))


@functools.lru_cache(maxsize=None)
def _host():
    from pywindow_amd import _lib

    return _lib.Context(-1)


def weights(U, beta):
    """(w, clamped) per value: x = -(beta*U), clamped at 700, w = pw_exp(x)."""
    x = -(beta * np.asarray(U, dtype=np.float64))
    hot = x > 700.0
    return K.internal_exp(_host(), np.where(hot, 700.0, x).reshape(-1)).reshape(x.shape), hot


def _tree(slots):
    """The chunk tree over the last axis (64 slots): halving pairwise is slot[t] += slot[t + k], t a multiple of 2k."""
    while slots.shape[-1] > 1:
        slots = slots[..., 0::2] + slots[..., 1::2]
    return slots[..., 0]


def _row_sums(group, values, n_groups):
    """Per group g the total of `values` (rows, nx) over the voxels with group == g: the chunk sums of the rows that
    hold a member, taken in row order from +0.0.  group (rows, nx), -1: no member."""
    rows, nx = group.shape
    total = np.zeros(n_groups)
    pairs = [(r, g) for r in range(rows) for g in np.unique(group[r][group[r] >= 0])]
    if not pairs:
        return total
    slots = np.zeros((len(pairs), 64))
    for p, (r, g) in enumerate(pairs):
        slots[p, :nx] = np.where(group[r] == g, values[r], 0.0)
    chunk = _tree(slots)
    for p, (r, g) in enumerate(pairs):
        total[g] = total[g] + chunk[p]
    return total


def definition(U, cap=INF, betas=(0.4,), b_cap=64, e_cap=256):
    """(out, basins, edges, labels) of the field U [l, j, i]: the records of the header; basins and edges hold the rows
    that are written."""
    from pywindow_amd import _lib

    nz, ny, nx = U.shape
    dims = (nx, ny, nz)
    V = nx * ny * nz
    flat = U.reshape(-1)
    key = key_of(flat)
    rank3 = np.arange(V).reshape(nz, ny, nx)
    with np.errstate(invalid="ignore"):
        allowed = ~np.isposinf(flat) & (flat <= cap)
    index = np.stack(np.unravel_index(np.arange(V), (nz, ny, nx))[::-1], axis=1)     # (V, 3): i, j, l
    # the parents: self, then -a, +a, -b, +b, -c, +c; a strict "before" keeps the earlier candidate
    best_key, best_rank, cross = key.copy(), np.arange(V), np.zeros((V, 3), dtype=np.int64)
    for k in range(3):
        axis = 2 - k
        if dims[k] == 1:
            continue
        for sign in (-1, 1):
            other = np.roll(rank3, -sign, axis=axis).reshape(-1)                 # the rank of v + sign e_k
            over = np.where(index[:, k] == (0 if sign < 0 else dims[k] - 1), sign, 0)
            better = allowed[other] & ((key[other] < best_key) | ((key[other] == best_key) & (other < best_rank)))
            best_key = np.where(better, key[other], best_key)
            best_rank = np.where(better, other, best_rank)
            cross[better] = 0
            cross[better, k] = over[better]
    parent = np.where(allowed, best_rank, -1)
    roots = np.flatnonzero(parent == np.arange(V))
    label = np.full(V, -1, dtype=np.int64)
    label[roots] = np.arange(len(roots))
    o = np.zeros((V, 3), dtype=np.int64)
    order = np.flatnonzero(allowed)
    order = order[np.lexsort((order, key[order]))]
    for v in order.tolist():
        p = parent[v]
        if p != v:
            assert label[p] >= 0
            label[v] = label[p]
            o[v] = cross[v] + o[p]
    B = len(roots)
    flags = RANGE if np.abs(o).max(initial=0) > MAX_OFFSET else 0
    # the faces
    edges = {}
    face_edge = np.full((3, V), -1, dtype=np.int64)
    face_term = np.zeros((3, V))
    for v in np.flatnonzero(allowed).tolist():
        for k in range(3):
            i = index[v].copy()
            c = 1 if i[k] == dims[k] - 1 else 0
            i[k] = (i[k] + 1) % dims[k]                                      # (n_k == 1: v' is v)
            w = int((i[2] * ny + i[1]) * nx + i[0])
            if not allowed[w]:
                continue
            a, b = int(label[v]), int(label[w])
            d = o[w] - o[v]
            d[k] += c
            d = tuple(int(x) for x in d)
            if a == b and d == (0, 0, 0):
                continue
            lead = next((x for x in d if x), 0)
            if a > b or (a == b and lead < 0):
                a, b, d = b, a, tuple(-x for x in d)
            if max(abs(x) for x in d) > MAX_OFFSET:
                flags |= RANGE
            term = flat[w] if key[w] > key[v] else flat[v]
            edges.setdefault((a, b) + d, []).append((v, k, term))
    if flags & RANGE:
        edges = {}
    names = sorted(edges)
    E = len(names)
    if B > b_cap or E > e_cap:
        flags |= OVERFLOW
    b_written = min(B, b_cap)
    e_written = 0 if flags & OVERFLOW else E
    L = len(betas)
    w_all, hot = zip(*[weights(np.where(allowed, flat, 0.0), beta) for beta in betas])
    if any((h & allowed).any() for h in hot):
        flags |= CLAMPED
    basins = np.zeros(b_written, dtype=_lib.BASINS_BASIN_DTYPE)
    shown = np.where(label < b_written, label, -1).reshape(nz * ny, nx)
    basins["root"] = roots[:b_written]
    basins["n_voxels"] = np.bincount(label[(label >= 0) & (label < b_written)], minlength=b_written)
    basins["u_min"] = flat[roots[:b_written]]
    for b in range(L):
        basins["z"][:, b] = _row_sums(shown, w_all[b].reshape(nz * ny, nx), b_written)
        with np.errstate(over="ignore"):                             # (w * U may be +-inf: so it is in the library)
            e_terms = (w_all[b] * np.where(allowed, flat, 0.0)).reshape(nz * ny, nx)
        basins["e"][:, b] = _row_sums(shown, e_terms, b_written)
    rows = np.zeros(e_written, dtype=_lib.BASINS_EDGE_DTYPE)
    if e_written:
        for e, name in enumerate(names):
            faces = edges[name]
            rows[e]["a"], rows[e]["b"], rows[e]["d"] = name[0], name[1], name[2:]
            rows[e]["n_faces"] = len(faces)
            keys = key_of(np.array([f[2] for f in faces]))
            v, k, term = faces[int(np.flatnonzero(keys == keys.min())[0])]       # (faces ascend in (v, k))
            rows[e]["saddle"], rows[e]["saddle_voxel"], rows[e]["saddle_k"] = term, v, k
            for v, k, term in faces:
                face_edge[k, v], face_term[k, v] = e, term
        for b, beta in enumerate(betas):
            w_face = weights(face_term, beta)[0]
            for k in range(3):
                rows["s"][:, b, k] = _row_sums(face_edge[k].reshape(nz * ny, nx), w_face[k].reshape(nz * ny, nx), E)
    labels = np.zeros(V, dtype=_lib.BASINS_LABEL_DTYPE)
    labels["basin"] = label
    labels["o"] = 0 if flags & RANGE else o
    out = np.zeros((), dtype=_lib.BASINS_OUT_DTYPE)
    low = order[0] if len(order) else -1
    out["n_basins"], out["n_edges"], out["n_basins_written"], out["n_edges_written"] = B, E, b_written, e_written
    out["n_blocked"], out["n_allowed"] = int(np.isposinf(flat).sum()), int(allowed.sum())
    out["u_min"] = flat[low] if low >= 0 else INF
    out["u_min_voxel"] = index[low] if low >= 0 else -1
    out["flags"] = flags
    return out, basins, rows, labels


_cache = {}


def reference_cached(c: Case):
    """(out, basins, edges, labels, field) of a case, computed once a case object and shared; read-only."""
    if id(c) not in _cache:
        U = PC.field_of(c)
        got = definition(U, c.cap, c.betas, c.b_cap, c.e_cap)
        for a in got[1:]:
            a.setflags(write=False)
        _cache[id(c)] = (c, got + (U,))
    return _cache[id(c)][1]


# ---- the cases -------------------------------------------------------------------------------------------------
def path_field(dims, path):
    """A field that is +inf but along `path` (voxels (i, j, l)), where it falls by one a step: the descent follows the
    path if it is induced -- no two voxels of it are neighbours but consecutive ones --, which is asserted."""
    nx, ny, nz = dims
    f = np.full((nz, ny, nx), INF)
    at = {p: q for q, p in enumerate(path)}
    assert len(at) == len(path)
    for q, (i, j, l) in enumerate(path):
        f[l, j, i] = -float(q)
        for k, n in enumerate(dims):
            for s in (-1, 1):
                p = [i, j, l]
                p[k] = (p[k] + s) % n
                r = at.get(tuple(p), q)
                assert abs(r - q) <= 1, (path[q], tuple(p))
    return f


def helix_path():
    """On 4 x 4 x 8: alternately a step along +a and a step in the (b, c) section, 17 positions of a walk in the section
    found by a depth-first search: self-avoiding, and two of its positions that are neighbours without being consecutive
    are 2 (mod 4) positions apart, so that they lie in slices that do not meet.  It starts at i = 3 and crosses the face
    of +a at its steps 1, 5, 9, 13 and 17."""
    ny, nz, n = 4, 8, 17
    cells = [(j, l) for l in range(nz) for j in range(ny)]
    near = {c: [((c[0] + dj) % ny, (c[1] + dl) % nz) for dj, dl in ((1, 0), (0, 1), (-1, 0), (0, -1))] for c in cells}

    def extend(walk):
        if len(walk) == n:
            return walk
        for c in near[walk[-1]]:
            if c in walk:
                continue
            t = len(walk)
            if any(walk[s] in near[c] and (t - s) % 4 != 2 for s in range(t - 1)):
                continue
            done = extend(walk + [c])
            if done:
                return done
        return None

    walk = extend([(0, 0)])
    assert walk is not None
    path, i = [], 3
    for j, l in walk:
        path.append((i, j, l))
        i = (i + 1) % 4
        path.append((i, j, l))
    return path


def serpentine_path(cells_wanted):
    """On 2 x 64 x 64: a serpentine of cells in the (b, c) section, every other cell with a step along a; a step along a
    from index 0 goes through the face of -a (the first candidate), so the path crosses it once every four cells."""
    cells, l, forward = [], 0, True
    while len(cells) < cells_wanted:
        cells += [(j, l) for j in (range(0, 62) if forward else range(61, -1, -1))]
        cells.append((61 if forward else 0, l + 1))
        l, forward = l + 2, not forward
    assert l < 62
    path, i = [], 0
    for q, (j, l) in enumerate(cells[:cells_wanted]):
        path.append((i, j, l))
        if q % 2 == 0:
            i = 1 - i
            path.append((i, j, l))
    return path


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernel and the host path can go wrong, as fields of the caller's."""
    out = []
    rng = np.random.default_rng(17)
    by_name = {c.name: c for c in PC.cases()}
    for name in ("channel-along-a", "staircase-111", "slab", "pocket-round-the-corner", "two-interleaved-channels",
                 "channel-along-a-walls-blocked", "double-helix", "double-helix-tiled-twice", "double-helix-in-high-walls",
                 "cubic-maze"):
        out.append(Case(name, by_name[name].field, b_cap=1024, e_cap=4096))
    for dims in ((3, 4, 5), (1, 5, 6), (2, 2, 7), (6, 5, 4)):
        nx, ny, nz = dims
        out.append(Case(f"ties-{dims}", rng.integers(-3, 4, (nz, ny, nx)).astype(np.float64), b_cap=128, e_cap=512, labels=True))
        out.append(Case(f"normal-{dims}", rng.normal(size=(nz, ny, nx)), b_cap=128, e_cap=512, betas=(0.4, 1.0, 2.5)))
        f = rng.integers(-2, 3, (nz, ny, nx)).astype(np.float64)
        f[rng.random((nz, ny, nx)) < 0.3] = INF
        out.append(Case(f"ties-blocked-{dims}", f, b_cap=128, e_cap=512, map=True))
    for nx in (1, 2, 63, 64):
        out.append(Case(f"nx={nx}", rng.normal(size=(2, 3, nx)), b_cap=256, e_cap=1024))
    for ny, nz in ((1, 1), (63, 1), (64, 1), (6, 43), (7, 37)):                       # ny*nz = 1, 63, 64, 258, 259
        f = rng.normal(size=(nz, ny, 2))
        f[rng.random((nz, ny, 2)) < 0.2] = INF
        out.append(Case(f"rows={ny}x{nz}", f, b_cap=512, e_cap=2048))
    out.append(Case("one-voxel", np.array([[[2.5]]]), labels=True))
    out.append(Case("all-blocked", np.full((3, 4, 5), INF), labels=True))
    f = np.full((3, 4, 5), INF)
    f[1, 2, 3] = -7.25
    out.append(Case("one-finite-voxel", f))
    out.append(Case("all-equal", np.full((3, 4, 5), 1.25)))
    # n_k == 2 along each direction: a descent from index 0 (through the face of -e_k) and one from index 1
    for k in range(3):
        for start in (0, 1):
            f = np.full([3 if q != 2 - k else 2 for q in range(3)], 5.0)
            at = [1, 1, 1]
            at[2 - k] = start
            f[tuple(at)] = 1.0
            at[2 - k] = 1 - start
            f[tuple(at)] = 0.0
            out.append(Case(f"two-along-{'abc'[k]}-from-{start}", f, labels=True))
    out.append(Case("helix-five-crossings", path_field((4, 4, 8), helix_path()), labels=True))
    out.append(Case("serpentine-leaves-the-range", path_field((2, 64, 64), serpentine_path(1040)), labels=True, brute=False))
    out.append(Case("serpentine-within-the-range", path_field((2, 64, 64), serpentine_path(1000)), brute=False))
    # the two zeros: at a root (the plateau of zeros) and at a saddle
    f = np.full((4, 4, 6), 3.0)
    f[2, 1, :] = -1.0
    f[2, 1, 1] = -0.0
    f[2, 1, 4] = 0.0
    out.append(Case("zeros-at-a-saddle", f))
    f = np.full((3, 3, 5), 2.0)
    f[1, 1, 1] = -0.0                                                # (the root: the lowest rank of the three that tie)
    f[1, 1, 2] = 0.0
    f[1, 1, 3] = -0.0
    out.append(Case("zeros-at-a-root", f))
    tiny = np.nextafter(0.0, 1.0)
    f = rng.choice(np.array([tiny, -tiny, 3 * tiny, 1e-310, -1e-310, 1e308, -1e308, 1.7e308, 0.0]), (4, 5, 3))
    out.append(Case("denormals-and-huge", f, betas=(1e-306, 1.0)))
    out.append(Case("clamped", np.array([[[-2000.0, 1.0, -1.0, 3.0]]]), betas=(0.25, 1.0)))
    # two wells at -2 and -1 joined over a saddle at 1 in walls at 4: the cap below, at and above the saddle
    f = np.full((3, 3, 7), 4.0)
    f[1, 1, 1:6] = [-2.0, 0.5, 1.0, 0.25, -1.0]
    for cap in (0.75, 1.0, 2.0, INF):
        out.append(Case(f"cap={cap}", f, cap=cap))
    # rows of many basins: a row of 64 voxels that holds 32 basins of one voxel each (no two voxels of a row that are not
    # neighbours can be more), a row whose 64 voxels belong to 64 different basins, and a row that holds three
    walls = np.full((1, 4, 64), INF)
    walls[0, 1, :] = -1.0 - rng.permutation(64)
    walls[0, 1, 1::2] = INF
    walls[0, 2, :] = 7.0
    out.append(Case("a-row-of-32-single-voxel-basins", walls, b_cap=64, e_cap=256))
    out.append(Case("a-row-of-64-basins", _separate_wells(), b_cap=64, e_cap=256))
    f = np.full((2, 3, 9), 6.0)
    f[0, 1, 1], f[0, 1, 4], f[0, 1, 7] = -1.0, -2.0, -3.0
    out.append(Case("a-row-of-three-basins", f, labels=True))
    # capacities exactly met and exceeded by one
    c = next(c for c in out if c.name == "normal-(6, 5, 4)")
    ref = definition(c.field, b_cap=4096, e_cap=4096)[0]
    B, E = int(ref["n_basins"]), int(ref["n_edges"])
    out.append(Case("b_cap-met", c.field, b_cap=B, e_cap=E))
    out.append(Case("b_cap-exceeded", c.field, b_cap=B - 1, e_cap=E))
    out.append(Case("e_cap-exceeded", c.field, b_cap=B, e_cap=E - 1))
    out.append(Case("no-capacity", c.field, b_cap=0, e_cap=0))
    out.append(Case("eight-betas", c.field, b_cap=B, e_cap=E, betas=tuple(0.1 * (b + 1) for b in range(8)), labels=True, map=True))
    return out


def _separate_wells():
    """1 x 3 x 64: the 64 voxels of the row j = 1 belong to 64 different basins, each draining into the well below it
    (even i) or above it (odd i).  64 basins of ONE voxel each cannot share a row: a root has no lower neighbour."""
    f = np.full((1, 3, 64), INF)
    f[0, 1, :] = 10.0 + np.arange(64.0)
    f[0, 0, 0::2] = -1.0 - np.arange(32.0)
    f[0, 2, 1::2] = -40.0 - np.arange(32.0)
    return f


@functools.lru_cache(maxsize=None)
def big_cases():
    """PC's 64^3 with four distinct values."""
    return [Case("grid-64", PC.big_cases()[0].field, b_cap=4096, e_cap=8192, brute=False)]


@functools.lru_cache(maxsize=None)
def atom_cases():
    """PC's jobs with atoms (0, 1, 128 and 129 atoms in an orthorhombic cell, a skewed cell, map on and off), with labels
    on and off and L = 1 and 8."""
    out = []
    for q, c in enumerate(PC.atom_cases()):
        out.append(Case(c.name, dims=c.dims, xyz=c.xyz, coef=c.coef, core2=c.core2, cutoff2=c.cutoff2, origin=c.origin, step=c.step,
                        map=c.map, brute=False, labels=q % 2 == 0, cap=INF if q % 3 else 50.0, b_cap=512, e_cap=2048,
                        betas=(0.4,) if q % 2 else tuple(0.05 * (b + 1) for b in range(8))))
    return out


def mixed_batch():
    """A batch of mixed grids, fields and atoms."""
    return [c for q, c in enumerate(cases()) if q % 4 == 0] + list(atom_cases()) + big_cases()


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    rng = np.random.default_rng(5)
    return [Case("before-a", rng.normal(size=(40, 3, 50)), b_cap=2048, e_cap=8192),
            Case("before-b", rng.integers(0, 3, (2, 33, 9)).astype(np.float64), b_cap=256, e_cap=1024)]


# ---- a call -------------------------------------------------------------------------------------------------------
def pack(jobs, hole: int = 0, reverse: bool = False):
    """The arguments of a call for a list of cases: (BASINS_JOB_DTYPE array, xyz, coef, field, rows of out, of basins, of
    edges, entries of labels, of map).  A job's outputs come one job after the other (`reverse`: the last job's first),
    `hole` entries that nobody owns in front of each; atoms and fields that several jobs hold (the same array) are stored
    once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.BASINS_JOB_DTYPE)
    xyz, coef, field, where = [np.zeros((0, 3))], [np.zeros((0, 2))], [np.zeros(0)], {}
    atoms = entries = 0
    for c in jobs:
        what = id(c.xyz) if c.field is None else id(c.field)
        if what in where:
            continue
        if c.field is None:
            where[what] = atoms
            xyz.append(c.xyz)
            coef.append(c.coef)
            atoms += len(c.xyz)
        else:
            where[what] = entries
            field.append(c.field.reshape(-1))
            entries += c.voxels
    row = basin = edge = label = at = 0
    for k in (range(len(jobs) - 1, -1, -1) if reverse else range(len(jobs))):
        c = jobs[k]
        lj = c.field is None
        a = where[id(c.xyz) if lj else id(c.field)]
        row, basin, edge = row + hole, basin + hole, edge + hole
        label += hole if c.labels else 0
        at += hole if c.map else 0
        betas = np.zeros(8)
        betas[:len(c.betas)] = c.betas
        rec[k] = (a if lj else 0, len(c.xyz) if lj else 0, a if lj else 0, -1 if lj else a, at if c.map else -1, basin, edge,
                  label if c.labels else -1, row, c.b_cap, c.e_cap, c.origin, c.step, c.core2, c.cutoff2, c.cap, betas, *c.dims,
                  len(c.betas))
        row, basin, edge = row + 1, basin + c.b_cap, edge + c.e_cap
        label += c.voxels if c.labels else 0
        at += c.voxels if c.map else 0
    return rec, np.concatenate(xyz), np.concatenate(coef), np.concatenate(field), row, basin, edge, label, at


def blank(n_out, n_basins, n_edges, n_labels, n_map):
    """(out, basins, edges, labels, map) with every byte SENTINEL."""
    from pywindow_amd import _lib

    def filled(dtype, n):
        return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dtype).itemsize * n), dtype=dtype).copy()

    return (filled(_lib.BASINS_OUT_DTYPE, n_out), filled(_lib.BASINS_BASIN_DTYPE, n_basins), filled(_lib.BASINS_EDGE_DTYPE, n_edges),
            filled(_lib.BASINS_LABEL_DTYPE, n_labels), filled(np.float64, n_map))


def expected(jobs, hole: int = 0, reverse: bool = False):
    """(out, basins, edges, labels, map) in the layout of `pack`, SENTINEL bytes where nobody writes."""
    rec = pack(jobs, hole, reverse)
    got = blank(*rec[4:9])
    for k, c in enumerate(jobs):
        o, basins, edges, labels, U = reference_cached(c)
        J = rec[0][k]
        got[0][int(J["out"])] = o
        got[1][int(J["basin_first"]):int(J["basin_first"]) + len(basins)] = basins
        got[2][int(J["edge_first"]):int(J["edge_first"]) + len(edges)] = edges
        if c.labels:
            got[3][int(J["label_first"]):int(J["label_first"]) + c.voxels] = labels
        if c.map:
            got[4][int(J["map_first"]):int(J["map_first"]) + c.voxels] = U.reshape(-1)
    return got


def raw(ctx, packed, workspace_bytes=None, timed=False, sizes=None, diagnostics=None):
    """pw_basins through ctypes into SENTINEL-filled arrays -- through the library's test entry when `workspace_bytes` is
    given (0: the default budget), `timed` or `diagnostics` (a list that receives (n_rounds, n_faces)).  `sizes`: other
    numbers of rows and entries of (xyz, coef, field, map, basins, edges, labels, out) to tell the entry, None for the
    true ones.  Returns (rc, (out, basins, edges, labels, map)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, coef, field, n_out, n_basins, n_edges, n_labels, n_map = packed
    rec = np.ascontiguousarray(rec, dtype=_lib.BASINS_JOB_DTYPE)
    got = blank(n_out, n_basins, n_edges, n_labels, n_map)
    told = [len(xyz), len(coef), len(field), n_map, n_basins, n_edges, n_labels, n_out]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, told[0], coef.ctypes.data, told[1], field.ctypes.data, told[2],
            got[4].ctypes.data, told[3], got[1].ctypes.data, told[4], got[2].ctypes.data, told[5], got[3].ctypes.data, told[6],
            got[0].ctypes.data, told[7]]
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None and not timed and diagnostics is None:
        rc = L.pw_basins(*args)
    else:
        n_rounds, n_faces = np.zeros(len(rec), dtype=np.int32), np.zeros(len(rec), dtype=np.int32)
        rc = L.pw_internal_basins(*args, int(workspace_bytes or 0), ctypes.byref(ms) if timed else None, n_rounds.ctypes.data,
                                  n_faces.ctypes.data)
        if diagnostics is not None:
            diagnostics.append((n_rounds, n_faces))
    return (rc, got, ms.value) if timed else (rc, got)


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def first_difference(got, want):
    """For an assertion's message: the first entry that differs."""
    for what, g, w in zip(NAMES, got, want):
        for k in range(len(w)):
            if g[k].tobytes() != w[k].tobytes():
                return what, k, g[k], w[k]
    return None


def run_field(ctx, U, cap=INF, betas=(0.4,), b_cap=4096, e_cap=16384):
    """(out record, basins, edges) of one field through Context.basins, the rows that were written."""
    from pywindow_amd import _lib

    nz, ny, nx = U.shape
    jobs = np.zeros(1, dtype=_lib.BASINS_JOB_DTYPE)
    b = np.zeros(8)
    b[:len(betas)] = betas
    jobs[0] = (0, 0, 0, 0, -1, 0, 0, -1, 0, b_cap, e_cap, (0.0, 0.0, 0.0), UNIT, 0.25, 0.0, cap, b, nx, ny, nz, len(betas))
    out, basins, edges, _, _ = ctx.basins(jobs, field=np.ascontiguousarray(U, dtype=np.float64).reshape(-1))
    return out[0], basins[:int(out[0]["n_basins_written"])], edges[:int(out[0]["n_edges_written"])]


def bad_batches():
    """[(packed, sizes, reason)]: two jobs of which job 1 is refused -- pw_percolation's list on pw_basins' arrays, and
    what is pw_basins' own."""
    good = cases()[0]
    other = next(c for c in atom_cases() if c.name == "skewed-cell")   # atoms, with a map and labels
    field2 = next(c for c in cases() if c.name == "eight-betas")      # a field, with a map and labels
    out = []

    def edit(fn, reason, sizes=None, second=other):
        packed = list(pack([good, second]))
        packed[0] = packed[0].copy()
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

    def element(name, q, value):
        def fn(p):
            p[0][name][1][q] = value
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
    edit(element("step", 3, np.inf), "the origin or a step is not finite")
    for q in (0, 2, 5):
        edit(element("step", q, 0.0), "ax, by or cz <= 0")
        edit(element("step", q, -0.5), "ax, by or cz <= 0")
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("core2", 1e-7), "core2 below 1e-6 or not finite")
    edit(field("core2", np.nan), "core2 below 1e-6 or not finite")
    edit(field("cutoff2", 0.1), "cutoff2 is neither 0 nor above core2")
    edit(field("n", -1), "a negative count")
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda p: None, "atoms outside xyz", sizes=(n_atoms - 1,) + (None,) * 7)
    edit(lambda p: None, "coefficients outside coef", sizes=(None, n_atoms - 1) + (None,) * 6)
    edit(field("field_first", -2), "the field is outside its array")
    edit(lambda p: None, "the field is outside its array", sizes=(None, None, V_good + V_f2 - 1) + (None,) * 5, second=field2)
    edit(value(np.nan), "a field value is -inf or not a number", second=field2)
    edit(value(-np.inf), "a field value is -inf or not a number", second=field2)
    edit(field("map_first", -2), "the map is outside its array")
    edit(lambda p: None, "the map is outside its array", sizes=(None, None, None, V_other - 1) + (None,) * 4)
    edit(lambda p: None, "the rows are outside basins", sizes=(None,) * 4 + (good.b_cap + other.b_cap - 1, None, None, None))
    edit(field("basin_first", -1), "the rows are outside basins")
    edit(lambda p: None, "the rows are outside edges", sizes=(None,) * 5 + (good.e_cap + other.e_cap - 1, None, None))
    edit(field("edge_first", -1), "the rows are outside edges")
    edit(field("label_first", -2), "the labels are outside their array")
    edit(lambda p: None, "the labels are outside their array", sizes=(None,) * 6 + (V_other - 1, None))
    edit(lambda p: None, "the row is outside out", sizes=(None,) * 7 + (1,))
    edit(field("out", -1), "the row is outside out")
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("basin_first", good.b_cap - 1), "shares rows of basins with an earlier job")
    edit(field("edge_first", good.e_cap - 1), "shares rows of edges with an earlier job")

    def both_maps(p):
        p[0]["map_first"][0] = V_other - 1                          # job 0 gets a map that meets job 1's
        p[8] = V_other - 1 + V_good
    edit(both_maps, "shares entries of map with an earlier job")

    def both_labels(p):
        p[0]["label_first"][0] = V_other - 1
        p[7] = V_other - 1 + V_good
    edit(both_labels, "shares labels with an earlier job")
    # pw_basins' own
    edit(field("b_cap", -1), "a negative capacity")
    edit(field("e_cap", -1), "a negative capacity")
    edit(field("n_betas", 0), "n_betas outside 1 .. PW_AFF_MAX_LEVELS (8)")
    edit(field("n_betas", 9), "n_betas outside 1 .. PW_AFF_MAX_LEVELS (8)")
    for beta in (0.0, -1.0, np.nan, np.inf):
        edit(element("betas", 0, beta), "a beta is not positive or not finite")
    edit(field("cap", np.nan), "the cap is -inf or not a number")
    edit(field("cap", -np.inf), "the cap is -inf or not a number")
    return out


# ---- library against library: the levels of pw_percolation from the edges -----------------------------------------
def percolation_keys_from_edges(out, basins, edges):
    """The six levels of pw_percolation's criteria as keys, from the rows of pw_basins with cap = +inf: a union-find over
    the basins, the basins and the edges entering in ascending key (a basin at its u_min, an edge at its saddle),
    carrying the offsets mod 2 and per set the subspace of (Z/2)^3 its closed walks span; a criterion's level is the key
    after whose entries some set meets it."""
    B = len(basins)
    parent, parity, space = list(range(B)), [0] * B, [1] * B               # (the subspace as a bit per element)

    def find(a):
        p = 0
        while parent[a] != a:
            p ^= parity[a]
            a = parent[a]
        return a, p

    events = sorted([(int(key_of(np.array([e["saddle"]]))[0]), q) for q, e in enumerate(edges)])
    levels = [None] * 6
    done = 0
    while done < len(events):
        level = events[done][0]
        touched = set()
        while done < len(events) and events[done][0] == level:
            e = edges[events[done][1]]
            done += 1
            w = int(e["d"][0] & 1) | (int(e["d"][1] & 1) << 1) | (int(e["d"][2] & 1) << 2)
            (ra, pa), (rb, pb) = find(int(e["a"])), find(int(e["b"]))
            if ra != rb:
                parent[rb], parity[rb] = ra, pa ^ pb ^ w
                for x in range(8):
                    if (space[rb] >> x) & 1:
                        space[ra] = PC._span(space[ra], x)
                touched.add(ra)
            else:
                space[ra] = PC._span(space[ra], pa ^ pb ^ w)
                touched.add(ra)
        for r in touched:
            r = find(r)[0]
            wraps = PC._wraps_of(space[r])
            for c in range(6):
                if levels[c] is None and PC.meets(wraps, c):
                    levels[c] = level
    return [0xFFF0000000000000 if v is None else v for v in levels]
