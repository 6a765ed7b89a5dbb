"""Inputs shared by tests/test_cluster.py (host path against the definition) and tests/test_gpu_cluster.py (device
against the host path and against the definition): the gromos clustering of frames over a distance matrix
(pw_cluster_gromos).  Every output is an integer: every comparison is np.array_equal.  numpy only and seeded; nothing
here is taken from pywindow_amd/csrc/pw_cluster.hpp -- `reference` is the definition of include/pywindow_amd.h written
directly."""
import ctypes
import functools

import numpy as np

SENTINEL = -77

#: the word (64), the tile (64 x 64), the padding of a row to an even number of words (65 .. 128 columns are two words,
#: 129 three padded to four) and 17 x 17 tiles with a last tile of one bit
NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1025)


def reference(d, cutoff):
    """(labels (n,), centres (n_clusters,), sizes (n_clusters,)) of the definition: a boolean neighbour matrix from the
    strict upper triangle, then argmax of the active counts (the first maximum is the smallest index) until no frame
    is active."""
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    nb = np.zeros((n, n), dtype=bool)
    nb[upper] = d[upper] <= cutoff
    nb |= nb.T
    np.fill_diagonal(nb, True)
    nbf = nb.astype(np.float64)                                      # (counts to 2^53 are exact)
    active = np.ones(n, dtype=bool)
    labels = np.full(n, -1, dtype=np.int32)
    centres, sizes = [], []
    while active.any():
        counts = np.where(active, nbf @ active.astype(np.float64), 0.0)
        c = int(np.argmax(counts))
        members = nb[c] & active
        labels[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        assert sizes[-1] == counts[c]
        active &= ~members
    return labels, np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32)


_cache = {}


def reference_cached(d, cutoff):
    """`reference`, computed once for a (matrix object, cutoff) and shared; the results are read-only."""
    key = (id(d), float(cutoff).hex())
    if key not in _cache:
        out = reference(d, cutoff)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (d, out)                                       # (the matrix is kept: its id stays its own)
    return _cache[key][1]


def distances(points):
    """The Euclidean distance matrix of points (n, k), symmetric with a zero diagonal."""
    diff = points[:, None, :] - points[None, :, :]
    return np.sqrt((diff * diff).sum(axis=2))


def cloud_matrix(n: int, seed: int, blobs: int = 4):
    """Distances between n points scattered around a few centres: clusters of different sizes at a middling cutoff."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-4.0, 4.0, (blobs, 3))
    pts = centres[rng.integers(0, blobs, n)] + rng.normal(0.0, 0.7, (n, 3))
    return distances(pts)


def upper_values(d):
    return d[np.triu_indices(len(d), 1)]


def ring(n: int):
    """Every frame a neighbour of the next and the last of the first at cutoff 1: every count is 3."""
    d = np.full((n, n), 5.0)
    i = np.arange(n)
    d[i, (i + 1) % n] = d[(i + 1) % n, i] = 1.0
    return d


def cliques(sizes, order=None):
    """Disjoint cliques (distance 1 inside, 5 between), frames in the order given."""
    n = sum(sizes)
    group = np.repeat(np.arange(len(sizes)), sizes)
    if order is not None:
        group = group[order]
    return np.where(group[:, None] == group[None, :], 1.0, 5.0), group


def late_tie():
    """Frames 0..4 a clique P, 5..9 a clique Q, 20..39 a clique G, 40..45 neighbours of frame 20 alone; every frame of P
    is a neighbour of 21, every frame of Q of 22 and 23.  At first Q's frames count 7 and P's 6; frame 20 (26) takes G
    and 40..45, and then P and Q tie at 5: P, the smaller index, is next although Q counted more before."""
    n = 70
    nb = np.zeros((n, n), dtype=bool)
    for lo, hi in ((0, 5), (5, 10), (20, 40)):
        nb[lo:hi, lo:hi] = True
    nb[20, 40:46] = nb[40:46, 20] = True
    nb[0:5, 21] = nb[21, 0:5] = True
    nb[5:10, 22] = nb[22, 5:10] = True
    nb[5:10, 23] = nb[23, 5:10] = True
    return np.where(nb, 1.0, 5.0)


def planted(seed: int = 11):
    """(matrix, cutoff, partition): three point clouds of 50 / 30 / 20 frames in a shuffled order, every cloud within a
    ball of radius 0.4 and the centres 10 apart."""
    rng = np.random.default_rng(seed)
    group = rng.permutation(np.repeat(np.arange(3), (50, 30, 20)))
    step = rng.normal(size=(100, 6))
    step *= (0.4 * rng.random(100) / np.linalg.norm(step, axis=1))[:, None]
    pts = 10.0 * np.eye(3, 6)[group] + step
    return distances(pts), 1.0, group


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, matrix, cutoff)]: the smallest shapes at which the kernels can go wrong."""
    out = []
    for n in NS:
        d = cloud_matrix(n, 100 + n)
        v = upper_values(d)
        lo, hi = (v.min(), v.max()) if len(v) else (1.0, 1.0)
        out.append((f"n={n}-middling", d, float(np.median(v)) if len(v) else 1.0))
        out.append((f"n={n}-all-singletons", d, 0.5 * lo))           # n rounds: several looks at the done flags
        out.append((f"n={n}-one-cluster", d, hi))                    # at the largest distance: <=
    d = cloud_matrix(65, 7)
    v = np.sort(upper_values(d))
    out.append(("cutoff-equal-to-a-distance", d, float(v[len(v) // 5])))
    out.append(("cutoff-just-below-that-distance", d, float(np.nextafter(v[len(v) // 5], 0.0))))
    rng = np.random.default_rng(3)
    pts = rng.normal(0.0, 1.0, (44, 3))[rng.integers(0, 44, 130)]    # duplicate frames: distances of exactly 0.0
    z = distances(pts)
    assert (upper_values(z) == 0.0).sum() > 100
    zm = np.where((z == 0.0) & (rng.random(z.shape) < 0.5), -0.0, z)
    assert np.signbit(upper_values(zm)).any()
    for name, m in (("zeros", z), ("signed-zeros", zm)):
        out.append((f"duplicates-{name}-cutoff-0", m, 0.0))
        out.append((f"duplicates-{name}-cutoff-minus-0", m, -0.0))
    d = cloud_matrix(129, 8)
    out.append(("cutoff-plus-inf", d, np.inf))
    out.append(("cutoff-minus-inf", d, -np.inf))
    out.append(("cutoff-negative", d, -1.0))
    di = d.copy()
    hole = np.random.default_rng(4).random(d.shape) < 0.3
    di[hole | hole.T] = np.inf
    out.append(("inf-entries", di, float(np.median(upper_values(d)))))
    out.append(("inf-entries-cutoff-plus-inf", di, np.inf))
    out.append(("ring-every-count-3", ring(70), 1.0))
    out.append(("two-equal-cliques", cliques((40, 40))[0], 1.0))
    out.append(("two-equal-cliques-interleaved", cliques((40, 40), np.random.default_rng(5).permutation(80))[0], 1.0))
    out.append(("tie-after-the-first-removal", late_tie(), 1.0))
    d = cloud_matrix(129, 9)
    cut = float(np.median(upper_values(d)))
    lower = np.tril(np.ones(d.shape, dtype=bool), -1)
    dn = d.copy()
    dn[lower] = np.nan
    np.fill_diagonal(dn, np.nan)
    out.append(("lower-triangle-and-diagonal-NaN", dn, cut))
    dc = d.copy()
    dc[lower] = np.where(d[lower] <= cut, 9.0, 0.0)                  # the lower triangle says the opposite
    np.fill_diagonal(dc, 99.0)
    out.append(("lower-triangle-contradicts", dc, cut))
    out.append(("upper-triangle-of-those", np.triu(d, 1), cut))
    p, pc, _ = planted()
    out.append(("planted-conformers", p, pc))
    return out


def call_cases():
    """Jobs (matrix, cutoff) of one call: five cutoffs over one matrix, around a job on another matrix and a job
    without frames."""
    a, b = cloud_matrix(257, 21), cloud_matrix(70, 22)
    va = upper_values(a)
    return [(a, float(np.quantile(va, 0.05))), (a, float(np.quantile(va, 0.3))), (b, float(np.median(upper_values(b)))),
            (a, float(va.min() * 0.5)), (np.zeros((0, 0)), 1.0), (a, float(va.max())), (a, float(np.quantile(va, 0.6)))]


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    return [(cloud_matrix(200, 31), 2.0), (cloud_matrix(33, 32), 0.1)]


def pack(jobs, hole: int = 0):
    """(CLUSTER_JOB_DTYPE array, dist) of a list of (matrix, cutoff).  A job with frames gets its entries one job after
    the other, `hole` entries that nobody owns in front of each; a matrix that several jobs hold (the same object) is
    stored once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.CLUSTER_JOB_DTYPE)
    parts, where, at, out = [], {}, 0, 0
    for k, (d, cutoff) in enumerate(jobs):
        n = len(d)
        if id(d) not in where:
            where[id(d)] = at
            parts.append(np.asarray(d, dtype=np.float64).reshape(-1))
            at += n * n
        out += hole if n else 0
        rec[k] = (where[id(d)], n, cutoff, out)
        out += n
    return rec, np.concatenate(parts) if parts else np.zeros(0)


def expected(jobs, hole: int = 0):
    """(labels, centres, sizes, n_clusters) in the layout of `pack`, SENTINEL where nobody writes."""
    rec, _ = pack(jobs, hole)
    size = int((rec["out_first"] + rec["n"]).max()) if len(rec) else 0
    labels, centres, sizes = (np.full(size, SENTINEL, dtype=np.int32) for _ in range(3))
    found = np.zeros(len(jobs), dtype=np.int64)
    for k, (d, cutoff) in enumerate(jobs):
        n, at = len(d), int(rec["out_first"][k])
        if n == 0:
            continue
        lab, cen, siz = reference_cached(d, cutoff)
        labels[at:at + n] = lab
        centres[at:at + n] = -1
        sizes[at:at + n] = 0
        centres[at:at + len(cen)] = cen
        sizes[at:at + len(siz)] = siz
        found[k] = len(cen)
    return labels, centres, sizes, found


def raw(ctx, rec, dist, workspace_bytes=None, rounds_per_check=0, n_dist=None, timed=False):
    """pw_cluster_gromos through ctypes into SENTINEL-filled arrays, or through the library's test entry when
    `workspace_bytes` is given (0: the default budget).  Returns (rc, (labels, centres, sizes, n_clusters)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.pw_internal_cluster_gromos.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, i64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.CLUSTER_JOB_DTYPE)
    d = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
    ok = rec[(rec["n"] >= 0) & (rec["n"] <= _lib.CLUSTER_MAX_N) & (rec["out_first"] >= 0)]
    size = int((ok["out_first"] + ok["n"]).max()) if len(ok) else 0
    labels, centres, sizes = (np.full(size, SENTINEL, dtype=np.int32) for _ in range(3))
    found = np.full(len(rec), SENTINEL, dtype=np.int64)
    ms = ctypes.c_float(0.0)
    n_dist = len(d) if n_dist is None else n_dist
    if workspace_bytes is None:
        rc = L.pw_cluster_gromos(ctx._h, rec.ctypes.data, len(rec), d.ctypes.data, n_dist, labels.ctypes.data,
                                 centres.ctypes.data, sizes.ctypes.data, found.ctypes.data)
    else:
        rc = L.pw_internal_cluster_gromos(ctx._h, rec.ctypes.data, len(rec), d.ctypes.data, n_dist, labels.ctypes.data,
                                          centres.ctypes.data, sizes.ctypes.data, found.ctypes.data, int(workspace_bytes),
                                          int(rounds_per_check), ctypes.byref(ms) if timed else None)
    out = (labels, centres, sizes, found)
    return (rc, out, ms.value) if timed else (rc, out)


def same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
                                         for g, w in zip(got, want))
