"""Cases and references for pw_covariance and pw_project (tests/test_cov.py, tests/test_gpu_cov.py).  numpy only,
seeded, nothing taken from the library's sources but the two sizes at which its kernels change path: the chunk of rows
(``_lib.COV_CHUNK``) and the width of a device tile (``TILE``).

References of a case:
  (i)   float64, two passes: the transforms applied by numpy, ``Y.mean(0)``, ``Z.T @ Z`` and ``Z @ V.T`` (BLAS);
  (iii) the truth in ``np.longdouble`` with a transform, a mean and sums of its own, and with it the sums of absolute
        values ``sum_t |z_a z_b|`` and ``sum_a |z_a V_a|`` that scale the floors of the bars.

The list holds the smallest shapes at which the kernels can go wrong.  D runs over 1, 2, 3 and one below, at and one
above TILE and 2 TILE at T = CHUNK + 1; T runs over 1, 2, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 at D = 3 and
D = TILE + 1; the corner (2 CHUNK + 1) x (2 TILE + 1) closes the list.  Transforms need a D that is a multiple of 3, so
the shapes with transforms take the multiples of 3 next to the same edges (126, 129, 255, 258)."""
import functools

import numpy as np

from pywindow_amd import _lib

LD = np.longdouble
CHUNK = _lib.COV_CHUNK
TILE = 128                       # the device's square tile of S (pw_cov.hip)
BATCHES = (1, 63, 64, 65, 257)
SENTINEL = np.uint64(0x7FF8DEADBEEF0001)     # a NaN no sum produces

D_PLAIN = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)
D_MOVED = (3, TILE - 2, TILE + 1, 2 * TILE - 1, 2 * TILE + 2)
T_EDGES = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)


def random_rotation(rng) -> np.ndarray:
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def transforms(rng, T: int, spread: float = 3.0) -> np.ndarray:
    """T arbitrary rigid transforms as rows of pw_superpose (fields the entries do not read hold garbage)."""
    tr = np.zeros(T, dtype=_lib.SUPERPOSE_OUT_DTYPE)
    for t in range(T):
        tr[t]["rotation"] = random_rotation(rng)
    tr["centre_mobile"] = spread * rng.standard_normal((T, 3))
    tr["centre_target"] = spread * rng.standard_normal((T, 3))
    tr["rmsd"], tr["lambda"], tr["sweeps"], tr["reserved"] = np.nan, np.inf, -7, 99
    return tr


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, X (T, D), transforms | None, scatter wanted)]"""
    rng = np.random.default_rng(20240607)
    out = []

    def add(name, X, tr=None, scatter=True):
        X = np.ascontiguousarray(X, dtype=np.float64)
        X.setflags(write=False)
        out.append((name, X, tr, scatter))

    def shape(T, D, moved):
        add(f"T={T} D={D}" + (" moved" if moved else ""), 2.0 * rng.standard_normal((T, D)) + rng.uniform(-5, 5, D),
            transforms(rng, T) if moved else None)

    for D in D_PLAIN:
        shape(CHUNK + 1, D, False)
    for D in D_MOVED:
        shape(CHUNK + 1, D, True)
    for T in T_EDGES:
        for D, moved in ((3, False), (3, True), (TILE + 1, False), (TILE + 1, True)):
            if T != CHUNK + 1:
                shape(T, D, moved)
    shape(2 * CHUNK + 1, 2 * TILE + 1, False)
    shape(2 * CHUNK + 1, 2 * TILE + 2, True)
    add("points with one atom T=40", rng.standard_normal((40, 3)), transforms(rng, 40))
    # 2.5 and its multiples up to 2.5 * 300 are exact, so the column's mean is 2.5 and its z exactly 0 on every path
    X = rng.standard_normal((300, 6))
    X[:, 2] = 2.5
    add("a constant column T=300 D=6", X)
    add("magnitude 1e-150 T=4 D=5", 1e-150 * rng.uniform(0.5, 1.0, (4, 5)) * rng.choice([-1.0, 1.0], (4, 5)))
    add("magnitude 1e+150 T=4 D=5", 1e+150 * rng.uniform(0.5, 1.0, (4, 5)) * rng.choice([-1.0, 1.0], (4, 5)))
    add("a mean large against the spread T=300 D=7", 1e6 + 1e-3 * rng.standard_normal((300, 7)))
    add("the mean only T=300 D=9", rng.standard_normal((300, 9)), None, False)
    add("the mean only, moved T=257 D=129", rng.standard_normal((CHUNK + 1, TILE + 1)), transforms(rng, CHUNK + 1), False)
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


def vectors(name, k: int) -> np.ndarray:
    """k seeded unit vectors of a case's D columns."""
    D = case(name)[1].shape[1]
    rng = np.random.default_rng(1000 * D + k)
    V = rng.standard_normal((k, D))
    return V / np.linalg.norm(V, axis=1, keepdims=True)


def moved(X, tr, dtype=np.float64):
    """The values y of a case in ``dtype``, by numpy's own arithmetic."""
    X = np.asarray(X).astype(dtype)
    if tr is None:
        return X
    T, D = X.shape
    R = tr["rotation"].astype(dtype)
    d = X.reshape(T, D // 3, 3) - tr["centre_mobile"].astype(dtype)[:, None, :]
    y = (d[:, :, None, :] * R[:, None, :, :]).sum(axis=3) + tr["centre_target"].astype(dtype)[:, None, :]
    return y.reshape(T, D)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{"mean", "scatter" (reference (i)), "mean_t", "scatter_t", "scatter_abs" (the truth (iii))}; read only."""
    _, X, tr, _ = case(name)
    Y = moved(X, tr)
    m = Y.mean(axis=0)
    Z = Y - m
    Yt = moved(X, tr, LD)
    mt = Yt.sum(axis=0) / LD(len(X))
    Zt = Yt - mt
    ref = {"mean": m, "scatter": Z.T @ Z, "mean_t": mt, "scatter_t": Zt.T @ Zt, "scatter_abs": np.abs(Zt).T @ np.abs(Zt),
           "z_t": Zt, "z": Z}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def projection_reference(name, V, mean):
    """(reference (i), truth, truth's sum of absolute values) of the projections of a case on V with the mean GIVEN."""
    _, X, tr, _ = case(name)
    Z = moved(X, tr) - mean
    Zt = moved(X, tr, LD) - mean.astype(LD)
    Vt = V.astype(LD)
    return Z @ V.T, Zt @ Vt.T, np.abs(Zt) @ np.abs(Vt).T


def held(ours, ref, truth, scale, what):
    """``ours`` within the bar of tests/test_cov.py; returns (largest error of ours) / (its bar)."""
    e_ours = np.abs(ours.astype(LD) - truth).astype(np.float64)
    e_ref = float(np.abs(ref.astype(LD) - truth).max())
    floor = 4.0 * np.spacing(scale.astype(np.float64))
    bar = np.maximum(8.0 * e_ref, floor)
    worst = float((e_ours / np.where(bar > 0, bar, 1.0)).max())
    print(f"{what}: ours {e_ours.max():.3e}  reference (i) {e_ref:.3e}  ours / bar {worst:.3f}")
    assert (e_ours <= bar).all(), what
    return worst


# ---- calls ----------------------------------------------------------------------------------------------------------
def sentinel(n: int) -> np.ndarray:
    return np.full(n, SENTINEL, dtype=np.uint64).view(np.float64)


def untouched(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint64) == SENTINEL


def pack(items, hole: int = 0):
    """``(jobs, data, transforms | None, mean, scatter, spans)`` for ``items`` = [(X, transforms | None, scatter
    wanted)]: every job's inputs one after another, its outputs behind ``hole`` entries nobody owns, the outputs filled
    with the sentinel.  spans[k] = (mean slice, scatter slice | None, D)."""
    jobs = np.zeros(len(items), dtype=_lib.COV_JOB_DTYPE)
    data, rows, spans = [], [], []
    at = row = m_at = s_at = 0
    for k, (X, tr, wanted) in enumerate(items):
        T, D = X.shape
        m_at += hole
        s_at += hole
        jobs[k] = (at, T, D, -1 if tr is None else row, m_at, s_at if wanted else -1)
        spans.append((slice(m_at, m_at + D), slice(s_at, s_at + D * D) if wanted else None, D))
        data.append(X.reshape(-1))
        at += X.size
        m_at += D
        if wanted:
            s_at += D * D
        if tr is not None:
            rows.append(tr)
            row += T
    return (jobs, np.concatenate(data), np.concatenate(rows) if rows else None, sentinel(m_at + hole), sentinel(s_at + hole),
            spans)


def run(ctx, items, hole: int = 0, **hook):
    """[(mean, scatter (D, D) | None)] of ``items`` from ONE call, and the two whole output arrays."""
    jobs, data, tr, mean, scatter, spans = pack(items, hole)
    ctx.covariance(jobs, data, tr, mean=mean, scatter=scatter, **hook)
    return [(mean[m].copy(), None if s is None else scatter[s].reshape(D, D).copy()) for m, s, D in spans], mean, scatter, spans


def one(ctx, name, **hook):
    _, X, tr, wanted = case(name)
    return run(ctx, [(X, tr, wanted)], **hook)[0][0]


def project_batch(ctx, parts, hole: int = 0):
    """[P (T, k)] of ``parts`` = [(X, transforms | None, mean, V (k, D))] from ONE pw_project call, the whole output
    array and every job's slice of it."""
    jobs = np.zeros(len(parts), dtype=_lib.PROJECT_JOB_DTYPE)
    data, rows, means, vecs, spans = [], [], [], [], []
    at = row = m_at = v_at = p_at = 0
    for k, (X, tr, mean, V) in enumerate(parts):
        T, D = X.shape
        p_at += hole
        jobs[k] = (at, T, D, -1 if tr is None else row, m_at, v_at, len(V), p_at)
        spans.append(slice(p_at, p_at + T * len(V)))
        data.append(X.reshape(-1))
        means.append(mean)
        vecs.append(V.reshape(-1))
        at, m_at, v_at, p_at = at + X.size, m_at + D, v_at + V.size, p_at + T * len(V)
        if tr is not None:
            rows.append(tr)
            row += T
    proj = sentinel(p_at + hole)
    ctx.project(jobs, np.concatenate(data), np.concatenate(means), np.concatenate(vecs), np.concatenate(rows) if rows else None,
                proj=proj)
    return [proj[s].reshape(len(X), len(V)).copy() for s, (X, _, _, V) in zip(spans, parts)], proj, spans


def project(ctx, X, tr, mean, V) -> np.ndarray:
    return project_batch(ctx, [(X, tr, mean, V)])[0][0]


def owned(total: int, slices) -> np.ndarray:
    mask = np.zeros(total, dtype=bool)
    for s in slices:
        if s is not None:
            mask[s] = True
    return mask


def small_items(count: int):
    """``count`` small jobs: a few shapes in turn, with and without transforms and the scatter matrix."""
    rng = np.random.default_rng(77)
    shapes = [(1, 1, False, True), (5, 3, True, True), (17, 4, False, True), (2, 6, True, False), (9, 9, True, True),
              (3, 2, False, False), (20, 7, False, True)]
    pool = [(np.ascontiguousarray(rng.standard_normal((T, D))), transforms(rng, T) if mv else None, sc)
            for T, D, mv, sc in shapes]
    return [pool[k % len(pool)] for k in range(count)]


def same(a, b) -> bool:
    return a.shape == b.shape and a.tobytes() == b.tobytes()
