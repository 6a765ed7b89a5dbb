"""Case list and references of the superposition tests (tests/test_superpose.py, tests/test_gpu_superpose.py).
numpy only, seeded.  Three references that owe nothing to pywindow_amd/csrc/pw_*.hpp:

  (i)   kabsch:  float64 SVD Kabsch with the reflection fix, RMSD as a direct residual sum;
  (ii)  horn:    float64 Horn quaternion through numpy.linalg.eigh -- also the judge of conditioning,
                 gap = (lambda_1 - lambda_2) / lambda_1;
  (iii) truth:   long double throughout -- sums, Horn's matrix, a cyclic Jacobi of its own, the residual sum.

The shapes are where a strided loop over 64 accumulators, the fold across the lanes and the lane-a-job solve can go
wrong: n around one, two and many multiples of 64, batches around 64 jobs."""
import ctypes
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "the truth of these tests needs a long double of 64 bits of mantissa or more"

SIZES = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 168, 4097)
BATCHES = (1, 63, 64, 65, 257)
#: below this relative gap of Horn's two largest eigenvalues the rotation is not compared (the RMSD always is)
WELL_CONDITIONED = 1e-3
#: what the rows of a result hold before a call where a test looks at rows nobody owns
SENTINEL = 0x5A


def rotation_matrix(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def random_rotation(rng):
    return rotation_matrix(rng.standard_normal(3), rng.uniform(0.2, 2.9))


def moved(x, R, t=(0.0, 0.0, 0.0), noise=0.0, rng=None):
    y = x @ R.T + np.asarray(t, dtype=np.float64)
    if noise:
        y = y + noise * rng.standard_normal(x.shape)
    return y


@functools.lru_cache(maxsize=None)
def cases():
    """((name, mobile (n, 3), target (n, 3), weights (n) | None), ...)"""
    rng = np.random.default_rng(20261018)
    out = []
    for n in SIZES:                                   # a random rotation, a shift and thermal noise at every size
        x = 5.0 * rng.standard_normal((n, 3))
        out.append((f"random n={n}", x, moved(x, random_rotation(rng), rng.uniform(-3, 3, 3), 0.05, rng), None))
    cage = 5.0 * rng.standard_normal((168, 3))
    mass = rng.choice([1.008, 12.011, 14.007, 15.999], 168)
    axis = rng.standard_normal(3)
    x65, x129, x127, x64 = cage[:65], cage[:129], cage[:127], cage[:64]
    out += [
        ("by 180 degrees n=65", x65, moved(x65, rotation_matrix(axis, np.pi), noise=0.01, rng=rng), None),
        ("by nearly 180 degrees n=168", cage, moved(cage, rotation_matrix(axis, np.pi - 1e-9), noise=1e-3, rng=rng), None),
        ("identical n=168", cage, cage.copy(), None),
        ("identical, weighted n=129", x129, x129.copy(), mass[:129]),
        ("mirror image n=168", cage, moved(cage * np.array([1.0, 1.0, -1.0]), random_rotation(rng)), None),
        ("offsets of 1e3 n=127", x127 + 1e3, moved(x127, random_rotation(rng), (-1e3, 2e3, 1e3), 0.05, rng), None),
        ("offsets of 1e3, masses n=168", cage + np.array([1e3, -1e3, 1e3]),
         moved(cage, random_rotation(rng), (1e3, 1e3, -1e3), 0.05, rng), mass),
        ("weights with zeros n=65", x65, moved(x65, random_rotation(rng), (1, 2, 3), 0.05, rng),
         np.where(np.arange(65) % 3 == 0, 0.0, mass[:65])),
        ("one weight not zero n=4", cage[:4], moved(cage[:4], random_rotation(rng), (1, 2, 3), 0.05, rng),
         np.array([0.0, 0.0, 2.5, 0.0])),
        ("weights all 1.0 n=168", cage, moved(cage, random_rotation(rng), (1, 2, 3), 0.05, rng), np.ones(168)),
        ("weights all 12.011 n=168", cage, moved(cage, random_rotation(rng), (1, 2, 3), 0.05, rng), np.full(168, 12.011)),
        ("masses n=168", cage, moved(cage, random_rotation(rng), (1, 2, 3), 0.1, rng), mass),
        ("noise of 1e-8 n=168", cage, moved(cage, random_rotation(rng), (1, 2, 3), 1e-8, rng), None),
        ("noise of 1e-8 n=64", x64, moved(x64, random_rotation(rng), (1, 2, 3), 1e-8, rng), None),
        ("large noise n=128", cage[:128], 5.0 * rng.standard_normal((128, 3)), None),
        ("collinear n=63", np.outer(rng.standard_normal(63), [1.0, 2.0, -1.0]),
         moved(np.outer(rng.standard_normal(63), [1.0, 2.0, -1.0]), random_rotation(rng), (1, 2, 3), 0.0, rng), None),
        ("planar n=64", x64 * np.array([1.0, 1.0, 0.0]), moved(x64 * np.array([1.0, 1.0, 0.0]), random_rotation(rng),
                                                            (1, 2, 3), 0.02, rng), None),
    ]
    return tuple((name, np.ascontiguousarray(x), np.ascontiguousarray(y), None if w is None else np.ascontiguousarray(w))
                 for name, x, y, w in out)


def batch(count):
    """`count` jobs cycling through the case list."""
    c = cases()
    return [c[k % len(c)][1:] for k in range(count)]


def pack(items, hole=0):
    """(jobs, xyz, weights) of a call: every item's mobile and target rows one after another, weights alongside (an
    entry per row of xyz); `hole` rows of the result nobody owns in front of every job's row."""
    from pywindow_amd import _lib

    xyz, wts, jobs = [], [], []
    at = 0
    for k, (x, y, w) in enumerate(items):
        n = len(x)
        jobs.append((at, at + n, -1 if w is None else at, n, k * (hole + 1) + hole))
        xyz += [x, y]
        wts += [np.zeros(n) if w is None else w, np.zeros(n)]
        at += 2 * n
    rec = np.array(jobs, dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    return rec, np.concatenate(xyz), np.concatenate(wts)


def raw(ctx, rec, xyz, weights, out=None, workspace_bytes=None, n_points=None, timed=False):
    """pw_superpose through ctypes into rows of the caller (`out` None: every byte SENTINEL), or through the library's
    test entry when `workspace_bytes` is given (0: the default budget; with `timed` the kernels' time by HIP events as
    well).  Returns (rc, rows[, kernel ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.pw_internal_superpose.argtypes = [vp, vp, i64, vp, vp, i64, vp, i64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if out is None:
        rows = int(rec["out"].max()) + 1 if len(rec) and (rec["out"] >= 0).all() else 4
        out = np.frombuffer(bytearray([SENTINEL]) * (rows * _lib.SUPERPOSE_OUT_DTYPE.itemsize), dtype=_lib.SUPERPOSE_OUT_DTYPE).copy()
    wp = None if w is None else w.ctypes.data
    n_points = len(x) if n_points is None else n_points
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None:
        rc = L.pw_superpose(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, wp, n_points, out.ctypes.data)
    else:
        rc = L.pw_internal_superpose(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, wp, n_points, out.ctypes.data,
                                     int(workspace_bytes), ctypes.byref(ms) if timed else None)
    return (rc, out, float(ms.value)) if timed else (rc, out)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(rows):
    """Which rows still hold the SENTINEL in every byte."""
    return (rows.view(np.uint8).reshape(len(rows), -1) == SENTINEL).all(axis=1)


# ---- references --------------------------------------------------------------------------------------------
def _weights(x, w, dtype=np.float64):
    return np.ones(len(x), dtype=dtype) if w is None else np.asarray(w, dtype=dtype)


def kabsch(x, y, w=None):
    """(i): (R, rmsd), float64 SVD."""
    w = _weights(x, w)
    W = w.sum()
    dx = x - (w[:, None] * x).sum(axis=0) / W
    dy = y - (w[:, None] * y).sum(axis=0) / W
    U, _, Vt = np.linalg.svd((dx * w[:, None]).T @ dy)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    return R, float(np.sqrt((w * ((dx @ R.T - dy) ** 2).sum(axis=1)).sum() / W))


def horn_matrix(M):
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = [M[a, b] for a in range(3) for b in range(3)]
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy]], dtype=M.dtype)


def quaternion_rotation(q):
    q0, qx, qy, qz = q
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                     [2 * (qx * qy + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                     [2 * (qx * qz - q0 * qy), 2 * (qy * qz + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]], dtype=q.dtype)


def horn(x, y, w=None):
    """(ii): (R, rmsd, relative gap of the two largest eigenvalues), float64 eigh."""
    w = _weights(x, w)
    W = w.sum()
    dx = x - (w[:, None] * x).sum(axis=0) / W
    dy = y - (w[:, None] * y).sum(axis=0) / W
    lam, vec = np.linalg.eigh(horn_matrix((dx * w[:, None]).T @ dy))
    R = quaternion_rotation(vec[:, -1] / np.sqrt((vec[:, -1] ** 2).sum()))
    gap = (lam[-1] - lam[-2]) / lam[-1] if lam[-1] > 0 else 0.0
    return R, float(np.sqrt((w * ((dx @ R.T - dy) ** 2).sum(axis=1)).sum() / W)), float(gap)


def _jacobi_ld(A):
    """Cyclic Jacobi on a symmetric 4 x 4 of long doubles: (eigenvalues, eigenvectors in columns)."""
    a = A.copy()
    v = np.eye(4, dtype=LD)
    one = LD(1)
    for _ in range(60):
        off = sum(abs(a[p, q]) for p in range(4) for q in range(p + 1, 4))
        if off == 0 or off <= LD(1e-45) * sum(abs(a[p, p]) for p in range(4)):
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if a[p, q] == 0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                G = np.eye(4, dtype=LD)
                G[p, p] = G[q, q] = c
                G[p, q], G[q, p] = s, -s
                a = G.T @ a @ G
                a[p, q] = a[q, p] = 0
                v = v @ G
    return np.diag(a).copy(), v


def _truth(x, y, w):
    x, y, w = x.astype(LD), y.astype(LD), _weights(x, w, LD)
    W = w.sum()
    dx = x - (w[:, None] * x).sum(axis=0) / W
    dy = y - (w[:, None] * y).sum(axis=0) / W
    M = np.array([[(w * (dx[:, a] * dy[:, b])).sum() for b in range(3)] for a in range(3)], dtype=LD)
    lam, vec = _jacobi_ld(horn_matrix(M))
    k = int(np.argmax(lam))
    q = vec[:, k] / np.sqrt((vec[:, k] ** 2).sum())
    R = quaternion_rotation(q)
    rmsd = np.sqrt((w * ((dx @ R.T - dy) ** 2).sum(axis=1)).sum() / W)
    return R, rmsd


@functools.lru_cache(maxsize=None)
def references():
    """{name: dict(kabsch=(R, rmsd), horn=(R, rmsd, gap), truth=(R long double, rmsd long double))}, computed once."""
    return {name: {"kabsch": kabsch(x, y, w), "horn": horn(x, y, w), "truth": _truth(x, y, w)} for name, x, y, w in cases()}
