"""Inputs shared by tests/test_kde2.py (host path, against SciPy and a long-double sum) and
tests/test_gpu_kde2.py (device against host path, bit for bit): joint (two-quantity) Gaussian KDE."""
import numpy as np

from _kde_cases import BW_METHODS, source_constant  # noqa: F401
from _util import GOLDEN


def correlated(n: int, rho: float, seed: int, mean=(7.2, 21.0), scale=(0.6, 1.5)):
    """n pairs of normals with correlation rho."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    return mean[0] + scale[0] * a, mean[1] + scale[1] * (rho * a + np.sqrt(1.0 - rho * rho) * b)


def axis(v, m, pad):
    return np.linspace(v.min() - pad, v.max() + pad, m)


def scipy_cases():
    """(name, samples_x, samples_y, x axis, y axis)."""
    g = np.load(GOLDEN / "md20.npz")
    x, y = np.array(g["pore_opt_d"], dtype=np.float64), np.array(g["maxd"], dtype=np.float64)
    out = [("cc3-pore_opt-maxd", x, y, axis(x, 32, 1.0), axis(y, 32, 1.0))]
    for name, n, rho, m in (("rho0.8-4000", 4000, 0.8, 48), ("rho0.999-4000", 4000, 0.999, 48), ("rho-0.5-10", 10, -0.5, 48),
                            ("rho0.8-400000", 400000, 0.8, 8)):
        x, y = correlated(n, rho, n + int(1000 * abs(rho)))
        out.append((name, x, y, axis(x, m, 1.0), axis(y, m, 1.0)))
    # axes of scale 1e-3 and 1e3, both at offset 1e5
    x, y = correlated(4000, 0.8, 77, mean=(1e5, 1e5), scale=(1e-3, 1e3))
    out.append(("scales-1e-3-1e3-at-1e5", x, y, axis(x, 48, 1e-3), axis(y, 48, 1e3)))
    # a mesh far beyond the samples (every bandwidth factor used here is below 1)
    x, y = correlated(4000, 0.8, 78)
    out.append(("far-tails", x, y, axis(x, 48, 60.0 * x.std(ddof=1)), axis(y, 48, 60.0 * y.std(ddof=1))))
    return out


def mesh_points(ax, ay):
    """(nx * ny, 2): point iy * nx + ix is (ax[ix], ay[iy])."""
    return np.stack([np.tile(ax, len(ay)), np.repeat(ay, len(ax))], axis=1)


def whitening(covariance):
    """(w00, w10, w11), root of the determinant: the definition written out once more, independent of the package."""
    l00 = np.sqrt(covariance[0, 0])
    l10 = covariance[1, 0] / l00
    l11 = np.sqrt(covariance[1, 1] - l10 * l10)
    return (1.0 / l00, -l10 / (l00 * l11), 1.0 / l11), l00 * l11


def mixed_batch():
    """64 small jobs with n around the chunk length and m around the tile width and the wave width, n = 0 / 1 and
    m = 1 included; arbitrary point lists, not meshes: (samples (n, 2), points (m, 2), (w00, w10, w11))."""
    chunk, tile = source_constant("KDE_CHUNK"), source_constant("KDE_WAVE") * source_constant("KDE2_LANE_POINTS")
    assert (chunk, tile) == (512, 128)
    rng = np.random.default_rng(642)
    ns = [0, 1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3, 17]
    ms = [1, 2, tile - 1, tile, tile + 1, 63, 64, 65, 2 * tile + 1, 5]
    jobs = []
    for k in range(64):
        n, m = ns[k % len(ns)], ms[(k // 3 + k) % len(ms)]
        xy = rng.normal((5.0 + 0.1 * k, -2.0), (0.5 + 0.01 * k, 0.3), (n, 2))
        pts = np.stack([np.linspace(2.0, 9.0 + 0.1 * k, m), rng.uniform(-3.5, -0.5, m)], axis=1)
        jobs.append((xy, pts, (1.0 / (0.05 + 0.01 * k), rng.uniform(-3.0, 3.0), 1.0 / (0.04 + 0.005 * k))))
    return jobs


def pack(jobs):
    """(KDE2_JOB_DTYPE array, samples (N, 2), points (M, 2)) of a list of (samples, points, (w00, w10, w11))."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.KDE2_JOB_DTYPE)
    rec["n_samples"] = [len(j[0]) for j in jobs]
    rec["n_points"] = [len(j[1]) for j in jobs]
    rec["sample_first"] = np.cumsum(rec["n_samples"]) - rec["n_samples"]
    rec["point_first"] = np.cumsum(rec["n_points"]) - rec["n_points"]
    for col, name in enumerate(("w00", "w10", "w11")):
        rec[name] = [j[2][col] for j in jobs]
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in parts]) if parts else np.zeros((0, 2))
    return rec, cat([j[0] for j in jobs]), cat([j[1] for j in jobs])


def numpy_sums(xy, pts, w):
    """The definition in plain NumPy doubles (np.exp, any order of the sum)."""
    dx = pts[:, None, 0] - xy[None, :, 0]
    dy = pts[:, None, 1] - xy[None, :, 1]
    z0 = dx * w[0]
    z1 = dx * w[1] + dy * w[2]
    return np.exp(-0.5 * (z0 * z0 + z1 * z1)).sum(axis=1)


def internal_sums(ctx, rec, samples, points, workspace_bytes: int = 0, timed: bool = False):
    """pw_kde2_sums through the library's test entry: the budget of the partial sums given (0: the default), and the
    kernels' time by HIP events when `timed` -- returns sums, or (sums, kernel ms)."""
    import ctypes

    from pywindow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_kde2_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.KDE2_JOB_DTYPE)
    x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, 2)
    g = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    sums = np.zeros(len(g))
    ms = ctypes.c_float(0.0)
    rc = L.pw_internal_kde2_sums(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, g.ctypes.data, sums.ctypes.data,
                                 int(workspace_bytes), ctypes.byref(ms) if timed else None)
    assert rc == 0, L.pw_last_error()
    return (sums, ms.value) if timed else sums
