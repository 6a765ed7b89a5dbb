"""Inputs shared by tests/test_kdew.py (host path: the definition, SciPy, a long-double sum, the bootstrap band) and
tests/test_gpu_kdew.py (device against host path, bit for bit)."""
import ctypes
from fractions import Fraction

import numpy as np

import _kde_cases as K

LD = np.longdouble
EPS = 2.0 ** -53


def tile() -> int:
    """Grid points of one work item of the device kernel."""
    return K.source_constant("KDE_WAVE") * K.source_constant("KDEW_LANE_POINTS")


def replica_tile() -> int:
    return K.source_constant("KDEW_REPLICAS")


def edge_weights(rng, n: int, replicas: int) -> np.ndarray:
    """(replicas, n) weights that mix exact zeros, integer multiplicities and magnitudes from 1e-150 to 1e150."""
    w = np.empty((replicas, n))
    for b in range(replicas):
        kind = b % 4
        if kind == 0:
            w[b] = rng.integers(0, 4, n)                        # bootstrap counts, zeros among them
        elif kind == 1:
            w[b] = 10.0 ** rng.uniform(-150.0, 150.0, n)
        elif kind == 2:
            w[b] = rng.random(n) * (rng.random(n) < 0.7)        # exact zeros among ordinary weights
        else:
            w[b] = 1.0
    return w


def edge_jobs():
    """Every (n, m, R) of n in {0, 1, 511, 512, 513, 1025} x five m x five R would be 150 jobs; the tail paths of the
    chunk, the point tile and the replica tile are independent of one another, so every value of each axis appears
    with at least two values of the others: (samples, points, weights (R, n), inv_bandwidth)."""
    chunk, T, RT = K.source_constant("KDE_CHUNK"), tile(), replica_tile()
    ns = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    ms = [1, T - 1, T, T + 1, 2 * T + 1]
    rs = [1, RT - 1, RT, RT + 1, 2 * RT + 1]
    rng = np.random.default_rng(77)
    jobs = []
    for k in range(30):
        n, m, r = ns[k % 6], ms[(k + k // 6) % 5], rs[(2 * k + k // 5) % 5]
        x = rng.normal(5.0, 0.6, n)
        jobs.append((x, np.linspace(2.5, 7.5, m), edge_weights(rng, n, r), 1.0 / (0.08 + 0.01 * k)))
    assert {len(j[0]) for j in jobs} == set(ns) and {len(j[1]) for j in jobs} == set(ms)
    assert {j[2].shape[0] for j in jobs} == set(rs)
    return jobs


def pack(jobs):
    """(KDEW_JOB_DTYPE array, samples, points, weights sample-major) of a list of (samples, points, weights (R, n),
    inv_bandwidth)."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.KDEW_JOB_DTYPE)
    rec["n_samples"] = [len(j[0]) for j in jobs]
    rec["n_points"] = [len(j[1]) for j in jobs]
    rec["n_replicas"] = [np.shape(j[2])[0] for j in jobs]
    rec["sample_first"] = np.cumsum(rec["n_samples"]) - rec["n_samples"]
    rec["point_first"] = np.cumsum(rec["n_points"]) - rec["n_points"]
    size = rec["n_samples"] * rec["n_replicas"]
    rec["weight_first"] = np.cumsum(size) - size
    size = rec["n_points"] * rec["n_replicas"]
    rec["out_first"] = np.cumsum(size) - size
    rec["inv_bandwidth"] = [j[3] for j in jobs]
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in parts]) if parts else np.zeros(0)
    return rec, cat([j[0] for j in jobs]), cat([j[1] for j in jobs]), cat([np.ascontiguousarray(np.asarray(j[2], dtype=np.float64).T) for j in jobs])


def unpack(rec, sums):
    """The (R, m) sums of every job."""
    out = []
    for j in rec:
        first, r, m = int(j["out_first"]), int(j["n_replicas"]), int(j["n_points"])
        out.append(sums[first:first + r * m].reshape(r, m))
    return out


def internal_wsums(ctx, rec, x, g, w, workspace_bytes: int = 0, timed: bool = False):
    """pw_kde_wsums through the library's hook with the budget of the partial sums given: the sums, and the
    kernels' milliseconds when `timed`."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_kde_wsums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.KDEW_JOB_DTYPE)
    x, g, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, g, w))
    sums = np.zeros(int((rec["out_first"] + rec["n_replicas"] * rec["n_points"]).max()) if len(rec) else 0)
    ms = ctypes.c_float(0.0)
    rc = L.pw_internal_kde_wsums(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, g.ctypes.data, w.ctypes.data,
                                 sums.ctypes.data, int(workspace_bytes), ctypes.byref(ms) if timed else None)
    assert rc == 0, L.pw_last_error()
    return (sums, float(ms.value)) if timed else sums


def fma(a: float, b: float, c: float) -> float:
    """round(a * b + c) with ONE rounding: exact rationals, and float() of a Fraction rounds to nearest even."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def restated(ctx, x, g, w, r):
    """The definition of pw_kde.hpp in plain Python, operation by operation: (R, m) sums.  The terms are kde_term's
    (numpy rounds each operation as the C source does; pw_exp comes from the library's element-wise entry)."""
    chunk = K.source_constant("KDE_CHUNK")
    x, g, w = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.zeros((w.shape[0], len(g)))
    for j, gj in enumerate(g):
        z = (gj - x) * r
        t = z * z
        term = K.internal_exp(ctx, -0.5 * t) if len(x) else np.zeros(0)
        for b in range(w.shape[0]):
            s = 0.0
            for c0 in range(0, len(x), chunk):
                p = 0.0
                for i in range(c0, min(c0 + chunk, len(x))):
                    p = fma(float(w[b, i]), float(term[i]), p)
                s = p if c0 == 0 else s + p
            out[b, j] = s
    return out


def long_double_wsums(x, g, w, r):
    """(sum_i w[b][i] exp(-0.5 ((g - x_i) r)^2), the same with |.| -- the weights are not negative, so itself) in
    long double, r a long double: (R, m)."""
    xl, wl = np.asarray(x).astype(LD), np.asarray(w).astype(LD)
    out = np.zeros((wl.shape[0], len(g)), dtype=LD)
    for j, gj in enumerate(np.asarray(g).astype(LD)):
        z = (gj - xl) * r
        out[:, j] = (wl * np.exp(LD(-0.5) * z * z)[None, :]).sum(axis=1)
    return out


def ar1_store(n: int, phi: float, seed: int):
    """A store of n frames, one unit a frame, whose pore diameter is an AR(1) series."""
    import _corr_cases as C
    from pywindow_amd import _lib, records

    recs = np.zeros(n, dtype=_lib.UNIT_OUT_DTYPE)
    recs["pore_d"] = 6.0 + 0.3 * C.ar1(n, phi, seed)
    for k in ("maxd", "avg_d", "pore_vol", "pore_opt_d", "pore_vol_opt"):
        recs[k] = 1.0
    return records.RecordStore(recs, np.arange(n))
