"""Inputs shared by tests/test_corr.py (host path, against a long-double sum, numpy and the definition itself) and
tests/test_gpu_corr.py (device against host path, bit for bit): lagged sums of a time correlation (pw_corr_sums)."""
import numpy as np

from _kde_cases import ROOT

EPS = 2.0 ** -53
LD = np.longdouble


def source_constant(name: str) -> int:
    import re

    text = (ROOT / "pywindow_amd" / "csrc" / "pw_corr.hpp").read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


def ar1(n: int, phi: float, seed: int, offset: float = 0.0):
    """A stationary AR(1) series x[t] = phi x[t - 1] + e[t] of unit variance, plus `offset`."""
    from scipy import signal

    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n) * np.sqrt(1.0 - phi * phi)
    e[0] = rng.standard_normal()
    return signal.lfilter([1.0], [1.0, -phi], e) + offset


def centred(x):
    return x - np.sum(x) / len(x)


def accuracy_cases():
    """(name, a, b, n_lags): a and b finite float64 series of one length; b is a itself for the autocorrelations."""
    out = []
    for n, lags in ((1000, 500), (100_000, 64), (400_000, 16)):
        x = centred(ar1(n, 0.95, n))
        out.append((f"ar1-0.95-{n}x{lags}", x, x, lags))
        y = centred(ar1(n, 0.5, n + 1, offset=1e3))             # the offset is there before centring
        out.append((f"ar1-0.5-offset-{n}x{lags}", y, y, lags))
        out.append((f"cross-{n}x{lags}", x, y, lags))
    t = np.arange(2000)
    c = np.cos(2.0 * np.pi * t / 50.0)
    out.append(("cosine-50", c, c, 1000))
    rng = np.random.default_rng(150)
    big = rng.standard_normal(1000) * 1e150                     # a term is at most ~2e301, a sum of 1000 below 1.8e308
    out.append(("scale-1e150", big, big[::-1].copy(), 500))
    small = rng.standard_normal(1000) * 1e-150                  # a term is ~1e-300: normal
    out.append(("scale-1e-150", small, small, 500))
    for n in (1, 2, 511, 512, 513, 1025):                       # chunk edges, empty last chunks
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        out.append((f"edges-{n}", a, b, n))
    return out


def mixed_batch():
    """64 jobs of mixed sizes around the chunk length and the tile width, n = 0 included, every third one with a sharing
    storage with b: (a, b or None, n_lags)."""
    chunk, tile = source_constant("CORR_CHUNK"), source_constant("CORR_WAVE") * source_constant("CORR_LANE_LAGS")
    assert (chunk, tile) == (512, 512)
    rng = np.random.default_rng(77)
    ns = [0, 1, 2, 7, 8, 9, 63, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 5, 1500, 17, 700]
    jobs = []
    for k in range(64):
        n = ns[(k * 5 + k // 16) % len(ns)]
        lags = 0 if n == 0 else [1, n, (n + 1) // 2, min(n, 9), max(1, n - 1)][k % 5]
        a = rng.standard_normal(n) * (1.0 + k)
        jobs.append((a, None if k % 3 == 0 else rng.standard_normal(n), lags))
    return jobs


def pack(jobs):
    """(CORR_JOB_DTYPE array, series) of a list of (a, b or None for a itself, n_lags); outputs one after the other."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.CORR_JOB_DTYPE)
    parts, at, out = [], 0, 0
    for k, (a, b, lags) in enumerate(jobs):
        a = np.asarray(a, dtype=np.float64)
        rec[k]["n"], rec[k]["n_lags"], rec[k]["out_first"], rec[k]["a_first"] = len(a), lags, out, at
        parts.append(a)
        at += len(a)
        if b is None or b is a:
            rec[k]["b_first"] = rec[k]["a_first"]
        else:
            rec[k]["b_first"] = at
            parts.append(np.asarray(b, dtype=np.float64))
            at += len(a)
        out += lags
    return rec, np.concatenate(parts) if parts else np.zeros(0)


def internal_sums(ctx, rec, series, workspace_bytes: int = 0, timed: bool = False):
    """pw_corr_sums through the library's test entry: the budget of the partial sums given (0: the default), and the
    kernels' time by HIP events when `timed` -- returns sums, or (sums, kernel ms)."""
    import ctypes

    from pywindow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_corr_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.CORR_JOB_DTYPE)
    x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
    sums = np.zeros(int((rec["out_first"] + rec["n_lags"]).max()) if len(rec) else 0)
    ms = ctypes.c_float(0.0)
    rc = L.pw_internal_corr_sums(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, sums.ctypes.data, int(workspace_bytes),
                                 ctypes.byref(ms) if timed else None)
    assert rc == 0, L.pw_last_error()
    return (sums, ms.value) if timed else sums


def long_double_sums(a, b, lags):
    """(S[k] summed in long double, sum of |terms| of lag k) for k < lags."""
    assert np.finfo(LD).nmant >= 63
    al, bl = a.astype(LD), b.astype(LD)
    n = len(a)
    truth, weight = np.zeros(lags, dtype=LD), np.zeros(lags, dtype=LD)
    for k in range(lags):
        terms = al[:n - k] * bl[k:]
        truth[k], weight[k] = np.sum(terms), np.sum(np.abs(terms))
    return truth, weight


def derived_bound(n, lags, weight):
    """One rounding per FMA of a chunk, one per chunk addition, 2 for the second-order terms."""
    chunk = source_constant("CORR_CHUNK")
    chunks = -(-(n - np.arange(lags)) // chunk)
    return (chunk + chunks + 2) * EPS * weight.astype(np.float64)
