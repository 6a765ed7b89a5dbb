"""Inputs shared by tests/test_dft.py (host path, against the definition, mpmath, a long-double sum, the FFT and SciPy)
and tests/test_gpu_dft.py (device against host path, bit for bit): sums of a spectrum at rational frequencies
(pw_dft_sums)."""
import ctypes
import math

import numpy as np

from _corr_cases import ar1, centred
from _kde_cases import ROOT

EPS = 2.0 ** -53
LD = np.longdouble
CHUNK = 512

#: DERIVED bound of a twiddle's absolute error, in units of 2^-53: the angle 2 pi q' / M, |q' / M| <= 1/2,
#: carries three relative roundings (the division, the constant 6.283185307179586, the product): 3 pi; pw_sincos adds
#: 0.55 ulp of a value of at most 1: 1.1
TWIDDLE_BOUND = 3.0 * math.pi + 1.1
#: DERIVED: both twiddles of a term (2 sqrt 2 twiddle bounds: |cA| + |sA| + |cB| + |sB| <= 2 sqrt 2) and the two roundings of
#: the rotation, rounded up over the second-order terms: 2 sqrt 2 (3 pi + 1.1) + 2 = 31.8
K = 32.0
assert 2.0 * math.sqrt(2.0) * TWIDDLE_BOUND + 2.0 <= K


def source_constant(name: str) -> int:
    import re

    text = (ROOT / "pywindow_amd" / "csrc" / "pw_dft.hpp").read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


def pack(jobs):
    """(DFT_JOB_DTYPE array, series) of a list of (a, period, j_first, j_step, n_freq); outputs one after the other."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.DFT_JOB_DTYPE)
    parts, at, out = [], 0, 0
    for k, (a, period, j_first, j_step, n_freq) in enumerate(jobs):
        a = np.asarray(a, dtype=np.float64)
        rec[k] = (at, len(a), period, j_first, j_step, n_freq, out)
        parts.append(a)
        at += len(a)
        out += n_freq if len(a) else 0
    return rec, np.concatenate(parts) if parts else np.zeros(0)


def internal_sums(ctx, rec, series, workspace_bytes: int = 0, timed: bool = False):
    """pw_dft_sums through the library's test entry: the budget of twiddles and partial sums given (0: the default),
    and the kernels' time by HIP events when `timed` -- returns the complex sums, or (sums, kernel ms)."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_dft_sums.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.DFT_JOB_DTYPE)
    x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
    size = int((rec["out_first"] + rec["n_freq"]).max()) if len(rec) else 0
    re, im = np.zeros(size), np.zeros(size)
    ms = ctypes.c_float(0.0)
    rc = L.pw_internal_dft_sums(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, re.ctypes.data, im.ctypes.data,
                                int(workspace_bytes), ctypes.byref(ms) if timed else None)
    assert rc == 0, L.pw_last_error()
    out = np.empty(size, dtype=np.complex128)
    out.real, out.imag = re, im
    return (out, ms.value) if timed else out


def twiddles(ctx, j: int, period: int, k):
    """(cosines, sines) of the phases of (j, k[i]) as the library defines them, on ctx's device or host."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_dft_twiddles.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_int64, vp, vp]
    k = np.ascontiguousarray(k, dtype=np.int64)
    c, s = np.zeros(len(k)), np.zeros(len(k))
    rc = L.pw_internal_dft_twiddles(ctx._h, int(j), int(period), k.ctypes.data, len(k), c.ctypes.data, s.ctypes.data)
    assert rc == 0
    return c, s


def twiddle_cases():
    """(j, period, k): random, period = 2^31, k near 2^31, the fold at 2 q = M, j = 0 and j = M - 1."""
    rng = np.random.default_rng(31)
    out = []
    for period in (2, 3, 1000, 5201, 80_001, (1 << 31) - 1, 1 << 31):
        for j in sorted({0, 1, period // 2, period - 1, int(rng.integers(0, period)), int(rng.integers(0, period))}):
            k = np.concatenate([rng.integers(0, 1 << 20, 40), rng.integers((1 << 31) - 1000, (1 << 31) + 1, 40),
                                np.arange(0, 8), [511, 512, 513, (1 << 31) - 512, 1 << 31, 1 << 32]])
            out.append((j, period, k.astype(np.int64)))
    return out


def edge_jobs(ns=(1, 2, 511, 512, 513, 1025)):
    """The definition's cases: every n x M in {n, 4 n + 1, 2^31} x j_step in {1, 2}: 5 frequencies with j = 0 (step 1:
    a job of its own), and j = M - 1 as the last of the progression."""
    rng = np.random.default_rng(17)
    jobs = []
    for n in ns:
        a = rng.standard_normal(n)
        for period in (max(n, 2), 4 * n + 1, 1 << 31):
            for step in (1, 2):
                count = min(5, (period - 1) // step + 1)
                jobs.append((a, period, period - 1 - (count - 1) * step, step, count))     # ends at j = M - 1
                jobs.append((a, period, 0, step, count))                                   # starts at j = 0
    return jobs


def accuracy_cases():
    """(name, a, period, j_first, j_step, n_freq), in the style of _corr_cases.accuracy_cases."""
    out = []
    for n, nf in ((1000, 500), (100_000, 64), (400_000, 16)):
        x = centred(ar1(n, 0.95, n))
        out.append((f"ar1-0.95-{n}x{nf}", x, 4 * n, 1, 1, nf))
        y = centred(ar1(n, 0.5, n + 1, offset=1e3))              # the offset is there before centring
        out.append((f"ar1-0.5-offset-{n}x{nf}", y, 4 * n + 1, 3, 2, nf))
    t = np.arange(2000)
    c = np.cos(2.0 * np.pi * t / 50.0)
    out.append(("cosine-50", c, 2000, 0, 1, 1000))
    rng = np.random.default_rng(150)
    out.append(("scale-1e150", rng.standard_normal(1000) * 1e150, 4000, 1, 1, 500))
    out.append(("scale-1e-150", rng.standard_normal(1000) * 1e-150, 1 << 31, (1 << 31) - 500, 1, 500))
    return out


def mixed_batch():
    """64 jobs of mixed sizes around the chunk length and the tile width, n = 0 and n_freq = 0 included."""
    tile = source_constant("DFT_WAVE") * source_constant("DFT_LANE_FREQS")
    assert (source_constant("DFT_CHUNK"), tile) == (CHUNK, 128)
    rng = np.random.default_rng(77)
    ns = [0, 1, 2, 7, 63, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 8 * CHUNK, 8 * CHUNK + 1, 3 * CHUNK + 5, 33 * CHUNK + 9, 17, 700,
          32 * CHUNK]
    nfs = [1, 0, tile - 1, tile, tile + 1, 9, 2 * tile + 3, 40]
    jobs = []
    for k in range(64):
        n = ns[(k * 5 + k // 16) % len(ns)]
        nf = nfs[(k * 3 + k // 8) % len(nfs)]
        step = 1 + k % 3
        period = [max(2, 4 * n + 1), 1 << 31, nf * step + 7][k % 3]
        nf = min(nf, (period - 1) // step + 1)
        first = [0, period - 1 - (nf - 1) * step if nf else 0, min(5, period - 1 - (nf - 1) * step) if nf else 0][(k // 3) % 3]
        jobs.append((rng.standard_normal(n) * (1.0 + k), period, first, step, nf))
    return jobs


def long_double_sums(a, period, j):
    """(sum_t a[t] exp(2 pi i j t / M) in long double with EXACT integer phases: re, im) for the integers j."""
    assert np.finfo(LD).nmant >= 63
    al = a.astype(LD)
    t = np.arange(len(a), dtype=np.int64)
    two_pi = 2 * np.arctan2(LD(0), LD(-1))
    re, im = np.zeros(len(j), dtype=LD), np.zeros(len(j), dtype=LD)
    for i, jj in enumerate(np.asarray(j, dtype=np.int64).tolist()):
        if jj < (1 << 31) and len(a) <= (1 << 31):
            q = (jj * t) % period                                    # below 2^62: exact in int64
        else:
            q = np.array([(jj * int(v)) % period for v in t], dtype=np.int64)
        ang = two_pi * q.astype(LD) / LD(period)
        re[i], im[i] = np.sum(al * np.cos(ang)), np.sum(al * np.sin(ang))
    return re, im


def derived_bound(n, weight):
    """One rounding per FMA of a chunk, one per chunk addition, K for both twiddles of a term and the rotation."""
    return (CHUNK + -(-n // CHUNK) + K) * EPS * weight
