"""Inputs shared by tests/test_gate.py (host path against the definition) and tests/test_gpu_gate.py (device against
the host path and against the definition): gating statistics of a series against many thresholds (pw_gate_counts).
Every output is an integer: every comparison is np.array_equal on int64."""
import ctypes
import functools
import re

import numpy as np

from _kde_cases import ROOT

FIELDS = 12
SENTINEL = -77


def source_constant(name: str) -> int:
    text = (ROOT / "pywindow_amd" / "csrc" / "pw_gate.hpp").read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


CHUNK = source_constant("GATE_CHUNK")
TILE = source_constant("GATE_TILE")


def reference(a, d, n_bins):
    """The definition (include/pywindow_amd.h: pw_gate_counts) for one series and one threshold."""
    s = np.where(np.isnan(a), -1, np.where(a >= d, 1, 0))
    cut = np.flatnonzero(np.diff(s)) + 1
    lo, hi = np.r_[0, cut], np.r_[cut, len(s)]
    c, h = np.zeros(12, np.int64), np.zeros((2, n_bins), np.int64)
    for i, (b, e) in enumerate(zip(lo, hi)):
        st, length = s[b], e - b
        if st < 0: continue
        k = 1 - st                                   # 0 open, 1 closed
        c[k] += length; c[2 + k] += 1; c[4 + k] = max(c[4 + k], length)
        left = i > 0 and s[lo[i - 1]] == 1 - st
        right = i + 1 < len(lo) and s[lo[i + 1]] == 1 - st
        if left: c[6 + k] += 1
        if left and right:
            c[8 + k] += 1; c[10 + k] += length
            if n_bins: h[k, min(length, n_bins) - 1] += 1
    return c, h


@functools.lru_cache(maxsize=None)
def _reference_cached(series: bytes, d: float, n_bins: int):
    with np.errstate(invalid="ignore"):
        return reference(np.frombuffer(series, dtype=np.float64), np.float64(d), n_bins)


def reference_rows(jobs, n_bins):
    """(counts (R, 12), hist (R, 2, n_bins)) of `reference` for a list of (a, thresholds), rows one job after the other
    (the layout of `pack`).  Computed once per (series, threshold, n_bins) and shared."""
    counts, hist = [], []
    for a, thresholds in jobs:
        a = np.ascontiguousarray(a, dtype=np.float64)
        if len(a) == 0:
            continue
        key = a.tobytes()
        for d in np.asarray(thresholds, dtype=np.float64):
            c, h = _reference_cached(key, float(d), n_bins)
            counts.append(c)
            hist.append(h)
    if not counts:
        return np.zeros((0, FIELDS), np.int64), np.zeros((0, 2, n_bins), np.int64)
    return np.array(counts), np.array(hist).reshape(len(counts), 2, n_bins)


def pack(jobs, hole: int = 0):
    """(GATE_JOB_DTYPE array, series, thresholds) of a list of (a, thresholds).  A job with n > 0 and n_thr > 0 gets
    its rows one job after the other, `hole` rows that nobody owns in front of each; arrays that several jobs hold
    (the same object) are stored once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.GATE_JOB_DTYPE)
    parts, where, at = [], {}, 0
    thr, thr_where, d_at = [], {}, 0
    out = 0
    for k, (a, thresholds) in enumerate(jobs):
        if id(a) not in where:
            where[id(a)] = at
            parts.append(np.asarray(a, dtype=np.float64))
            at += len(a)
        if id(thresholds) not in thr_where:
            thr_where[id(thresholds)] = d_at
            thr.append(np.asarray(thresholds, dtype=np.float64).reshape(-1))
            d_at += len(thr[-1])
        live = len(a) > 0 and len(thresholds) > 0
        out += hole if live else 0
        rec[k] = (where[id(a)], len(a), thr_where[id(thresholds)], len(thresholds), out)
        out += len(thresholds) if live else 0
    return rec, np.concatenate(parts) if parts else np.zeros(0), np.concatenate(thr) if thr else np.zeros(0)


def raw_counts(ctx, rec, series, thresholds, n_bins, counts=None, hist="allocate", workspace_bytes=None, timed=False):
    """pw_gate_counts through ctypes into arrays of the caller (`counts` None: prefilled with SENTINEL; `hist` None: a
    NULL pointer), or through the library's test entry when `workspace_bytes` is given (0: the default budget; with
    `timed` the kernels' time by HIP events as well).  Returns (rc, counts, hist[, kernel ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.pw_internal_gate_counts.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.GATE_JOB_DTYPE)
    x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
    d = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    live = rec[(rec["n"] > 0) & (rec["n_thr"] > 0)]
    rows = int((live["out_first"] + live["n_thr"]).max()) if len(live) else 0
    if counts is None:
        counts = np.full((rows, FIELDS), SENTINEL, dtype=np.int64)
    if isinstance(hist, str):
        hist = np.full((rows, 2, max(n_bins, 0)), SENTINEL, dtype=np.int64)
    hp = hist.ctypes.data if hist is not None else None
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None:
        rc = L.pw_gate_counts(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, d.ctypes.data, int(n_bins), counts.ctypes.data, hp)
    else:
        rc = L.pw_internal_gate_counts(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, d.ctypes.data, int(n_bins),
                                       counts.ctypes.data, hp, int(workspace_bytes), ctypes.byref(ms) if timed else None)
    return (rc, counts, hist, ms.value) if timed else (rc, counts, hist)


# ---- series -----------------------------------------------------------------------------------------------------
OPEN, CLOSED, GAP = 2.0, 0.0, np.nan       # against the threshold 1.0


def from_runs(runs, swap: bool = False):
    """A series of (value, length) runs; `swap`: open and closed change places."""
    flip = {OPEN: CLOSED, CLOSED: OPEN}
    return np.concatenate([np.full(n, flip.get(v, v) if swap else v) for v, n in runs])


def smooth_noise(n: int, seed: int, gaps: float = 0.1):
    """A random series (a short moving average of white noise) with about `gaps` of its entries NaN."""
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.standard_normal(n + 7), np.ones(8) / np.sqrt(8.0), mode="valid")[:n]
    x[rng.random(n) < gaps] = np.nan
    return x


EDGE_NS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK + 1)
EDGE_THRS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGE_BINS = (0, 1, 2, 7)


@functools.lru_cache(maxsize=None)
def edge_grid():
    """Every n of EDGE_NS x every n_thr of EDGE_THRS: the first n_thr of one unsorted list of thresholds, so that the
    reference of a (series, threshold) serves every job that holds it."""
    rng = np.random.default_rng(3)
    every = rng.uniform(-2.0, 2.0, max(EDGE_THRS))
    series = [smooth_noise(n, 100 + n) for n in EDGE_NS]
    return [(a, every[:m]) for a in series for m in EDGE_THRS]


def chunk_edge_cases():
    """(name, a, thresholds): runs against the edges of a chunk, C = CHUNK; every pattern for open runs and, swapped,
    for closed ones.  The thresholds: 1.0 separates OPEN from CLOSED; -1.0 and 3.0 make the series one state."""
    C = CHUNK
    thr = np.array([1.0, -1.0, 3.0, 1.0])
    patterns = {
        "run-exactly-[C-1,C]": [(CLOSED, C - 1), (OPEN, 2), (CLOSED, C)],
        "run-ends-at-C-1-next-starts-at-C": [(CLOSED, 3), (OPEN, C - 3), (CLOSED, C), (OPEN, 2)],
        "run-of-2C+3-from-C-2": [(CLOSED, C - 2), (OPEN, 2 * C + 3), (CLOSED, 5)],
        "run-of-2C+3-from-C-2-to-the-end": [(CLOSED, C - 2), (OPEN, 2 * C + 3)],
        "gap-at-C-1": [(CLOSED, 2), (OPEN, C - 3), (GAP, 1), (OPEN, 4), (CLOSED, 3)],
        "gap-at-C": [(CLOSED, 2), (OPEN, C - 2), (GAP, 1), (OPEN, 4), (CLOSED, 3)],
        "gap-at-C-1-and-C": [(CLOSED, 2), (OPEN, C - 3), (GAP, 2), (OPEN, 4), (CLOSED, 3)],
        "gaps-around-a-boundary-run": [(CLOSED, 2), (OPEN, 3), (GAP, C - 7), (OPEN, 4), (GAP, 1), (CLOSED, 2), (OPEN, 2)],
        "censored-gap-left": [(OPEN, 1), (GAP, 2), (OPEN, C), (CLOSED, 2), (OPEN, 1)],
        "censored-gap-right": [(CLOSED, 1), (OPEN, C), (GAP, 2), (CLOSED, 2), (OPEN, 1)],
        "complete-across-the-boundary": [(CLOSED, C - 5), (OPEN, 9), (CLOSED, C), (OPEN, C + 1), (CLOSED, 1)],
        "two-runs-a-chunk": [(OPEN, C // 2), (CLOSED, C), (OPEN, C), (CLOSED, C // 2)],
    }
    out = []
    for name, runs in patterns.items():
        out.append((name, from_runs(runs), thr))
        out.append((name + "-swapped", from_runs(runs, swap=True), thr))
    return out


def degenerate_cases():
    C = CHUNK
    thr = np.array([1.0, 0.5])
    alternating = np.where(np.arange(2 * C + 1) % 2 == 0, OPEN, CLOSED)
    lone = np.full(C + 3, np.nan)
    lone[C] = OPEN
    return [("all-open", np.full(2 * C + 1, OPEN), thr), ("all-closed", np.full(2 * C + 1, CLOSED), thr),
            ("all-gap", np.full(2 * C + 1, np.nan), thr), ("alternating", alternating, thr),
            ("alternating-closed-first", alternating[1:], thr), ("one-valid-entry-between-gaps", lone, thr),
            ("one-entry", np.array([OPEN]), thr), ("one-gap", np.array([np.nan]), thr)]


def exactness_cases():
    """A threshold equal to a value is open, the next double above it closed, -0.0 and 0.0 are one number; thresholds
    unsorted and repeated."""
    rng = np.random.default_rng(8)
    values = np.concatenate([rng.standard_normal(40), [0.0, -0.0, 5e-324, -5e-324, 1e308, -1e308, 0.1, 0.3]])
    a = values[rng.integers(0, len(values), 3 * CHUNK + 1)]
    thr = np.concatenate([values, np.nextafter(values, np.inf), np.nextafter(values, -np.inf), [0.0, -0.0, 0.0, -0.0]])
    thr = np.concatenate([thr, thr[::3]])[rng.permutation(len(thr) + len(thr[::3]))]
    zeros = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0])
    return [("values-and-neighbours", a, thr), ("signed-zeros", zeros, np.array([0.0, -0.0, 5e-324, -5e-324]))]


def overflow_case():
    """Complete runs of B - 1, B and B + 1 entries of either state with B = 4."""
    return from_runs([(CLOSED, 1), (OPEN, 3), (CLOSED, 4), (OPEN, 4), (CLOSED, 5), (OPEN, 5), (CLOSED, 3), (OPEN, 1)]), np.array([1.0]), 4


def small_cases():
    """(name, a, thresholds, n_bins) of everything small enough for the definition in Python."""
    out = [(n, a, t, 7) for n, a, t in chunk_edge_cases() + degenerate_cases() + exactness_cases()]
    a, t, b = overflow_case()
    return out + [("overflow", a, t, b), ("overflow-no-hist", a, t, 0), ("overflow-one-bin", a, t, 1)]


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """64 jobs of mixed sizes around the chunk and the tile, n == 0 and n_thr == 0 included; every fourth job shares
    the series of the one before it, every eighth its thresholds too."""
    rng = np.random.default_rng(64)
    C = CHUNK
    ns = [0, 1, 2, 7, 63, C - 1, C, C + 1, 2 * C, 4 * C + 1, 3 * C + 5, 17, 700, 2 * C + 7, 2 * C + 1, C // 2]
    ms = [1, 0, TILE - 1, TILE, TILE + 1, 9, 2 * TILE + 3, 40]
    jobs = []
    for k in range(64):
        n = ns[(k * 5 + k // 16) % len(ns)]
        m = ms[(k * 3 + k // 8) % len(ms)]
        a = smooth_noise(n, 1000 + k, gaps=0.05 * (k % 4))
        thr = rng.uniform(-1.5, 1.5, m)
        if k % 4 == 3:
            a = jobs[-1][0]
        if k % 8 == 7:
            thr = jobs[-1][1]
        jobs.append((a, thr))
    return jobs


@functools.lru_cache(maxsize=None)
def long_job():
    """One job of 200 000 entries x 2048 thresholds (4e8 steps), a slow series with gaps."""
    n, m = 200_000, 2048
    rng = np.random.default_rng(2048)
    x = np.cumsum(rng.standard_normal(n)) * 0.05 + np.sin(np.arange(n) * 0.01) + 0.3 * rng.standard_normal(n)
    x[rng.random(n) < 0.01] = np.nan
    return x, np.linspace(np.nanmin(x), np.nanmax(x), m)
