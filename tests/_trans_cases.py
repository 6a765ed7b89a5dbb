"""Inputs shared by tests/test_trans.py (host path against the definition) and tests/test_gpu_trans.py (device against
the host path and against the definition): lagged state-transition counts of a series (pw_trans_counts).  Every output
is an integer: every comparison is np.array_equal on int64."""
import ctypes
import functools
import re

import numpy as np

from _kde_cases import ROOT

SENTINEL = -77


def source_constant(name: str) -> int:
    text = (ROOT / "pywindow_amd" / "csrc" / "pw_trans.hpp").read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


CHUNK = source_constant("TRANS_CHUNK")        # entries
TILE = source_constant("TRANS_TILE")          # lags
WINDOW = source_constant("TRANS_WINDOW")      # entries of the partner window that fit LDS


def reference(a, edges, lags, n_states):
    """The definition (include/pywindow_amd.h: pw_trans_counts) for one series: counts (len(lags), n_states, n_states)."""
    a = np.asarray(a, dtype=np.float64)
    gap = np.isnan(a)
    s = np.searchsorted(np.asarray(edges, dtype=np.float64), a, side="right")
    out = np.zeros((len(lags), n_states, n_states), np.int64)
    for q, k in enumerate(lags):
        k = int(k)
        if k >= len(a):
            continue
        ok = ~gap[:len(a) - k] & ~gap[k:]
        np.add.at(out[q], (s[:len(a) - k][ok], s[k:][ok]), 1)
    return out


def lags_of(grid):
    first, step, count = grid
    return first + step * np.arange(count, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _reference_cached(series: bytes, edges: bytes, grid, n_states: int):
    return reference(np.frombuffer(series, dtype=np.float64), np.frombuffer(edges, dtype=np.float64), lags_of(grid), n_states)


def reference_rows(jobs, n_states):
    """counts (R, S, S) of `reference` for a list of (a, edges, (first, step, count)), rows one job after the other (the
    layout of `pack`).  Computed once per job and shared."""
    rows = [np.zeros((0, n_states, n_states), np.int64)]
    for a, edges, grid in jobs:
        a = np.ascontiguousarray(a, dtype=np.float64)
        if len(a) == 0 or grid[2] == 0:
            continue
        rows.append(_reference_cached(a.tobytes(), np.ascontiguousarray(edges, dtype=np.float64).tobytes(), tuple(grid), n_states))
    return np.concatenate(rows)


def pack(jobs, hole: int = 0):
    """(TRANS_JOB_DTYPE array, series, edges) of a list of (a, edges, (first, step, count)).  A job with n > 0 and
    n_lags > 0 gets its rows one job after the other, `hole` rows that nobody owns in front of each; arrays that several
    jobs hold (the same object) are stored once."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.TRANS_JOB_DTYPE)
    parts, where, at = [], {}, 0
    eds, e_where, e_at = [], {}, 0
    out = 0
    for k, (a, edges, (first, step, count)) in enumerate(jobs):
        if id(a) not in where:
            where[id(a)] = at
            parts.append(np.asarray(a, dtype=np.float64))
            at += len(a)
        if id(edges) not in e_where:
            e_where[id(edges)] = e_at
            eds.append(np.asarray(edges, dtype=np.float64).reshape(-1))
            e_at += len(eds[-1])
        live = len(a) > 0 and count > 0
        out += hole if live else 0
        rec[k] = (where[id(a)], len(a), e_where[id(edges)], len(edges), first, step, count, out)
        out += count if live else 0
    return rec, np.concatenate(parts) if parts else np.zeros(0), np.concatenate(eds) if eds else np.zeros(0)


def raw_counts(ctx, rec, series, edges, n_states, counts=None, workspace_bytes=None, timed=False):
    """pw_trans_counts through ctypes into an array of the caller (`counts` None: prefilled with SENTINEL), or through
    the library's test entry when `workspace_bytes` is given (0: the default budget; with `timed` the kernels' time by
    HIP events as well).  Returns (rc, counts[, kernel ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.pw_internal_trans_counts.argtypes = [vp, vp, i64, vp, vp, i64, vp, i64, ctypes.POINTER(ctypes.c_float)]
    rec = np.ascontiguousarray(rec, dtype=_lib.TRANS_JOB_DTYPE)
    x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    live = rec[(rec["n"] > 0) & (rec["n_lags"] > 0)]
    rows = int((live["out_first"] + live["n_lags"]).max()) if len(live) else 0
    side = min(max(int(n_states), 1), 16)
    if counts is None:
        counts = np.full((rows, side, side), SENTINEL, dtype=np.int64)
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None:
        rc = L.pw_trans_counts(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, e.ctypes.data, int(n_states), counts.ctypes.data)
    else:
        rc = L.pw_internal_trans_counts(ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, e.ctypes.data, int(n_states),
                                        counts.ctypes.data, int(workspace_bytes), ctypes.byref(ms) if timed else None)
    return (rc, counts, ms.value) if timed else (rc, counts)


# ---- series -----------------------------------------------------------------------------------------------------
def noise(n: int, seed: int, gaps: float = 0.1):
    """A random series (a short moving average of white noise) with about `gaps` of its entries NaN."""
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.standard_normal(n + 7), np.ones(8) / np.sqrt(8.0), mode="valid")[:n]
    x[rng.random(n) < gaps] = np.nan
    return x


def edges_for(n_edges: int):
    return np.linspace(-1.2, 1.2, n_edges) if n_edges > 1 else np.array([0.1])[:n_edges]


EDGE_NS = (1, 2, 31, 32, 33, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
# a lag_step at which tile * lag_step entries no longer fit the window a work item stages in LDS
FAR_STEP = WINDOW // TILE + 40


@functools.lru_cache(maxsize=None)
def groups():
    """{n_states: [(name, a, edges, (first, step, count)), ...]}: the jobs of one call share n_states."""
    C = CHUNK
    out = {1: [], 2: [], 3: [], 4: [], 5: [], 16: []}
    e2 = edges_for(2)
    # n around a word, a wave of the pack kernel and a chunk; the lags 0 .. 33 and n - 1 .. n + 5
    for n in EDGE_NS:
        a = noise(n, 100 + n)
        out[3].append((f"n={n}-lags-0..33", a, e2, (0, 1, 34)))
        out[3].append((f"n={n}-lags-n-1..n+5", a, e2, (n - 1, 1, 7)))
    # lag_step: within the LDS window and beyond it; n_lags around the tile
    long = noise(2 * C + 1, 7)
    for step in (1, 2, 7, 32, FAR_STEP):
        out[3].append((f"lag_step={step}", long, e2, (3, step, TILE + 1)))
    mid = noise(C + 1, 8)
    for count in (1, TILE - 1, TILE, TILE + 1):
        out[2].append((f"n_lags={count}", mid, edges_for(1), (0, 1, count)))
    # n_states: every instantiation, one with fewer edges than the call allows
    for S in (1, 2, 3, 4, 5, 16):
        out[S].append((f"n_states={S}", mid, edges_for(S - 1), (0, 5, 40)))
    out[5].append(("n_edges-below-n_states-1", mid, edges_for(2), (0, 3, 20)))
    out[16].append(("16-states-two-chunks-far", long, edges_for(15), (1, FAR_STEP, 12)))
    # values
    rng = np.random.default_rng(5)
    values = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 0.25, -0.25, 1.0, np.nextafter(0.25, 1), np.nextafter(0.25, 0)])
    exact = values[rng.integers(0, len(values), 700)]
    out[5].append(("entries-equal-to-an-edge-signed-zeros-denormals", exact, np.array([-0.25, 0.0, 5e-324, 0.25]), (0, 1, 70)))
    out[2].append(("signed-zeros-at-edge-0", np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0]), np.array([0.0]), (0, 1, 9)))
    out[2].append(("minus-zero-edge", np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0]), np.array([-0.0]), (0, 1, 9)))
    out[3].append(("all-gap", np.full(C + 3, np.nan), e2, (0, 1, 40)))
    out[3].append(("no-gap", noise(C + 3, 9, gaps=0.0), e2, (0, 1, 40)))
    for at in (31, 32, 63, 64, C - 1, C):
        a = noise(C + 70, 10, gaps=0.0)
        a[at] = np.nan
        out[3].append((f"gap-at-{at}", a, e2, (0, 1, 70)))
    return out


def call_cases():
    """(jobs, n_states): two jobs sharing a series with different edges, a job with n == 0 and one with n_lags == 0."""
    a, b = noise(3000, 21), noise(700, 22)
    e1, e3 = edges_for(1), edges_for(3)
    return [(a, e3, (0, 1, 300)), (a, e1, (5, 3, 100)), (np.zeros(0), e1, (0, 1, 5)), (b, e3, (0, 1, 0)), (b, e3, (690, 1, 20))], 4


def markov_chain(n: int, p01: float, p10: float, seed: int):
    """A two-state Markov chain as a series of 0.0 / 1.0."""
    u = np.random.default_rng(seed).random(n)
    s = np.zeros(n)
    state = 0
    for t in range(n):
        s[t] = state
        state = (1 if u[t] < p01 else 0) if state == 0 else (0 if u[t] < p10 else 1)
    return s
