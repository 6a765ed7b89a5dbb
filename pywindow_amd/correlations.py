"""Dynamics of analysis results: lagged auto- and cross-correlation over the frame axis, summed on the GPU.

What a trajectory can answer and a pile of static structures cannot: how long a cage's pore keeps its size, whether
the pore follows the windows or leads them, and how many INDEPENDENT samples the frames really hold (how far the
curves of ``distribution()`` can be trusted).  The reference has no counterpart.  The lagged sums
``S[k] = sum_t a[t] b[t + k]`` are computed by ``pw_corr_sums`` (include/pywindow_amd.h; csrc/pw_corr.hip) -- many
series in one call, defined to the bit, the same on the device and on the host path -- and normalised here.  Gaps
(frames without a value) are handled exactly: the centred series carry zeros there, and the number of valid pairs
of every lag comes from the same call by correlating the two 0/1 masks.

* :func:`time_correlation` -- one pair of series (or one series with itself);
  :func:`time_correlation_batch` -- many, one call.
* ``RecordStore.series`` / ``.correlation`` (records.py) and ``DLPOLY.correlation`` (trajectory.py) take the series
  from the records of an analysis.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["TimeCorrelation", "time_correlation", "time_correlation_batch"]


@dataclasses.dataclass(frozen=True)
class TimeCorrelation:
    """``sums[k] = sum_t (a[t] - mean_a) (b[t + k] - mean_b)`` over the ``pairs[k]`` pairs of valid entries ``k`` steps
    apart, at ``lag[k]`` frames; ``covariance = sums / pairs`` (nan where there is no pair) and ``correlation =
    covariance / sqrt(C_aa[0] C_bb[0])``.  ``n``: valid entries of ``a``.  For an autocorrelation ``time`` is the
    integrated correlation time ``0.5 + sum(correlation[1:k0])`` in steps of the series, cut at the first lag ``k0``
    whose correlation is not positive, and ``n_effective = n / (2 time)`` the number of independent samples; both
    are ``None`` for a cross-correlation."""

    lag: np.ndarray
    sums: np.ndarray
    pairs: np.ndarray
    covariance: np.ndarray
    correlation: np.ndarray
    mean_a: float
    mean_b: float
    n: int
    time: float | None
    n_effective: float | None


def _centred(values, valid, what: str):
    """``(centred series with zeros in the gaps, mask as 0.0 / 1.0, mean, number of valid entries)``."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    ok = np.ones(len(v), dtype=bool) if valid is None else np.ascontiguousarray(valid, dtype=bool).reshape(-1)
    if len(ok) != len(v):
        raise ValueError(f"{what}: one flag per entry")
    count = int(ok.sum())
    if count < 2:
        raise ValueError(f"{what}: fewer than two valid entries")
    if not np.isfinite(v[ok]).all():
        raise ValueError(f"{what}: a valid entry is NaN or infinite")
    mean = float(np.sum(v[ok]) / count)
    centred = np.zeros(len(v))
    centred[ok] = v[ok] - mean
    return centred, ok.astype(np.float64), mean, count


def time_correlation_batch(pairs, max_lag=None, device=None, stride: int = 1) -> list:
    """One :class:`TimeCorrelation` per ``(a, b, valid_a, valid_b)`` of ``pairs`` (``b`` ``None``: the autocorrelation
    of ``a``; a mask ``None``: every entry is valid), all from ONE ``pw_corr_sums`` call: per pair the job of the
    centred series, the job of the masks, and for a cross-correlation the two lag-0 autocovariances.  ``max_lag``:
    one for all or one per pair; ``None``: ``(T - 1) // 2``; ``stride`` (frames per step) likewise.  ``device``: the HIP
    ordinal (``None``: the process's); ``-1`` the explicit host path."""
    pairs = list(pairs)
    lags = list(max_lag) if isinstance(max_lag, (list, tuple, np.ndarray)) else [max_lag] * len(pairs)
    strides = list(stride) if isinstance(stride, (list, tuple, np.ndarray)) else [stride] * len(pairs)
    if len(lags) != len(pairs) or len(strides) != len(pairs):
        raise ValueError("one max_lag and one stride per pair")
    series, jobs, plan = [], [], []
    at = out = 0

    def push(x):
        nonlocal at
        series.append(x)
        at += len(x)
        return at - len(x)

    def job(a_first, b_first, n, n_lags):
        nonlocal out
        jobs.append((a_first, b_first, n, out, n_lags))
        out += n_lags
        return out - n_lags

    for (a, b, valid_a, valid_b), lag in zip(pairs, lags):
        ca, ma, mean_a, count_a = _centred(a, valid_a, "a")
        t = len(ca)
        auto = b is None
        if not auto:
            cb, mb, mean_b, _ = _centred(b, valid_b, "b")
            if len(cb) != t:
                raise ValueError("a and b are series over the same frames: their lengths differ")
        lag = (t - 1) // 2 if lag is None else int(lag)
        if lag < 0 or lag >= t:
            raise ValueError(f"max_lag = {lag} for a series of {t} entries: it must be within 0 .. T - 1")
        fa, fma = push(ca), push(ma)
        if auto:
            s, p = job(fa, fa, t, lag + 1), job(fma, fma, t, lag + 1)
            plan.append((lag + 1, s, p, s, s, count_a, count_a, mean_a, mean_a, True))
        else:
            fb, fmb = push(cb), push(mb)
            s, p = job(fa, fb, t, lag + 1), job(fma, fmb, t, lag + 1)
            plan.append((lag + 1, s, p, job(fa, fa, t, 1), job(fb, fb, t, 1), count_a, int(mb.sum()), mean_a, mean_b, False))
    if not pairs:
        return []
    sums = engine.context(device).corr_sums(np.array(jobs, dtype=np.int64).view(_lib.CORR_JOB_DTYPE).reshape(-1),
                                            np.concatenate(series))
    result = []
    for (n_lags, s, p, saa, sbb, count_a, count_b, mean_a, mean_b, auto), step in zip(plan, strides):
        raw = sums[s:s + n_lags].copy()
        count = np.rint(sums[p:p + n_lags]).astype(np.int64)
        var_a, var_b = sums[saa] / count_a, sums[sbb] / count_b
        if not var_a > 0.0 or not var_b > 0.0:
            raise ValueError("a constant series (zero variance) has no correlation")
        with np.errstate(divide="ignore", invalid="ignore"):
            covariance = np.where(count > 0, raw / count, np.nan)
        correlation = covariance / math.sqrt(var_a * var_b)
        time = n_eff = None
        if auto:
            stop = np.flatnonzero(~(correlation[1:] > 0.0))
            k0 = 1 + int(stop[0]) if len(stop) else n_lags
            time = 0.5 + float(np.sum(correlation[1:k0]))
            n_eff = count_a / (2.0 * time)
        result.append(TimeCorrelation(int(step) * np.arange(n_lags, dtype=np.int64), raw, count, covariance, correlation,
                                      mean_a, mean_b, count_a, time, n_eff))
    return result


def time_correlation(a, b=None, max_lag=None, valid_a=None, valid_b=None, device=None, stride: int = 1) -> TimeCorrelation:
    """Lagged correlation of ``a[t]`` with ``b[t + k]``, ``k = 0 .. max_lag`` (``b`` ``None``: of ``a`` with itself;
    negative lags: swap ``a`` and ``b``).  ``valid_a`` / ``valid_b`` flag the entries that hold a value -- the rest are
    gaps and what they hold is ignored.  Means are taken over the valid entries.  ``stride``: frames per step, for
    :attr:`TimeCorrelation.lag`.  A constant series, fewer than two valid entries or ``max_lag >= T``: ``ValueError``."""
    return time_correlation_batch([(a, b, valid_a, valid_b)], max_lag, device, stride)[0]
