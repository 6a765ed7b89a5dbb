"""Spectra of analysis results: the generalised Lomb-Scargle periodogram over the frame axis, summed on the GPU.

A correlation function shows THAT a pore oscillates; the spectrum says at which frequency the cage breathes.  The
series of a trajectory have gaps (frames without windows, non-porous frames, absent frames), so an FFT does not
apply; the generalised (floating-mean) Lomb-Scargle periodogram is the exact least-squares fit of a sinusoid plus a
constant to the valid frames only.  Its raw sums ``sum_t a[t] exp(2 pi i j t / M)`` are computed by ``pw_dft_sums``
(include/pywindow_amd.h; csrc/pw_dft.hip) -- many series in one call, at rational frequencies ``j / M`` whose phases
are exact integers, defined to the bit, the same on the device and on the host path -- and combined here.

* :func:`dft_sums` / :func:`dft_sums_batch` -- the raw sums;
* :func:`lomb_scargle` -- one series; :func:`lomb_scargle_batch` -- many, one call;
* ``RecordStore.spectrum`` (records.py) and ``DLPOLY.spectrum`` (trajectory.py) take the series from the records of
  an analysis.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["Spectrum", "dft_sums", "dft_sums_batch", "lomb_scargle", "lomb_scargle_batch"]

_MAX = 1 << 31


@dataclasses.dataclass(frozen=True)
class Spectrum:
    """Generalised Lomb-Scargle periodogram of a series with gaps at ``frequency = j / (period * stride * dt)``
    (``period = oversample * T`` samples; ``stride`` frames a sample, ``dt`` time a frame).  ``power`` is the share of
    the variance a sinusoid plus a constant fitted at that frequency explains (0 .. 1; nan where the fit is singular),
    ``amplitude`` the amplitude of that sinusoid.  ``sums``: the raw sums of the three jobs as a ``(3, n_freq)``
    complex array -- the centred series at ``j``, the 0/1 mask at ``j``, the mask at ``2 j``.  ``n_valid``: entries
    that hold a value; ``mean`` their mean.  ``peak_frequency``, ``peak_power``, ``peak_period`` (``1 /
    peak_frequency``): the largest power."""

    frequency: np.ndarray
    j: np.ndarray
    period: int
    power: np.ndarray
    amplitude: np.ndarray
    sums: np.ndarray
    n_valid: int
    mean: float
    peak_frequency: float
    peak_power: float
    peak_period: float


def _progression(j):
    """``(first, step, count)`` when the integers ``j`` are an arithmetic progression with a step >= 1, else None."""
    if len(j) == 1:
        return int(j[0]), 1, 1
    step = int(j[1] - j[0])
    if step >= 1 and (np.diff(j) == step).all():
        return int(j[0]), step, len(j)
    return None


def dft_sums_batch(jobs, device=None) -> list:
    """One complex array ``sum_t a[t] exp(2 pi i j t / period)`` per ``(a, j, period)`` of ``jobs``, all from ONE
    ``pw_dft_sums`` call.  ``j``: integers within ``0 .. period - 1`` (an arithmetic progression is one job of the
    call, anything else one job per frequency); ``2 <= period <= 2^31``.  ``device``: the HIP ordinal (``None``: the
    process's); ``-1`` the explicit host path."""
    series, recs, spans = [], [], []
    at = out = 0
    for a, j, period in jobs:
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        j = np.asarray(j)
        if j.size and not np.issubdtype(j.dtype, np.integer):
            raise ValueError("the frequencies j are integers (frequency j / period)")
        j = j.astype(np.int64).reshape(-1)
        period = int(period)
        if len(j) and (j.min() < 0 or j.max() >= period):
            raise ValueError("a frequency outside 0 .. period - 1")
        series.append(a)
        runs = [] if len(j) == 0 else [_progression(j)] if _progression(j) else [(int(v), 1, 1) for v in j]
        spans.append((out, len(j)))
        for first, step, count in runs:
            recs.append((at, len(a), period, first, step, count, out))
            out += count
        at += len(a)
    if not recs:
        return [np.zeros(n, dtype=np.complex128) for _, n in spans]
    sums = engine.context(device).dft_sums(np.array(recs, dtype=np.int64).view(_lib.DFT_JOB_DTYPE).reshape(-1),
                                           np.concatenate(series))
    sums = np.concatenate([sums, np.zeros(out - len(sums), dtype=np.complex128)])     # (jobs of empty series)
    return [sums[first:first + n].copy() for first, n in spans]


def dft_sums(a, j, period, device=None) -> np.ndarray:
    """``sum_t a[t] exp(2 pi i j t / period)`` for the integers ``j``: :func:`dft_sums_batch` of one job."""
    return dft_sums_batch([(a, j, period)], device)[0]


def _frequencies(n: int, oversample: int, max_frequency: float):
    period = int(oversample) * n
    if int(oversample) < 1 or period > _MAX:
        raise ValueError("oversample >= 1 and oversample * T <= 2^31")
    if not 0.0 < max_frequency <= 0.5:
        raise ValueError("max_frequency is in cycles per sample: within (0, 0.5]")
    top = min(-(-period // 2) - 1, int(math.floor(max_frequency * period)))
    if top < 1:
        raise ValueError("no frequency below max_frequency: the series is too short")
    return period, top


def lomb_scargle_batch(series_list, oversample: int = 4, max_frequency: float = 0.5, stride=1, dt: float = 1.0,
                       device=None) -> list:
    """One :class:`Spectrum` per ``(a, valid)`` of ``series_list`` (``valid`` ``None``: every entry holds a value),
    all from ONE ``pw_dft_sums`` call: per series the job of the series centred over its valid entries with zeros in
    the gaps, the job of the 0/1 mask, both at ``j = 1 .. min(ceil(M / 2) - 1, floor(max_frequency M))`` with ``M =
    oversample * T``, and the job of the mask at ``2 j``.  ``stride`` (frames a sample): one for all or one per series.
    Fewer than 3 valid entries or a constant series: ``ValueError``."""
    series_list = list(series_list)
    strides = list(stride) if isinstance(stride, (list, tuple, np.ndarray)) else [stride] * len(series_list)
    if len(strides) != len(series_list):
        raise ValueError("one stride per series")
    series, recs, plan = [], [], []
    at = out = 0
    for a, valid in series_list:
        v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        ok = np.ones(len(v), dtype=bool) if valid is None else np.ascontiguousarray(valid, dtype=bool).reshape(-1)
        if len(ok) != len(v):
            raise ValueError("one flag per entry")
        count = int(ok.sum())
        if count < 3:
            raise ValueError("fewer than three valid entries")
        if not np.isfinite(v[ok]).all():
            raise ValueError("a valid entry is NaN or infinite")
        mean = float(np.sum(v[ok]) / count)
        y = np.zeros(len(v))
        y[ok] = v[ok] - mean
        yy = float(np.sum(y * y) / count)
        if not yy > 0.0:
            raise ValueError("a constant series (zero variance) has no spectrum")
        period, top = _frequencies(len(v), oversample, max_frequency)
        series += [y, ok.astype(np.float64)]
        n = len(v)
        recs += [(at, n, period, 1, 1, top, out), (at + n, n, period, 1, 1, top, out + top),
                 (at + n, n, period, 2, 2, top, out + 2 * top)]
        plan.append((out, top, period, count, mean, yy))
        at += 2 * n
        out += 3 * top
    if not series_list:
        return []
    sums = engine.context(device).dft_sums(np.array(recs, dtype=np.int64).view(_lib.DFT_JOB_DTYPE).reshape(-1),
                                           np.concatenate(series))
    result = []
    for (first, top, period, count, mean, yy), step in zip(plan, strides):
        raw = sums[first:first + 3 * top].reshape(3, top).copy()
        n = float(count)
        c, s = raw[1].real / n, raw[1].imag / n
        yc, ys = raw[0].real / n, raw[0].imag / n
        cc = (1.0 + raw[2].real / n) / 2.0 - c * c
        ss = (1.0 - raw[2].real / n) / 2.0 - s * s
        cs = raw[2].imag / (2.0 * n) - c * s
        d = cc * ss - cs * cs
        with np.errstate(divide="ignore", invalid="ignore"):
            good = d > 0.0
            power = np.where(good, (ss * yc * yc + cc * ys * ys - 2.0 * cs * yc * ys) / (yy * d), np.nan)
            amplitude = np.where(good, np.hypot(ss * yc - cs * ys, cc * ys - cs * yc) / d, np.nan)
        j = np.arange(1, top + 1, dtype=np.int64)
        frequency = j / (float(period) * float(step) * float(dt))
        if not np.isfinite(power).any():
            raise ValueError("the fit is singular at every frequency")
        at_peak = int(np.nanargmax(power))
        result.append(Spectrum(frequency, j, int(period), power, amplitude, raw, count, mean, float(frequency[at_peak]),
                               float(power[at_peak]), float(1.0 / frequency[at_peak])))
    return result


def lomb_scargle(a, valid=None, oversample: int = 4, max_frequency: float = 0.5, stride: int = 1, dt: float = 1.0,
                 device=None) -> Spectrum:
    """Generalised (floating-mean) Lomb-Scargle periodogram of ``a`` over its valid entries -- the rest are gaps and
    what they hold is ignored -- at the frequencies ``j / (oversample * T)`` cycles per sample up to
    ``max_frequency``.  ``stride`` (frames a sample) and ``dt`` (time a frame) scale :attr:`Spectrum.frequency`."""
    return lomb_scargle_batch([(a, valid)], oversample, max_frequency, stride, dt, device)[0]
