"""Gating statistics of analysis results: how often and for how long a series stays above or below a threshold.

The question a trajectory is usually run for: for a guest of diameter ``d``, what fraction of the time does the cage
admit it, how often does it open, and how long does an opening or a closure last?  Those are statements about RUNS of
consecutive frames above or below ``d`` -- a density curve or an autocorrelation gives neither: two series with the
same distribution can gate completely differently (rare long openings, or constant flicker).  The reference has no
counterpart.  The counts are computed by ``pw_gate_counts`` (include/pywindow_amd.h; csrc/pw_gate.hip) -- many series
and many thresholds in one call, all integers, the same on the device and on the host path.  Gaps (frames without a
value) are a state of their own: they end a run without being counted as the opposite state.

* :func:`gate_statistics` -- one series; :func:`gate_statistics_batch` -- many, one call.
* ``RecordStore.gating`` (records.py) and ``DLPOLY.gating`` (trajectory.py) take the series from the records of an
  analysis.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine

__all__ = ["Gating", "gate_statistics", "gate_statistics_batch"]


@dataclasses.dataclass(frozen=True)
class Gating:
    """One entry per threshold (``Q`` of them).  An entry of the series is OPEN when its value is ``>= threshold``,
    CLOSED when it is below, and a GAP when it holds no value; the series falls into maximal runs of one state.
    ``n_valid`` entries hold a value, ``open_fraction`` of them are open.  ``open_runs`` / ``closed_runs`` count the
    runs whatever bounds them, ``longest_open`` / ``longest_closed`` are the longest in frames; ``openings`` counts the
    open runs that follow a closed run directly (closed at one sample, open at the next), ``closings`` the reverse.

    CENSORING.  A run's true length is known only when a run of the opposite state bounds it on BOTH sides; a run that
    touches a gap or an end of the series may have gone on unseen and is censored.  ``mean_open`` / ``mean_closed``
    (frames; nan where there is none) and the histograms ``open_lengths`` / ``closed_lengths`` ``(Q, B)`` are taken
    over the complete runs alone: bin ``b`` counts those of ``length[b]`` frames, the last bin every longer one too.
    ``counts`` ``(Q, 12)`` are the raw integers of ``pw_gate_counts`` (columns: ``_lib.GATE_FIELDS``), in samples."""

    threshold: np.ndarray
    n_valid: int
    open_fraction: np.ndarray
    openings: np.ndarray
    closings: np.ndarray
    open_runs: np.ndarray
    closed_runs: np.ndarray
    longest_open: np.ndarray
    longest_closed: np.ndarray
    mean_open: np.ndarray
    mean_closed: np.ndarray
    open_lengths: np.ndarray
    closed_lengths: np.ndarray
    length: np.ndarray
    counts: np.ndarray


def _with_gaps(values, valid):
    """``(the series with NaN in the gaps, number of valid entries)``."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    ok = np.ones(len(v), dtype=bool) if valid is None else np.ascontiguousarray(valid, dtype=bool).reshape(-1)
    if len(ok) != len(v):
        raise ValueError("a: one flag per entry")
    count = int(ok.sum())
    if count < 1:
        raise ValueError("a: no valid entry")
    if not np.isfinite(v[ok]).all():
        raise ValueError("a: a valid entry is NaN or infinite")
    return np.where(ok, v, np.nan), count


def gate_statistics_batch(items, n_bins: int = 0, stride=1, device=None) -> list:
    """One :class:`Gating` per ``(a, thresholds, valid)`` of ``items`` (``valid`` ``None``: every entry holds a value),
    all from ONE ``pw_gate_counts`` call.  Entries whose flag is false are gaps, whatever they hold.  ``n_bins``: bins
    of the run-length histograms (0: none); ``stride`` (frames per sample): one for all or one per item.  ``device``:
    the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    items = list(items)
    strides = list(stride) if isinstance(stride, (list, tuple, np.ndarray)) else [stride] * len(items)
    if len(strides) != len(items):
        raise ValueError("one stride per item")
    n_bins = int(n_bins)
    if n_bins < 0:
        raise ValueError("n_bins is negative")
    series, thresholds, jobs, plan = [], [], [], []
    at = d_at = out = 0
    for a, thr, valid in items:
        x, count = _with_gaps(a, valid)
        d = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
        if len(d) < 1:
            raise ValueError("thresholds: at least one")
        if not np.isfinite(d).all():
            raise ValueError("thresholds: a threshold is NaN or infinite")
        jobs.append((at, len(x), d_at, len(d), out))
        plan.append((out, d, count))
        series.append(x)
        thresholds.append(d)
        at, d_at, out = at + len(x), d_at + len(d), out + len(d)
    if not items:
        return []
    counts, hist = engine.context(device).gate_counts(np.array(jobs, dtype=np.int64).view(_lib.GATE_JOB_DTYPE).reshape(-1),
                                                      np.concatenate(series), np.concatenate(thresholds), n_bins)
    result = []
    for (first, d, count), step in zip(plan, strides):
        step = int(step)
        c = counts[first:first + len(d)].copy()
        h = hist[first:first + len(d)]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_open = np.where(c[:, 8] > 0, step * c[:, 10] / c[:, 8], np.nan)
            mean_closed = np.where(c[:, 9] > 0, step * c[:, 11] / c[:, 9], np.nan)
        result.append(Gating(d.copy(), count, c[:, 0] / count, c[:, 6].copy(), c[:, 7].copy(), c[:, 2].copy(), c[:, 3].copy(),
                             step * c[:, 4], step * c[:, 5], mean_open, mean_closed, h[:, 0].copy(), h[:, 1].copy(),
                             step * np.arange(1, n_bins + 1, dtype=np.int64), c))
    return result


def gate_statistics(a, thresholds, valid=None, n_bins: int = 0, stride: int = 1, device=None) -> Gating:
    """Gating of the series ``a`` at every one of ``thresholds`` (finite, at least one, any order): see
    :class:`Gating`.  ``valid`` flags the entries that hold a value -- the rest are gaps and what they hold is
    ignored; a NaN or an infinity in a valid entry: ``ValueError``.  ``n_bins``: bins of the histograms of the complete
    runs' lengths; ``stride``: frames per sample, for the lengths."""
    return gate_statistics_batch([(a, thresholds, valid)], n_bins, stride, device)[0]
