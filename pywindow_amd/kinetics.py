"""Trajectory kinetics: lagged state-transition counts of analysis results, and what follows from them.

A gating result raises the next question at once: what are the rates, and is the process Markovian at the frame
spacing?  A dwell time at lag 1 cannot tell flicker on top of a slow mode from a single slow process, and a cage has more
than two states (closed, partly open, open; 0 to 4 windows open to a guest at once).  The standard instrument is the
lagged count matrix ``C_k[i][j] = #{t : s[t] = i, s[t + k] = j}`` over many lags ``k``: its row-normalised form is the
transition matrix ``T(k)``, its row sums the populations, ``-k / ln lambda_i(T(k))`` the implied timescales -- flat in
``k`` for a Markov process -- and ``T(k)^m`` against ``T(m k)`` the Chapman-Kolmogorov test.  The reference has no
counterpart.  The counts are computed by ``pw_trans_counts`` (include/pywindow_amd.h; csrc/pw_trans.hip) -- many series
and many lags in one call, all integers, the same on the device and on the host path.  A gap (a frame without a value)
has no state: a pair with a gap at either end is counted nowhere.

* :func:`transition_counts` -- one series; :func:`transition_counts_batch` -- many, one call.
* ``RecordStore.kinetics`` (records.py) and ``DLPOLY.kinetics`` (trajectory.py) take the series from the records of an
  analysis.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine
from .gating import _with_gaps

__all__ = ["Kinetics", "transition_counts", "transition_counts_batch"]


@dataclasses.dataclass(frozen=True)
class Kinetics:
    """One entry per lag (``L`` of them) over ``S = len(edges) + 1`` states; the state of a value is the number of
    ``edges`` that are ``<=`` it (``np.searchsorted(edges, a, side="right")``).  ``lag`` is in frames.  ``counts[k, i, j]``
    is the number of pairs ``s[t] = i, s[t + lag[k]] = j`` with a value at both ends, ``n_pairs[k]`` their sum,
    ``population[k, i]`` the share of the pairs that start in ``i`` and ``transition[k]`` the row-normalised counts (a row
    nobody starts from is nan).  ``timescales[k, i - 1] = -lag[k] / ln(lambda_i)`` over the eigenvalues of
    ``transition[k]`` (``numpy.linalg.eigvals``) sorted by decreasing modulus, the leading one left out; nan where
    ``lambda_i`` is not real and in ``(0, 1)``, where a row of ``transition[k]`` is missing and at lag 0."""

    edges: np.ndarray
    lag: np.ndarray
    counts: np.ndarray
    n_pairs: np.ndarray
    population: np.ndarray
    transition: np.ndarray
    timescales: np.ndarray

    @classmethod
    def from_counts(cls, edges, lag, counts) -> "Kinetics":
        """The derived quantities of ``counts`` ``(L, S, S)`` at the lags ``lag`` (frames)."""
        edges = np.array(edges, dtype=np.float64).reshape(-1)
        lag = np.array(lag, dtype=np.int64).reshape(-1)
        counts = np.array(counts, dtype=np.int64)
        S = len(edges) + 1
        if counts.shape != (len(lag), S, S):
            raise ValueError("counts: one (S, S) matrix per lag with S = len(edges) + 1")
        n_pairs = counts.sum(axis=(1, 2))
        origin = counts.sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            population = origin / n_pairs[:, None]
            transition = counts / origin[:, :, None]
        timescales = np.full((len(lag), S - 1), np.nan)
        for k in range(len(lag)):
            if S < 2 or lag[k] == 0 or not np.isfinite(transition[k]).all():
                continue
            ev = np.linalg.eigvals(transition[k])
            ev = ev[np.argsort(-np.abs(ev), kind="stable")][1:]
            good = (np.abs(ev.imag) == 0.0) & (ev.real > 0.0) & (ev.real < 1.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                timescales[k] = np.where(good, -float(lag[k]) / np.log(np.where(good, ev.real, 0.5)), np.nan)
        return cls(edges, lag, counts, n_pairs, population, transition, timescales)

    def ck_error(self, base: int):
        """Chapman-Kolmogorov test: ``(lags, error)`` with ``lags = m * base`` for ``m = 1, 2, ...`` up to the largest lag
        and ``error[m - 1] = max |transition[base]^m - transition[m * base]|`` (0 for a Markov chain observed without
        noise).  ``base`` is in frames; the grid of lags must hold ``base`` and every multiple of it up to its end:
        ``ValueError`` otherwise."""
        base = int(base)
        if base < 1:
            raise ValueError("base: a lag of at least one frame")
        where = {int(v): k for k, v in enumerate(self.lag.tolist())}
        multiples = np.arange(base, int(self.lag.max()) + 1, base, dtype=np.int64) if len(self.lag) else np.zeros(0, np.int64)
        if len(multiples) < 2 or any(int(v) not in where for v in multiples):
            raise ValueError(f"the lags do not hold {base} and its multiples: pass a grid that does")
        T = self.transition[where[base]]
        power, error = np.eye(len(T)), np.zeros(len(multiples))
        for m, v in enumerate(multiples.tolist()):
            power = power @ T
            error[m] = np.max(np.abs(power - self.transition[where[v]]))
        return multiples, error


def _lag_grid(lags):
    """``(first, step, count)`` in samples."""
    if isinstance(lags, (bool, np.bool_)):
        raise ValueError("lags: max_lag or (first, step, count), not a bool")
    if isinstance(lags, (int, np.integer)):
        first, step, count = 0, 1, int(lags) + 1
    else:
        try:
            first, step, count = (int(v) for v in lags)
        except (TypeError, ValueError):
            raise ValueError("lags: max_lag or (first, step, count)") from None
    if first < 0 or step < 1 or count < 1:
        raise ValueError("lags: first >= 0, step >= 1 and at least one lag")
    return first, step, count


def _edges(edges) -> np.ndarray:
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if len(e) > _lib.TRANS_MAX_STATES - 1:
        raise ValueError(f"edges: at most {_lib.TRANS_MAX_STATES - 1}")
    if not np.isfinite(e).all():
        raise ValueError("edges: an edge is NaN or infinite")
    if (np.diff(e) <= 0).any():
        raise ValueError("edges: not strictly increasing")
    return e


def transition_counts_batch(items, lags, stride=1, device=None) -> list:
    """One :class:`Kinetics` per ``(a, edges, valid)`` of ``items`` (``valid`` ``None``: every entry holds a value), all
    from ONE ``pw_trans_counts`` call.  Entries whose flag is false are gaps, whatever they hold.  ``lags``: an int
    ``max_lag`` for the lags ``0 .. max_lag``, or ``(first, step, count)``, in samples; one for all or a list with one
    per item.  ``stride`` (frames per sample): one for all or one per item; ``Kinetics.lag`` is ``stride * k``.
    ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    items = list(items)
    strides = list(stride) if isinstance(stride, (list, tuple, np.ndarray)) else [stride] * len(items)
    if len(strides) != len(items):
        raise ValueError("one stride per item")
    grids = [_lag_grid(g) for g in lags] if isinstance(lags, list) else [_lag_grid(lags)] * len(items)
    if len(grids) != len(items):
        raise ValueError("one grid of lags per item")
    series, every, jobs, plan = [], [], [], []
    at = e_at = out = 0
    for (a, edges, valid), (first, step, count) in zip(items, grids):
        x, _ = _with_gaps(a, valid)
        e = _edges(edges)
        jobs.append((at, len(x), e_at, len(e), first, step, count, out))
        plan.append((out, e, first + step * np.arange(count, dtype=np.int64)))
        series.append(x)
        every.append(e)
        at, e_at, out = at + len(x), e_at + len(e), out + count
    if not items:
        return []
    n_states = max(len(e) for e in every) + 1
    counts = engine.context(device).trans_counts(np.array(jobs, dtype=np.int64).view(_lib.TRANS_JOB_DTYPE).reshape(-1),
                                                 np.concatenate(series), np.concatenate(every), n_states)
    result = []
    for (first, e, k), step in zip(plan, strides):
        S = len(e) + 1
        result.append(Kinetics.from_counts(e, int(step) * k, counts[first:first + len(k), :S, :S]))
    return result


def transition_counts(a, edges, lags, valid=None, stride: int = 1, device=None) -> Kinetics:
    """Lagged transition counts of the series ``a`` between the states that ``edges`` cut the value axis into (finite,
    strictly increasing, at most 15): see :class:`Kinetics`.  ``valid`` flags the entries that hold a value -- the rest
    are gaps and what they hold is ignored; a NaN or an infinity in a valid entry: ``ValueError``.  ``lags``: ``max_lag``
    or ``(first, step, count)`` in samples; ``stride``: frames per sample."""
    return transition_counts_batch([(a, edges, valid)], lags, stride, device)[0]
