"""Distributions of analysis results: one-dimensional Gaussian kernel density estimates on the GPU.

The step the reference's trajectory examples take right after ``DLPOLY.analysis()``
(examples/example_7.py:55-80, example_8.py:50-75): every window diameter, optimised pore diameter and
maximum diameter of the trajectory goes through ``scipy.stats.gaussian_kde(samples)(grid)``.  The
n x m sum of Gaussians is computed by ``pw_kde_sums`` (include/pywindow_amd.h; csrc/pw_kde.hip) -- many
curves in one launch -- and normalised here.  The bandwidth is SciPy's, to the bit (see
:func:`bandwidth`); the curve agrees with SciPy's to rounding ("Trajectory distributions").

* :func:`gaussian_kde_1d` -- one curve;  :func:`gaussian_kde_batch` -- many curves, one launch.
* ``RecordStore.samples`` / ``RecordStore.distribution`` (records.py) and ``DLPOLY.distribution``
  (trajectory.py) take the samples from the records of an analysis.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["Distribution", "bandwidth", "gaussian_kde_1d", "gaussian_kde_batch"]


@dataclasses.dataclass(frozen=True)
class Distribution:
    """A density curve: ``density[j]`` at ``x[j]``, from ``n`` samples with a Gaussian kernel of standard
    deviation ``bandwidth`` = ``factor`` x the samples' standard deviation (``ddof=1``)."""

    x: np.ndarray
    density: np.ndarray
    n: int
    bandwidth: float
    factor: float


def bandwidth(samples, bw_method="scott") -> tuple[float, float]:
    """``(h, factor)`` with SciPy's meaning of ``bw_method``: ``"scott"`` (``n**-0.2``), ``"silverman"``
    (``(3n/4)**-0.2``) or a positive float, the factor itself; ``h**2`` is the factor squared times the sample
    variance (``ddof=1``).

    ``h`` equals ``sqrt(scipy.stats.gaussian_kde(samples, bw_method).covariance[0, 0])`` bit for bit, which
    fixes the route: SciPy takes the variance with uniform weights ``1/n`` (``np.cov(..., aweights=...)``),
    counts the samples as ``1 / sum(weights**2)`` -- not always exactly ``n`` -- and scales the variance, not
    its root.  Fewer than two samples, or samples that are all equal, raise ``ValueError``."""
    x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    n = len(x)
    if n < 2:
        raise ValueError(f"a density estimate needs at least two samples, got {n}")
    if not np.isfinite(x).all():
        raise ValueError("the samples contain NaN or infinity")
    weights = np.ones(n) / n
    neff = 1.0 / np.sum(weights ** 2)
    if isinstance(bw_method, str):
        if bw_method == "scott":
            factor = np.power(neff, -1.0 / 5.0)
        elif bw_method == "silverman":
            factor = np.power(neff * 3.0 / 4.0, -1.0 / 5.0)
        else:
            raise ValueError(f"bw_method must be 'scott', 'silverman' or a positive number, not {bw_method!r}")
    else:
        factor = float(bw_method)
        if not (math.isfinite(factor) and factor > 0.0):
            raise ValueError(f"bw_method must be 'scott', 'silverman' or a positive number, not {bw_method!r}")
    variance = float(np.cov(x, rowvar=True, bias=False, aweights=weights))
    if not variance > 0.0:
        raise ValueError("the samples are all equal: their variance is zero and no bandwidth follows from it")
    h = math.sqrt(variance * factor ** 2)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError("the bandwidth is not a positive finite number")
    return h, float(factor)


def gaussian_kde_batch(sample_sets, point_sets, bw_method="scott", device=None) -> list:
    """One :class:`Distribution` per (samples, points) pair, all from ONE ``pw_kde_sums`` call.  ``device``:
    the HIP ordinal (``None``: the process's, ``engine.resolve_device``); ``-1`` the explicit host path."""
    xs = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in sample_sets]
    gs = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1) for p in point_sets]
    if len(xs) != len(gs):
        raise ValueError("one set of points per set of samples")
    hs = [bandwidth(x, bw_method) for x in xs]
    for g in gs:
        if not np.isfinite(g).all():
            raise ValueError("the points contain NaN or infinity")
    jobs = np.zeros(len(xs), dtype=_lib.KDE_JOB_DTYPE)
    jobs["n_samples"] = [len(x) for x in xs]
    jobs["n_points"] = [len(g) for g in gs]
    jobs["sample_first"] = np.cumsum(jobs["n_samples"]) - jobs["n_samples"]
    jobs["point_first"] = np.cumsum(jobs["n_points"]) - jobs["n_points"]
    jobs["inv_bandwidth"] = [1.0 / h for h, _ in hs]
    if not len(xs):
        return []
    sums = engine.context(device).kde_sums(jobs, np.concatenate(xs), np.concatenate(gs))
    out = []
    for job, g, (h, factor) in zip(jobs, gs, hs):
        n = int(job["n_samples"])
        s = sums[int(job["point_first"]):int(job["point_first"]) + len(g)]
        out.append(Distribution(g, s / (n * h * math.sqrt(2.0 * math.pi)), n, h, factor))
    return out


def gaussian_kde_1d(samples, points, bw_method="scott", device=None) -> Distribution:
    """``scipy.stats.gaussian_kde(samples, bw_method)(points)`` for one-dimensional samples, summed on the GPU."""
    return gaussian_kde_batch([samples], [points], bw_method, device)[0]


def grid(samples, points=1000, pad: float = 1.0) -> np.ndarray:
    """``points`` as an int: ``np.linspace(min - pad, max + pad, points)`` as the reference's examples do; an
    array is used as given."""
    if isinstance(points, (int, np.integer)):
        s = np.asarray(samples, dtype=np.float64)
        if not len(s):
            raise ValueError("no samples: a density estimate needs at least two")
        return np.linspace(s.min() - pad, s.max() + pad, int(points))
    return np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
