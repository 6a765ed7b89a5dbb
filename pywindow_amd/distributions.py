"""Distributions of analysis results: Gaussian kernel density estimates on the GPU, of one quantity or of two.

The step the reference's trajectory examples take right after ``DLPOLY.analysis()``
(examples/example_7.py:55-80, example_8.py:50-75): every window diameter, optimised pore diameter and
maximum diameter of the trajectory goes through ``scipy.stats.gaussian_kde(samples)(grid)``.  The
n x m sum of Gaussians is computed by ``pw_kde_sums`` (include/pywindow_amd.h; csrc/pw_kde.hip) -- many
curves in one launch -- and normalised here.  The bandwidth is SciPy's, to the bit (see
:func:`bandwidth`); the curve agrees with SciPy's to rounding ("Trajectory distributions").

* :func:`gaussian_kde_1d` -- one curve;  :func:`gaussian_kde_batch` -- many curves, one launch.
* :func:`gaussian_kde_2d` -- the joint density of two quantities on a mesh (``gaussian_kde`` with a ``2 x n``
  dataset; ``pw_kde2_sums``);  :func:`gaussian_kde_2d_batch` -- many maps, one call.
* ``RecordStore.samples`` / ``.distribution`` / ``.sample_pairs`` / ``.joint_distribution`` (records.py) and
  ``DLPOLY.distribution`` / ``.joint_distribution`` (trajectory.py) take the samples from the records of an analysis.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["Distribution", "Distribution2D", "bandwidth", "bandwidth_2d", "gaussian_kde_1d", "gaussian_kde_batch",
           "gaussian_kde_2d", "gaussian_kde_2d_batch", "grid", "grid_2d"]


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


# ---- two quantities ----------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Distribution2D:
    """A joint density on a mesh: ``density[iy, ix]`` at ``(x[ix], y[iy])``, from ``n`` sample pairs with a
    Gaussian kernel of covariance ``covariance`` = ``factor**2`` x the samples' covariance (``ddof=1``)."""

    x: np.ndarray
    y: np.ndarray
    density: np.ndarray
    n: int
    covariance: np.ndarray
    factor: float


def _whitening(covariance) -> tuple[float, float, float, float]:
    """``(w00, w10, w11, l00 * l11)``: the inverse of the Cholesky factor ``L`` of a 2 x 2 covariance and the root
    of its determinant.  ``ValueError`` when the matrix is not positive definite."""
    c00, c10, c11 = float(covariance[0, 0]), float(covariance[1, 0]), float(covariance[1, 1])
    if not (math.isfinite(c00) and c00 > 0.0):
        raise ValueError("the kernel's covariance is not positive definite: the first quantity is constant (its variance is zero)")
    if not (math.isfinite(c11) and c11 > 0.0):
        raise ValueError("the kernel's covariance is not positive definite: the second quantity is constant (its variance is zero)")
    l00 = math.sqrt(c00)
    l10 = c10 / l00
    rest = c11 - l10 * l10
    # (l10 * l10 carries two roundings: a remainder within 8 * 2^-53 of c11 is zero as far as doubles can tell)
    if not (math.isfinite(rest) and rest > 8.0 * 2.0 ** -53 * c11):
        raise ValueError("the kernel's covariance is not positive definite: the two quantities are exactly linearly dependent")
    l11 = math.sqrt(rest)
    w = (1.0 / l00, -l10 / (l00 * l11), 1.0 / l11, l00 * l11)
    if not all(math.isfinite(v) for v in w) or not w[3] > 0.0:
        raise ValueError("the kernel's covariance is not positive definite: its factors are not finite")
    return w


def bandwidth_2d(samples, bw_method="scott") -> tuple[np.ndarray, float]:
    """``(covariance, factor)`` of the kernel for a ``2 x n`` dataset, SciPy's meaning of ``bw_method``:
    ``"scott"`` (``n**(-1/6)``), ``"silverman"`` (``(n (d + 2) / 4)**(-1 / (d + 4))``, which for ``d = 2`` IS Scott's
    factor, to the bit) or a positive float, the factor itself.

    ``covariance`` equals ``scipy.stats.gaussian_kde(samples, bw_method).covariance`` bit for bit, which fixes the
    route: ``np.cov`` with uniform weights ``1/n``, the samples counted as ``1 / sum(weights**2)``, the matrix scaled
    by the squared factor.  Fewer than three pairs, a NaN or infinity, or a covariance that is not positive
    definite (one quantity constant, or the two exactly linearly dependent) raise ``ValueError``."""
    d = np.ascontiguousarray(samples, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != 2:
        raise ValueError(f"the samples of a joint density are a 2 x n array, got shape {d.shape}")
    n = d.shape[1]
    if n < 3:
        raise ValueError(f"a joint density estimate needs at least three sample pairs, got {n}")
    if not np.isfinite(d).all():
        raise ValueError("the samples contain NaN or infinity")
    weights = np.ones(n) / n
    neff = 1.0 / np.sum(weights ** 2)
    if isinstance(bw_method, str):
        if bw_method == "scott":
            factor = np.power(neff, -1.0 / (2 + 4))
        elif bw_method == "silverman":
            factor = np.power(neff * (2 + 2.0) / 4.0, -1.0 / (2 + 4))
        else:
            raise ValueError(f"bw_method must be 'scott', 'silverman' or a positive number, not {bw_method!r}")
    else:
        factor = float(bw_method)
        if not (math.isfinite(factor) and factor > 0.0):
            raise ValueError(f"bw_method must be 'scott', 'silverman' or a positive number, not {bw_method!r}")
    covariance = np.atleast_2d(np.cov(d, rowvar=True, bias=False, aweights=weights)) * factor ** 2
    _whitening(covariance)
    return covariance, float(factor)


def grid_2d(samples_x, samples_y, points=128, pad: float = 1.0) -> tuple[np.ndarray, np.ndarray]:
    """The two axes of a mesh.  ``points``: an int, or a pair of ints, for ``np.linspace(min - pad, max + pad, .)`` per
    axis; or the two axes themselves, used as given."""
    if isinstance(points, (int, np.integer)):
        points = (points, points)
    if len(points) != 2:
        raise ValueError("points: an int, a pair of ints, or the two axes of the mesh")
    return grid(samples_x, points[0], pad), grid(samples_y, points[1], pad)


def gaussian_kde_2d_batch(sample_sets, axes_sets, bw_method="scott", device=None) -> list:
    """One :class:`Distribution2D` per ((samples_x, samples_y), (x axis, y axis)) pair, all from ONE ``pw_kde2_sums``
    call.  ``device`` as in :func:`gaussian_kde_batch`."""
    sample_sets, axes_sets = list(sample_sets), list(axes_sets)
    if len(sample_sets) != len(axes_sets):
        raise ValueError("one pair of axes per set of samples")
    data, kernels, axes = [], [], []
    for (sx, sy), (ax, ay) in zip(sample_sets, axes_sets):
        sx = np.ascontiguousarray(sx, dtype=np.float64).reshape(-1)
        sy = np.ascontiguousarray(sy, dtype=np.float64).reshape(-1)
        if len(sx) != len(sy):
            raise ValueError(f"the two quantities have {len(sx)} and {len(sy)} samples: a joint density needs pairs")
        d = np.stack([sx, sy])
        covariance, factor = bandwidth_2d(d, bw_method)
        ax = np.ascontiguousarray(ax, dtype=np.float64).reshape(-1)
        ay = np.ascontiguousarray(ay, dtype=np.float64).reshape(-1)
        if not (np.isfinite(ax).all() and np.isfinite(ay).all()):
            raise ValueError("the points contain NaN or infinity")
        data.append(d)
        kernels.append((covariance, factor, _whitening(covariance)))
        axes.append((ax, ay))
    if not data:
        return []
    jobs = np.zeros(len(data), dtype=_lib.KDE2_JOB_DTYPE)
    jobs["n_samples"] = [d.shape[1] for d in data]
    jobs["n_points"] = [len(ax) * len(ay) for ax, ay in axes]
    jobs["sample_first"] = np.cumsum(jobs["n_samples"]) - jobs["n_samples"]
    jobs["point_first"] = np.cumsum(jobs["n_points"]) - jobs["n_points"]
    for name, col in (("w00", 0), ("w10", 1), ("w11", 2)):
        jobs[name] = [k[2][col] for k in kernels]
    # point j = iy * nx + ix of a mesh is (x[ix], y[iy]): the sums come back as density's (ny, nx)
    mesh = [np.stack([np.tile(ax, len(ay)), np.repeat(ay, len(ax))], axis=1) for ax, ay in axes]
    sums = engine.context(device).kde2_sums(jobs, np.concatenate([d.T for d in data]), np.concatenate(mesh))
    out = []
    for job, d, (ax, ay), (covariance, factor, w) in zip(jobs, data, axes, kernels):
        n, first = d.shape[1], int(job["point_first"])
        s = sums[first:first + len(ax) * len(ay)].reshape(len(ay), len(ax))
        out.append(Distribution2D(ax, ay, s / (n * (2.0 * math.pi) * w[3]), n, covariance, factor))
    return out


def gaussian_kde_2d(samples_x, samples_y, points=128, bw_method="scott", device=None, pad: float = 1.0) -> Distribution2D:
    """``scipy.stats.gaussian_kde(np.vstack([samples_x, samples_y]), bw_method)`` on the mesh of :func:`grid_2d`
    (``points``, ``pad``), summed on the GPU: ``density[iy, ix]`` is SciPy's value at ``(x[ix], y[iy])``."""
    return gaussian_kde_2d_batch([(samples_x, samples_y)], [grid_2d(samples_x, samples_y, points, pad)], bw_method, device)[0]
