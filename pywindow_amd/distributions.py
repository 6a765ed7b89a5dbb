"""Distributions of analysis results: Gaussian kernel density estimates on the GPU, of one quantity or of two.

The step the reference's trajectory examples take right after ``DLPOLY.analysis()``
(examples/example_7.py:55-80, example_8.py:50-75): every window diameter, optimised pore diameter and
maximum diameter of the trajectory goes through ``scipy.stats.gaussian_kde(samples)(grid)``.  The
n x m sum of Gaussians is computed by ``pw_kde_sums`` (include/pywindow_amd.h; csrc/pw_kde.hip) -- many
curves in one launch -- and normalised here.  The bandwidth is SciPy's, to the bit (see
:func:`bandwidth`); the curve agrees with SciPy's to rounding ("Trajectory distributions").

* :func:`gaussian_kde_1d` -- one curve;  :func:`gaussian_kde_batch` -- many curves, one launch; both take
  ``weights=`` (SciPy's), which go through ``pw_kde_wsums``.
* :func:`gaussian_kde_replicas` -- one sample set under many weight vectors at a fixed bandwidth, every exponential
  computed once (``pw_kde_wsums``);  :func:`block_bootstrap_counts` -- the weight vectors of a circular moving-block
  bootstrap;  ``RecordStore.distribution_band`` / ``DLPOLY.distribution_band`` -> :class:`DistributionBand`, a curve
  with a pointwise error band that knows how correlated the frames are.
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

__all__ = ["Distribution", "Distribution2D", "DistributionBand", "bandwidth", "bandwidth_2d", "block_bootstrap_counts",
           "gaussian_kde_1d", "gaussian_kde_batch", "gaussian_kde_2d", "gaussian_kde_2d_batch", "gaussian_kde_replicas",
           "gaussian_kde_replicas_batch", "grid", "grid_2d"]


@dataclasses.dataclass(frozen=True)
class Distribution:
    """A density curve: ``density[j]`` at ``x[j]``, from ``n`` samples with a Gaussian kernel of standard
    deviation ``bandwidth`` = ``factor`` x the samples' standard deviation (``ddof=1``)."""

    x: np.ndarray
    density: np.ndarray
    n: int
    bandwidth: float
    factor: float


@dataclasses.dataclass(frozen=True)
class DistributionBand:
    """A density curve with a pointwise bootstrap band: ``density`` is the :class:`Distribution`'s own, ``lower`` and
    ``upper`` the ``(1 - level) / 2`` and ``1 - (1 - level) / 2`` quantiles over ``replicas`` block-bootstrap replicas
    (blocks of ``block`` steps of the frame axis), each a KDE of the resampled set at the ORIGINAL ``bandwidth``."""

    x: np.ndarray
    density: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    n: int
    bandwidth: float
    factor: float
    replicas: int
    block: int
    level: float


def _weights(weights, n: int) -> np.ndarray:
    """The weights of ``n`` samples as SciPy keeps them: a float array divided by its sum."""
    w = np.atleast_1d(weights).astype(float)
    if w.ndim != 1 or len(w) != n:
        raise ValueError(f"one weight per sample: {n} samples, weights of shape {w.shape}")
    if not np.isfinite(w).all() or (w < 0.0).any():
        raise ValueError("the weights must be finite and not negative")
    total = np.sum(w)
    if not total > 0.0:
        raise ValueError("the weights sum to zero")
    w /= total
    return w


def bandwidth(samples, bw_method="scott", weights=None) -> tuple[float, float]:
    """``(h, factor)`` with SciPy's meaning of ``bw_method``: ``"scott"`` (``n**-0.2``), ``"silverman"``
    (``(3n/4)**-0.2``) or a positive float, the factor itself; ``h**2`` is the factor squared times the sample
    variance (``ddof=1``).

    ``h`` equals ``sqrt(scipy.stats.gaussian_kde(samples, bw_method).covariance[0, 0])`` bit for bit, which
    fixes the route: SciPy takes the variance with uniform weights ``1/n`` (``np.cov(..., aweights=...)``),
    counts the samples as ``1 / sum(weights**2)`` -- not always exactly ``n`` -- and scales the variance, not
    its root.  Fewer than two samples, or samples that are all equal, raise ``ValueError``.

    ``weights`` (one per sample, not negative): ``h`` equals ``sqrt(gaussian_kde(samples, bw_method,
    weights=weights).covariance[0, 0])`` bit for bit by the same route -- the weights divided by their sum, the samples
    counted as ``neff = 1 / sum(w**2)``, ``np.cov(aweights=w)``.  Weights of the wrong length, negative, not finite or
    summing to zero raise ``ValueError``."""
    x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    n = len(x)
    if n < 2:
        raise ValueError(f"a density estimate needs at least two samples, got {n}")
    if not np.isfinite(x).all():
        raise ValueError("the samples contain NaN or infinity")
    weights = np.ones(n) / n if weights is None else _weights(weights, n)
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


def gaussian_kde_batch(sample_sets, point_sets, bw_method="scott", device=None, weights=None) -> list:
    """One :class:`Distribution` per (samples, points) pair, all from ONE ``pw_kde_sums`` call.  ``device``:
    the HIP ordinal (``None``: the process's, ``engine.resolve_device``); ``-1`` the explicit host path.
    ``weights``: a list with one array of weights (SciPy's ``weights=``) or ``None`` per set; the weighted sets go
    through one ``pw_kde_wsums`` call, the others through ``pw_kde_sums`` as before."""
    xs = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in sample_sets]
    gs = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1) for p in point_sets]
    if len(xs) != len(gs):
        raise ValueError("one set of points per set of samples")
    ws = [None] * len(xs) if weights is None else list(weights)
    if len(ws) != len(xs):
        raise ValueError("one array of weights, or None, per set of samples")
    hs = [bandwidth(x, bw_method, w) for x, w in zip(xs, ws)]
    for g in gs:
        if not np.isfinite(g).all():
            raise ValueError("the points contain NaN or infinity")
    if not len(xs):
        return []
    out = [None] * len(xs)
    plain = [k for k, w in enumerate(ws) if w is None]
    if plain:
        jobs = np.zeros(len(plain), dtype=_lib.KDE_JOB_DTYPE)
        jobs["n_samples"] = [len(xs[k]) for k in plain]
        jobs["n_points"] = [len(gs[k]) for k in plain]
        jobs["sample_first"] = np.cumsum(jobs["n_samples"]) - jobs["n_samples"]
        jobs["point_first"] = np.cumsum(jobs["n_points"]) - jobs["n_points"]
        jobs["inv_bandwidth"] = [1.0 / hs[k][0] for k in plain]
        sums = engine.context(device).kde_sums(jobs, np.concatenate([xs[k] for k in plain]), np.concatenate([gs[k] for k in plain]))
        for job, k in zip(jobs, plain):
            n, (h, factor) = int(job["n_samples"]), hs[k]
            s = sums[int(job["point_first"]):int(job["point_first"]) + len(gs[k])]
            out[k] = Distribution(gs[k], s / (n * h * math.sqrt(2.0 * math.pi)), n, h, factor)
    heavy = [k for k, w in enumerate(ws) if w is not None]
    if heavy:
        rows = [_weights(ws[k], len(xs[k]))[None, :] for k in heavy]
        curves = gaussian_kde_replicas_batch([xs[k] for k in heavy], [gs[k] for k in heavy], rows, [hs[k][0] for k in heavy], device)
        for k, c in zip(heavy, curves):
            out[k] = Distribution(gs[k], c[0], len(xs[k]), hs[k][0], hs[k][1])
    return out


def gaussian_kde_1d(samples, points, bw_method="scott", device=None, weights=None) -> Distribution:
    """``scipy.stats.gaussian_kde(samples, bw_method, weights=weights)(points)`` for one-dimensional samples, summed
    on the GPU."""
    return gaussian_kde_batch([samples], [points], bw_method, device, None if weights is None else [weights])[0]


def gaussian_kde_replicas_batch(sample_sets, point_sets, weight_sets, bandwidths, device=None) -> list:
    """One ``(R_k, m_k)`` array of densities per (samples ``(n_k,)``, points ``(m_k,)``, weights ``(R_k, n_k)``,
    bandwidth ``h_k``), all from ONE ``pw_kde_wsums`` call: row ``b`` is the KDE of the samples under the weights
    ``weights[b]`` -- each row normalised by its own sum -- with a Gaussian kernel of standard deviation ``h_k``.  Every
    exponential is computed once and shared by the set's rows."""
    xs = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in sample_sets]
    gs = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1) for p in point_sets]
    ws = [np.ascontiguousarray(w, dtype=np.float64) for w in weight_sets]
    hs = [float(h) for h in bandwidths]
    if not (len(xs) == len(gs) == len(ws) == len(hs)):
        raise ValueError("one set of points, one array of weights and one bandwidth per set of samples")
    norms = []
    for x, g, w, h in zip(xs, gs, ws, hs):
        if w.ndim != 2 or w.shape[1] != len(x) or w.shape[0] < 1:
            raise ValueError(f"the weights of {len(x)} samples are an (R, {len(x)}) array with R >= 1, got shape {w.shape}")
        if not (np.isfinite(x).all() and np.isfinite(g).all()):
            raise ValueError("the samples or the points contain NaN or infinity")
        if not np.isfinite(w).all() or (w < 0.0).any():
            raise ValueError("the weights must be finite and not negative")
        if not (math.isfinite(h) and h > 0.0):
            raise ValueError("the bandwidth is not a positive finite number")
        total = np.sum(w, axis=1)
        if not (total > 0.0).all():
            raise ValueError("a row of weights sums to zero")
        norms.append(total * (h * math.sqrt(2.0 * math.pi)))
    if not xs:
        return []
    jobs = np.zeros(len(xs), dtype=_lib.KDEW_JOB_DTYPE)
    jobs["n_samples"] = [len(x) for x in xs]
    jobs["n_points"] = [len(g) for g in gs]
    jobs["n_replicas"] = [w.shape[0] for w in ws]
    jobs["sample_first"] = np.cumsum(jobs["n_samples"]) - jobs["n_samples"]
    jobs["point_first"] = np.cumsum(jobs["n_points"]) - jobs["n_points"]
    sizes = jobs["n_samples"] * jobs["n_replicas"]
    jobs["weight_first"] = np.cumsum(sizes) - sizes
    sizes = jobs["n_points"] * jobs["n_replicas"]
    jobs["out_first"] = np.cumsum(sizes) - sizes
    jobs["inv_bandwidth"] = [1.0 / h for h in hs]
    # (sample-major for the kernel: a sample's weights under all replicas lie side by side)
    sums = engine.context(device).kde_wsums(jobs, np.concatenate(xs), np.concatenate(gs),
                                            np.concatenate([np.ascontiguousarray(w.T).reshape(-1) for w in ws]))
    out = []
    for job, g, w, norm in zip(jobs, gs, ws, norms):
        first = int(job["out_first"])
        out.append(sums[first:first + w.shape[0] * len(g)].reshape(w.shape[0], len(g)) / norm[:, None])
    return out


def gaussian_kde_replicas(samples, points, weights, bandwidth, device=None) -> np.ndarray:
    """``(R, m)`` densities: the KDE of ``samples`` at ``points`` under each of the ``R`` rows of ``weights`` (``(R, n)``,
    each row normalised by its own sum; a row that sums to zero is a ``ValueError``) with a Gaussian kernel of standard
    deviation ``bandwidth``.  The replicas of a bootstrap are such rows: integer multiplicities."""
    return gaussian_kde_replicas_batch([samples], [points], [weights], [bandwidth], device)[0]


def block_bootstrap_counts(n_times: int, block: int, replicas: int, seed=0) -> np.ndarray:
    """``(replicas, n_times)`` int64: how often every time of a series of ``n_times`` steps is drawn by each replica of
    a CIRCULAR MOVING-BLOCK bootstrap.  A replica takes ``ceil(n_times / block)`` blocks of ``block`` consecutive
    times, their starts drawn by ``np.random.default_rng(seed).integers(0, n_times, (replicas, blocks))``; blocks wrap
    round the end of the series and the last one is cut so that every row sums to exactly ``n_times``.  ``block = 1``
    is the ordinary bootstrap; ``block`` about twice the correlation time keeps the dependence of neighbouring frames
    inside the blocks."""
    n_times, block, replicas = int(n_times), int(block), int(replicas)
    if n_times < 1 or block < 1 or replicas < 1:
        raise ValueError("n_times, block and replicas must be at least 1")
    blocks = -(-n_times // block)
    starts = np.random.default_rng(seed).integers(0, n_times, (replicas, blocks))
    step = np.arange(n_times)                                    # the draws of a replica, in order: block, offset in it
    drawn = (starts[:, step // block] + step % block) % n_times
    rows = np.repeat(np.arange(replicas), n_times)
    return np.bincount(rows * n_times + drawn.reshape(-1), minlength=replicas * n_times).reshape(replicas, n_times).astype(np.int64)


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
