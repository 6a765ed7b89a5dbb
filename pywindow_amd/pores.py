"""Pore sizes of a cage on the GPU: the probe-occupiable volume and the geometric pore size distribution for a ladder of
probes (``pw_pore_sizes``, include/pywindow_amd.h).

:func:`pywindow_amd.cavity_grid` gives the reach of a probe's CENTRE.  The room a guest of radius ``p`` can actually
fill is that reach dilated by the probe sphere (the probe-occupiable volume, Ongari et al., Langmuir 2017), and the
geometric pore size distribution (Gelb and Gubbins 1999) says, for every point of the void, how large a sphere can
contain it, fit between the atoms and be brought there from the pore centre.  One kernel gives both for up to 64 probes
a call: per level the cavity of ``pw_cavity`` for that probe, swept by a ball of ``K = floor(p^2 / h^2)`` in squared
voxel distances (by comparisons, nothing is divided), cut to the void at the first probe (the domain), and every voxel
of the domain attributed to the LARGEST level that covers it.  Every output of the kernel is an integer, so the result
is the same on the device and on the explicit host path (``device=-1``); volumes are ``count * spacing**3``.

The resolution in the probe radius is the grid's: a probe below ``spacing`` has ``K = 0`` and sweeps nothing beyond its
centres, and on a grid the raw swept volumes (``occupiable_volume``) need not fall monotonically with the probe --
``cumulative``, the reverse cumulative sum of the ``histogram``, does.  The reference has no counterpart.

* :func:`pore_size_distribution` -- one frame; :func:`pore_size_distribution_batch` -- many frames in one call;
  :class:`PoreSizes` -- the result, whose :meth:`PoreSizes.series` goes straight into
  :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
  :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`.
* ``Molecule.calculate_pore_size_distribution`` (molecular.py) and ``DLPOLY.pore_sizes`` (trajectory.py) seed at the
  optimised pore centre and close at the windows of the analysis, exactly as the cavity does.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .cavity import _grid, unpack_mask

__all__ = ["PoreSizes", "pore_size_distribution", "pore_size_distribution_batch"]

_LEVEL_SERIES = ("reach_volume", "occupiable_volume", "histogram", "cumulative", "distribution")
_FRAME_SERIES = ("mean_diameter", "median_diameter", "largest_probe", "domain_volume")


@dataclasses.dataclass(frozen=True)
class PoreSizes:
    """The pore sizes of one frame (``levels`` ``(L,)``, scalars) or of ``T`` frames (``levels`` ``(T, L)``, arrays with
    a leading frame axis) for the ladder ``probes`` ``(L,)``.  ``levels`` (``_lib.PORES_LEVEL_DTYPE``) and ``raw``
    (``_lib.PORES_OUT_DTYPE``) hold the integers of ``pw_pore_sizes``; ``origin`` is the centre of voxel ``(0, 0, 0)``
    and ``shape`` the grid ``(nx, ny, nz)``; ``masks``, when asked for, is a list of ``L`` ``(nz, ny, nx)`` bool arrays,
    the swept voxels of every level inside the domain (a list of such lists for many frames)."""

    levels: np.ndarray
    raw: np.ndarray
    probes: np.ndarray
    origin: np.ndarray
    shape: np.ndarray
    spacing: float
    masks: object = None
    frames: np.ndarray | None = None

    @property
    def _h3(self):
        return self.spacing * self.spacing * self.spacing

    @property
    def diameter(self) -> np.ndarray:
        """``2 * probes``: the sphere diameter of every level."""
        return 2.0 * self.probes

    @property
    def k2(self) -> np.ndarray:
        """``K`` of every level: the largest integer with ``K * spacing**2 <= probe**2``."""
        return self.levels["k2"]

    @property
    def reach_volume(self) -> np.ndarray:
        """Per level, what :func:`pywindow_amd.cavity_grid` gives for that probe: the reach of the probe's centre."""
        return self.levels["n_reach"] * self._h3

    @property
    def occupiable_volume(self) -> np.ndarray:
        """Per level, the probe-occupiable volume: the reach swept by the probe sphere, inside the domain."""
        return self.levels["n_swept"] * self._h3

    @property
    def histogram(self) -> np.ndarray:
        """Per level, the volume of the domain whose largest covering level it is."""
        return self.levels["n_largest"] * self._h3

    @property
    def cumulative(self) -> np.ndarray:
        """Per level, the volume that this level or a larger one covers: the reverse cumulative sum of ``histogram``,
        which never rises with the probe."""
        return np.cumsum(self.levels["n_largest"][..., ::-1], axis=-1)[..., ::-1] * self._h3

    @property
    def bin_width(self) -> np.ndarray:
        """The width in diameter of every level's bin: up to the next level; the last one as wide as the one before it
        (a single level: ``2 * spacing``, the resolution of the grid)."""
        d = self.diameter
        return np.append(np.diff(d), d[-1] - d[-2] if len(d) > 1 else 2.0 * self.spacing)

    @property
    def distribution(self) -> np.ndarray:
        """``histogram / bin_width``: the pore size distribution as a density in the diameter."""
        return self.histogram / self.bin_width

    @property
    def domain_volume(self):
        """The volume of the void at the first probe of the ladder, which the levels share out."""
        v = self.raw["n_domain"] * self._h3
        return v if self.raw.ndim else v[()]

    @property
    def mean_diameter(self):
        """The mean of ``diameter`` over the histogram; NaN for an empty domain."""
        n = self.levels["n_largest"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (n * self.diameter).sum(axis=-1) / n.sum(axis=-1)
        return v if self.raw.ndim else v[()]

    @property
    def median_diameter(self):
        """The diameter of the first level at which the histogram, summed from the smallest level up, holds half of the
        attributed voxels; NaN for an empty domain."""
        n = self.levels["n_largest"]
        below, total = np.cumsum(n, axis=-1), n.sum(axis=-1)
        first = np.argmax(2 * below >= total[..., None], axis=-1)
        v = np.where(total > 0, self.diameter[first], np.nan)
        return v if self.raw.ndim else v[()]

    @property
    def largest_probe(self):
        """The probe of the largest level whose reach is not empty; NaN if no level has one."""
        some = self.levels["n_reach"] > 0
        last = some.shape[-1] - 1 - np.argmax(some[..., ::-1], axis=-1)
        v = np.where(some.any(axis=-1), self.probes[last], np.nan)
        return v if self.raw.ndim else v[()]

    @property
    def closed(self):
        """The domain touches no face of its box and the seed was open at the first probe, as ``Cavity.closed``."""
        first = self.levels[..., 0]
        v = (first["n_face"] == 0) & ((first["flags"] & _lib.CAV_SEED_CLOSED) == 0)
        return v if self.raw.ndim else bool(v)

    def series(self, name: str = "occupiable_volume", level=None):
        """``(values, valid)`` of a quantity over the frames -- float64 values and ``valid = closed`` -- ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
        :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`.  ``name``: a quantity per
        level (``reach_volume``, ``occupiable_volume``, ``histogram``, ``cumulative``, ``distribution``) with its
        ``level``, or one per frame (``mean_diameter``, ``median_diameter``, ``largest_probe``, ``domain_volume``)."""
        if name in _LEVEL_SERIES:
            if level is None:
                raise ValueError(f"series: {name} needs a level, 0 .. {len(self.probes) - 1}")
            values = getattr(self, name)[..., int(level)]
        elif name in _FRAME_SERIES:
            values = getattr(self, name)
        else:
            raise KeyError(f"series: one of {_LEVEL_SERIES + _FRAME_SERIES}")
        return (np.atleast_1d(np.asarray(values, dtype=np.float64)).copy(),
                np.atleast_1d(np.asarray(self.closed, dtype=bool)).copy())


def default_probes(half_width: float, spacing: float) -> np.ndarray:
    """``0, spacing / 2, spacing, ...`` up to the half width, at most ``_lib.PORES_MAX_LEVELS`` levels."""
    step = spacing / 2.0
    return step * np.arange(min(int(math.floor(half_width / step)) + 1, _lib.PORES_MAX_LEVELS), dtype=np.float64)


def pore_size_distribution_batch(xyz, radii, seeds, probes=None, spacing: float = 0.5, half_widths=None, planes=None,
                                 masks: bool = False, device=None, frames=None) -> PoreSizes:
    """:func:`pore_size_distribution` for ``T`` frames of the same ``n`` atoms in ONE ``pw_pore_sizes`` call: ``xyz``
    ``(T, n, 3)``, ``radii`` ``(n,)``, ``seeds`` ``(T, 3)``, ``half_widths`` ``None`` or ``(T,)``, ``planes`` ``None`` or a
    list of ``T`` arrays ``(m_t, 4)`` (``None`` or an empty array: no planes for that frame).  Every frame has the same
    ladder (``probes=None``: up to the largest half width).  The fields of the result are arrays over the frames."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    r = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    if len(r) != n:
        raise ValueError("radii: one radius per atom")
    s = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    if len(s) != T:
        raise ValueError("seeds: one seed per frame")
    spacing = float(spacing)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError("spacing: a positive number")
    if half_widths is None:
        hw = (np.sqrt(((x - s[:, None, :]) ** 2).sum(axis=2)) + r[None, :]).max(axis=1) if n else np.full(T, spacing)
    else:
        hw = np.broadcast_to(np.asarray(half_widths, dtype=np.float64), (T,))
    if not np.isfinite(hw).all() or (hw <= 0.0).any():
        raise ValueError("half_width: positive and finite")
    q = default_probes(float(hw.max()) if T else spacing, spacing) if probes is None else \
        np.ascontiguousarray(probes, dtype=np.float64).reshape(-1)
    L = len(q)
    if L < 1 or L > _lib.PORES_MAX_LEVELS:
        raise ValueError(f"probes: at least one and at most {_lib.PORES_MAX_LEVELS} levels")
    if not np.isfinite(q).all() or (q < 0.0).any() or (np.diff(q) <= 0.0).any():
        raise ValueError("probes: finite, not negative and strictly ascending")
    jobs = np.zeros(T, dtype=_lib.PORES_JOB_DTYPE)
    cuts, at, words = [], 0, 0
    for t in range(T):
        g = _grid(float(hw[t]), spacing)
        p = None if planes is None else planes[t]
        p = np.zeros((0, 4)) if p is None else np.asarray(p, dtype=np.float64).reshape(-1, 4)
        jobs[t] = (t * n, n, 0, at, len(p), 0, L, t * L, words if masks else -1, t, s[t] - spacing * (g // 2 - 0.5), spacing,
                   g, g, g, (g // 2 - 1,) * 3)
        cuts.append(p)
        at += len(p)
        words += L * g * g if masks else 0
    levels, out, bits = engine.context(device).pore_sizes(jobs, x.reshape(-1, 3), r, q, np.concatenate(cuts) if cuts else None)
    unpacked = None
    if masks:
        unpacked = []
        for j in jobs:
            g, first = int(j["ny"]) * int(j["nz"]), int(j["mask_first"])
            unpacked.append([unpack_mask(bits[first + l * g:first + (l + 1) * g], int(j["nx"]), int(j["ny"]), int(j["nz"]))
                             for l in range(L)])
    shape = np.stack([jobs["nx"], jobs["ny"], jobs["nz"]], axis=1).astype(np.int64)
    return PoreSizes(levels.reshape(T, L), out, q, jobs["origin"].copy(), shape, spacing, unpacked,
                     None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def pore_size_distribution(xyz, radii, seed, probes=None, spacing: float = 0.5, half_width=None, planes=None,
                           masks: bool = False, device=None) -> PoreSizes:
    """The pore sizes around ``seed`` of the atoms ``xyz`` ``(n, 3)`` with the radii ``radii``: see :class:`PoreSizes`.
    The grid is exactly :func:`pywindow_amd.cavity_grid`'s -- centred on ``seed`` with an even
    ``G = 2 ceil(half_width / spacing)`` voxels an axis, ``G > 64`` a ``ValueError`` --, and so are ``planes`` and
    ``half_width``.  ``probes``: the ladder of probe radii, finite, not negative, strictly ascending, at most 64;
    ``None``: ``0, spacing / 2, spacing, ...`` up to the half width.  A ladder need not start at 0: the domain is the
    reach at its first probe.  ``masks=True`` keeps the swept voxels of every level.  ``xyz`` ``(T, n, 3)`` with ``seed``
    ``(T, 3)`` is :func:`pore_size_distribution_batch` with the same planes and half width for every frame.
    ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        T = len(x)
        return pore_size_distribution_batch(x, radii, seed, probes, spacing, None if half_width is None else np.full(T, half_width),
                                            None if planes is None else [planes] * T, masks, device)
    x = x.reshape(-1, 3)
    many = pore_size_distribution_batch(x[None], radii, np.asarray(seed, dtype=np.float64).reshape(1, 3), probes, spacing,
                                        None if half_width is None else [half_width], None if planes is None else [planes],
                                        masks, device)
    return PoreSizes(many.levels[0], many.raw[0], many.probes, many.origin[0], many.shape[0], many.spacing,
                     None if many.masks is None else many.masks[0])
