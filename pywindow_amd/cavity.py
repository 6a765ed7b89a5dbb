"""The cavity of a cage on the GPU: a voxel flood fill from the pore centre, closed at the windows (``pw_cavity``,
include/pywindow_amd.h).

``pore_volume`` and ``pore_volume_opt`` are ``4/3 pi r^3`` of the largest inscribed sphere, as in the reference: a lower
bound on the void.  The cavity here is the region that the CENTRE of a probe of radius ``probe`` can reach from a seed
point without entering an atom's van der Waals sphere (grown by the probe) and without crossing a plane laid through a
window (:func:`pywindow_amd.utilities.window_planes`).  It is counted on a grid of at most 64 voxels an axis; every
output of the kernel is an integer, so the result is the same on the device and on the explicit host path
(``device=-1``), and volume, centroid and gyration tensor are a few IEEE operations on those integers.  The volume is
that of the probe centre's reach; the probe-swept (dilated) one is :mod:`pywindow_amd.pores`.  The reference has no
counterpart.

* :func:`cavity_grid` -- one frame, or many frames in one call; :class:`Cavity` -- the result, whose
  :meth:`Cavity.series` goes straight into :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`,
  :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics` and
  :func:`pywindow_amd.transition_counts`.
* ``Molecule.calculate_cavity`` (molecular.py) and ``DLPOLY.cavity`` (trajectory.py) seed at the optimised pore centre
  and close at the windows of the analysis.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["Cavity", "cavity_grid", "cavity_grid_batch"]

_SERIES = ("volume", "n_voxels", "n_open", "n_surface", "n_face", "asphericity", "acylindricity",
           "relative_shape_anisotropy")


@dataclasses.dataclass(frozen=True)
class Cavity:
    """One cavity (scalars, ``centroid`` (3,), ``gyration`` (3, 3)) or one per frame (arrays with a leading frame axis).
    ``raw`` holds the integers of ``pw_cavity`` (``_lib.CAVITY_OUT_DTYPE``); ``origin`` is the centre of voxel
    ``(0, 0, 0)`` and ``shape`` the grid ``(nx, ny, nz)``; ``mask``, when asked for, is a ``(nz, ny, nx)`` bool array (a
    list of them for many frames).  ``closed``: the cavity touches no face of its box and the seed was open -- only then
    is ``volume`` the volume of a cavity rather than of whatever part of space the box cut out.  ``words``: with a
    mask, the same voxels as ``pw_cavity`` wrote them -- ``ny * nz`` uint64 a frame, row ``(j, l)`` at ``l * ny + j``,
    bit ``i`` voxel ``i`` -- which is what :func:`pywindow_amd.surface_area` hands on."""

    raw: np.ndarray
    origin: np.ndarray
    shape: np.ndarray
    spacing: float
    probe: float
    mask: object = None
    frames: np.ndarray | None = None
    words: object = None

    def _field(self, name):
        v = self.raw[name]
        return v if self.raw.ndim else v[()]

    @property
    def n_voxels(self):
        return self._field("n_voxels")

    @property
    def n_open(self):
        return self._field("n_open")

    @property
    def n_surface(self):
        return self._field("n_surface")

    @property
    def n_face(self):
        return self._field("n_face")

    @property
    def seed_closed(self):
        return (self._field("flags") & _lib.CAV_SEED_CLOSED) != 0

    @property
    def closed(self):
        return (self._field("n_face") == 0) & ~self.seed_closed

    @property
    def volume(self):
        """``n_voxels * spacing**3``."""
        return self._field("n_voxels") * (self.spacing * self.spacing * self.spacing)

    def _mean_index(self):
        n = np.asarray(self.raw["n_voxels"], dtype=np.float64)[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.asarray(self.raw["first"], dtype=np.float64) / n, n

    @property
    def centroid(self) -> np.ndarray:
        """``origin + spacing * sum(i, j, l) / n_voxels``; NaN for an empty cavity."""
        mean, _ = self._mean_index()
        return self.origin + self.spacing * mean

    @property
    def gyration(self) -> np.ndarray:
        """The gyration tensor of the voxel centres, ``spacing**2 * (sum(ab) / n - sum(a) sum(b) / n**2)``, (3, 3)."""
        mean, n = self._mean_index()
        s = np.asarray(self.raw["second"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            m2 = s / n
        g = np.empty(mean.shape[:-1] + (3, 3))
        for (a, b), col in (((0, 0), 0), ((1, 1), 1), ((2, 2), 2), ((0, 1), 3), ((0, 2), 4), ((1, 2), 5)):
            g[..., a, b] = g[..., b, a] = (m2[..., col] - mean[..., a] * mean[..., b]) * (self.spacing * self.spacing)
        return g

    def _eigenvalues(self) -> np.ndarray:
        g = self.gyration
        ok = np.isfinite(g).all(axis=(-1, -2))
        ev = np.full(g.shape[:-1], np.nan)
        if ok.any():
            ev[ok] = np.linalg.eigvalsh(g[ok])[..., ::-1]            # descending, as utilities' sorted eigenvalues
        return ev

    @property
    def asphericity(self):
        """``l0 - (l1 + l2) / 2`` of the descending eigenvalues of ``gyration`` (the formula of ``calc_asphericity``)."""
        ev = self._eigenvalues()
        return ev[..., 0] - (ev[..., 1] + ev[..., 2]) / 2.0

    @property
    def acylindricity(self):
        """``l1 - l2`` (``calc_acylidricity``)."""
        ev = self._eigenvalues()
        return ev[..., 1] - ev[..., 2]

    @property
    def relative_shape_anisotropy(self):
        """``1 - 3 (l0 l1 + l0 l2 + l1 l2) / (l0 + l1 + l2)**2`` (``calc_relative_shape_anisotropy``)."""
        ev = self._eigenvalues()
        tr = (ev[..., 0] + ev[..., 1]) + ev[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            return 1.0 - 3.0 * ((((ev[..., 0] * ev[..., 1]) + (ev[..., 0] * ev[..., 2])) + (ev[..., 1] * ev[..., 2])) / (tr * tr))

    def series(self, name: str = "volume"):
        """``(values, valid)`` of a quantity over the frames -- float64 values and ``valid = closed`` -- ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
        :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        values = np.atleast_1d(np.asarray(getattr(self, name), dtype=np.float64)).copy()
        return values, np.atleast_1d(np.asarray(self.closed, dtype=bool)).copy()


def _grid(half_width: float, spacing: float) -> int:
    g = 2 * int(math.ceil(half_width / spacing))
    g = max(g, 2)
    if g > _lib.CAVITY_MAX_G:
        need = half_width / (_lib.CAVITY_MAX_G // 2)
        raise ValueError(f"cavity_grid: a box of half width {half_width:.6g} needs {g} voxels an axis at spacing "
                         f"{spacing:.6g}, more than {_lib.CAVITY_MAX_G}: the smallest spacing that fits is {need:.6g}")
    return g


def unpack_mask(words: np.ndarray, nx: int, ny: int, nz: int) -> np.ndarray:
    """The ``ny * nz`` words of a job's mask as a ``(nz, ny, nx)`` bool array."""
    bits = (words.reshape(nz, ny, 1) >> np.arange(nx, dtype=np.uint64)) & np.uint64(1)
    return bits.astype(bool)


def cavity_grid_batch(xyz, radii, seeds, probe: float = 0.0, spacing: float = 0.5, half_widths=None, planes=None,
                      mask: bool = False, device=None, frames=None) -> Cavity:
    """:func:`cavity_grid` for ``T`` frames of the same ``n`` atoms in ONE ``pw_cavity`` call: ``xyz`` ``(T, n, 3)``,
    ``radii`` ``(n,)``, ``seeds`` ``(T, 3)``, ``half_widths`` ``None`` or ``(T,)``, ``planes`` ``None`` or a list of ``T``
    arrays ``(m_t, 4)`` (``None`` or an empty array: no planes for that frame).  The fields of the result are arrays
    over the frames."""
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
    spacing, probe = float(spacing), float(probe)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError("spacing: a positive number")
    if half_widths is None:
        hw = (np.sqrt(((x - s[:, None, :]) ** 2).sum(axis=2)) + r[None, :]).max(axis=1) if n else np.full(T, spacing)
    else:
        hw = np.broadcast_to(np.asarray(half_widths, dtype=np.float64), (T,))
    if not np.isfinite(hw).all() or (hw <= 0.0).any():
        raise ValueError("half_width: positive and finite")
    jobs = np.zeros(T, dtype=_lib.CAVITY_JOB_DTYPE)
    cuts, at, words = [], 0, 0
    for t in range(T):
        g = _grid(float(hw[t]), spacing)
        p = None if planes is None else planes[t]
        p = np.zeros((0, 4)) if p is None else np.asarray(p, dtype=np.float64).reshape(-1, 4)
        jobs[t] = (t * n, n, 0, at, len(p), words if mask else -1, t, s[t] - spacing * (g // 2 - 0.5), spacing, probe,
                   g, g, g, (g // 2 - 1,) * 3)
        cuts.append(p)
        at += len(p)
        words += g * g if mask else 0
    out, bits = engine.context(device).cavity(jobs, x.reshape(-1, 3), r, np.concatenate(cuts) if cuts else None)
    masks = words = None
    if mask:
        words = [bits[int(j["mask_first"]):int(j["mask_first"]) + int(j["ny"]) * int(j["nz"])] for j in jobs]
        masks = [unpack_mask(w, int(j["nx"]), int(j["ny"]), int(j["nz"])) for w, j in zip(words, jobs)]
    shape = np.stack([jobs["nx"], jobs["ny"], jobs["nz"]], axis=1).astype(np.int64)
    return Cavity(out, jobs["origin"].copy(), shape, spacing, probe, masks,
                  None if frames is None else np.array(frames, dtype=np.int64).reshape(-1), words)


def cavity_grid(xyz, radii, seed, probe: float = 0.0, spacing: float = 0.5, half_width=None, planes=None,
                mask: bool = False, device=None) -> Cavity:
    """The cavity around ``seed`` of the atoms ``xyz`` ``(n, 3)`` with the radii ``radii`` for a probe of radius
    ``probe``: see :class:`Cavity`.  The box is centred on ``seed`` with an even ``G = 2 ceil(half_width / spacing)``
    voxels an axis, its origin ``seed - spacing (G/2 - 0.5)`` and the seed voxel ``G/2 - 1`` (the voxel centres straddle
    the seed; nothing is divided on any path); ``half_width`` defaults to the largest ``|atom - seed| + radius``.
    ``G > 64``: ``ValueError`` naming the smallest spacing that fits -- the grid is never coarsened silently.
    ``planes``: rows ``(a, b, c, d)``; only voxels with ``a x + b y + c z <= d`` for every row are open.  ``xyz``
    ``(T, n, 3)`` with ``seed`` ``(T, 3)`` is :func:`cavity_grid_batch` with the same planes and half width for every
    frame.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        T = len(x)
        return cavity_grid_batch(x, radii, seed, probe, spacing, None if half_width is None else np.full(T, half_width),
                                 None if planes is None else [planes] * T, mask, device)
    x = x.reshape(-1, 3)
    many = cavity_grid_batch(x[None], radii, np.asarray(seed, dtype=np.float64).reshape(1, 3), probe, spacing,
                             None if half_width is None else [half_width], None if planes is None else [planes], mask,
                             device)
    return Cavity(many.raw[0], many.origin[0], many.shape[0], many.spacing, many.probe,
                  None if many.mask is None else many.mask[0], None, None if many.words is None else many.words[0])
