"""Guest percolation on the GPU: the energy levels at which the voids of a crystal connect for a guest
(``pw_percolation``, include/pywindow_amd.h; the definition and its proofs in pywindow_amd/csrc/pw_percolate.hpp).

:func:`pywindow_amd.channel_network` answers the hard-sphere question -- is the void a network, in how many dimensions,
up to which probe radius.  A soft wall lets a guest pass that is wider than the static window; what decides passage is
the energy barrier.  Here the periodic Lennard-Jones landscape of one guest is computed on the cell's own grid, and for
each of six connection criteria -- the landscape connects to its own periodic images in at least 1, 2, 3 dimensions; a
closed path winds along a, b, c -- the lowest energy level is found at which the sub-level set holds a component that
meets it: the minimax (bottleneck) barrier of diffusion.  ``activation = barrier - well`` is the activation energy of
diffusion in that many dimensions, or along that axis.  Every output is a comparison of doubles or an integer count, so
the device and the explicit host path (``device=-1``) return the same bytes.  Limits that are part of the definition:
windings that are all even read as none (:mod:`pywindow_amd.channels`), there is one guest in an empty framework
without charges, and the bottleneck is that of the grid at its spacing.  The reference has no counterpart.

* :func:`guest_percolation` -- one cell; :func:`guest_percolation_batch` -- frames in ONE call;
  :func:`percolation_field` -- any periodic scalar field; :class:`Percolation` -- the result, whose
  :meth:`Percolation.series` goes into :func:`pywindow_amd.time_correlation` and the other statistical entries.
* ``MolecularSystem.calculate_guest_percolation`` (molecular.py) for a loaded cell and ``DLPOLY.percolation``
  (trajectory.py) for a periodic trajectory.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .affinity import R, lj_coefficients
from .channels import cell_grid, cell_images_many, triangular_lattice

__all__ = ["Percolation", "guest_percolation", "guest_percolation_batch", "percolation_field"]

_SERIES = ("activation", "barrier", "well", "axis_activation")


@dataclasses.dataclass(frozen=True)
class Percolation:
    """The percolation levels of one cell (``raw`` a record, ``levels`` ``(6,)``) or of ``T`` frames (``raw`` ``(T,)``,
    ``levels`` ``(T, 6)``).  ``levels`` holds ``pw_percolation``'s rows (``_lib.PERCOLATION_LEVEL_DTYPE``), criterion
    after criterion: connected in at least 1, 2, 3 dimensions, then winding along a, b, c; ``raw`` the job's row
    (``_lib.PERCOLATION_OUT_DTYPE``).  ``shape`` is the grid ``(nx, ny, nz)``, ``origin`` the centre of voxel (0, 0, 0)
    and ``step`` the six step components in the frame of the triangular cell ``lattice``, ``rotation`` the ``Q`` of
    :func:`pywindow_amd.channels.triangular_lattice`.  ``maps``: with ``maps=True`` the energy of every voxel, ``(nz, ny,
    nx)`` (a list over the frames), ``+inf`` where an atom's core blocks it.  Energies in kJ/mol."""

    levels: np.ndarray
    raw: np.ndarray
    shape: np.ndarray
    origin: np.ndarray
    step: np.ndarray
    lattice: np.ndarray
    rotation: np.ndarray
    spacing: float
    guest: object = None
    maps: object = None
    frames: np.ndarray | None = None
    charges_converged: object = None      # of a rigid guest's field with charges="qeq-cell": whether the frame's charges converged

    @property
    def barrier(self):
        """``(..., 3)``: the lowest levels at which the landscape connects in at least 1, 2, 3 dimensions; ``+inf``
        where it never does."""
        return self.levels["level"][..., :3]

    @property
    def axis_barrier(self):
        """``(..., 3)``: the lowest levels at which a closed path winds along a, b, c."""
        return self.levels["level"][..., 3:]

    @property
    def well(self):
        """``(..., 3)``: the lowest energy inside the component that connects at ``barrier``."""
        return self.levels["well"][..., :3]

    @property
    def axis_well(self):
        return self.levels["well"][..., 3:]

    @staticmethod
    def _rise(level, well):
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(level), level - well, np.inf)

    @property
    def activation(self):
        """``barrier - well``: the activation energy of diffusion in at least 1, 2, 3 dimensions; ``+inf`` without."""
        return self._rise(self.barrier, self.well)

    @property
    def axis_activation(self):
        return self._rise(self.axis_barrier, self.axis_well)

    @property
    def never(self):
        """``(..., 6)``: the criterion holds at no finite level."""
        return (self.levels["flags"] & _lib.PERC_NEVER) != 0

    @property
    def u_min(self):
        return self.raw["u_min"]

    @property
    def n_blocked(self):
        return self.raw["n_blocked"]

    @property
    def components(self):
        """``first``, ``n_voxels``, ``wraps`` and ``rank`` of the component that meets each criterion at its level."""
        return self.levels[["first", "n_voxels", "wraps", "rank"]]

    def _position(self, name):
        v = np.asarray(self.levels[name], dtype=np.float64)                    # (..., 6, 3)
        o, s = np.asarray(self.origin)[..., None, :], np.asarray(self.step)[..., None, :]
        i, j, l = v[..., 0], v[..., 1], v[..., 2]
        x = ((o[..., 0] + i * s[..., 0]) + j * s[..., 1]) + l * s[..., 3]
        y = (o[..., 1] + j * s[..., 2]) + l * s[..., 4]
        z = o[..., 2] + l * s[..., 5]
        p = np.stack([x, y, z], axis=-1)
        p = np.matmul(p, np.swapaxes(np.asarray(self.rotation), -1, -2))        # rows: x = x_triangular @ Q^T
        return np.where((v < 0.0).any(axis=-1)[..., None], np.nan, p)

    @property
    def saddle_position(self):
        """``(..., 6, 3)``: the centre of every criterion's saddle voxel in the coordinates the atoms were given in;
        NaN without one."""
        return self._position("saddle")

    @property
    def well_position(self):
        return self._position("well_voxel")

    def dimensionality_at(self, energy):
        """In how many dimensions the landscape connects at the level ``energy``: the number of ``d`` with
        ``barrier[d] <= energy``."""
        return (self.barrier <= np.asarray(energy, dtype=np.float64)[..., None]).sum(axis=-1)

    def transmission(self, temperature: float):
        """``exp(-activation / RT)``, ``(..., 3)`` (plain numpy on the defined result; 0 where nothing connects)."""
        with np.errstate(over="ignore"):
            return np.exp(-self.activation / (R * float(temperature)))

    def series(self, name: str = "activation", dim: int = 3, axis: int | None = None):
        """``(values, valid)`` over the frames: ``"activation"``, ``"barrier"`` or ``"well"`` of the connection in at
        least ``dim`` dimensions, or ``"axis_activation"`` along cell vector ``axis``; ``valid`` is false where the
        level is ``+inf`` or, with ``charges="qeq-cell"``, the frame's charges did not converge.  Ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`,
        :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics` and
        :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        if name == "axis_activation":
            if axis not in (0, 1, 2):
                raise ValueError("series: axis 0, 1 or 2 for axis_activation")
            column, level = int(axis), self.axis_barrier
        else:
            if dim not in (1, 2, 3):
                raise ValueError("series: dim 1, 2 or 3")
            column, level = int(dim) - 1, self.barrier
        v = np.atleast_2d(np.asarray(getattr(self, name), dtype=np.float64))[:, column].copy()
        valid = np.isfinite(np.atleast_2d(level)[:, column])
        if self.charges_converged is not None:
            valid = valid & np.atleast_1d(np.asarray(self.charges_converged, dtype=bool))
        return v, valid


def _coefficients(elements_or_coef, guest, n: int) -> np.ndarray:
    coef = np.asarray(elements_or_coef)
    if coef.dtype.kind in "fiu" and coef.ndim == 2 and coef.shape[1] == 2:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
    else:
        coef = lj_coefficients(list(elements_or_coef), guest)
    if len(coef) != n:
        raise ValueError("elements_or_coef: one element or one row (A, B) per atom")
    return coef


def plan_jobs(xyz, elements_or_coef, lattice, guest="Xe", spacing: float = 0.5, cutoff: float = 12.0, core2: float = 0.25,
              maps: bool = False):
    """What :func:`guest_percolation_batch` hands to ``Context.percolation``, and what it keeps for the result:
    ``(jobs, atoms, coef, cells (T, 3, 3), rotations (T, 3, 3), shapes (T, 3))`` -- job ``t`` is frame ``t``; its atoms
    are the periodic images within ``cutoff`` of the cell (:func:`pywindow_amd.channels.cell_images_many`), each with
    the row ``(A, B)`` of the atom it is an image of."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    coef = _coefficients(elements_or_coef, guest, n)
    spacing, cutoff, core2 = float(spacing), float(cutoff), float(core2)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError("spacing: a positive number")
    if not (math.isfinite(cutoff) and math.isfinite(core2) and cutoff > 0.0 and cutoff * cutoff > core2):
        raise ValueError("cutoff: a positive number whose square is above core2")
    if not np.isfinite(x).all():
        raise ValueError("xyz: finite")
    lat = np.asarray(lattice, dtype=np.float64)
    lat = np.broadcast_to(lat, (T, 3, 3)) if lat.ndim == 2 else lat
    if lat.shape != (T, 3, 3):
        raise ValueError("lattice: (3, 3) or one (3, 3) per frame")
    Rs, Qs = np.zeros((T, 3, 3)), np.zeros((T, 3, 3))
    for t in range(T):
        Rs[t], Qs[t] = triangular_lattice(lat[t])
    if T:
        inv = np.linalg.inv(Rs)
        width = float((1.0 / np.sqrt((inv * inv).sum(axis=2))).min())
        if cutoff > width:
            raise ValueError(f"guest_percolation: a cutoff of {cutoff:.6g} is above the cell's smallest perpendicular width "
                             f"{width:.6g} (more than 27 images would matter): the largest cutoff that fits is {width:.6g}")
    atoms, _, counts, source = cell_images_many(np.matmul(x, Qs), np.zeros(n), Rs, cutoff, sources=True)
    jobs = np.zeros(T, dtype=_lib.PERCOLATION_JOB_DTYPE)
    shapes = np.zeros((T, 3), dtype=np.int64)
    at = voxels = 0
    for t in range(T):
        dims, origin, step = cell_grid(Rs[t], spacing)
        shapes[t] = dims
        jobs[t] = (at, counts[t], at, -1, voxels if maps else -1, 6 * t, t, origin, step, core2, cutoff * cutoff, *dims, 0)
        voxels += dims[0] * dims[1] * dims[2] if maps else 0
        at += int(counts[t])
    return jobs, atoms, np.ascontiguousarray(coef[source]), Rs, Qs, shapes


def _result(jobs, levels, out, fields, Rs, Qs, shapes, spacing, guest, frames) -> Percolation:
    T = len(jobs)
    maps = None
    if fields is not None:
        maps = [fields[int(j["map_first"]):int(j["map_first"]) + int(j["nx"]) * int(j["ny"]) * int(j["nz"])]
                .reshape(int(j["nz"]), int(j["ny"]), int(j["nx"])) for j in jobs]
    return Percolation(levels.reshape(T, _lib.PERC_CRITERIA), out, shapes, jobs["origin"].copy(), jobs["step"].copy(), Rs, Qs,
                       float(spacing), guest, maps, None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def guest_percolation_batch(xyz, elements_or_coef, lattice, guest="Xe", spacing: float = 0.5, cutoff: float = 12.0,
                            core2: float = 0.25, maps: bool = False, device=None, frames=None, kernel_ms=None,
                            diagnostics=None) -> Percolation:
    """:func:`guest_percolation` for ``T`` frames of the same ``n`` atoms, all jobs in ONE ``pw_percolation`` call:
    ``xyz`` ``(T, n, 3)``, ``lattice`` ``(3, 3)`` or ``(T, 3, 3)``.  The fields of the result are arrays over the
    frames.  ``kernel_ms``: a list that receives the time of the device work by HIP events; ``diagnostics``: a list that
    receives ``(n_evaluations, n_fills)`` per job."""
    jobs, atoms, coef, Rs, Qs, shapes = plan_jobs(xyz, elements_or_coef, lattice, guest, spacing, cutoff, core2, maps)
    levels, out, fields = engine.context(device).percolation(jobs, atoms, coef, kernel_ms=kernel_ms, diagnostics=diagnostics)
    return _result(jobs, levels, out, fields if maps else None, Rs, Qs, shapes, spacing, guest, frames)


def _one(many: Percolation) -> Percolation:
    return Percolation(many.levels[0], many.raw[0], many.shape[0], many.origin[0], many.step[0], many.lattice[0],
                       many.rotation[0], many.spacing, many.guest, None if many.maps is None else many.maps[0], None)


def guest_percolation(xyz, elements_or_coef, lattice, guest="Xe", spacing: float = 0.5, cutoff: float = 12.0,
                      core2: float = 0.25, maps: bool = False, device=None) -> Percolation:
    """The energy levels at which the voids of the cell ``lattice`` (columns as vectors, the convention of
    ``system["lattice"]``) filled with the atoms ``xyz`` ``(n, 3)`` connect for the one-site Lennard-Jones guest
    ``guest`` (a name of ``affinity.GUESTS`` or ``(sigma, eps_kJ_per_mol)``): see :class:`Percolation`.

    ``elements_or_coef``: element symbols (UFF, Lorentz-Berthelot mixed: :func:`pywindow_amd.lj_coefficients`) or rows
    ``(A, B)``.  The grid, the rotation into the triangular cell and the periodic images are those of
    :func:`pywindow_amd.channel_network` with the reach of every atom equal to ``cutoff``: an image further than that
    from the cell does not count in any voxel, so the result is that of the infinite crystal truncated at ``cutoff``.
    A ``cutoff`` above the cell's smallest perpendicular width raises and names the largest that fits; more than 64
    voxels along a cell vector raises and names the smallest spacing that fits.  A voxel within ``sqrt(core2)`` of an
    atom is blocked.  ``maps=True`` keeps the energy of every voxel.  ``xyz`` ``(T, n, 3)`` is
    :func:`guest_percolation_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host
    path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return guest_percolation_batch(x, elements_or_coef, lattice, guest, spacing, cutoff, core2, maps, device)
    return _one(guest_percolation_batch(x.reshape(1, -1, 3), elements_or_coef, lattice, guest, spacing, cutoff, core2, maps, device))


def percolation_field(field, device=None) -> Percolation:
    """:func:`guest_percolation` of any periodic scalar field ``(nz, ny, nx)`` (finite values or ``+inf`` for a blocked
    voxel) on a grid of unit steps along the axes: the levels at which its sub-level sets connect through the periodic
    faces."""
    f = np.ascontiguousarray(field, dtype=np.float64)
    if f.ndim != 3 or f.size == 0:
        raise ValueError("field: (nz, ny, nx)")
    nz, ny, nx = f.shape
    jobs = np.zeros(1, dtype=_lib.PERCOLATION_JOB_DTYPE)
    jobs[0] = (0, 0, 0, 0, -1, 0, 0, (0.0, 0.0, 0.0), (1.0, 0.0, 1.0, 0.0, 0.0, 1.0), 0.25, 0.0, nx, ny, nz, 0)
    levels, out, _ = engine.context(device).percolation(jobs, field=f.reshape(-1))
    cell = np.diag([float(nx), float(ny), float(nz)])[None]
    return _one(_result(jobs, levels, out, None, cell, np.eye(3)[None], np.array([[nx, ny, nz]]), 1.0, None, None))
