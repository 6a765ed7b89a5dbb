"""The accessible surface of a cage on the GPU, and how much of it faces the cavity (``pw_sasa``,
include/pywindow_amd.h).

The solvent-accessible surface for a probe of radius ``probe`` after Shrake and Rupley (1973): every atom carries
``points`` test points on the sphere of its van der Waals radius grown by the probe, a point is exposed when it lies in
no other atom's grown sphere, and an atom's area is its sphere's area times the exposed fraction.  With a
:class:`pywindow_amd.Cavity` made with ``mask=True`` and the same probe, an exposed point is INSIDE when one of the
voxels at the corners of the grid cell that holds it belongs to the cavity: ``internal_area`` is the part of the surface
that faces the void, ``external_area`` the rest.  ``Cavity.n_surface`` counts boundary voxels and does not converge to
an area; this does.  The kernel returns integers only -- the exposed and the inside points of every atom -- so the
device and the explicit host path (``device=-1``) agree to the byte, and the areas are a few IEEE operations on those
integers.  The reference has no counterpart.

* :func:`sphere_directions` -- the default test directions, the golden spiral on the unit sphere.
* :func:`surface_area`, :func:`surface_area_batch` -- one frame, or many frames in one call; :class:`Surface` -- the
  result, whose :meth:`Surface.series` goes straight into :func:`pywindow_amd.time_correlation`,
  :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics` and
  :func:`pywindow_amd.transition_counts`.
* ``Molecule.calculate_surface_area`` (molecular.py) and ``DLPOLY.surface`` (trajectory.py).
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine

__all__ = ["Surface", "sphere_directions", "surface_area", "surface_area_batch"]

_SERIES = ("area", "internal_area", "external_area", "exposed", "inside")


def sphere_directions(points: int) -> np.ndarray:
    """THE DEFINITION of the default test directions: ``points`` unit vectors ``(P, 3)`` on the golden spiral,
    ``z_k = 1 - (2k + 1) / P``, azimuth ``k`` times the golden angle ``pi (3 - sqrt 5)``,
    ``(sqrt(1 - z^2) cos, sqrt(1 - z^2) sin, z)``, in numpy float64.  They are data handed through the ABI: the kernel
    evaluates no transcendental, and any other set of unit vectors may be passed to ``Context.sasa``."""
    P = int(points)
    if not 1 <= P <= _lib.SASA_MAX_POINTS:
        raise ValueError(f"points: 1 .. {_lib.SASA_MAX_POINTS}")
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


@dataclasses.dataclass(frozen=True)
class Surface:
    """The surface of one frame (``exposed`` and ``inside`` ``(n,)``, scalar areas) or of ``T`` frames (``(T, n)`` and
    ``(T,)``).  ``exposed`` / ``inside``: the test points of every atom that no other atom buries / that also face the
    cavity (all zero without a cavity); ``raw`` holds the rows of ``pw_sasa`` (``_lib.SASA_OUT_DTYPE``: their sums and
    the flags); ``radii`` the atoms' radii, ``probe`` the probe radius, ``points`` the number ``P`` of test points an
    atom.  ``closed``: the cavity's ``closed`` when there was one, else ``None``."""

    raw: np.ndarray
    exposed: np.ndarray
    inside: np.ndarray
    radii: np.ndarray
    probe: float
    points: int
    closed: object = None
    frames: np.ndarray | None = None

    def _sphere(self):
        R = self.radii + self.probe
        return 4.0 * math.pi * R * R

    @property
    def area_atoms(self) -> np.ndarray:
        """``4 pi R_i^2 * (exposed_i / P)`` with ``R_i = radius_i + probe``."""
        return self._sphere() * (self.exposed / self.points)

    @property
    def area(self):
        """The sum of ``area_atoms`` over the atoms."""
        return self.area_atoms.sum(axis=-1)

    @property
    def internal_area(self):
        """The sum of ``4 pi R_i^2 * (inside_i / P)``: the part of ``area`` that faces the cavity."""
        return (self._sphere() * (self.inside / self.points)).sum(axis=-1)

    @property
    def external_area(self):
        """``area - internal_area``."""
        return self.area - self.internal_area

    def series(self, name: str = "area"):
        """``(values, valid)`` of a quantity over the frames -- float64 values; ``valid`` all true, or the cavity's
        ``closed`` when there was one -- ready for :func:`pywindow_amd.time_correlation`,
        :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics`
        and :func:`pywindow_amd.transition_counts`.  ``exposed`` and ``inside`` are the sums over the atoms."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = self.raw[name] if name in ("exposed", "inside") else getattr(self, name)
        values = np.atleast_1d(np.asarray(v, dtype=np.float64)).copy()
        valid = np.ones(len(values), dtype=bool) if self.closed is None else np.atleast_1d(np.asarray(self.closed, dtype=bool)).copy()
        return values, valid


def pack_mask(mask: np.ndarray) -> np.ndarray:
    """The ``ny * nz`` words of a ``(nz, ny, nx)`` bool array (the inverse of ``cavity.unpack_mask``)."""
    nx = mask.shape[2]
    return (mask.astype(np.uint64) << np.arange(nx, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).reshape(-1)


def surface_area_batch(xyz, radii, probe: float = 0.0, points: int = 960, cavity=None, device=None, frames=None,
                       kernel_ms=None) -> Surface:
    """:func:`surface_area` for ``T`` frames of the same ``n`` atoms in ONE ``pw_sasa`` call: ``xyz`` ``(T, n, 3)``,
    ``radii`` ``(n,)``, ``cavity`` ``None`` or the :class:`pywindow_amd.Cavity` of the same ``T`` frames
    (``cavity_grid_batch(..., mask=True)`` with the same probe).  The fields of the result are arrays over the frames.
    ``kernel_ms``: a list that receives the time of the kernel by HIP events (the library's measurement entry)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    r = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    if len(r) != n:
        raise ValueError("radii: one radius per atom")
    probe = float(probe)
    u = sphere_directions(points)
    jobs = np.zeros(T, dtype=_lib.SASA_JOB_DTYPE)
    jobs["atom_first"] = np.arange(T) * n
    jobs["n"] = n
    jobs["count_first"] = np.arange(T) * n
    jobs["word_first"] = -1
    jobs["out"] = np.arange(T)
    jobs["probe"] = probe
    words = closed = None
    if cavity is not None:
        if cavity.mask is None:
            raise ValueError("cavity: a Cavity made with mask=True")
        if float(cavity.probe) != probe:
            raise ValueError(f"cavity: made for the probe {cavity.probe}, not {probe}")
        masks = [cavity.mask] if cavity.raw.ndim == 0 else list(cavity.mask)
        if len(masks) != T:
            raise ValueError("cavity: one cavity per frame")
        if cavity.words is not None:                                 # (as pw_cavity wrote them: nothing to pack)
            packed = [cavity.words] if cavity.raw.ndim == 0 else list(cavity.words)
        else:
            packed = [pack_mask(m) for m in masks]
        jobs["word_first"] = np.concatenate([[0], np.cumsum([len(p) for p in packed])[:-1]]) if T else 0
        jobs["origin"] = np.asarray(cavity.origin, dtype=np.float64).reshape(T, 3)
        jobs["spacing"] = cavity.spacing
        shape = np.asarray(cavity.shape).reshape(T, 3)
        jobs["nx"], jobs["ny"], jobs["nz"] = shape[:, 0], shape[:, 1], shape[:, 2]
        words = np.concatenate(packed) if packed else None
        closed = np.atleast_1d(np.asarray(cavity.closed, dtype=bool)).copy()
    out, exposed, inside = engine.context(device).sasa(jobs, x.reshape(-1, 3), r, u, words, kernel_ms=kernel_ms)
    return Surface(out, exposed.reshape(T, n), inside.reshape(T, n), r, probe, int(points), closed,
                   None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def surface_area(xyz, radii, probe: float = 0.0, points: int = 960, cavity=None, device=None) -> Surface:
    """The accessible surface of the atoms ``xyz`` ``(n, 3)`` with the radii ``radii`` for a probe of radius ``probe``,
    ``points`` test points an atom on :func:`sphere_directions`: see :class:`Surface`.  ``cavity``: the
    :class:`pywindow_amd.Cavity` of the same atoms, made with ``mask=True`` and the same probe (another probe is a
    ``ValueError``: its void would not be the one this surface bounds); its words, origin, shape and spacing become the
    grid that says which exposed points face the void.  ``xyz`` ``(T, n, 3)`` is :func:`surface_area_batch`.
    ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return surface_area_batch(x, radii, probe, points, cavity, device)
    many = surface_area_batch(x.reshape(1, -1, 3), radii, probe, points, cavity, device)
    return Surface(many.raw[0], many.exposed[0], many.inside[0], many.radii, many.probe, many.points,
                   None if many.closed is None else bool(many.closed[0]))
