"""Rigid linear guests (N2, CO2, O2) in the crystal on the GPU: the orientation-averaged free-energy field of the guest's
centre over the periodic cell (``pw_rigid_cell``, include/pywindow_amd.h; the definition and the proof of its atom skip
in pywindow_amd/csrc/pw_rigid_cell.hpp), and on that field the percolation levels and the diffusion tensor.

:mod:`pywindow_amd.percolation` and :mod:`pywindow_amd.diffusion` handle a guest that is a sphere;
:mod:`pywindow_amd.rigid` handles a rigid line of sites, but inside one isolated cage.  Here the rigid guest is inserted
with its centre at every voxel of the cell's own skewed grid in every one of ``M`` orientations, against the framework
and its periodic images; per voxel and temperature the Boltzmann factors are averaged over the orientations in a defined
order of additions, so the device and the explicit host path (``device=-1``) return the same bytes.  ``-R T ln zbar`` is the
free energy of the guest's centre at that temperature: a periodic scalar field, which ``pw_percolation`` and ``pw_basins``
take as a caller's field.  Every temperature has its own field.

Charges.  A cutoff Coulomb sum over images is not a defined periodic energy; with ``charges=`` (the framework's point
charges, one per atom or one row a frame) the jobs go through ``pw_rigid_cell_ewald`` and every pose energy carries the
Ewald sum of the framework's charges on the guest's site charges (:mod:`pywindow_amd.ewald`,
pywindow_amd/csrc/pw_ewald.hpp): the real-space term in the pair loop, the reciprocal term added last.  Without
``charges`` the calls are ``pw_rigid_cell``'s exactly as before.

``charges="qeq-cell"`` makes them by periodic charge equilibration first (``pw_charges_cell``,
:mod:`pywindow_amd.charges_cell`): one call over the same frames with the call's own ``cutoff`` and ``ewald_tolerance``,
then everything proceeds as with given charges; the result carries ``charges_converged`` and a frame whose charges did not
converge is not valid.  ``charges="qeq"`` stays refused: it is the isolated-molecule model.

What is left out.  A framework that is not neutral (no background term); the guest's interaction with its own images.  Non-linear
guests.  Guest-guest terms: infinite dilution.  The fields travel through host memory between the three entries.  The
reference has no counterpart.

* :func:`rigid_guest_field` / ``_batch`` -- :class:`RigidField`; :func:`rigid_guest_percolation` / ``_batch`` -- one
  :class:`pywindow_amd.Percolation` per temperature; :func:`rigid_guest_diffusion` / ``_batch`` -- a
  :class:`pywindow_amd.Diffusion`.
* ``MolecularSystem.calculate_rigid_guest_percolation`` / ``_diffusion`` (molecular.py) and ``DLPOLY.rigid_field``,
  ``.rigid_percolation``, ``.rigid_diffusion`` (trajectory.py).
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .affinity import _PER_BAR, R
from .diffusion import Diffusion, _basins_jobs, _frame, _one as _one_diffusion, _run
from .ewald import ewald_parameters, framework_charges
from .percolation import _one as _one_percolation, _result as _percolation_result, plan_jobs
from .rigid import COULOMB, M_DEFAULT, _guest as _linear_guest, rigid_coefficients
from .rigid_body import is_body
from .surface import sphere_directions

__all__ = ["RIGID_GUEST_MASSES", "RigidField", "rigid_guest_field", "rigid_guest_field_batch", "rigid_guest_percolation",
           "rigid_guest_percolation_batch", "rigid_guest_diffusion", "rigid_guest_diffusion_batch"]

#: molar masses in g/mol of the guests of ``RIGID_GUESTS``
RIGID_GUEST_MASSES = {"N2": 28.0134, "CO2": 44.0095, "O2": 31.9988}

_SERIES = ("boltzmann_volume", "henry", "mean_energy", "heat", "min_energy", "n_dead")


@dataclasses.dataclass(frozen=True)
class RigidField:
    """The orientation-averaged field of one cell (``raw`` a record, ``levels`` ``(L,)``, ``zbar`` ``(L, nz, ny, nx)``) or of
    ``T`` frames (``raw`` ``(T,)``, ``levels`` ``(T, L)``, ``zbar`` a list of ``(L, nz, ny, nx)``) at the ``L``
    ``temperatures``.  ``raw`` holds ``pw_rigid_cell``'s row (``_lib.RIGID_OUT_DTYPE``), ``levels`` its ``(Z, E)`` rows;
    ``zbar`` the orientation-averaged Boltzmann factor of every voxel at every temperature and ``u_min_map`` ``(nz, ny,
    nx)`` the lowest pose energy of every voxel, ``+inf`` where every pose is blocked.  ``shape`` is the grid ``(nx, ny,
    nz)``, ``origin`` and ``step`` the grid in the frame of the triangular cell ``lattice``, ``rotation`` the ``Q`` of
    :func:`pywindow_amd.channels.triangular_lattice`; ``directions`` as they were given, in the caller's frame.  Energies
    in kJ/mol."""

    raw: np.ndarray
    levels: np.ndarray
    temperatures: np.ndarray
    zbar: object
    u_min_map: object
    shape: np.ndarray
    origin: np.ndarray
    step: np.ndarray
    lattice: np.ndarray
    rotation: np.ndarray
    spacing: float
    directions: np.ndarray
    guest: object = None
    frames: np.ndarray | None = None
    charges_converged: object = None      # with charges="qeq-cell": whether the frame's charge equilibration converged

    @property
    def n_voxels(self):
        return self.raw["n_voxels"][()]

    @property
    def n_dead(self):
        """Voxels at which every orientation is blocked."""
        return self.raw["n_dead"][()]

    @property
    def n_blocked_poses(self):
        return self.raw["n_blocked_poses"][()]

    @property
    def clamped(self):
        """An exponent above 700 was taken as 700: the sums of that frame are not to be used."""
        return (self.raw["flags"] & _lib.AFF_CLAMPED) != 0

    @property
    def voxel_volume(self):
        s = np.asarray(self.step)
        return s[..., 0] * s[..., 2] * s[..., 5]

    @property
    def boltzmann_volume(self):
        """``Z v`` in cubic Angstrom per cell and temperature; ``v`` the volume of a voxel."""
        return self.levels["z"] * np.asarray(self.voxel_volume)[..., None]

    @property
    def henry(self):
        """The Henry coefficient of the cell, ``boltzmann_volume / (k_B T)``, in molecules per cell and bar."""
        return self.boltzmann_volume * (_PER_BAR / (R * self.temperatures))

    @property
    def mean_energy(self):
        """``E / Z``, the Boltzmann average of the guest's energy over positions and orientations, kJ/mol."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.levels["e"] / self.levels["z"]

    @property
    def heat(self):
        """The heat of adsorption at infinite dilution, ``R T - mean_energy``, kJ/mol."""
        return R * self.temperatures - self.mean_energy

    @property
    def min_energy(self):
        """The lowest energy of a pose that no core blocks, kJ/mol; ``+inf`` without one."""
        return self.raw["u_min"][()]

    @property
    def min_position(self):
        """The centre of the voxel of ``min_energy`` in the coordinates the atoms were given in; NaN without one."""
        v = np.asarray(self.raw["min_voxel"], dtype=np.float64)
        o, s = np.asarray(self.origin), np.asarray(self.step)
        i, j, l = v[..., 0], v[..., 1], v[..., 2]
        p = np.stack([((o[..., 0] + i * s[..., 0]) + j * s[..., 1]) + l * s[..., 3], (o[..., 1] + j * s[..., 2]) + l * s[..., 4],
                      o[..., 2] + l * s[..., 5]], axis=-1)
        p = np.matmul(p[..., None, :], np.swapaxes(np.asarray(self.rotation), -1, -2))[..., 0, :]   # x = x_triangular @ Q^T
        return np.where((v < 0.0).any(axis=-1)[..., None], np.nan, p)

    @property
    def min_direction(self):
        """The direction of the pose of ``min_energy``, as it was given; NaN without one."""
        o = np.asarray(self.raw["min_dir"])
        return np.where((o < 0)[..., None], np.nan, self.directions[np.maximum(o, 0)])

    def free_energy(self, level: int = 0, t=None):
        """``-R T ln zbar`` ``(nz, ny, nx)`` in kJ/mol at temperature ``level`` (of frame ``t`` of many), ``+inf`` where
        ``zbar == 0``: the free energy of the guest's centre, which :func:`pywindow_amd.percolation_field` and
        :func:`pywindow_amd.diffusion_field` accept."""
        many = self.raw.ndim == 1
        if many != (t is not None):
            raise ValueError("free_energy: t for a result over many frames, and only then")
        if not 0 <= int(level) < len(self.temperatures):
            raise ValueError("free_energy: level 0 .. L - 1")
        return _free_energy((self.zbar[t] if many else self.zbar)[int(level)], self.temperatures[int(level)])

    def selectivity(self, other):
        """The ratio of this guest's Henry coefficient to ``other``'s, a :class:`RigidField` of the same frames, grid and
        temperatures."""
        if not isinstance(other, RigidField):
            raise TypeError("selectivity: a RigidField")
        if not np.array_equal(self.temperatures, other.temperatures):
            raise ValueError("selectivity: the two results are for different temperatures")
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.boltzmann_volume / other.boltzmann_volume

    def series(self, name: str = "boltzmann_volume", level: int = 0):
        """``(values, valid)`` of a quantity over the frames at temperature ``level``, with the validity rule of
        :meth:`pywindow_amd.RigidAffinity.series` for a plain grid: the frame was not clamped and the value is finite --
        and, with ``charges="qeq-cell"``, the frame's charges converged."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = np.asarray(getattr(self, name), dtype=np.float64)
        if name in ("boltzmann_volume", "henry", "mean_energy", "heat"):
            v = v[..., level]
        values = np.atleast_1d(v).copy()
        valid = np.isfinite(values) & ~np.atleast_1d(self.clamped)
        if self.charges_converged is not None:
            valid &= np.atleast_1d(np.asarray(self.charges_converged, dtype=bool))
        return values, valid


def _guest(guest):
    """The model of a linear guest.  A rigid body (:mod:`pywindow_amd.rigid_body`) is refused: the cell's proved atom
    skip (pw_rigid_cell.hpp) states its reach for offsets along directions, not for pose tables."""
    if is_body(guest):
        raise ValueError("rigid_guest_field: rigid bodies are not built for the cell yet")
    return _linear_guest(guest)


def _free_energy(zbar, temperature):
    with np.errstate(divide="ignore"):
        return np.where(zbar == 0.0, np.inf, -(R * temperature) * np.log(zbar))


def _temperatures(temperatures):
    temps = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=np.float64)))
    if temps.ndim != 1 or not 1 <= len(temps) <= _lib.AFF_MAX_LEVELS or not (np.isfinite(temps) & (temps > 0.0)).all():
        raise ValueError(f"temperatures: 1 .. {_lib.AFF_MAX_LEVELS} positive numbers")
    return temps


def plan_field(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
               core2: float = 0.25, directions=None):
    """What :func:`rigid_guest_field_batch` hands to ``Context.rigid_cell`` and keeps for the result (:func:`_plan`)."""
    return _plan(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions)[0]


def plan_charged_field(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                       cutoff: float = 12.0, core2: float = 0.25, directions=None, charges=None, ewald_tolerance: float = 1e-6):
    """:func:`plan_field` for a framework with the point charges ``charges`` (``(n,)`` or ``(T, n)``, e): ``(planned, ew)``,
    ``ew`` what ``Context.rigid_cell_ewald`` takes beyond the plan -- ``jobs`` (``_lib.RIGID_CELL_EWALD_JOB_DTYPE``, every
    job charged), ``coef`` the rows ``(A, B, C)`` with ``C = COULOMB q_site q_atom`` image by image, ``site_q``, ``cell``
    the rows ``(x, y, z, q)`` of each frame's own atoms in its triangular frame and ``kvecs`` the rows of
    :func:`pywindow_amd.ewald_parameters` of each frame's cell at ``cutoff`` and ``ewald_tolerance``."""
    planned, source, x, lat = _plan(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions)
    jobs, atoms, coef, offsets = planned[:4]
    Qs, g = planned[9], planned[11]
    T, n = x.shape[:2]
    q = framework_charges(charges, T, n)
    S = len(offsets)
    site_q = np.ascontiguousarray(g.charges, dtype=np.float64)
    ew_jobs = np.zeros(T, dtype=_lib.RIGID_CELL_EWALD_JOB_DTYPE)
    ew_jobs["cell"] = jobs
    rows, kvecs = [], []
    for t in range(T):
        a, m = int(jobs["atom_first"][t]), int(jobs["n"][t])
        ab = coef[S * a:S * (a + m)].reshape(S, m, 2)
        c = COULOMB * site_q[:, None] * q[t, source[a:a + m]][None, :]
        rows.append(np.concatenate([ab, c[:, :, None]], axis=2).reshape(-1, 3))
        alpha, kv = ewald_parameters(lat[t], cutoff, ewald_tolerance)
        ew_jobs["alpha"][t] = alpha
        ew_jobs["k_first"][t] = sum(len(v) for v in kvecs)
        ew_jobs["n_k"][t] = len(kv)
        kvecs.append(kv)
    ew_jobs["cell_first"] = n * np.arange(T)
    ew_jobs["n_cell"] = n
    ew_jobs["charged"] = 1
    cell = np.concatenate([np.matmul(x, Qs), q[:, :, None]], axis=2).reshape(-1, 4)
    return planned, {"jobs": ew_jobs, "coef": np.concatenate(rows) if rows else np.zeros((0, 3)), "site_q": site_q,
                     "cell": np.ascontiguousarray(cell), "kvecs": np.concatenate(kvecs) if kvecs else np.zeros((0, 4))}


def _plan(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions):
    """``(planned, source, xyz, lattices)``: what :func:`rigid_guest_field_batch` hands to ``Context.rigid_cell`` and keeps
    for the result, ``planned = (jobs, atoms, coef, offsets, dirs, betas, given, temps, Rs, Qs, shapes, g)``.  Job ``t`` is frame ``t``; the grid, the rotation and the
    images are :func:`pywindow_amd.percolation.plan_jobs`'s with the reach ``cutoff + max|t_s| * max|d_o|`` in place of
    the cutoff; the rows ``(A, B)`` of every site are repeated image by image; the directions are rotated into each
    frame's triangular cell.  ``source``: for every image the atom it is an image of."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    g = _guest(guest)
    S = len(g.offsets)
    coef = np.asarray(elements_or_coef)
    if coef.dtype.kind in "fiu" and coef.ndim == 3 and coef.shape[2] == 2:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
    else:
        coef = np.ascontiguousarray(rigid_coefficients(list(elements_or_coef), g)[:, :, :2])
    if coef.shape != (S, n, 2):
        raise ValueError("elements_or_coef: one element per atom, or rows (A, B) (S, n, 2)")
    temps = _temperatures(temperatures)
    given = sphere_directions(M_DEFAULT) if directions is None else np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    if not 1 <= len(given) <= _lib.RIGID_MAX_DIRS or not np.isfinite(given).all():
        raise ValueError(f"directions: 1 .. {_lib.RIGID_MAX_DIRS} finite rows of three")
    offsets = np.ascontiguousarray(g.offsets, dtype=np.float64)
    cutoff, core2 = float(cutoff), float(core2)
    if not (math.isfinite(cutoff) and math.isfinite(core2) and cutoff > 0.0 and cutoff * cutoff > core2):
        raise ValueError("cutoff: a positive number whose square is above core2")
    arm = float(np.abs(offsets).max()) * float(np.sqrt((given * given).sum(axis=1)).max())
    lat = np.asarray(lattice, dtype=np.float64)
    lat = np.broadcast_to(lat, (T, 3, 3)) if lat.ndim == 2 else lat
    if lat.shape != (T, 3, 3):
        raise ValueError("lattice: (3, 3) or one (3, 3) per frame")
    if T:
        inv = np.linalg.inv(lat)
        width = float((1.0 / np.sqrt((inv * inv).sum(axis=2))).min())      # (between the faces k: 1 / |row k of the inverse|)
        if cutoff + arm > width:
            raise ValueError(f"rigid_guest_field: a reach of {cutoff + arm:.6g} (cutoff {cutoff:.6g} + the guest's arm {arm:.6g}) is "
                             f"above the cell's smallest perpendicular width {width:.6g} (more than 27 images would matter): "
                             f"the largest cutoff that fits is {width - arm:.6g}")
    index = np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)         # (the rows come back image by image)
    perc, atoms, source, Rs, Qs, shapes = plan_jobs(x, index, lat, None, spacing, cutoff + arm, core2, False)
    source = source[:, 0].astype(np.int64)
    L, M = len(temps), len(given)
    jobs = np.zeros(T, dtype=_lib.RIGID_CELL_JOB_DTYPE)
    rows = []
    for name in ("atom_first", "n", "origin", "step", "nx", "ny", "nz"):
        jobs[name] = perc[name]
    voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
    for t in range(T):
        a, m = int(jobs["atom_first"][t]), int(jobs["n"][t])
        rows.append(coef[:, source[a:a + m], :].reshape(-1, 2))                  # row s * m + image
    jobs["coef_first"] = S * jobs["atom_first"]
    jobs["n_betas"], jobs["n_sites"], jobs["n_dirs"] = L, S, M
    jobs["dir_first"] = M * np.arange(T)
    jobs["level_first"] = L * np.arange(T)
    jobs["map_first"] = (L + 1) * (np.cumsum(voxels) - voxels)
    jobs["out"] = np.arange(T)
    jobs["core2"], jobs["cutoff2"] = core2, cutoff * cutoff
    dirs = np.clip(np.matmul(given[None], Qs), -1.0, 1.0).reshape(-1, 3)         # rows: d_triangular = d @ Q
    coef_rows = np.concatenate(rows) if rows else np.zeros((0, 2))
    return (jobs, atoms, coef_rows, offsets, dirs, 1.0 / (R * temps), given, temps, Rs, Qs, shapes, g), source, x, lat


def _field(planned, ctx, spacing, frames, kernel_ms=None, diagnostics=None, ew=None) -> RigidField:
    jobs, atoms, coef, offsets, dirs, betas, given, temps, Rs, Qs, shapes, g = planned
    if ew is None:
        out, levels, maps = ctx.rigid_cell(jobs, atoms, coef, offsets, dirs, betas, kernel_ms=kernel_ms, diagnostics=diagnostics)
    else:
        out, levels, maps = ctx.rigid_cell_ewald(ew["jobs"], atoms, ew["coef"], offsets, dirs, betas, ew["site_q"], ew["cell"],
                                                 ew["kvecs"], kernel_ms=kernel_ms, diagnostics=diagnostics)
    T, L = len(jobs), len(temps)
    zbar, low = [], []
    for J in jobs:
        nx, ny, nz = int(J["nx"]), int(J["ny"]), int(J["nz"])
        planes = maps[int(J["map_first"]):int(J["map_first"]) + (L + 1) * nx * ny * nz].reshape(L + 1, nz, ny, nx)
        zbar.append(planes[:L])
        low.append(planes[L])
    return RigidField(out, levels.reshape(T, L), temps, zbar, low, shapes, jobs["origin"].copy(), jobs["step"].copy(),
                      np.matmul(Qs, Rs), Qs, float(spacing), given, g,
                      None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def _one_field(many: RigidField) -> RigidField:
    return dataclasses.replace(many, raw=many.raw[0], levels=many.levels[0], zbar=many.zbar[0], u_min_map=many.u_min_map[0],
                               shape=many.shape[0], origin=many.origin[0], step=many.step[0], lattice=many.lattice[0],
                               rotation=many.rotation[0], frames=None, charges_converged=_first(many.charges_converged))


def _first(converged):
    return None if converged is None else converged[0]


def _cell_charges(xyz, elements_or_coef, lattice, cutoff, ewald_tolerance, charges, device):
    """``(charges, converged)``: ``charges`` as they were given and ``None``, or for ``"qeq-cell"`` the ``(T, n)`` charges of ONE
    ``pw_charges_cell`` call over the frames at the call's own ``cutoff`` and ``ewald_tolerance`` and whether each frame's
    converged.  (A frame without charges gets zeros: it is not valid anyway.)"""
    if not (isinstance(charges, str) and charges == "qeq-cell"):
        return charges, None
    from .charges_cell import equilibrate_cell_charges_batch

    coef = np.asarray(elements_or_coef)
    if coef.dtype.kind in "fiu":
        raise ValueError('charges="qeq-cell" needs the elements, not ready rows')
    made = equilibrate_cell_charges_batch(xyz, list(elements_or_coef), lattice, cutoff, ewald_tolerance, device=device)
    return np.where(np.isfinite(made.charges), made.charges, 0.0), np.atleast_1d(made.converged).copy()


def rigid_guest_field_batch(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                            cutoff: float = 12.0, core2: float = 0.25, directions=None, device=None, frames=None,
                            kernel_ms=None, diagnostics=None, charges=None, ewald_tolerance: float = 1e-6) -> RigidField:
    """:func:`rigid_guest_field` for ``T`` frames of the same ``n`` atoms, all jobs in ONE ``pw_rigid_cell`` call: ``xyz``
    ``(T, n, 3)``, ``lattice`` ``(3, 3)`` or ``(T, 3, 3)``.  ``kernel_ms``: a list that receives the time of the device work
    by HIP events; ``diagnostics``: a list that receives ``(n_pairs, instances)``.  ``charges`` ``(n,)`` or ``(T, n)``: the
    framework's point charges, one ``pw_rigid_cell_ewald`` call (``None``: ``pw_rigid_cell`` as before); ``"qeq-cell"``: ONE
    ``pw_charges_cell`` call over the same frames makes them first (:func:`_cell_charges`)."""
    _guest(guest)                                                    # (a rigid body is refused before any charges are made)
    if charges is None:
        planned = plan_field(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions)
        return _field(planned, engine.context(device), spacing, frames, kernel_ms, diagnostics)
    charges, converged = _cell_charges(np.asarray(xyz, dtype=np.float64), elements_or_coef, lattice, cutoff, ewald_tolerance, charges,
                                       device)
    planned, ew = plan_charged_field(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions, charges,
                                     ewald_tolerance)
    field = _field(planned, engine.context(device), spacing, frames, kernel_ms, diagnostics, ew)
    return field if converged is None else dataclasses.replace(field, charges_converged=converged)


def rigid_guest_field(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
                      core2: float = 0.25, directions=None, device=None, charges=None, ewald_tolerance: float = 1e-6) -> RigidField:
    """The orientation-averaged Boltzmann factor of the rigid linear guest ``guest`` (a name of ``RIGID_GUESTS`` or a
    :class:`pywindow_amd.RigidGuest`) at every voxel of the cell ``lattice`` (columns as vectors) filled with the atoms
    ``xyz`` ``(n, 3)``, at every temperature of ``temperatures`` (1 to 8, in K): see :class:`RigidField`.

    ``elements_or_coef``: element symbols (:func:`pywindow_amd.rigid_coefficients` without charges) or rows ``(A, B)``
    ``(S, n, 2)``.  The grid, the rotation into the triangular cell and the periodic images are those of
    :func:`pywindow_amd.guest_percolation` with the reach ``cutoff + max|t_s| * max|d_o|`` -- the cutoff of a site plus
    the guest's longest arm -- in place of the cutoff: a reach above the cell's smallest perpendicular width raises and
    names the largest cutoff that fits.  ``directions``: ``(M, 3)``, at most 1024 (``None``:
    ``pywindow_amd.sphere_directions(64)``), in the frame of ``xyz``; they are data, neither normalised nor checked for
    length.  A pose with a site within ``sqrt(core2)`` of an atom is blocked.  ``charges``: the framework's point charges in
    e, one per atom (or one row a frame): every pose energy then carries the Ewald sum of those charges on the guest's site
    charges, real-space part cut at ``cutoff``, parameters by :func:`pywindow_amd.ewald_parameters` at ``ewald_tolerance``; a
    framework that is not neutral within ``1e-8 * sum |q|`` and ``"qeq"`` are refused.  ``"qeq-cell"``: the library makes the
    charges itself by periodic charge equilibration at the same ``cutoff`` and ``ewald_tolerance``
    (:func:`pywindow_amd.equilibrate_cell_charges`, its defaults otherwise; needs the elements); ``charges_converged`` says
    whether that converged, and a frame where it did not is not valid.  ``None``: the jobs are uncharged.
    ``xyz`` ``(T, n, 3)`` is :func:`rigid_guest_field_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1``
    the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    args = (elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions, device)
    kw = dict(charges=charges, ewald_tolerance=ewald_tolerance)
    if x.ndim == 3:
        return rigid_guest_field_batch(x, *args, **kw)
    return _one_field(rigid_guest_field_batch(x.reshape(1, -1, 3), *args, **kw))


def _field_jobs(field: RigidField):
    """``pw_percolation`` jobs on the free energies of a field over ``T`` frames, job ``t * L + l`` frame ``t`` at
    temperature ``l``: ``(jobs, the fields one after the other)``."""
    T, L = len(field.raw), len(field.temperatures)
    jobs = np.zeros(T * L, dtype=_lib.PERCOLATION_JOB_DTYPE)
    values, at = [], 0
    for t in range(T):
        nx, ny, nz = (int(v) for v in field.shape[t])
        for l in range(L):
            k = t * L + l
            jobs[k] = (0, 0, 0, at, -1, 6 * k, k, field.origin[t], field.step[t], 0.25, 0.0, nx, ny, nz, 0)
            values.append(field.free_energy(l, t).reshape(-1))
            at += nx * ny * nz
    return jobs, np.concatenate(values) if values else np.zeros(0)


def rigid_guest_percolation_batch(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                                  cutoff: float = 12.0, core2: float = 0.25, directions=None, device=None, frames=None,
                                  charges=None, ewald_tolerance: float = 1e-6):
    """:func:`rigid_guest_percolation` for ``T`` frames: one ``pw_rigid_cell`` call, then every (frame, temperature) as a
    job on its free-energy field in ONE ``pw_percolation`` call.  A list, one :class:`pywindow_amd.Percolation` over the
    frames per temperature."""
    field = rigid_guest_field_batch(xyz, elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions, device,
                                    frames, charges=charges, ewald_tolerance=ewald_tolerance)
    jobs, values = _field_jobs(field)
    levels, out, _ = engine.context(device).percolation(jobs, field=values)
    T, L = len(field.raw), len(field.temperatures)
    Rs = np.matmul(np.swapaxes(field.rotation, -1, -2), field.lattice)
    made = [_percolation_result(jobs[l::L], levels.reshape(T * L, 6)[l::L].copy(), out[l::L].copy(), None, Rs, field.rotation,
                                field.shape, spacing, field.guest, frames) for l in range(L)]
    return [dataclasses.replace(p, charges_converged=field.charges_converged) for p in made]


def rigid_guest_percolation(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                            cutoff: float = 12.0, core2: float = 0.25, directions=None, device=None, charges=None,
                            ewald_tolerance: float = 1e-6):
    """The levels at which the free-energy landscape of a rigid linear guest's centre connects through the crystal: per
    temperature a :class:`pywindow_amd.Percolation` of ``-R T ln zbar`` (:func:`rigid_guest_field`, the same arguments);
    energies are free energies at that temperature, in kJ/mol.  A list over the temperatures."""
    x = np.asarray(xyz, dtype=np.float64)
    args = (elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions, device)
    kw = dict(charges=charges, ewald_tolerance=ewald_tolerance)
    if x.ndim == 3:
        return rigid_guest_percolation_batch(x, *args, **kw)
    return [dataclasses.replace(_one_percolation(p), charges_converged=_first(p.charges_converged))
            for p in rigid_guest_percolation_batch(x.reshape(1, -1, 3), *args, **kw)]


def rigid_guest_diffusion_batch(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                                cutoff: float = 12.0, core2: float = 0.25, directions=None, cap: float = 100.0, merge=None,
                                mass=None, labels: bool = False, device=None, frames=None, charges=None,
                                ewald_tolerance: float = 1e-6) -> Diffusion:
    """:func:`rigid_guest_diffusion` for ``T`` frames: one ``pw_rigid_cell`` call, then every (frame, temperature) as a
    ``pw_basins`` job on that temperature's free-energy field with that one beta, all in ONE ``pw_basins`` call (and one
    more for the jobs that overflowed the first capacities)."""
    g = _guest(guest)
    if mass is None:
        if not isinstance(guest, str) or guest not in RIGID_GUEST_MASSES:
            raise ValueError("mass: the guest's molar mass in g/mol (built in for the names of RIGID_GUEST_MASSES only)")
        mass = RIGID_GUEST_MASSES[guest]
    mass = float(mass)
    temps = _temperatures(temperatures)
    merge = float(R * temps.min()) if merge is None else float(merge)
    cap = float(cap)
    if math.isnan(cap) or math.isnan(merge) or merge < 0.0 or not mass > 0.0:
        raise ValueError("cap: a number; merge: >= 0; mass: positive")
    field = rigid_guest_field_batch(xyz, elements_or_coef, lattice, g, temps, spacing, cutoff, core2, directions, device, frames,
                                    charges=charges, ewald_tolerance=ewald_tolerance)
    perc, values = _field_jobs(field)
    T, L = len(field.raw), len(temps)
    jobs = _basins_jobs(perc, temps[:1], cap, False, labels)
    jobs["betas"][:, 0] = np.tile(1.0 / (R * temps), T)              # job t * L + l: the one beta of its temperature
    ran = _run(engine.context(device), jobs, None, None, values)
    out, per_b, per_e, _, labelled = ran
    made = [_frame(jobs[k], out[k], per_b[k], per_e[k], temps[k % L:k % L + 1], mass, merge) for k in range(T * L)]
    Qs = field.rotation
    tensor = np.stack([np.stack([np.einsum("ab,bc,dc->ad", Qs[t], made[t * L + l]["tensor"][0], Qs[t]) for l in range(L)])
                       for t in range(T)]) if T else np.zeros((0, L, 3, 3))
    for k, m in enumerate(made):                                     # (the positions come back in the caller's frame)
        m["sites"]["position"] = m["sites"]["position"] @ Qs[k // L].T
        m["hops"]["vector"] = m["hops"]["vector"] @ Qs[k // L].T

    def per(name, pick=lambda v: v):
        return [[pick(made[t * L + l][name]) for l in range(L)] for t in range(T)]

    def table(name, dtype, pick=lambda v: v):
        return np.array(per(name, pick), dtype=dtype).reshape(T, L)

    cut = None
    if labels:
        cut = [[labelled[int(J["label_first"]):int(J["label_first"]) + int(J["nx"]) * int(J["ny"]) * int(J["nz"])]
                .reshape(int(J["nz"]), int(J["ny"]), int(J["nx"])) for J in jobs[t * L:(t + 1) * L]] for t in range(T)]
    valid = table("valid", bool).all(axis=1)
    if field.charges_converged is not None:
        valid = valid & field.charges_converged
    return Diffusion(tensor, temps, out.reshape(T, L), out["n_basins"].reshape(T, L).copy(),
                     table("sites", np.int64, len), table("trapped", np.float64, lambda v: v[0]),
                     table("barrierless", bool), table("rank", np.int64), valid, per("sites"),
                     per("Z"), per("hops"), per("rates"), field.lattice, Qs, field.shape, float(spacing), merge, mass, g,
                     None, cut, None if frames is None else np.array(frames, dtype=np.int64).reshape(-1),
                     [made[t * L]["volume"] for t in range(T)], field.charges_converged)


def rigid_guest_diffusion(xyz, elements_or_coef, lattice, guest="CO2", temperatures=298.0, spacing: float = 0.5,
                          cutoff: float = 12.0, core2: float = 0.25, directions=None, cap: float = 100.0, merge=None, mass=None,
                          labels: bool = False, device=None, charges=None, ewald_tolerance: float = 1e-6) -> Diffusion:
    """The self-diffusion tensor of a rigid linear guest through the crystal at every temperature of ``temperatures``: the
    model of :func:`pywindow_amd.guest_diffusion` on the free energy of the guest's centre, ``-R T ln zbar`` of
    :func:`rigid_guest_field` (the same arguments), each temperature on its own field with its own basins and hop network.
    ``tensor`` is ``(L, 3, 3)``; ``raw``, ``n_basins``, ``n_sites``, ``trapped_fraction``, ``barrierless`` and
    ``winding_rank`` are per temperature, ``sites``, ``populations``, ``hops``, ``rates`` (and ``labels``) lists over the
    temperatures whose entries have one level; ``valid`` holds when every temperature is valid.  ``merge`` defaults to
    ``R * min(temperatures)`` for every temperature; ``mass`` (g/mol) comes from ``RIGID_GUEST_MASSES`` for N2, CO2 and O2
    and is required for a caller's :class:`pywindow_amd.RigidGuest`.  The orientational part of the transition state is
    in the field; the mass is the molecule's, so the rotational kinetic prefactor is left out.  ``charges`` /
    ``ewald_tolerance``: :func:`rigid_guest_field`'s; with ``"qeq-cell"`` a frame whose charges did not converge is not
    ``valid``."""
    x = np.asarray(xyz, dtype=np.float64)
    args = (elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, directions, cap, merge, mass, labels, device)
    kw = dict(charges=charges, ewald_tolerance=ewald_tolerance)
    if x.ndim == 3:
        return rigid_guest_diffusion_batch(x, *args, **kw)
    many = rigid_guest_diffusion_batch(x.reshape(1, -1, 3), *args, **kw)
    return dataclasses.replace(_one_diffusion(many), charges_converged=_first(many.charges_converged))
