"""Rigid linear guests (N2, CO2, O2) in a cage on the GPU: the orientation-averaged affinity (``pw_rigid_affinity``,
include/pywindow_amd.h).

:mod:`pywindow_amd.affinity` treats the guest as one Lennard-Jones sphere.  The molecules porous cages are studied for
above all -- CO2, N2, O2 -- are not spheres: a linear molecule threads a window end-on and lies along a wall.  Here the
guest is a rigid line of sites (Lennard-Jones centres and optional point charges at offsets along one axis).  It is
inserted with its centre at every voxel of a region -- the mask of a :class:`pywindow_amd.Cavity`, or a whole grid -- in
every one of ``M`` orientations; a pose's energy is the sum of the pair terms of all its sites with every atom of the
cage, and per voxel the Boltzmann factors are averaged over the orientations, all in a defined order of additions, so
the device and the explicit host path (``device=-1``) return the same bytes.  From the sums, as for a one-site guest:
``boltzmann_volume``, ``henry``, ``mean_energy``, ``heat``, ``min_energy`` with its position and direction, and
``selectivity`` -- "CO2 over N2?".

What is left out.  This module's guests are linear (all sites on one axis); rigid bodies -- H2O, CH4, SF6 -- are
:mod:`pywindow_amd.rigid_body`, which returns the same :class:`RigidAffinity`.  No guest-guest term: infinite dilution.  The bundled
cage model (UFF) carries no partial charges, so without ``charges`` the job is uncharged and the guest's own charges do
nothing; ``charges`` are the caller's, one set for all frames or one a frame, or ``"qeq"``: the library equilibrates them
itself, frame by frame (:mod:`pywindow_amd.charges`).  Passage and hopping of a rigid guest go through
:meth:`RigidAffinity.free_energy_field`, which :func:`pywindow_amd.passage_field` accepts.

Parameters.  The framework atoms are UFF as in :mod:`pywindow_amd.affinity`, Lorentz-Berthelot mixed with each site.
The guests are the TraPPE models: N2 and CO2 from J. J. Potoff and J. I. Siepmann, AIChE J. 47, 1676 (2001); O2 from
L. Zhang and J. I. Siepmann, Theor. Chem. Acc. 115, 391 (2006).  The values in ``RIGID_GUESTS`` have not been checked
against those papers line by line: they sit in that one table, so a correction is one line.  Energies are kJ/mol,
lengths Angstrom, charges e.  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine
from .affinity import _PER_BAR, R, UFF, Affinity
from .surface import sphere_directions

__all__ = ["COULOMB", "M_DEFAULT", "RIGID_GUESTS", "RigidAffinity", "RigidGuest", "rigid_coefficients",
           "rigid_guest_affinity", "rigid_guest_affinity_batch"]

#: e^2 / (4 pi eps_0) in kJ Angstrom / mol
COULOMB = 1389.35457644382
#: the default number of orientations: the smallest of 16, 32, 64, 128, 256 whose Henry coefficient on CC3 is within 1 %
#: of the 1024-orientation value for both CO2 and N2 at 298 K (DESIGN.md 7q has the table)
M_DEFAULT = 64


@dataclasses.dataclass(frozen=True)
class RigidGuest:
    """A rigid linear guest: per site the offset along the axis from the centre (Angstrom), ``sigma`` (Angstrom),
    ``eps / k_B`` (K; 0: no Lennard-Jones term, the site still blocks) and the charge (e)."""

    name: str
    offsets: tuple
    sigma: tuple
    eps_k: tuple
    charges: tuple

    def __post_init__(self):
        S = len(self.offsets)
        if not 1 <= S <= _lib.RIGID_MAX_SITES or not (len(self.sigma) == len(self.eps_k) == len(self.charges) == S):
            raise ValueError(f"RigidGuest: 1 .. {_lib.RIGID_MAX_SITES} sites with one sigma, eps_k and charge each")


#: name -> model.  TraPPE: N2 and CO2 Potoff and Siepmann 2001, O2 Zhang and Siepmann 2006 (see the module's docstring)
RIGID_GUESTS = {
    "N2": RigidGuest("N2", (-0.55, 0.0, 0.55), (3.31, 0.0, 3.31), (36.0, 0.0, 36.0), (-0.482, 0.964, -0.482)),
    "CO2": RigidGuest("CO2", (-1.16, 0.0, 1.16), (3.05, 2.80, 3.05), (79.0, 27.0, 79.0), (-0.35, 0.70, -0.35)),
    "O2": RigidGuest("O2", (-0.605, 0.0, 0.605), (3.02, 0.0, 3.02), (49.0, 0.0, 49.0), (-0.113, 0.226, -0.113)),
}

_SERIES = ("boltzmann_volume", "henry", "mean_energy", "heat", "min_energy", "n_voxels", "n_dead")


def _guest(guest):
    """The model of a guest: a name of ``RIGID_GUESTS``, or a model as it is (a :class:`RigidGuest`, or a
    :class:`pywindow_amd.RigidBody`, which has the same ``sigma``, ``eps_k`` and ``charges``)."""
    return RIGID_GUESTS[guest] if isinstance(guest, str) else guest


def rigid_coefficients(elements, guest, charges=None) -> np.ndarray:
    """Rows ``(A, B, C)`` ``(S, n, 3)`` between every site of ``guest`` (a name of ``RIGID_GUESTS``, a
    :class:`RigidGuest` or a :class:`pywindow_amd.RigidBody`) and every framework atom: ``A = 4 eps sigma^12`` and
    ``B = 4 eps sigma^6`` from UFF, Lorentz-Berthelot mixed as :func:`pywindow_amd.lj_coefficients` does (a site with ``eps = 0`` gets ``A = B = 0``; it
    still blocks within the core), and ``C = COULOMB q_a q_s`` with ``charges`` the ``(n,)`` framework charges in e.
    With ``charges=None`` the column is zero and a job made from the rows is uncharged: the guest's charges do
    nothing, because the bundled cage model carries no charges.  ``charges`` ``(F, n)``, one row a frame, gives
    ``(F, S, n, 3)``: frame ``f``'s rows are those of ``charges[f]``.  An element without UFF parameters raises
    ``KeyError``."""
    if charges is not None and np.ndim(charges) == 2:
        per_frame = np.asarray(charges, dtype=np.float64)
        return np.stack([rigid_coefficients(elements, guest, row) for row in per_frame]) if len(per_frame) else \
            np.zeros((0, len(_guest(guest).sigma), len(list(elements)), 3))
    g = _guest(guest)
    rows = np.array([UFF[str(e).upper()] for e in elements], dtype=np.float64).reshape(-1, 2)
    n = len(rows)
    q = np.zeros(n) if charges is None else np.asarray(charges, dtype=np.float64).reshape(-1)
    if len(q) != n:
        raise ValueError("charges: one per atom")
    out = np.zeros((len(g.sigma), n, 3))
    for s, (sigma_s, eps_k, q_s) in enumerate(zip(g.sigma, g.eps_k, g.charges)):
        sigma = (rows[:, 0] / 2.0 ** (1.0 / 6.0) + float(sigma_s)) / 2.0
        eps = np.sqrt(4.184 * rows[:, 1] * (R * float(eps_k)))
        s6 = sigma ** 6
        if eps_k != 0.0:
            out[s, :, 0], out[s, :, 1] = 4.0 * eps * s6 * s6, 4.0 * eps * s6
        out[s, :, 2] = COULOMB * q * float(q_s)
    return out


@dataclasses.dataclass(frozen=True)
class RigidAffinity:
    """The orientation-averaged affinity of one frame (``raw`` a record, ``levels`` ``(L,)``) or of ``T`` frames (``raw``
    ``(T,)``, ``levels`` ``(T, L)``) at the ``L`` ``temperatures``.  ``raw`` holds ``pw_rigid_affinity``'s row
    (``_lib.RIGID_OUT_DTYPE``), ``levels`` its ``(Z, E)`` rows; ``maps`` (when asked for) per voxel of the region in
    rank order ``(zbar at temperature map_level, the lowest pose energy)``, a list of arrays for many frames.
    ``closed``: the cavity's (``None`` for a plain grid)."""

    raw: np.ndarray
    levels: np.ndarray
    temperatures: np.ndarray
    origin: np.ndarray
    shape: np.ndarray
    spacing: float
    directions: np.ndarray
    guest: object = None
    closed: object = None
    maps: object = None
    map_level: int = -1
    charged: bool = False
    frames: np.ndarray | None = None
    charges_converged: object = None      # with charges="qeq": whether the frame's charge equilibration converged
    rotations: object = None              # of a rigid body (pywindow_amd.rigid_body): the (M, 3, 3) rotations of its poses
    poses: object = None                  # of a rigid body: the (M, S, 3) displacements of the sites, pose by pose

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
    def boltzmann_volume(self):
        """``Z h^3`` in cubic Angstrom, per temperature; ``Z`` the sum of the orientation-averaged Boltzmann factors."""
        return self.levels["z"] * (self.spacing * self.spacing * self.spacing)

    @property
    def henry(self):
        """The Henry coefficient of the cage, ``boltzmann_volume / (k_B T)``, in molecules per cage and bar."""
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
        """The centre of the voxel of ``min_energy``; NaN without one."""
        v = np.asarray(self.raw["min_voxel"], dtype=np.float64)
        return np.where(v < 0.0, np.nan, self.origin + self.spacing * v)

    @property
    def min_direction(self):
        """The direction of the pose of ``min_energy``; NaN without one."""
        o = np.asarray(self.raw["min_dir"])
        d = self.directions[np.maximum(o, 0)]
        return np.where((o < 0)[..., None], np.nan, d)

    @property
    def min_rotation(self):
        """The rotation ``(3, 3)`` of the pose of ``min_energy`` of a rigid body; NaN without one, and for a result that
        has no ``rotations``."""
        o = np.asarray(self.raw["min_dir"])
        if self.rotations is None:
            return np.full(o.shape + (3, 3), np.nan)
        return np.where((o < 0)[..., None, None], np.nan, np.asarray(self.rotations)[np.maximum(o, 0)])

    @property
    def min_sites(self):
        """The positions ``(S, 3)`` of the guest's sites in the pose of ``min_energy``, for looking at it; NaN without
        one."""
        o = np.asarray(self.raw["min_dir"])
        if self.poses is not None:
            p = np.asarray(self.poses)[np.maximum(o, 0)]
        else:
            p = np.asarray(self.guest.offsets, dtype=np.float64)[:, None] * self.directions[np.maximum(o, 0)][..., None, :]
        return np.where((o < 0)[..., None, None], np.nan, self.min_position[..., None, :] + p)

    def selectivity(self, other):
        """The ratio of this guest's Henry coefficient to ``other``'s, a :class:`RigidAffinity` or an
        :class:`pywindow_amd.Affinity` (same frames, region and temperatures)."""
        if not isinstance(other, (RigidAffinity, Affinity)):
            raise TypeError("selectivity: a RigidAffinity or an Affinity")
        if not np.array_equal(self.temperatures, other.temperatures):
            raise ValueError("selectivity: the two results are for different temperatures")
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.boltzmann_volume / other.boltzmann_volume

    def series(self, name: str = "boltzmann_volume", level: int = 0):
        """``(values, valid)`` of a quantity over the frames at temperature ``level``, with the validity rule of
        :meth:`pywindow_amd.Affinity.series`: the cavity is closed (always, for a plain grid), the frame was not
        clamped and the value is finite -- and, with ``charges="qeq"``, the frame's charges converged."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = np.asarray(getattr(self, name), dtype=np.float64)
        if name in ("boltzmann_volume", "henry", "mean_energy", "heat"):
            v = v[..., level]
        values = np.atleast_1d(v).copy()
        valid = np.isfinite(values) & ~np.atleast_1d(self.clamped)
        if self.closed is not None:
            valid &= np.atleast_1d(np.asarray(self.closed, dtype=bool))
        if self.charges_converged is not None:
            valid &= np.atleast_1d(np.asarray(self.charges_converged, dtype=bool))
        return values, valid

    def free_energy_field(self, t=None):
        """``-R T ln zbar`` ``(nz, ny, nx)`` in kJ/mol of a grid job made with ``maps=True`` (frame ``t`` of many), ``+inf``
        where ``zbar == 0``: the orientation-averaged free energy of the guest's centre, which
        :func:`pywindow_amd.passage_field` accepts as its field."""
        if self.maps is None or self.closed is not None:
            raise ValueError("free_energy_field: a result over a grid made with maps=True")
        many = self.raw.ndim == 1
        if many != (t is not None):
            raise ValueError("free_energy_field: t for a result over many frames, and only then")
        maps, shape = (self.maps[t], self.shape[t]) if many else (self.maps, self.shape)
        zbar = maps[:, 0].reshape(int(shape[2]), int(shape[1]), int(shape[0]))
        with np.errstate(divide="ignore"):
            return np.where(zbar == 0.0, np.inf, -(R * self.temperatures[self.map_level]) * np.log(zbar))


def rigid_guest_affinity_batch(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, directions=None,
                               charges=None, maps: bool = False, level: int = 0, core2: float = 0.25,
                               cutoff2: float = 0.0, device=None, frames=None, kernel_ms=None) -> RigidAffinity:
    """:func:`rigid_guest_affinity` for ``T`` frames of the same ``n`` atoms in ONE ``pw_rigid_affinity`` call: ``xyz``
    ``(T, n, 3)``; ``cavity`` the :class:`pywindow_amd.Cavity` of the same ``T`` frames made with ``mask=True``, or
    ``grid = (origin (3,) or (T, 3), spacing, (nx, ny, nz))``.  The frames share the coefficients, the directions and
    the temperatures; ``charges`` may be ``(n,)`` for all frames or ``(T, n)``, one row a frame (the coefficient rows are
    then per frame), or ``"qeq"``: ONE ``pw_charges`` call over the same frames makes them
    (:func:`pywindow_amd.equilibrate_charges_batch`, total charge 0), and a frame whose charges did not converge is not
    valid in :meth:`RigidAffinity.series`.  ``kernel_ms``: a list that receives the time of the device work by HIP
    events."""
    d = sphere_directions(M_DEFAULT) if directions is None else np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    if not 1 <= len(d) <= _lib.RIGID_MAX_DIRS:
        raise ValueError(f"directions: 1 .. {_lib.RIGID_MAX_DIRS} rows of three")
    return _batch(xyz, elements_or_coef, _guest(guest), temperatures, cavity, grid, d, None, None, charges, maps, level, core2,
                  cutoff2, device, frames, kernel_ms)


def _batch(xyz, elements_or_coef, g, temperatures, cavity, grid, d, poses, rotations, charges, maps, level, core2, cutoff2,
           device, frames, kernel_ms) -> RigidAffinity:
    """What :func:`rigid_guest_affinity_batch` and :func:`pywindow_amd.rigid_body_affinity_batch` share: the coefficient
    rows, the charges, the jobs over the cavities or the grid, the call and the result.  ``poses`` ``None``: the linear
    guest ``g`` in the directions ``d`` through ``pw_rigid_affinity``; otherwise the ``(M, S, 3)`` pose table of the
    body ``g`` through ``pw_rigid_body_affinity``, with ``d`` and ``rotations`` kept for the result."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    S = len(g.sigma)
    charges_converged = None
    coef = np.asarray(elements_or_coef)
    if coef.dtype.kind in "fiu" and coef.ndim == 3 and coef.shape[2] == 3:
        if isinstance(charges, str):
            raise ValueError('charges="qeq" needs the elements, not ready rows')
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        charged = bool((coef[:, :, 2] != 0.0).any())
    else:
        if isinstance(charges, str):
            if charges != "qeq":
                raise ValueError('charges: None, one per atom, one row a frame or "qeq"')
            from .charges import equilibrate_charges_batch

            made = equilibrate_charges_batch(x, list(elements_or_coef), device=device)
            charges_converged = np.atleast_1d(made.converged).copy()
            charges = np.where(np.isfinite(made.charges), made.charges, 0.0)   # (NaN: a frame that is not valid anyway)
        coef = rigid_coefficients(list(elements_or_coef), g, charges)
        charged = charges is not None
    per_frame_coef = coef.ndim == 4
    if coef.shape != ((T, S, n, 3) if per_frame_coef else (S, n, 3)):
        raise ValueError("elements_or_coef: one element per atom, or rows (A, B, C) (S, n, 3); charges: (n,) or (T, n)")
    temps = np.atleast_1d(np.asarray(temperatures, dtype=np.float64))
    if temps.ndim != 1 or not 1 <= len(temps) <= _lib.AFF_MAX_LEVELS or not (np.isfinite(temps) & (temps > 0.0)).all():
        raise ValueError(f"temperatures: 1 .. {_lib.AFF_MAX_LEVELS} positive numbers")
    if maps and not 0 <= int(level) < len(temps):
        raise ValueError("level: one of the temperatures")
    if (cavity is None) == (grid is None):
        raise ValueError("one of cavity and grid")
    jobs = np.zeros(T, dtype=_lib.RIGID_JOB_DTYPE if poses is None else _lib.RIGID_BODY_JOB_DTYPE)
    jobs["atom_first"] = np.arange(T) * n
    if per_frame_coef:
        jobs["coef_first"] = np.arange(T) * (S * n)
    jobs["n"] = n
    jobs["n_betas"] = len(temps)
    jobs["n_sites"] = S
    jobs["n_dirs"] = len(d) if poses is None else len(poses)
    jobs["level_first"] = np.arange(T) * len(temps)
    jobs["out"] = np.arange(T)
    jobs["core2"], jobs["cutoff2"] = float(core2), float(cutoff2)
    jobs["charged"] = int(charged)
    words = closed = None
    if cavity is not None:
        if cavity.words is None:
            raise ValueError("cavity: a Cavity made with mask=True")
        packed = [cavity.words] if cavity.raw.ndim == 0 else list(cavity.words)
        if len(packed) != T:
            raise ValueError("cavity: one cavity per frame")
        jobs["word_first"] = np.concatenate([[0], np.cumsum([len(p) for p in packed])[:-1]]) if T else 0
        jobs["origin"] = np.asarray(cavity.origin, dtype=np.float64).reshape(T, 3)
        jobs["spacing"] = spacing = float(cavity.spacing)
        shape = np.asarray(cavity.shape).reshape(T, 3)
        words = np.concatenate(packed) if packed else None
        closed = np.atleast_1d(np.asarray(cavity.closed, dtype=bool)).copy()
        voxels = np.atleast_1d(np.asarray(cavity.n_voxels, dtype=np.int64))
    else:
        origin, spacing, dims = grid
        jobs["word_first"] = -1
        jobs["origin"] = np.broadcast_to(np.asarray(origin, dtype=np.float64), (T, 3))
        jobs["spacing"] = spacing = float(spacing)
        shape = np.broadcast_to(np.asarray(dims, dtype=np.int64), (T, 3))
        voxels = shape.prod(axis=1)
    jobs["nx"], jobs["ny"], jobs["nz"] = shape[:, 0], shape[:, 1], shape[:, 2]
    jobs["map_level"], jobs["map_first"] = -1, -1
    buf = None
    if maps:
        jobs["map_level"] = int(level)
        jobs["map_first"] = 2 * np.concatenate([[0], np.cumsum(voxels)[:-1]]) if T else 0
        buf = np.zeros(2 * int(voxels.sum()))
    ctx, betas = engine.context(device), 1.0 / (R * temps)
    if poses is None:
        out, levels, buf = ctx.rigid_affinity(jobs, x.reshape(-1, 3), coef.reshape(-1, 3), np.asarray(g.offsets), d, betas, words,
                                              maps=buf, kernel_ms=kernel_ms)
    else:
        out, levels, buf = ctx.rigid_body_affinity(jobs, x.reshape(-1, 3), coef.reshape(-1, 3), poses.reshape(-1, 3), betas, words,
                                                   maps=buf, kernel_ms=kernel_ms)
    per_frame = None
    if maps:
        per_frame = [buf[int(f):int(f) + 2 * int(v)].reshape(-1, 2) for f, v in zip(jobs["map_first"], voxels)]
    return RigidAffinity(out, levels.reshape(T, len(temps)), temps, jobs["origin"].copy(), np.array(shape, dtype=np.int64),
                         spacing, d, g, closed, per_frame, int(level) if maps else -1, charged,
                         None if frames is None else np.array(frames, dtype=np.int64).reshape(-1), charges_converged, rotations,
                         poses)


def _one(many: RigidAffinity) -> RigidAffinity:
    """The only frame of a result over one frame."""
    return dataclasses.replace(many, raw=many.raw[0], levels=many.levels[0], origin=many.origin[0], shape=many.shape[0],
                               closed=None if many.closed is None else many.closed[0],
                               maps=None if many.maps is None else many.maps[0], frames=None,
                               charges_converged=None if many.charges_converged is None else many.charges_converged[0])


def rigid_guest_affinity(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, directions=None, charges=None,
                         maps: bool = False, level: int = 0, core2: float = 0.25, cutoff2: float = 0.0,
                         device=None) -> RigidAffinity:
    """The orientation-averaged affinity of the cage ``xyz`` ``(n, 3)`` for a rigid linear guest at the
    ``temperatures`` (K, at most 8): see :class:`RigidAffinity`.  ``guest``: a name of ``RIGID_GUESTS`` or a
    :class:`RigidGuest`.  ``elements_or_coef``: the atoms' element symbols (:func:`rigid_coefficients`, with
    ``charges`` the framework's partial charges in e, or ``"qeq"``: made by
    :func:`pywindow_amd.equilibrate_charges`), or ready rows ``(A, B, C)`` ``(S, n, 3)`` (charged when some
    ``C`` is not zero).  With elements and ``charges=None`` the job is uncharged and the guest's charges do nothing: the
    bundled cage model carries no charges.  The region is the mask of ``cavity`` (made with ``mask=True``) or every
    voxel of ``grid = (origin, spacing, (nx, ny, nz))``.  ``directions``: ``(M, 3)`` unit vectors, at most 1024
    (``None``: ``pywindow_amd.sphere_directions(M_DEFAULT)``); they are data, neither normalised nor checked for
    length.  A pose with a site within ``sqrt(core2)`` of an atom is blocked: it adds nothing.  ``cutoff2``: the square
    of a cutoff, ``0``: none.  ``maps=True`` keeps per voxel ``zbar`` at temperature ``level`` and the lowest pose
    energy.  ``xyz`` ``(T, n, 3)`` is :func:`rigid_guest_affinity_batch`.  ``device``: the HIP ordinal (``None``: the
    process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return rigid_guest_affinity_batch(x, elements_or_coef, guest, temperatures, cavity, grid, directions, charges, maps,
                                          level, core2, cutoff2, device)
    return _one(rigid_guest_affinity_batch(x.reshape(1, -1, 3), elements_or_coef, guest, temperatures, cavity, grid, directions,
                                           charges, maps, level, core2, cutoff2, device))
