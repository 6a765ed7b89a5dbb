"""Rigid non-linear guests (H2O, CH4, SF6) in a cage on the GPU: the affinity averaged over rotations
(``pw_rigid_body_affinity``, include/pywindow_amd.h).

:mod:`pywindow_amd.rigid` places a line of sites along a direction on the sphere.  Water, methane and sulfur hexafluoride
are not lines: their orientation is a full rotation (three Euler angles), and their sites do not lie on one line through
the voxel's centre.  Here the guest is a :class:`RigidBody` -- site positions in a body frame --, the orientations are a
set of rotation matrices (:func:`rotation_set`), and the two together make a POSE TABLE (:func:`body_poses`): per pose
and site the displacement of the site from the guest's centre.  The table is data handed through the ABI: the kernel
adds a row to the voxel's centre and knows nothing of rotations.  Everything after the site's position -- the pair
terms, the core, the charges, the Boltzmann average over the poses in a defined order, the sums -- is
``pw_rigid_affinity``'s, so the result is the same :class:`pywindow_amd.RigidAffinity` (``henry``, ``heat``,
``selectivity``, ``series``, ``free_energy_field`` ...), the device and the explicit host path (``device=-1``) return
the same bytes, and a linear guest written as a table returns ``pw_rigid_affinity``'s bytes.

What is left out.  The crystal cell: ``rigid_guest_field`` and its kin refuse a :class:`RigidBody`, because the cell's
proved atom skip has its reach stated for offsets along directions, not for pose tables.  Guest-guest terms (infinite
dilution).  Flexible guests: a table may hold several conformers, each in its rotations, but nothing here builds one.
Bodies of more than 8 sites (benzene, for one).

Parameters.  The framework atoms are UFF, Lorentz-Berthelot mixed with each site, as in :mod:`pywindow_amd.rigid`.  The
guest models of ``RIGID_BODIES``: H2O is SPC/E (H. J. C. Berendsen, J. R. Grigera and T. P. Straatsma, J. Phys. Chem. 91,
6269 (1987)); CH4 is the five-site OPLS-AA methane (W. L. Jorgensen, D. S. Maxwell and J. Tirado-Rives, J. Am. Chem. Soc.
118, 11225 (1996)); SF6 is the seven-site model of D. Dellis and J. Samios, Fluid Phase Equilib. 291, 81 (2010).  The
values in ``RIGID_BODIES`` were written down without the papers at hand and have not been checked against them line by
line: they sit in that one table, so a correction is one line.  The geometry is exact by construction: the tetrahedral
angle ``acos(-1/3)`` for H2O (SPC/E's 109.47 degrees) and CH4, the octahedron for SF6, every body placed on its centre of
mass.  Energies are kJ/mol, lengths Angstrom, charges e.  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib
from .affinity import R
from .rigid import RIGID_GUESTS, RigidAffinity, _batch, _one
from .surface import sphere_directions

__all__ = ["AXES_DEFAULT", "SPINS_DEFAULT", "RIGID_BODIES", "RIGID_BODY_MASSES", "RigidBody", "body_poses", "rotation_set",
           "rigid_body_affinity", "rigid_body_affinity_batch"]

#: the default rotation set ``rotation_set(AXES_DEFAULT, SPINS_DEFAULT)``, 1024 rotations, the entry's cap.  The rule was
#: the smallest set of 64 .. 512 rotations whose Henry coefficient on CC3 at 298 K is within 1 % of the (128, 8) value for
#: H2O, CH4 and SF6, and the largest when none is: none is (SF6 is 5 % off at (64, 8)).  DESIGN.md 7za has the table -- and
#: what it shows about SF6, for which ``rotation_set(204, 5)`` is the better set (see :func:`rotation_set`)
AXES_DEFAULT = 128
SPINS_DEFAULT = 8


@dataclasses.dataclass(frozen=True)
class RigidBody:
    """A rigid guest that need not be linear.  ``positions``: ``(S, 3)`` in Angstrom in the body frame, relative to the
    point that is placed at the voxel -- the centre of mass --, so a rotation turns the body about that point.  Per site
    ``sigma`` (Angstrom), ``eps / k_B`` (K; 0: no Lennard-Jones term, the site still blocks) and the charge (e)."""

    name: str
    positions: tuple
    sigma: tuple
    eps_k: tuple
    charges: tuple

    def __post_init__(self):
        p = np.asarray(self.positions, dtype=np.float64)
        S = len(self.sigma)
        if not 1 <= S <= _lib.RIGID_MAX_SITES or p.shape != (S, 3) or not (len(self.eps_k) == len(self.charges) == S):
            raise ValueError(f"RigidBody: 1 .. {_lib.RIGID_MAX_SITES} sites with a position (x, y, z), a sigma, an eps_k and a charge each")
        if not np.isfinite(p).all():
            raise ValueError("RigidBody: the positions are finite")
        object.__setattr__(self, "positions", tuple(tuple(float(v) for v in row) for row in p))


def _about_the_centre_of_mass(positions, masses):
    p, m = np.asarray(positions, dtype=np.float64), np.asarray(masses, dtype=np.float64)
    return p - (m[:, None] * p).sum(axis=0) / m.sum()


_TET = math.acos(-1.0 / 3.0)                              # the tetrahedral angle, 109.47 degrees
_M_H, _M_C, _M_O, _M_F, _M_S = 1.00794, 12.0107, 15.9994, 18.9984032, 32.065
_KCAL_K = 4.184 / R                                      # kcal/mol -> K


def _h2o():
    r, half = 1.0, 0.5 * _TET                            # SPC/E: r(OH) = 1 Angstrom, HOH the tetrahedral angle
    p = [(0.0, 0.0, 0.0), (r * math.sin(half), 0.0, -r * math.cos(half)), (-r * math.sin(half), 0.0, -r * math.cos(half))]
    return RigidBody("H2O", _about_the_centre_of_mass(p, (_M_O, _M_H, _M_H)), (3.166, 0.0, 0.0), (78.2, 0.0, 0.0),
                     (-0.8476, 0.4238, 0.4238))


def _ch4():
    r = 1.09 / math.sqrt(3.0)                            # OPLS-AA: r(CH) = 1.09 Angstrom, the vertices of a tetrahedron
    p = [(0.0, 0.0, 0.0), (r, r, r), (r, -r, -r), (-r, r, -r), (-r, -r, r)]
    return RigidBody("CH4", p, (3.50,) + (2.50,) * 4, (0.066 * _KCAL_K,) + (0.030 * _KCAL_K,) * 4, (-0.24,) + (0.06,) * 4)


def _sf6():
    r = 1.565                                            # Dellis and Samios: r(SF) = 1.565 Angstrom, the vertices of an octahedron
    p = [(0.0, 0.0, 0.0), (r, 0.0, 0.0), (-r, 0.0, 0.0), (0.0, r, 0.0), (0.0, -r, 0.0), (0.0, 0.0, r), (0.0, 0.0, -r)]
    return RigidBody("SF6", p, (3.228,) + (2.947,) * 6, (165.14,) + (27.02,) * 6, (0.66,) + (-0.11,) * 6)


#: name -> model: SPC/E water, OPLS-AA methane, Dellis and Samios SF6 (see the module's docstring: not checked line by line)
RIGID_BODIES = {"H2O": _h2o(), "CH4": _ch4(), "SF6": _sf6()}
#: name -> molar mass in g/mol
RIGID_BODY_MASSES = {"H2O": 2.0 * _M_H + _M_O, "CH4": _M_C + 4.0 * _M_H, "SF6": _M_S + 6.0 * _M_F}
assert not set(RIGID_BODIES) & set(RIGID_GUESTS), "a name is a linear guest or a body, not both"


def is_body(guest) -> bool:
    """Whether ``guest`` is a :class:`RigidBody` or a name of ``RIGID_BODIES``."""
    return isinstance(guest, RigidBody) or (isinstance(guest, str) and guest in RIGID_BODIES)


def _body(guest) -> RigidBody:
    return guest if isinstance(guest, RigidBody) else RIGID_BODIES[guest]


def _to_axis(d) -> np.ndarray:
    """The Rodrigues rotation taking ``z`` to the unit vector ``d`` (about ``z x d``, by the angle between them), built
    from the unit quaternion of half that angle so that it stays orthonormal to rounding next to ``-z``; ``d = -z``: the
    half turn about ``x``."""
    dx, dy, dz = (float(v) for v in d)
    rho = math.hypot(dx, dy)
    if rho == 0.0:
        return np.diag([1.0, 1.0, 1.0]) if dz > 0.0 else np.diag([1.0, -1.0, -1.0])
    c = max(-1.0, min(1.0, dz / math.hypot(rho, dz)))
    w, sh = math.sqrt(0.5 * (1.0 + c)), math.sqrt(0.5 * (1.0 - c))
    x, y = -dy / rho * sh, dx / rho * sh                             # the axis z x d, normalised, times sin(half the angle)
    norm = math.sqrt(w * w + x * x + y * y)
    w, x, y = w / norm, x / norm, y / norm
    return np.array([[1.0 - 2.0 * y * y, 2.0 * x * y, 2.0 * y * w],
                     [2.0 * x * y, 1.0 - 2.0 * x * x, -2.0 * x * w],
                     [-2.0 * y * w, 2.0 * x * w, 1.0 - 2.0 * (x * x + y * y)]])


def rotation_set(axes: int = AXES_DEFAULT, spins: int = SPINS_DEFAULT) -> np.ndarray:
    """``(axes * spins, 3, 3)`` proper rotations: for each ``d`` of ``pywindow_amd.sphere_directions(axes)`` and each of
    the ``spins`` angles ``phi_k = 2 pi (k + 1/2) / spins`` the rotation ``A(d) @ Rz(phi_k)``, ``A(d)`` the Rodrigues
    rotation taking ``z`` to ``d`` (``d = -z``: the half turn about ``x``).  Axes outer, spins inner: rotation
    ``a * spins + k``.  The body's ``z`` axis goes to ``d`` and the body is spun about it.  At most 1024 in all.

    A spin that is a symmetry of the body adds nothing.  SF6 has a four-fold axis on its ``z``: with ``spins = 4`` every
    axis holds one distinct pose four times, with 8 the angles 22.5 and 67.5 degrees, mirror images of each other; CH4
    has a two-fold axis there.  On CC3 the Henry coefficient of SF6 is 348 /bar at ``(128, 8)`` and 643, 641, 637 and 639
    at ``(102, 5)``, ``(204, 5)``, ``(146, 7)`` and ``(113, 9)``: for such a body take a number of spins
    that shares no factor with the order of the axis."""
    axes, spins = int(axes), int(spins)
    if axes < 1 or spins < 1 or axes * spins > _lib.RIGID_MAX_DIRS:
        raise ValueError(f"rotation_set: axes * spins in 1 .. {_lib.RIGID_MAX_DIRS}")
    out = np.zeros((axes * spins, 3, 3))
    for a, d in enumerate(sphere_directions(axes)):
        A = _to_axis(d)
        for k in range(spins):
            phi = 2.0 * math.pi * (k + 0.5) / spins
            c, s = math.cos(phi), math.sin(phi)
            out[a * spins + k] = A @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return out


def body_poses(body, rotations) -> np.ndarray:
    """The pose table ``(M, S, 3)`` of ``body`` (a :class:`RigidBody` or a name of ``RIGID_BODIES``) in the ``(M, 3, 3)``
    ``rotations``: row ``[o, s]`` is ``R_o p_s``, element by element in the written association
    ``(R[:, :, 0] * p0 + R[:, :, 1] * p1) + R[:, :, 2] * p2`` -- no ``matmul``, whose order of additions is not defined.
    A body on the ``z`` axis (``p = (0, 0, t)``, ``t != 0``) in rotations whose third column is ``d`` therefore gives
    exactly ``t * d``, the site of a linear guest (with ``t = 0`` a zero of either sign)."""
    p = np.asarray(_body(body).positions, dtype=np.float64)
    rot = np.ascontiguousarray(rotations, dtype=np.float64)
    if rot.ndim != 3 or rot.shape[1:] != (3, 3):
        raise ValueError("rotations: (M, 3, 3)")
    c0, c1, c2 = rot[:, None, :, 0], rot[:, None, :, 1], rot[:, None, :, 2]
    return (c0 * p[None, :, 0, None] + c1 * p[None, :, 1, None]) + c2 * p[None, :, 2, None]


def _table(body, rotations):
    rot = rotation_set() if rotations is None else np.ascontiguousarray(rotations, dtype=np.float64)
    if rot.ndim != 3 or rot.shape[1:] != (3, 3) or not 1 <= len(rot) <= _lib.RIGID_MAX_DIRS:
        raise ValueError(f"rotations: (M, 3, 3), M in 1 .. {_lib.RIGID_MAX_DIRS}")
    return rot, np.ascontiguousarray(body_poses(body, rot))


def rigid_body_affinity_batch(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, rotations=None, charges=None,
                              maps: bool = False, level: int = 0, core2: float = 0.25, cutoff2: float = 0.0, device=None,
                              frames=None, kernel_ms=None) -> RigidAffinity:
    """:func:`rigid_body_affinity` for ``T`` frames of the same ``n`` atoms in ONE ``pw_rigid_body_affinity`` call; the
    arguments are :func:`pywindow_amd.rigid_guest_affinity_batch`'s with ``rotations`` in place of ``directions``.  The
    frames share the coefficients, the pose table and the temperatures."""
    body = _body(guest)
    rot, poses = _table(body, rotations)
    return _batch(xyz, elements_or_coef, body, temperatures, cavity, grid, np.ascontiguousarray(rot[:, :, 2]), poses, rot, charges,
                  maps, level, core2, cutoff2, device, frames, kernel_ms)


def rigid_body_affinity(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, rotations=None, charges=None,
                        maps: bool = False, level: int = 0, core2: float = 0.25, cutoff2: float = 0.0,
                        device=None) -> RigidAffinity:
    """The affinity of the cage ``xyz`` ``(n, 3)`` for a rigid body, averaged over ``rotations``, at the ``temperatures``
    (K, at most 8): a :class:`pywindow_amd.RigidAffinity` with ``rotations``, ``min_rotation`` and ``min_sites``; its
    ``directions`` are the images of the body's ``z`` axis.  ``guest``: a name of ``RIGID_BODIES`` or a
    :class:`RigidBody`.  ``rotations``: ``(M, 3, 3)``, at most 1024; ``None``: ``rotation_set()``, all 1024 -- no set of
    the ladder 64 .. 512 had its Henry coefficient on CC3 at 298 K within 1 % of the ``(128, 8)`` value for H2O (with
    and without framework charges), CH4 and SF6 alike, so the default is the largest; for SF6 it is still not converged
    (DESIGN.md 7za has the table, :func:`rotation_set` the reason and the remedy).  They are data: the pose
    table :func:`body_poses` makes of them is what the library sees, and nothing checks that they are rotations.
    ``elements_or_coef``, ``charges`` (``None``, one per atom, one row a frame or ``"qeq"``), ``cavity`` / ``grid``,
    ``maps`` / ``level``, ``core2``, ``cutoff2`` and ``device`` are :func:`pywindow_amd.rigid_guest_affinity`'s; ready
    rows are ``(S, n, 3)`` with ``S`` the body's sites.  ``xyz`` ``(T, n, 3)`` is :func:`rigid_body_affinity_batch`."""
    x = np.asarray(xyz, dtype=np.float64)
    args = (elements_or_coef, guest, temperatures, cavity, grid, rotations, charges, maps, level, core2, cutoff2, device)
    if x.ndim == 3:
        return rigid_body_affinity_batch(x, *args)
    return _one(rigid_body_affinity_batch(x.reshape(1, -1, 3), *args))
