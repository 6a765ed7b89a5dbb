"""Ewald electrostatics on the periodic cell: the parameters of the sum and the potential of a framework's point charges
(``pw_rigid_cell_ewald``, include/pywindow_amd.h; the definition in pywindow_amd/csrc/pw_ewald.hpp).

The energy of a charge ``q`` at ``x`` among the point charges ``q_j`` of a neutral periodic framework is split at
``alpha``: a real-space part ``COULOMB q q_j erfc(alpha r) / r`` over the images within the cutoff, which the field kernel
of :mod:`pywindow_amd.rigid_cell` adds to its pair term, and a reciprocal part ``sum_k w_k Re[S(k) exp(-i k.x)] q`` over half
of the reciprocal lattice, ``S(k) = sum_j q_j exp(i k.x_j)`` and ``w_k = COULOMB (8 pi / V) exp(-k^2 / (4 alpha^2)) / k^2``.
The library takes ``alpha`` and the rows ``(h, k, l, w)`` as data; :func:`ewald_parameters` makes them.

What is left out: the guest's interaction with its own images (infinite dilution); any self or background term (none
arises between a guest and a neutral framework, and a framework that is not neutral is refused); non-linear guests.
Periodic charge equilibration is ``pw_charges_cell`` (:mod:`pywindow_amd.charges_cell`, ``charges="qeq-cell"``);
``charges="qeq"`` on a cell stays refused: it is the isolated-molecule model.  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .rigid import COULOMB, RigidGuest

__all__ = ["EwaldPotential", "ewald_parameters", "ewald_potential", "framework_charges"]

#: a framework is neutral when ``|sum q| <= NEUTRAL * sum |q|``
NEUTRAL = 1e-8


def _half_space(lat, alpha, kmax):
    """The rows ``(h, k, l, w)`` of the half space ``h > 0``, or ``h == 0 and k > 0``, or ``h == k == 0 and l > 0`` with
    ``0 < |k| <= kmax``, in the order of ``(h, k, l)`` ascending, and the largest ``|index|`` that was tried."""
    recip = 2.0 * math.pi * np.linalg.inv(lat)                       # rows: 2 pi a*, 2 pi b*, 2 pi c*
    lengths = np.sqrt((lat * lat).sum(axis=0))
    top = np.floor(kmax * lengths / (2.0 * math.pi)).astype(np.int64)   # |h| <= k . a / 2 pi <= kmax |a| / 2 pi
    if (top > 4 * _lib.EWALD_MAX_INDEX).any():
        return None, int(top.max())
    h, k, l = np.meshgrid(np.arange(0, top[0] + 1), np.arange(-top[1], top[1] + 1), np.arange(-top[2], top[2] + 1), indexing="ij")
    h, k, l = h.reshape(-1), k.reshape(-1), l.reshape(-1)            # (C order: (h, k, l) ascending)
    half = (h > 0) | ((h == 0) & (k > 0)) | ((h == 0) & (k == 0) & (l > 0))
    vec = h[:, None] * recip[0] + k[:, None] * recip[1] + l[:, None] * recip[2]
    k2 = (vec * vec).sum(axis=1)
    keep = half & (k2 <= kmax * kmax)
    h, k, l, k2 = h[keep], k[keep], l[keep], k2[keep]
    volume = abs(float(np.linalg.det(lat)))
    w = COULOMB * (8.0 * math.pi / volume) * np.exp(-k2 / (4.0 * alpha * alpha)) / k2
    rows = np.stack([h.astype(np.float64), k.astype(np.float64), l.astype(np.float64), w], axis=1)
    return rows, int(max(np.abs(rows[:, :3]).max(), 0)) if len(rows) else 0


def ewald_parameters(lattice, cutoff: float, tolerance: float = 1e-6):
    """``(alpha, rows)`` of the Ewald sum on the cell ``lattice`` (columns as vectors) whose real-space part is cut at
    ``cutoff``: ``alpha = sqrt(-ln tolerance) / cutoff``, so that ``erfc(alpha cutoff) ~ tolerance``; ``kmax = 2 alpha
    sqrt(-ln tolerance)``, so that ``exp(-kmax^2 / (4 alpha^2)) = tolerance``; and the rows ``(h, k, l, w)`` ``(K, 4)`` of the
    reciprocal vectors ``k = 2 pi (h a* + k b* + l c*)`` with ``0 < |k| <= kmax`` in the half space ``h > 0``, or ``h == 0``
    and ``k > 0``, or ``h == k == 0`` and ``l > 0``, listed with ``(h, k, l)`` ascending, ``w = COULOMB (8 pi / V) exp(-k^2 /
    (4 alpha^2)) / k^2`` in kJ/mol per squared charge.  The indices refer to the cell's own vectors, so they hold in the
    triangular frame the library works in.  More than ``PW_EWALD_MAX_K`` rows or an index above ``PW_EWALD_MAX_INDEX``:
    ``ValueError`` that names the tolerance that fits."""
    lat = np.asarray(lattice, dtype=np.float64)
    cutoff, tolerance = float(cutoff), float(tolerance)
    if lat.shape != (3, 3) or not np.isfinite(lat).all() or abs(float(np.linalg.det(lat))) == 0.0:
        raise ValueError("lattice: a finite (3, 3) array of three vectors that span a cell")
    if not (math.isfinite(cutoff) and cutoff > 0.0 and 0.0 < tolerance < 1.0):
        raise ValueError("cutoff: a positive number; tolerance: within (0, 1)")

    def rows_at(tol):
        root = math.sqrt(-math.log(tol))
        alpha = root / cutoff
        rows, top = _half_space(lat, alpha, 2.0 * alpha * root)
        fits = rows is not None and len(rows) <= _lib.EWALD_MAX_K and top <= _lib.EWALD_MAX_INDEX
        return alpha, rows, fits

    alpha, rows, fits = rows_at(tolerance)
    if not fits:
        tol = tolerance
        while tol < 0.5 and not rows_at(tol)[2]:
            tol *= 10.0 ** 0.25
        raise ValueError(f"ewald_parameters: tolerance {tolerance:.3g} at cutoff {cutoff:.6g} needs "
                         f"{'more than the cap of' if rows is None else len(rows)} rows of the reciprocal sum, the library takes "
                         f"{_lib.EWALD_MAX_K} with indices up to {_lib.EWALD_MAX_INDEX}: the tolerance that fits is {tol:.3g}")
    return alpha, np.ascontiguousarray(rows)


def framework_charges(charges, T: int, n: int):
    """``charges`` as ``(T, n)`` float64: one value per atom, or one row a frame.  ``"qeq"`` is refused -- that is the
    isolated-molecule model; the periodic one is ``"qeq-cell"``, which :mod:`pywindow_amd.rigid_cell` turns into numbers
    before it comes here -- and so is a frame whose charges do not sum to zero within ``1e-8 * sum |q|``: the Ewald sum has
    no background term."""
    if isinstance(charges, str):
        if charges == "qeq":
            raise ValueError("charges: \"qeq\" is the isolated-molecule model (pw_charges equilibrates one molecule in vacuum); "
                             "on a cell use \"qeq-cell\" (pw_charges_cell, periodic charge equilibration) or give the cell's "
                             "charges as numbers")
        raise ValueError("charges: one value per atom, or one row a frame")
    q = np.asarray(charges, dtype=np.float64)
    if q.ndim == 1:
        q = np.broadcast_to(q, (T, len(q)))
    if q.shape != (T, n) or not np.isfinite(q).all():
        raise ValueError("charges: finite, one value per atom, or one row a frame")
    total, size = np.abs(q.sum(axis=1)), np.abs(q).sum(axis=1)
    bad = np.nonzero(total > NEUTRAL * size)[0]
    if len(bad):
        t = int(bad[0])
        raise ValueError(f"charges: the framework of frame {t} is not neutral (sum {float(q[t].sum()):.6g} against sum |q| "
                         f"{float(size[t]):.6g}): the Ewald sum has no background term")
    return np.ascontiguousarray(q)


@dataclasses.dataclass(frozen=True)
class EwaldPotential:
    """``phi`` ``(nz, ny, nx)``: the energy in kJ/mol of a unit point charge (+1 e) at every voxel centre of the cell's grid,
    ``+inf`` within ``sqrt(core2)`` of an atom.  ``shape`` ``(nx, ny, nz)``, ``origin`` and ``step`` the grid in the frame of
    the triangular cell, ``rotation`` the ``Q`` of :func:`pywindow_amd.channels.triangular_lattice` (voxel centres in the
    caller's frame: ``x_triangular @ Q.T``); ``alpha`` and ``n_k`` the parameters of the sum."""

    phi: np.ndarray
    shape: np.ndarray
    origin: np.ndarray
    step: np.ndarray
    rotation: np.ndarray
    alpha: float
    n_k: int

    def positions(self):
        """The voxel centres ``(nz, ny, nx, 3)`` in the caller's frame."""
        nx, ny, nz = (int(v) for v in self.shape)
        l, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        o, s = self.origin, self.step
        p = np.stack([((o[0] + i * s[0]) + j * s[1]) + l * s[3], (o[1] + j * s[2]) + l * s[4], o[2] + l * s[5]], axis=-1)
        return p @ self.rotation.T


def ewald_potential(xyz, charges, lattice, spacing: float = 0.5, cutoff: float = 12.0, tolerance: float = 1e-6,
                    core2: float = 0.25, device=None) -> EwaldPotential:
    """The electrostatic potential energy of a unit point charge on the grid of the cell ``lattice`` (columns as vectors)
    filled with the point charges ``charges`` ``(n,)`` (e) at ``xyz`` ``(n, 3)``: one ``pw_rigid_cell_ewald`` job with one
    site of charge 1 at the centre, one direction, ``A = B = 0`` and maps -- the lowest pose energy of a voxel is the
    energy of its one pose.  ``cutoff`` is the real-space cutoff (at most the cell's smallest perpendicular width) and
    ``tolerance`` that of :func:`ewald_parameters`.  See :class:`EwaldPotential`."""
    from . import rigid_cell

    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(1, -1, 3)
    n = x.shape[1]
    probe = RigidGuest("unit charge", (0.0,), (0.0,), (0.0,), (1.0,))
    planned, ew = rigid_cell.plan_charged_field(x, np.zeros((1, n, 2)), lattice, probe, 298.0, spacing, cutoff, core2,
                                                np.array([[0.0, 0.0, 1.0]]), charges, tolerance)
    field = rigid_cell._field(planned, engine.context(device), spacing, None, ew=ew)
    return EwaldPotential(field.u_min_map[0], field.shape[0], field.origin[0], field.step[0], field.rotation[0],
                          float(ew["jobs"]["alpha"][0]), int(ew["jobs"]["n_k"][0]))
