"""Partial charges of a crystal cell on the GPU: periodic charge equilibration (``pw_charges_cell``,
include/pywindow_amd.h; the definition in pywindow_amd/csrc/pw_charges_cell.hpp).

:mod:`pywindow_amd.charges` equilibrates one molecule in vacuum.  A cage cut out of a crystal is not in vacuum: where
cages touch, the neighbours polarise it, and the charged fields of :mod:`pywindow_amd.rigid_cell` need the charges of the
cell itself.  Here the charges minimise ``sum chi_i q_i + 1/2 q^T A q`` at ``sum q = 0`` over the whole periodic cell,
``A = D + R + G``: the point-charge lattice sum is Ewald's (:func:`pywindow_amd.ewald_parameters` makes ``alpha`` and the
rows), and the Ohno-Klopman shielding of :mod:`pywindow_amd.charges` corrects it at short range, taken smoothly to zero
between ``shield[0]`` and ``shield[1]``.

The switch is a model parameter.  The shielding correction ``K / sqrt(r^2 + a^2) - K / r`` falls off as ``r^-3`` and is not
separable, so neutrality does not cancel it: cut at the Ewald cutoff the charges never settle, and Gaussian shielding is
indefinite with the bundled parameters.  With the switch the matrix is positive definite on the neutral subspace and the
charges no longer depend on the cutoff or the Ewald tolerance -- but they do depend on the switch: moving it by 2
Angstrom moves the largest charge of the CC3 cell by about 0.025 e.  A molecule wider than ``shield[0]`` therefore does
not reproduce :func:`pywindow_amd.equilibrate_charges` even in a huge cell.

What is left out: Slater integrals, the hydrogen hardness correction, any dependence on a guest; ``QEQ_PARAMETERS`` is
still unchecked against the paper (:mod:`pywindow_amd.charges`).  Charges in e, lengths in Angstrom, energies in eV.
The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .channels import triangular_lattice
from .charges import COULOMB_EV, _params
from .ewald import ewald_parameters
from .rigid import COULOMB

__all__ = ["CellCharges", "equilibrate_cell_charges", "equilibrate_cell_charges_batch", "plan_cell_charges"]

_SERIES = ("potential", "q_max", "q_min", "energy")


@dataclasses.dataclass(frozen=True)
class CellCharges:
    """The equilibrated charges of one cell (``charges`` ``(n,)``, ``raw`` a record) or of ``T`` frames (``charges``
    ``(T, n)``, ``raw`` ``(T,)``), in the caller's atom order.  ``raw`` holds ``pw_charges_cell``'s row
    (``_lib.CHARGES_CELL_OUT_DTYPE``); ``cutoff``, ``tolerance`` and ``shield`` are the call's; ``frames``: the trajectory's
    frame numbers, when the result comes from one."""

    charges: np.ndarray
    raw: np.ndarray
    cutoff: float = 12.0
    tolerance: float = 1e-6
    shield: tuple = (4.0, 6.0)
    tol: float = 1e-10
    frames: np.ndarray | None = None

    @property
    def potential(self):
        """The equalised electronegativity ``mu``, eV; it does not depend on the Ewald splitting."""
        return self.raw["mu"][()]

    @property
    def energy(self):
        """``chi.q / 2``, the electrostatic energy of the model at its minimum, eV per cell."""
        return self.raw["energy"][()]

    @property
    def q_min(self):
        return self.raw["q_min"][()]

    @property
    def q_max(self):
        return self.raw["q_max"][()]

    @property
    def iterations(self):
        return self.raw["iterations"][()]

    @property
    def flags(self):
        return self.raw["flags"][()]

    @property
    def converged(self):
        """The solver reached ``tol`` within ``max_iter`` and the charges are numbers."""
        return (np.asarray(self.raw["flags"]) == 0)[()]

    def series(self, name="potential"):
        """``(values, valid)`` of a quantity over the frames -- ``"potential"``, ``"q_max"``, ``"q_min"``, ``"energy"`` or
        ``("charge", atom)`` -- as the statistics of the package take them (:meth:`pywindow_amd.Charges.series`);
        ``valid`` is where the frame converged."""
        if isinstance(name, tuple) and len(name) == 2 and name[0] == "charge":
            q = np.atleast_2d(self.charges)
            atom = int(name[1])
            if not -q.shape[1] <= atom < q.shape[1]:
                raise IndexError(f"series: atom {atom} of {q.shape[1]}")
            v = q[:, atom]
        elif name in _SERIES:
            v = np.asarray(getattr(self, name), dtype=np.float64)
        else:
            raise KeyError(f'series: one of {_SERIES} or ("charge", atom)')
        values = np.atleast_1d(v).astype(np.float64)
        valid = np.atleast_1d(self.converged) & np.isfinite(values)
        return values, valid


def plan_cell_charges(xyz, elements_or_params, lattice, cutoff: float = 12.0, tolerance: float = 1e-6, shield=(4.0, 6.0),
                      tol: float = 1e-10, max_iter: int = 1000):
    """``(jobs, atoms, params, kvecs)``: what :func:`equilibrate_cell_charges_batch` hands to ``Context.charges_cell``.
    Job ``t`` is frame ``t``: its atoms rotated into the triangular cell of its lattice
    (:func:`pywindow_amd.channels.triangular_lattice`) and wrapped into it, the cell's edges, ``alpha`` and the rows of
    :func:`pywindow_amd.ewald_parameters` at ``cutoff`` and ``tolerance`` with the weights in eV."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    if n < 1:
        raise ValueError("xyz: at least one atom")
    p = _params(elements_or_params, n)
    cutoff = float(cutoff)
    on, off = (float(v) for v in shield)
    if not (math.isfinite(cutoff) and cutoff > 0.0):
        raise ValueError("cutoff: a positive number")
    if not (math.isfinite(on) and math.isfinite(off) and 0.0 <= on < off <= cutoff):
        raise ValueError("shield: (on, off) with 0 <= on < off <= cutoff")
    lat = np.asarray(lattice, dtype=np.float64)
    lat = np.broadcast_to(lat, (T, 3, 3)) if lat.ndim == 2 else lat
    if lat.shape != (T, 3, 3):
        raise ValueError("lattice: (3, 3) or one (3, 3) per frame")
    jobs = np.zeros(T, dtype=_lib.CHARGES_CELL_JOB_DTYPE)
    atoms, kvecs, made = np.zeros((T, n, 3)), [], {}
    for t in range(T):
        R, Q = triangular_lattice(lat[t])
        inv = np.linalg.inv(R)
        width = float((1.0 / np.sqrt((inv * inv).sum(axis=1))).min())   # (between the faces k: 1 / |row k of the inverse|)
        if cutoff > width:
            raise ValueError(f"equilibrate_cell_charges: a cutoff of {cutoff:.6g} is above the cell's smallest perpendicular "
                             f"width {width:.6g} (more than 27 images would matter): the largest cutoff that fits is {width:.6g}")
        frac = (x[t] @ Q) @ inv.T
        frac = frac - np.floor(frac)
        atoms[t] = frac @ R.T
        key = lat[t].tobytes()
        if key not in made:                                          # (the frames of a rigid cell share one set of rows)
            alpha, kv = ewald_parameters(lat[t], cutoff, tolerance)
            kv = kv.copy()
            kv[:, 3] *= COULOMB_EV / COULOMB
            made[key] = (alpha, sum(len(v) for v in kvecs), len(kv))
            kvecs.append(kv)
        jobs["alpha"][t], jobs["k_first"][t], jobs["n_k"][t] = made[key]
        jobs["edges"][t] = (R[0, 0], R[0, 1], R[1, 1], R[0, 2], R[1, 2], R[2, 2])
    jobs["xyz_first"] = jobs["charge_first"] = np.arange(T) * n
    jobs["n"] = n
    jobs["coulomb"] = COULOMB_EV
    jobs["cutoff2"], jobs["shield_on2"], jobs["shield_off2"] = cutoff * cutoff, on * on, off * off
    jobs["tol"], jobs["max_iter"] = float(tol), int(max_iter)
    jobs["out"] = np.arange(T)
    return jobs, atoms.reshape(-1, 3), p, np.concatenate(kvecs) if kvecs else np.zeros((0, 4))


def equilibrate_cell_charges_batch(xyz, elements_or_params, lattice, cutoff: float = 12.0, tolerance: float = 1e-6,
                                   shield=(4.0, 6.0), tol: float = 1e-10, max_iter: int = 1000, device=None, frames=None,
                                   kernel_ms=None) -> CellCharges:
    """:func:`equilibrate_cell_charges` for ``T`` frames of the same ``n`` atoms in ONE ``pw_charges_cell`` call: ``xyz``
    ``(T, n, 3)``, ``lattice`` ``(3, 3)`` or ``(T, 3, 3)``.  The frames share the parameters and the settings.
    ``kernel_ms``: a list that receives ``(count, rows, solver)``, the times of the kernels by HIP events."""
    jobs, atoms, p, kvecs = plan_cell_charges(xyz, elements_or_params, lattice, cutoff, tolerance, shield, tol, max_iter)
    T = len(jobs)
    q, out = engine.context(device).charges_cell(jobs, atoms, p, kvecs, kernel_ms=kernel_ms)
    return CellCharges(q.reshape(T, -1), out, float(cutoff), float(tolerance), tuple(float(v) for v in shield), float(tol),
                       None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def equilibrate_cell_charges(xyz, elements_or_params, lattice, cutoff: float = 12.0, tolerance: float = 1e-6, shield=(4.0, 6.0),
                             tol: float = 1e-10, max_iter: int = 1000, device=None) -> CellCharges:
    """The partial charges of the atoms ``xyz`` ``(n, 3)`` of the periodic cell ``lattice`` (columns as vectors) by charge
    equilibration over the whole crystal: see :class:`CellCharges` and the module's docstring.

    ``elements_or_params``: the atoms' element symbols (``QEQ_PARAMETERS``; an element without a row raises ``KeyError``),
    or ready rows ``(chi, J)`` ``(n, 2)`` in eV.  ``cutoff``: where the real-space sum is cut, at most the cell's smallest
    perpendicular width (above it the call raises and names the largest cutoff that fits); ``tolerance``: that of
    :func:`pywindow_amd.ewald_parameters`.  ``shield`` ``(on, off)``: the Ohno-Klopman shielding acts in full below ``on``
    and not at all above ``off``, ``0 <= on < off <= cutoff`` -- a model parameter, see the module's docstring.  The solver
    stops at ``rz <= tol^2 rz0`` (``tol`` in ``1e-14 .. 1e-2``) or after ``max_iter`` steps (``1 .. 100000``): then
    ``converged`` is false and the charges are those of the last step.  A matrix that is not positive definite on the
    neutral subspace gives NaN charges and a flag, not an error.  The atoms may lie anywhere: they are wrapped into the
    cell, and the charges come back in the caller's order.  ``xyz`` ``(T, n, 3)`` is
    :func:`equilibrate_cell_charges_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit
    host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return equilibrate_cell_charges_batch(x, elements_or_params, lattice, cutoff, tolerance, shield, tol, max_iter, device)
    many = equilibrate_cell_charges_batch(x.reshape(1, -1, 3), elements_or_params, lattice, cutoff, tolerance, shield, tol,
                                          max_iter, device)
    return dataclasses.replace(many, charges=many.charges[0], raw=many.raw[0], frames=None)
