"""Partial charges of a cage on the GPU: charge equilibration (``pw_charges``, include/pywindow_amd.h).

:mod:`pywindow_amd.rigid` needs the framework's partial charges before the quadrupole of CO2 or N2 does anything, and
the bundled cage model (UFF) carries none.  Here the library makes them itself, frame by frame, so that a breathing
cage gets the charges of each of its shapes: the charges minimise ``sum chi_i q_i + 1/2 q^T A q`` at a fixed total
charge (QEq, A. K. Rappe and W. A. Goddard III, J. Phys. Chem. 95, 3358 (1991)), with ``A_ii = J_i`` and
``A_ij = K / sqrt(r_ij^2 + a^2)``, ``a = 2 K / (J_i + J_j)``.  That is one symmetric positive-definite ``n x n`` problem a
frame, solved by Jacobi-preconditioned conjugate gradients in a defined order of operations
(pywindow_amd/csrc/pw_charges.hpp), so the device and the explicit host path (``device=-1``) return the same bytes.

What is left out.  The Slater overlap integrals of the paper are replaced by the Ohno-Klopman shielding above, which
has the same limits (``K / r`` far away, ``(J_i + J_j) / 2`` at ``r = 0``).  There is no charge-dependent hardness for
hydrogen, so H is somewhat over-polarised.  There is no Ewald sum: an isolated molecule only.  The charges do not depend
on a guest.

Parameters.  ``QEQ_PARAMETERS`` holds the electronegativity ``chi`` and the hardness ``J`` of eleven elements in eV.
They were written down from memory of Rappe and Goddard's table and have NOT been checked against the paper line by
line: they sit in that one table, so a correction is one line, and no test asserts a physical value.  Charges are in e,
lengths in Angstrom, energies in eV.  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine

__all__ = ["COULOMB_EV", "QEQ_PARAMETERS", "Charges", "equilibrate_charges", "equilibrate_charges_batch", "qeq_parameters"]

#: e^2 / (4 pi eps_0) in eV Angstrom: ``pywindow_amd.rigid.COULOMB`` (kJ Angstrom / mol) over eV in kJ/mol
COULOMB_EV = 1389.35457644382 / 96.4853321233

#: element -> (chi, J) in eV (see the module's docstring: not checked against the paper)
QEQ_PARAMETERS = {
    "H": (4.528, 13.8904),
    "C": (5.343, 10.126),
    "N": (6.899, 11.760),
    "O": (8.741, 13.364),
    "F": (10.874, 14.948),
    "SI": (4.168, 6.974),
    "P": (5.463, 8.000),
    "S": (6.928, 8.972),
    "CL": (8.564, 9.892),
    "BR": (7.790, 8.850),
    "I": (6.822, 7.524),
}

_SERIES = ("dipole_norm", "potential", "q_max", "q_min", "energy")


def qeq_parameters(elements) -> np.ndarray:
    """Rows ``(chi, J)`` ``(n, 2)`` in eV of the element symbols (upper-cased as everywhere in the package); an
    element without a row raises ``KeyError`` naming it."""
    rows = []
    for e in elements:
        key = str(e).upper()
        if key not in QEQ_PARAMETERS:
            raise KeyError(f"QEQ_PARAMETERS has no row for element {str(e)!r}")
        rows.append(QEQ_PARAMETERS[key])
    return np.array(rows, dtype=np.float64).reshape(-1, 2)


@dataclasses.dataclass(frozen=True)
class Charges:
    """The equilibrated charges of one frame (``charges`` ``(n,)``, ``raw`` a record) or of ``F`` frames (``charges``
    ``(F, n)``, ``raw`` ``(F,)``).  ``raw`` holds ``pw_charges``' row (``_lib.CHARGES_OUT_DTYPE``); ``frames``: the
    trajectory's frame numbers, when the result comes from one."""

    charges: np.ndarray
    raw: np.ndarray
    total_charge: float = 0.0
    tol: float = 1e-10
    frames: np.ndarray | None = None

    @property
    def potential(self):
        """The equalised electronegativity ``mu`` (the chemical potential of the electrons with its sign changed), eV."""
        return self.raw["mu"][()]

    @property
    def energy(self):
        """``(chi.q + mu Q) / 2``, the electrostatic energy of the model at its minimum, eV."""
        return self.raw["energy"][()]

    @property
    def dipole(self):
        """``sum q_i x_i`` in e Angstrom (for a charged molecule it depends on the origin)."""
        return self.raw["dipole"][()]

    @property
    def dipole_norm(self):
        d = np.asarray(self.raw["dipole"])
        return np.sqrt((d * d).sum(axis=-1))[()]

    @property
    def q_min(self):
        return self.raw["q_min"][()]

    @property
    def q_max(self):
        return self.raw["q_max"][()]

    @property
    def iterations(self):
        """The steps of the two systems ``A s = -chi`` and ``A t = 1``: ``(2,)`` or ``(F, 2)``."""
        return self.raw["iterations"][()]

    @property
    def flags(self):
        return self.raw["flags"][()]

    @property
    def converged(self):
        """Both systems reached ``tol`` within ``max_iter`` and the charges are numbers."""
        return (np.asarray(self.raw["flags"]) == 0)[()]

    def series(self, name="dipole_norm"):
        """``(values, valid)`` of a quantity over the frames -- ``"dipole_norm"``, ``"potential"``, ``"q_max"``,
        ``"q_min"``, ``"energy"`` or ``("charge", atom)`` -- as :func:`pywindow_amd.time_correlation`,
        :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics`
        and :func:`pywindow_amd.transition_counts` take them; ``valid`` is where the job converged."""
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


def _params(elements_or_params, n: int) -> np.ndarray:
    p = np.asarray(elements_or_params)
    if p.dtype.kind in "fiu" and p.ndim == 2 and p.shape[1] == 2:
        p = np.ascontiguousarray(p, dtype=np.float64)
    else:
        p = qeq_parameters(list(elements_or_params))
    if len(p) != n:
        raise ValueError("elements_or_params: one element per atom, or rows (chi, J) (n, 2)")
    return p


def equilibrate_charges_batch(xyz, elements_or_params, total_charge: float = 0.0, tol: float = 1e-10, max_iter: int = 1000,
                              device=None, frames=None, kernel_ms=None) -> Charges:
    """:func:`equilibrate_charges` for ``F`` frames of the same ``n`` atoms in ONE ``pw_charges`` call: ``xyz``
    ``(F, n, 3)``.  The frames share the parameters, the total charge, ``tol`` and ``max_iter``.  ``kernel_ms``: a list
    that receives the time of the kernels by HIP events."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (F, n, 3)")
    F, n = x.shape[:2]
    p = _params(elements_or_params, n)
    jobs = np.zeros(F, dtype=_lib.CHARGES_JOB_DTYPE)
    jobs["xyz_first"] = jobs["charge_first"] = np.arange(F) * n
    jobs["n"] = n
    jobs["total_charge"], jobs["coulomb"] = float(total_charge), COULOMB_EV
    jobs["tol"], jobs["max_iter"] = float(tol), int(max_iter)
    jobs["out"] = np.arange(F)
    q, out = engine.context(device).charges(jobs, x.reshape(-1, 3), p, kernel_ms=kernel_ms)
    return Charges(q.reshape(F, n), out, float(total_charge), float(tol),
                   None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def equilibrate_charges(xyz, elements_or_params, total_charge: float = 0.0, tol: float = 1e-10, max_iter: int = 1000,
                        device=None) -> Charges:
    """The partial charges of the isolated molecule ``xyz`` ``(n, 3)`` by charge equilibration: see :class:`Charges`.
    ``elements_or_params``: the atoms' element symbols (``QEQ_PARAMETERS``; an element without a row raises
    ``KeyError``), or ready rows ``(chi, J)`` ``(n, 2)`` in eV.  ``total_charge``: the sum of the charges, e.  The two
    linear systems stop at a relative residual of ``tol`` (``1e-14 .. 1e-2``) or after ``max_iter`` steps
    (``1 .. 100000``): then ``converged`` is false and the charges are those of the last step.  A matrix that is not
    positive definite gives NaN charges and a flag, not an error.  ``xyz`` ``(F, n, 3)`` is
    :func:`equilibrate_charges_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host
    path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return equilibrate_charges_batch(x, elements_or_params, total_charge, tol, max_iter, device)
    many = equilibrate_charges_batch(x.reshape(1, -1, 3), elements_or_params, total_charge, tol, max_iter, device)
    return Charges(many.charges[0], many.raw[0], many.total_charge, many.tol, None)
