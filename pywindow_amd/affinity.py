"""Guest affinity of a cage on the GPU: the Lennard-Jones energy map of its cavity for a one-site guest and the Boltzmann
sums over it (``pw_affinity``, include/pywindow_amd.h).

``pw_cavity`` gives the void and ``pw_pore_sizes`` the room a hard sphere can fill; this module answers how strongly
the cage holds a given guest.  Every voxel of a region -- the mask of a :class:`pywindow_amd.Cavity`, or a whole grid
-- is a test position of the guest; its energy ``U`` is the sum of 12-6 pair terms with every atom of the cage, and per
temperature the kernel returns ``Z = sum exp(-U / RT)`` and ``E = sum U exp(-U / RT)`` in a defined order of additions,
so the device and the explicit host path (``device=-1``) return the same bytes.  From them:

* ``boltzmann_volume = Z h^3``: the Boltzmann-weighted volume of the cavity (Widom insertion on a grid) -- the helium
  void volume for He, and up to ``1 / RT`` the Henry coefficient of the cage for any guest;
* ``mean_energy = E / Z``, ``heat = RT - mean_energy`` (the isosteric heat of adsorption at infinite dilution),
  ``min_energy`` and ``min_position`` (the binding site on the grid), a ``histogram`` of the energies;
* ``selectivity``: the ratio of two guests' Henry coefficients.

Parameters.  The framework atoms are UFF (A. K. Rappe, C. J. Casewit, K. S. Colwell, W. A. Goddard III, W. M. Skiff,
J. Am. Chem. Soc. 114, 10024 (1992)): the table's distance ``x`` (Angstrom) and well depth ``D`` (kcal/mol), as
``sigma = x / 2^(1/6)`` and ``eps = 4.184 D`` kJ/mol.  The guests are one-site Lennard-Jones models, ``sigma`` in
Angstrom and ``eps / k_B`` in K, the values in common use in adsorption simulation: He as in O. Talu and A. L. Myers,
AIChE J. 47, 1160 (2001), the helium void volume; Ar, Kr and Xe as tabulated by J. O. Hirschfelder, C. F. Curtiss and
R. B. Bird, Molecular Theory of Gases and Liquids (Wiley, 1954); CH4 the united atom of M. G. Martin and J. I. Siepmann,
J. Phys. Chem. B 102, 2569 (1998); H2 from V. Buch, J. Chem. Phys. 100, 7610 (1994).  Unlike pairs by
Lorentz-Berthelot mixing.  Energies are kJ/mol, lengths Angstrom.  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine

__all__ = ["Affinity", "GUESTS", "UFF", "guest_affinity", "guest_affinity_batch", "lj_coefficients"]

#: the gas constant, kJ / (mol K)
R = 8.31446261815324e-3
#: molecules per (kJ/mol) / (bar Angstrom^3): N_A * 1e-25 J / (bar A^3) / (1e3 J/kJ)
_PER_BAR = 6.02214076e23 * 1e-28

#: UFF: element -> (x / Angstrom, D / (kcal/mol))
UFF = {
    "H": (2.886, 0.044), "B": (4.083, 0.180), "C": (3.851, 0.105), "N": (3.660, 0.069), "O": (3.500, 0.060),
    "F": (3.364, 0.050), "SI": (4.295, 0.402), "P": (4.147, 0.305), "S": (4.035, 0.274), "CL": (3.947, 0.227),
    "BR": (4.189, 0.251), "I": (4.500, 0.339),
}
#: one-site guests: name -> (sigma / Angstrom, (eps / k_B) / K)
GUESTS = {
    "He": (2.64, 10.9), "H2": (2.96, 34.2), "Ar": (3.405, 119.8), "Kr": (3.636, 166.4), "Xe": (4.10, 221.0),
    "CH4": (3.73, 148.0),
}

_SERIES = ("boltzmann_volume", "henry", "mean_energy", "heat", "min_energy", "n_voxels", "n_blocked")


def _guest(guest):
    """``(sigma, eps in kJ/mol)`` of a guest's name or of a ``(sigma, eps_kJ_per_mol)`` pair."""
    if isinstance(guest, str):
        sigma, eps_k = GUESTS[guest]
        return float(sigma), R * eps_k
    sigma, eps = guest
    return float(sigma), float(eps)


def lj_coefficients(elements, guest) -> np.ndarray:
    """Rows ``(A, B) = (4 eps sigma^12, 4 eps sigma^6)`` of the 12-6 term between every framework atom (UFF) and the
    guest (a name of ``GUESTS`` or a ``(sigma, eps_kJ_per_mol)`` pair), Lorentz-Berthelot mixed:
    ``sigma = (sigma_i + sigma_g) / 2`` and ``eps = sqrt(eps_i eps_g)``, kJ/mol and Angstrom.  An element without UFF
    parameters here raises ``KeyError``, as the van der Waals table does."""
    sigma_g, eps_g = _guest(guest)
    rows = np.array([UFF[str(e).upper()] for e in elements], dtype=np.float64).reshape(-1, 2)
    sigma = (rows[:, 0] / 2.0 ** (1.0 / 6.0) + sigma_g) / 2.0
    eps = np.sqrt(4.184 * rows[:, 1] * eps_g)
    s6 = sigma ** 6
    return np.stack([4.0 * eps * s6 * s6, 4.0 * eps * s6], axis=1)


@dataclasses.dataclass(frozen=True)
class Affinity:
    """The affinity of one frame (``raw`` a record, ``levels`` ``(L,)``) or of ``T`` frames (``raw`` ``(T,)``,
    ``levels`` ``(T, L)``) at the ``L`` ``temperatures``.  ``raw`` holds ``pw_affinity``'s row
    (``_lib.AFFINITY_OUT_DTYPE``), ``levels`` its ``(Z, E)`` rows, ``counts`` the histogram's ``E`` cumulative counts
    below ``edges``; ``energies`` (when asked for) the energy of every voxel of the region in rank order, ``+inf`` where
    an atom's core blocks it (a list of arrays for many frames).  ``closed``: the cavity's (``None`` for a plain
    grid)."""

    raw: np.ndarray
    levels: np.ndarray
    counts: np.ndarray
    temperatures: np.ndarray
    edges: np.ndarray
    origin: np.ndarray
    shape: np.ndarray
    spacing: float
    guest: object = None
    closed: object = None
    energies: object = None
    frames: np.ndarray | None = None

    @property
    def n_voxels(self):
        return self.raw["n_voxels"][()]

    @property
    def n_blocked(self):
        return self.raw["n_blocked"][()]

    @property
    def clamped(self):
        """An exponent above 700 was taken as 700: the sums of that frame are not to be used."""
        return (self.raw["flags"] & _lib.AFF_CLAMPED) != 0

    @property
    def boltzmann_volume(self):
        """``Z h^3`` in cubic Angstrom, per temperature."""
        return self.levels["z"] * (self.spacing * self.spacing * self.spacing)

    @property
    def henry(self):
        """The Henry coefficient of the cage, ``boltzmann_volume / (k_B T)``, in molecules per cage and bar."""
        return self.boltzmann_volume * (_PER_BAR / (R * self.temperatures))

    @property
    def mean_energy(self):
        """``E / Z``, the Boltzmann average of the guest's energy in kJ/mol; NaN where ``Z`` is 0."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.levels["e"] / self.levels["z"]

    @property
    def heat(self):
        """The heat of adsorption at infinite dilution, ``R T - mean_energy``, kJ/mol."""
        return R * self.temperatures - self.mean_energy

    @property
    def min_energy(self):
        """The lowest energy of a voxel that no core blocks, kJ/mol; ``+inf`` when every voxel is blocked."""
        return self.raw["u_min"][()]

    @property
    def min_position(self):
        """The centre of the voxel of ``min_energy``; NaN without one."""
        v = np.asarray(self.raw["min_voxel"], dtype=np.float64)
        return np.where(v < 0.0, np.nan, self.origin + self.spacing * v)

    @property
    def histogram(self):
        """Voxels per bin ``[edges[k], edges[k + 1])``, from the cumulative counts."""
        return np.diff(self.counts, axis=-1)

    def selectivity(self, other: "Affinity"):
        """The ratio of this guest's Henry coefficient to ``other``'s (same frames, region and temperatures)."""
        if not np.array_equal(self.temperatures, other.temperatures):
            raise ValueError("selectivity: the two results are for different temperatures")
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.boltzmann_volume / other.boltzmann_volume

    def series(self, name: str = "boltzmann_volume", level: int = 0):
        """``(values, valid)`` of a quantity over the frames at temperature ``level`` -- float64 values; ``valid``: the
        cavity is closed (always, for a plain grid), the frame was not clamped and the value is finite -- ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
        :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = np.asarray(getattr(self, name), dtype=np.float64)
        if name in ("boltzmann_volume", "henry", "mean_energy", "heat"):
            v = v[..., level]
        values = np.atleast_1d(v).copy()
        valid = np.isfinite(values) & ~np.atleast_1d(self.clamped)
        if self.closed is not None:
            valid &= np.atleast_1d(np.asarray(self.closed, dtype=bool))
        return values, valid


def guest_affinity_batch(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, edges=None,
                         energies: bool = False, core2: float = 0.25, cutoff2: float = 0.0, device=None, frames=None,
                         kernel_ms=None) -> Affinity:
    """:func:`guest_affinity` for ``T`` frames of the same ``n`` atoms in ONE ``pw_affinity`` call: ``xyz``
    ``(T, n, 3)``; ``cavity`` the :class:`pywindow_amd.Cavity` of the same ``T`` frames made with ``mask=True``, or
    ``grid = (origin (3,) or (T, 3), spacing, (nx, ny, nz))`` for every voxel of a box.  The frames share the atoms'
    coefficients, the temperatures and the edges.  The fields of the result are arrays over the frames.  ``kernel_ms``:
    a list that receives the time of the device work by HIP events (the library's measurement entry)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    coef = np.asarray(elements_or_coef)
    if coef.dtype.kind in "fiu" and coef.ndim == 2 and coef.shape[1] == 2:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
    else:
        coef = lj_coefficients(list(elements_or_coef), guest)
    if len(coef) != n:
        raise ValueError("elements_or_coef: one element or one row (A, B) per atom")
    temps = np.atleast_1d(np.asarray(temperatures, dtype=np.float64))
    if temps.ndim != 1 or not 1 <= len(temps) <= _lib.AFF_MAX_LEVELS or not (np.isfinite(temps) & (temps > 0.0)).all():
        raise ValueError(f"temperatures: 1 .. {_lib.AFF_MAX_LEVELS} positive numbers")
    e = np.zeros(0) if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if (cavity is None) == (grid is None):
        raise ValueError("one of cavity and grid")
    jobs = np.zeros(T, dtype=_lib.AFFINITY_JOB_DTYPE)
    jobs["atom_first"] = np.arange(T) * n
    jobs["n"] = n
    jobs["n_betas"] = len(temps)
    jobs["n_edges"] = len(e)
    jobs["level_first"] = np.arange(T) * len(temps)
    jobs["hist_first"] = np.arange(T) * len(e)
    jobs["out"] = np.arange(T)
    jobs["core2"], jobs["cutoff2"] = float(core2), float(cutoff2)
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
    jobs["energy_first"] = -1
    maps = None
    if energies:
        jobs["energy_first"] = np.concatenate([[0], np.cumsum(voxels)[:-1]]) if T else 0
        maps = np.zeros(int(voxels.sum()))
    out, levels, hist, maps = engine.context(device).affinity(jobs, x.reshape(-1, 3), coef, 1.0 / (R * temps), words, e,
                                                              energies=maps, kernel_ms=kernel_ms)
    if energies:
        maps = [maps[int(f):int(f) + int(v)] for f, v in zip(jobs["energy_first"], voxels)]
    return Affinity(out, levels.reshape(T, len(temps)), hist.reshape(T, len(e)), temps, e, jobs["origin"].copy(),
                    np.array(shape, dtype=np.int64), spacing, guest, closed, maps if energies else None,
                    None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def guest_affinity(xyz, elements_or_coef, guest, temperatures, cavity=None, grid=None, edges=None, energies: bool = False,
                   core2: float = 0.25, cutoff2: float = 0.0, device=None) -> Affinity:
    """The affinity of the cage ``xyz`` ``(n, 3)`` for a guest at the ``temperatures`` (K, at most 8): see
    :class:`Affinity`.  ``elements_or_coef``: the atoms' element symbols (UFF with ``guest`` a name of ``GUESTS`` or a
    ``(sigma, eps_kJ_per_mol)`` pair, :func:`lj_coefficients`), or ready rows ``(A, B)`` ``(n, 2)``.  The region is the
    mask of ``cavity`` (a :class:`pywindow_amd.Cavity` made with ``mask=True``) or every voxel of
    ``grid = (origin, spacing, (nx, ny, nz))``.  A voxel within ``sqrt(core2)`` of an atom is blocked: it adds nothing.
    ``cutoff2``: the square of a cutoff, ``0``: none.  ``edges``: at most 16 ascending energies for the histogram.
    ``energies=True`` keeps the energy of every voxel.  ``xyz`` ``(T, n, 3)`` is :func:`guest_affinity_batch`.
    ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return guest_affinity_batch(x, elements_or_coef, guest, temperatures, cavity, grid, edges, energies, core2, cutoff2, device)
    many = guest_affinity_batch(x.reshape(1, -1, 3), elements_or_coef, guest, temperatures, cavity, grid, edges, energies,
                                core2, cutoff2, device)
    return Affinity(many.raw[0], many.levels[0], many.counts[0], many.temperatures, many.edges, many.origin[0], many.shape[0],
                    many.spacing, many.guest, None if many.closed is None else many.closed[0],
                    None if many.energies is None else many.energies[0], None)
