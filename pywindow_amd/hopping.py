"""Guest hopping rates on the GPU: the free-energy profile of a guest through every window of a cage (``pw_hop``,
include/pywindow_amd.h) and the transition-state-theory rate built on it.

``pw_passage`` gives the energy of the saddle a guest crosses; a rate needs more: how wide the saddle is and how roomy
the well behind it.  Transition-state theory says

    ``k = sqrt(k_B T / 2 pi m) * A(T) / V_well(T)``

with ``A`` the Boltzmann-weighted area of the dividing surface in the window and ``V_well`` the Boltzmann-weighted
volume behind it.  For every window the cage is turned so that the line from the pore centre to the window is ``z``
(:func:`window_frame`), a lattice of ``spacing`` is laid across and slabs along it, and ``pw_hop`` returns for every
slab the 2-D component of voxels round the axis whose Lennard-Jones energy is at most ``cap`` -- the other windows'
planes held shut -- with its Boltzmann sum ``Z``.  ``h^2 Z`` is a slab's weighted area, ``-RT ln(h^2 Z)`` the free
energy profile along the axis; the dividing surface is the slab of the smallest ``Z`` beyond the well, and the well the
slabs before it (see :class:`Hopping` for the one written rule).  ``D = k lambda^2 / 6`` follows.

Known limit: a slab's component is found in its own plane.  A 2-D section of a cavity that is not convex can miss lobes
that join the rest only through other slabs, so ``well_volume`` can fall short of ``pw_affinity``'s
``boltzmann_volume`` of the same region (for CC3 the two agree to a percent or so: DESIGN.md, section 7p).

Everything the kernel returns is defined to the byte, so the device and the explicit host path (``device=-1``) agree
exactly; what is derived from it here is plain numpy, the same on both.  Parameters and units as in
:mod:`pywindow_amd.affinity` (UFF atoms, one-site guests, Lorentz-Berthelot mixing, kJ/mol, Angstrom, K).  The reference
has no counterpart.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .affinity import GUESTS, R, lj_coefficients

__all__ = ["Hopping", "guest_hopping", "guest_hopping_batch", "window_frame", "hopping_profile", "GUEST_MASSES"]

#: molar masses of the one-site guests of ``pywindow_amd.affinity.GUESTS``, g/mol
GUEST_MASSES = {"He": 4.002602, "H2": 2.01588, "Ar": 39.948, "Kr": 83.798, "Xe": 131.293, "CH4": 16.04246}
assert set(GUEST_MASSES) == set(GUESTS)

_KB = 1.380649e-23            # J/K
_AMU = 1.66053906660e-27      # kg
_SERIES = ("rate", "free_barrier", "escape_rate", "area", "well_volume")


def window_frame(centre, window_centre) -> np.ndarray:
    """The rows ``(u, v, n)`` of the rotation into a window's own frame: ``n = (w - c) / |w - c|``, ``a`` the unit axis
    of the smallest ``|n|`` component (the lowest index on a tie), ``u = n x a`` normalised, ``v = n x u``.  Rotated
    coordinates are ``(x - c) @ frame.T``: the pore centre goes to the origin and the window to ``(0, 0, |w - c|)``.
    Plain numpy, shared by the device and the host path."""
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    w = np.asarray(window_centre, dtype=np.float64).reshape(3)
    v = w - c
    d = math.sqrt(float((v * v).sum()))
    if not d > 0.0:
        raise ValueError("window_frame: the window centre coincides with the centre")
    n = v / d
    a = np.zeros(3)
    a[int(np.argmin(np.abs(n)))] = 1.0
    u = np.cross(n, a)
    u = u / math.sqrt(float((u * u).sum()))
    return np.stack([u, np.cross(n, u), n])


def hopping_profile(Z, n, n_face, q, centre_slab: int) -> dict:
    """The one written rule that turns a window's slabs into a well and a dividing surface, on plain sequences: ``Z``
    the slabs' Boltzmann sums, ``n`` and ``n_face`` their counts, ``q`` their offsets from the window plane,
    ``centre_slab`` the slab nearest the pore centre.

    A slab is closed when ``n > 0`` and ``n_face == 0``.  The run is the maximal run of consecutive closed slabs that
    holds ``centre_slab``; if that slab is not closed the window is invalid (``seed_closed``).  ``l_w`` is the slab of
    the largest ``Z`` in the run with ``q <= 0``, ``l_t`` the slab of the smallest ``Z`` from ``l_w`` to the end of the
    run, both the lowest index on a tie.  ``free_exit``: ``l_t`` is the run's last slab.  ``well_truncated``: the run
    starts at slab 0.  ``z_area = Z[l_t]`` and ``z_well`` = the sum of ``Z`` over the run's slabs before ``l_t``."""
    Z = [float(v) for v in Z]
    closed = [int(a) > 0 and int(b) == 0 for a, b in zip(n, n_face)]
    out = {"seed_closed": True, "l_w": -1, "l_t": -1, "first": -1, "last": -1, "free_exit": False, "well_truncated": False,
           "z_area": math.nan, "z_well": math.nan}
    c = int(centre_slab)
    if not (0 <= c < len(Z)) or not closed[c]:
        return out
    first = last = c
    while first > 0 and closed[first - 1]:
        first -= 1
    while last + 1 < len(Z) and closed[last + 1]:
        last += 1
    inside = [l for l in range(first, last + 1) if float(q[l]) <= 0.0]
    if not inside:
        return out
    l_w = inside[0]
    for l in inside:
        if Z[l] > Z[l_w]:
            l_w = l
    l_t = l_w
    for l in range(l_w, last + 1):
        if Z[l] < Z[l_t]:
            l_t = l
    z_well = 0.0
    for l in range(first, l_t):
        z_well += Z[l]
    out.update(seed_closed=False, l_w=l_w, l_t=l_t, first=first, last=last, free_exit=l_t == last,
               well_truncated=first == 0, z_area=Z[l_t], z_well=z_well)
    return out


@dataclasses.dataclass(frozen=True)
class Hopping:
    """The hopping profile of ``T`` frames with up to ``W`` windows, ``S`` slabs and ``L`` temperatures
    (:func:`guest_hopping`: one frame -- ``single`` -- whose properties and derived quantities come without the first
    axis; the raw fields below keep it).

    Raw, padded as :class:`pywindow_amd.Passage` pads: ``slabs`` ``(T, W, S)`` of ``_lib.HOP_SLAB_DTYPE`` (padding:
    ``n = n_face = -1``, NaN ``u_min``), ``Z`` and ``E`` ``(T, W, S, L)`` (padding NaN), ``flags`` ``(T, W)``,
    ``n_windows`` ``(T,)``, ``n_slabs`` ``(T, W)`` and ``distance`` ``(T, W)``, the pore centre to the window.  Slab
    ``l`` of a window lies at ``z = -back + l * spacing`` on the window's axis.

    Derived, plain numpy on the defined result under the rule of :func:`hopping_profile`: ``l_w``, ``l_t``,
    ``seed_closed``, ``free_exit``, ``well_truncated``, ``area = h^2 Z[l_t]``, ``well_volume = h^3 sum Z`` over the
    run's slabs before ``l_t``, ``rate = sqrt(k_B T / 2 pi m) area / well_volume`` per second,
    ``free_barrier = F[l_t] - F[l_w]`` -- each ``(T, W, L)`` -- and ``valid``: the window has a closed centre slab and a
    well of positive volume."""

    slabs: np.ndarray
    Z: np.ndarray
    E: np.ndarray
    flags: np.ndarray
    n_windows: np.ndarray
    n_slabs: np.ndarray
    distance: np.ndarray
    spacing: float
    back: float
    temperatures: np.ndarray
    mass: float
    guest: object = None
    frames: np.ndarray | None = None
    single: bool = False

    def _view(self, a):
        return a[0] if self.single else a

    @property
    def q(self):
        """The offset of every slab from its window's plane along the axis, Angstrom: negative inside the cage."""
        S = self.slabs.shape[-1]
        return self._view((-self.back + self.spacing * np.arange(S))[None, None, :] - self.distance[:, :, None])

    @property
    def n(self):
        return self._view(self.slabs["n"])

    @property
    def lateral_open(self):
        """The slab's component reaches a lateral face of the lattice: its area depends on the lattice."""
        return self._view(self.slabs["n_face"] > 0)

    @property
    def clamped(self):
        return self._view((self.flags & _lib.HOP_CLAMPED) != 0)

    @property
    def free_energy(self):
        """``-RT ln(Z h^2)`` of every slab at every temperature, kJ/mol; ``+inf`` for an empty slab."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._view(-(R * self.temperatures) * np.log(self.Z * (self.spacing * self.spacing)))

    def _derived(self):
        cached = self.__dict__.get("_cache")
        if cached is not None:
            return cached
        T, W, S = self.slabs.shape
        L = len(self.temperatures)
        ints = {k: np.full((T, W, L), -1, dtype=np.int64) for k in ("l_w", "l_t")}
        flags = {k: np.zeros((T, W, L), dtype=bool) for k in ("seed_closed", "free_exit", "well_truncated")}
        z_area, z_well = np.full((T, W, L), np.nan), np.full((T, W, L), np.nan)
        centre = int(round(self.back / self.spacing))
        q = (-self.back + self.spacing * np.arange(S))[None, None, :] - self.distance[:, :, None]
        for t in range(T):
            for w in range(int(self.n_windows[t])):
                s = int(self.n_slabs[t, w])
                for b in range(L):
                    p = hopping_profile(self.Z[t, w, :s, b], self.slabs["n"][t, w, :s], self.slabs["n_face"][t, w, :s],
                                        q[t, w, :s], centre)
                    for k in ints:
                        ints[k][t, w, b] = p[k]
                    for k in flags:
                        flags[k][t, w, b] = p[k]
                    z_area[t, w, b], z_well[t, w, b] = p["z_area"], p["z_well"]
        h = self.spacing
        out = dict(ints)
        out.update(flags)
        out["area"] = z_area * (h * h)
        out["well_volume"] = z_well * (h * h * h)
        out["valid"] = ~flags["seed_closed"] & (ints["l_t"] >= 0) & (out["well_volume"] > 0.0)
        speed = np.sqrt(_KB * self.temperatures / (2.0 * math.pi * self.mass * _AMU)) * 1e10      # Angstrom / s
        with np.errstate(divide="ignore", invalid="ignore"):
            out["rate"] = np.where(out["valid"], speed * out["area"] / out["well_volume"], np.nan)
            zw = np.take_along_axis(np.moveaxis(self.Z, 2, 3), np.maximum(ints["l_w"], 0)[..., None], axis=3)[..., 0]
            out["free_barrier"] = np.where(ints["l_t"] >= 0, -(R * self.temperatures) * np.log(z_area / zw), np.nan)
        object.__setattr__(self, "_cache", out)
        return out

    def __getattr__(self, name):
        if name in ("l_w", "l_t", "seed_closed", "free_exit", "well_truncated", "area", "well_volume", "valid", "rate",
                    "free_barrier"):
            return self._view(self._derived()[name])
        raise AttributeError(name)

    @property
    def padding(self):
        return self._view(np.arange(self.slabs.shape[1])[None, :] >= self.n_windows[:, None])

    @property
    def escape_rate(self):
        """The sum of ``rate`` over the frame's valid windows, per second: ``(T, L)``."""
        d = self._derived()
        return self._view(np.where(d["valid"], d["rate"], 0.0).sum(axis=1))

    def diffusion(self, jump_length: float):
        """``escape_rate * jump_length^2 / 6``: the diffusion coefficient of a guest that hops ``jump_length`` Angstrom
        between cages, Angstrom^2 / s."""
        return self.escape_rate * (float(jump_length) ** 2 / 6.0)

    def mean_rate(self):
        """The ensemble transition-state-theory rate of every window over the frames: ``sqrt(k_B T / 2 pi m)`` times the
        sum of ``area`` over the sum of ``well_volume`` of the valid frames, ``(W, L)``, per second; NaN without one."""
        d = self._derived()
        a = np.where(d["valid"], d["area"], 0.0).sum(axis=0)
        v = np.where(d["valid"], d["well_volume"], 0.0).sum(axis=0)
        speed = np.sqrt(_KB * self.temperatures / (2.0 * math.pi * self.mass * _AMU)) * 1e10
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(v > 0.0, speed * a / v, np.nan)

    def series(self, name: str = "rate", window=None, level: int = 0):
        """``(values, valid)`` of a quantity over the frames at temperature ``level`` -- ``window``: a column, or ``None``
        for each frame's valid window of the largest rate (``escape_rate`` has no window).  Ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
        :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        d = self._derived()
        ok = d["valid"][:, :, level]
        if name == "escape_rate":
            return np.where(ok, d["rate"][:, :, level], 0.0).sum(axis=1), ok.any(axis=1)
        rows = np.arange(len(ok))
        if window is None:
            column = np.where(ok, d["rate"][:, :, level], -np.inf).argmax(axis=1)
        else:
            column = np.full(len(ok), int(window))
        v = np.asarray(d[name][:, :, level], dtype=np.float64)[rows, column]
        return v.copy(), (ok[rows, column] & np.isfinite(v)).copy()


def _lattice(half_width: float, spacing: float) -> int:
    k = int(round(half_width / spacing))
    g = 2 * k + 1
    if g > 64:
        raise ValueError(f"guest_hopping: {g} voxels across at spacing {spacing} (at most 64): use a spacing of at least "
                         f"{2.0 * half_width / 63.0:.3f}")
    return g


def hop_jobs(x, c, wins, g: int, spacing: float, back: float, ahead: float, L: int, cap: float, core2: float, cutoff2: float):
    """The records of one ``pw_hop`` call for the frames ``x`` ``(T, n, 3)`` with the centres ``c`` ``(T, 3)`` and the
    window centres ``wins`` (``T`` arrays ``(W_t, 3)``), a job a (frame, window) in frame order: ``(jobs, atoms (J, n, 3)
    rotated into each window's frame, planes (a list of (m, 4) arrays), distance (T, W), n_slabs (T, W), [(t, w)])``.
    Job ``k`` reads the atoms ``k * n ..``, ``L`` betas from 0 and writes its slabs and sums one after the other."""
    T, n = x.shape[:2]
    W = max([len(w) for w in wins] + [1])
    J = sum(len(w) for w in wins)
    jobs = np.zeros(J, dtype=_lib.HOP_JOB_DTYPE)
    atoms = np.zeros((J, n, 3))
    cuts, where = [], []
    distance = np.full((T, W), np.nan)
    n_slabs = np.zeros((T, W), dtype=np.int64)
    k = at = slab_at = 0
    for t in range(T):
        v = wins[t] - c[t]
        for w in range(len(wins[t])):
            frame = window_frame(c[t], wins[t][w])
            d = math.sqrt(float((v[w] * v[w]).sum()))
            nz = int(math.floor((d + ahead + back) / spacing)) + 1
            if nz > 64:
                raise ValueError(f"guest_hopping: {nz} slabs along the window's axis at spacing {spacing} (at most 64): use "
                                 f"a spacing of at least {(d + ahead + back) / 63.0:.3f} or a shorter back and ahead")
            atoms[k] = (x[t] - c[t]) @ frame.T
            others = [j for j in range(len(wins[t])) if j != w]
            rows = np.zeros((len(others), 4))
            for r, j in enumerate(others):
                nj = v[j] / math.sqrt(float((v[j] * v[j]).sum()))
                rows[r, :3] = frame @ nj
                rows[r, 3] = float((nj * v[j]).sum())                # (n . w - n . c: the plane in coordinates from c)
            cuts.append(rows)
            jobs[k] = (k * n, n, 0, at, len(rows), -1, 0, L, slab_at, slab_at * L, -1, k,
                       (-(g // 2) * spacing, -(g // 2) * spacing, -back), spacing, float(core2), float(cutoff2), float(cap),
                       g, g, nz, (g // 2, g // 2), 0)
            distance[t, w], n_slabs[t, w] = d, nz
            where.append((t, w))
            at += len(rows)
            slab_at += nz
            k += 1
    return jobs, atoms, cuts, distance, n_slabs, where


def guest_hopping_batch(xyz, elements_or_coef, guest, centres, window_centres, temperatures, spacing: float = 0.25,
                        half_width: float = 5.75, back: float = 4.0, ahead: float = 4.0, cap: float = 100.0, mass=None,
                        core2: float = 0.25, cutoff2: float = 0.0, device=None, frames=None, kernel_ms=None) -> Hopping:
    """:func:`guest_hopping` for ``T`` frames of the same ``n`` atoms, every (frame, window) a job of ONE ``pw_hop``
    call: ``xyz`` ``(T, n, 3)``, ``centres`` ``(T, 3)``, ``window_centres`` a list of ``T`` arrays ``(W_t, 3)`` (``None``
    or empty: the frame has no window).  ``kernel_ms``: a list that receives ``(total, field, slabs)`` in ms by HIP
    events (the library's measurement entry)."""
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
    if mass is None:
        if not isinstance(guest, str) or guest not in GUEST_MASSES:
            raise ValueError("mass: the guest's molar mass in g/mol (built in for the names of affinity.GUESTS only)")
        mass = GUEST_MASSES[guest]
    mass = float(mass)
    temps = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=np.float64)))
    if not (1 <= len(temps) <= _lib.AFF_MAX_LEVELS) or not np.isfinite(temps).all() or (temps <= 0.0).any() or not mass > 0.0:
        raise ValueError("temperatures: 1 to 8 positive numbers; mass: positive")
    c = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
    if len(c) != T or len(window_centres) != T:
        raise ValueError("centres and window_centres: one entry per frame")
    spacing, back, ahead = float(spacing), float(back), float(ahead)
    if not (spacing > 0.0 and math.isfinite(spacing) and back >= 0.0 and ahead >= 0.0 and half_width > 0.0):
        raise ValueError("spacing and half_width: positive; back and ahead: not negative")
    g = _lattice(float(half_width), spacing)
    L = len(temps)
    wins = [np.zeros((0, 3)) if w is None else np.asarray(w, dtype=np.float64).reshape(-1, 3) for w in window_centres]
    n_windows = np.array([len(w) for w in wins], dtype=np.int64)
    W = int(n_windows.max()) if T else 0
    jobs, atoms, cuts, distance, n_slabs, where = hop_jobs(x, c, wins, g, spacing, back, ahead, L, cap, core2, cutoff2)
    J = len(jobs)
    betas = 1.0 / (R * temps)
    slabs, sums, out, _ = engine.context(device).hop(jobs, betas, atoms.reshape(-1, 3), coef,
                                                     np.concatenate(cuts) if cuts else None, kernel_ms=kernel_ms)
    S = int(n_slabs.max()) if J else 1
    raw = np.zeros((T, max(W, 1), S), dtype=_lib.HOP_SLAB_DTYPE)
    raw["n"] = raw["n_face"] = raw["min_i"] = raw["min_j"] = -1
    raw["u_min"] = np.nan
    Z = np.full((T, max(W, 1), S, L), np.nan)
    E = np.full((T, max(W, 1), S, L), np.nan)
    flags = np.zeros((T, max(W, 1)), dtype=np.int32)
    for k, (t, w) in enumerate(where):
        first, nz = int(jobs["slab_first"][k]), int(jobs["nz"][k])
        raw[t, w, :nz] = slabs[first:first + nz]
        pairs = sums[first * L:(first + nz) * L].reshape(nz, L)
        Z[t, w, :nz], E[t, w, :nz] = pairs["z"], pairs["e"]
        flags[t, w] = out["flags"][k]
    return Hopping(raw, Z, E, flags, n_windows, n_slabs, distance, spacing, back, temps, mass, guest,
                   None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def guest_hopping(xyz, elements_or_coef, guest, centre, window_centres, temperatures, spacing: float = 0.25,
                  half_width: float = 5.75, back: float = 4.0, ahead: float = 4.0, cap: float = 100.0, mass=None,
                  core2: float = 0.25, cutoff2: float = 0.0, device=None) -> Hopping:
    """The free-energy profile of a one-site Lennard-Jones guest through every window of the cage ``xyz`` ``(n, 3)`` and
    the hopping rate built on it: see :class:`Hopping`.  ``elements_or_coef``: the atoms' element symbols (UFF with
    ``guest`` a name of ``pywindow_amd.affinity.GUESTS`` or a ``(sigma, eps_kJ_per_mol)`` pair), or ready rows ``(A, B)``.
    ``centre``: the pore centre; ``window_centres`` ``(W, 3)``.  For window ``k`` the cage is turned by
    :func:`window_frame`; the lattice across has ``2 round(half_width / spacing) + 1`` voxels a side with the axis through
    its middle, and slab ``l`` lies at ``z = -back + l * spacing``, up to ``|w - c| + ahead`` -- more than 64 either way
    is a ``ValueError`` that names the spacing.  The other windows' planes are held shut; a voxel within ``sqrt(core2)``
    of an atom or above ``cap`` kJ/mol is left out (without a cap every slab leaks to the lattice's edge at once: the cap
    is part of the definition, and the rate does not hang on it).  ``temperatures``: up to 8, K.  ``mass``: g/mol, built
    in for the names of ``GUESTS``.  ``xyz`` ``(T, n, 3)`` with ``centre`` ``(T, 3)`` and a list of window centres is
    :func:`guest_hopping_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return guest_hopping_batch(x, elements_or_coef, guest, centre, window_centres, temperatures, spacing, half_width,
                                   back, ahead, cap, mass, core2, cutoff2, device)
    many = guest_hopping_batch(x.reshape(1, -1, 3), elements_or_coef, guest, np.asarray(centre, dtype=np.float64).reshape(1, 3),
                               [window_centres], temperatures, spacing, half_width, back, ahead, cap, mass, core2, cutoff2,
                               device)
    return dataclasses.replace(many, single=True)
