"""Guest passage on the GPU: the energy barrier a guest crosses at every window of a cage (``pw_passage``,
include/pywindow_amd.h).

``pw_affinity`` says how strongly a cage holds a guest; this module says what it costs the guest to get in or out.  The
Lennard-Jones energy of the guest at every voxel of the box is a landscape; for window ``k`` the other windows' planes
stay shut, and the ``barrier`` is the lowest energy level at which the basin around the pore centre connects to the
outside -- the minimax (bottleneck) path through that window, found by flood fills under a bisection of the level.
``well`` is the lowest energy the guest finds on the inside of that level and ``activation = barrier - well`` the
activation energy of the hop for the cage as it stands in that frame.  A trajectory of such numbers shows the window
breathing: a guest wider than the static window passes when the frames with a low barrier are frequent enough.

When the saddle lies on a face of the box (``free_exit``) the window is no obstacle of its own: the energy only falls
towards the centre, and ``barrier`` is the energy where the path left the box, which depends on the box.

Everything the kernel returns is a comparison of doubles or a count, so the device and the explicit host path
(``device=-1``) return the same bytes.  Parameters and units as in :mod:`pywindow_amd.affinity` (UFF atoms, one-site
guests, Lorentz-Berthelot mixing, kJ/mol and Angstrom).  The reference has no counterpart.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .affinity import R, lj_coefficients
from .cavity import _grid

__all__ = ["Passage", "guest_passage", "guest_passage_batch", "passage_field"]

_SERIES = ("activation", "barrier", "well", "u_seed", "n_basin", "basin_volume")


@dataclasses.dataclass(frozen=True)
class Passage:
    """The passage of one frame (``raw`` ``(M,)``, one entry a window) or of ``T`` frames (``raw`` ``(T, M)``, ``M`` the
    largest number of rows of a frame).  ``raw`` holds ``pw_passage``'s rows (``_lib.PASSAGE_OUT_DTYPE``) in the order of
    the frame's planes -- its windows --; a frame without planes has one row, the passage to anywhere outside the box.
    Entries past a frame's rows are padding: NaN energies, ``-1`` voxels and counts.  ``n_windows``: the planes of the
    frame.  ``origin`` is the centre of voxel ``(0, 0, 0)`` and ``shape`` the grid ``(nx, ny, nz)``."""

    raw: np.ndarray
    n_windows: object
    origin: np.ndarray
    shape: np.ndarray
    spacing: float
    guest: object = None
    frames: np.ndarray | None = None

    @property
    def n_rows(self):
        """The rows of each frame that are results rather than padding: ``max(n_windows, 1)``."""
        return np.maximum(self.n_windows, 1)

    @property
    def padding(self):
        return np.arange(self.raw.shape[-1]) >= np.asarray(self.n_rows)[..., None]

    @property
    def barrier(self):
        """The lowest level at which the seed's basin reaches a face of the box through each window, kJ/mol; ``+inf``
        when nothing does."""
        return self.raw["barrier"]

    @property
    def well(self):
        """The lowest energy inside that level, kJ/mol."""
        return self.raw["well"]

    @property
    def u_seed(self):
        return self.raw["u_seed"]

    @property
    def activation(self):
        """``barrier - well``, kJ/mol; ``+inf`` without an exit, NaN when the seed was closed."""
        with np.errstate(invalid="ignore"):
            return self.raw["barrier"] - self.raw["well"]

    @property
    def seed_closed(self):
        return (self.raw["flags"] & _lib.PAS_SEED_CLOSED) != 0

    @property
    def no_exit(self):
        """No level connects the seed to a face of the box through this window."""
        return (self.raw["flags"] & _lib.PAS_NO_EXIT) != 0

    @property
    def free_exit(self):
        """The saddle lies on a face of the box: the window is no obstacle of its own and ``barrier`` depends on the
        box."""
        v = self.raw["saddle"]
        top = (np.asarray(self.shape)[..., None, :] - 1) if self.raw.ndim == 2 else np.asarray(self.shape) - 1
        return (v[..., 0] >= 0) & ((v == 0) | (v == top)).any(axis=-1)

    def _position(self, name):
        v = np.asarray(self.raw[name], dtype=np.float64)
        origin = self.origin[..., None, :] if self.raw.ndim == 2 else self.origin
        return np.where(v < 0.0, np.nan, origin + self.spacing * v)

    @property
    def saddle_position(self):
        """The centre of the saddle voxel of every window, ``(..., M, 3)``; NaN without one."""
        return self._position("saddle")

    @property
    def well_position(self):
        return self._position("well_voxel")

    @property
    def n_basin(self):
        """The voxels of the seed's basin strictly below the barrier."""
        return self.raw["n_basin"]

    @property
    def n_fill(self):
        return self.raw["n_fill"]

    @property
    def basin_volume(self):
        """``n_basin * spacing**3`` in cubic Angstrom; NaN for padding."""
        n = np.asarray(self.raw["n_basin"], dtype=np.float64)
        return np.where(n < 0.0, np.nan, n * (self.spacing * self.spacing * self.spacing))

    def transmission(self, temperature: float):
        """``exp(-activation / RT)``: the Boltzmann factor of the hop through each window (plain numpy on the defined
        result; 0 without an exit)."""
        with np.errstate(invalid="ignore", over="ignore"):
            return np.exp(-self.activation / (R * float(temperature)))

    def series(self, name: str = "activation", window=None):
        """``(values, valid)`` of a quantity over the frames -- float64 values; ``valid``: the value is finite and the
        row has no flag.  ``window``: a column, or ``None`` for each frame's window of the lowest activation among its
        valid ones.  Ready for :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`,
        :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics` and
        :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = np.atleast_2d(np.asarray(getattr(self, name), dtype=np.float64))
        ok = np.isfinite(v) & (np.atleast_2d(self.raw["flags"]) == 0) & ~np.atleast_2d(self.padding)
        if window is None:
            act = np.where(ok & np.isfinite(np.atleast_2d(self.activation)), np.atleast_2d(self.activation), np.inf)
            column = act.argmin(axis=1)
        else:
            column = np.full(len(v), int(window))
        rows = np.arange(len(v))
        return v[rows, column].copy(), ok[rows, column].copy()


def _pad(out, jobs, T):
    """The rows of a call as ``(T, M)``, padded."""
    rows = np.maximum(jobs["m"], 1)
    M = int(rows.max()) if T else 1
    raw = np.zeros((T, M), dtype=_lib.PASSAGE_OUT_DTYPE)
    for name in ("barrier", "well", "u_seed"):
        raw[name] = np.nan
    for name in ("n_fill", "n_basin", "saddle", "well_voxel"):
        raw[name] = -1
    for t in range(T):
        first = int(jobs["out_first"][t])
        raw[t, :int(rows[t])] = out[first:first + int(rows[t])]
    return raw


def guest_passage_batch(xyz, elements_or_coef, guest, seeds, planes=None, spacing: float = 0.5, half_widths=None,
                        core2: float = 0.25, cutoff2: float = 0.0, device=None, frames=None, kernel_ms=None,
                        fills=None) -> Passage:
    """:func:`guest_passage` for ``T`` frames of the same ``n`` atoms in ONE ``pw_passage`` call: ``xyz`` ``(T, n, 3)``,
    ``seeds`` ``(T, 3)``, ``half_widths`` ``None`` or ``(T,)``, ``planes`` ``None`` or a list of ``T`` arrays ``(m_t, 4)``
    (``None`` or an empty array: no planes for that frame).  The boxes are those of
    :func:`pywindow_amd.cavity_grid_batch`.  The fields of the result are ``(T, max m)`` arrays.  ``kernel_ms`` / ``fills``:
    lists that receive the time of the device work by HIP events and the flood fills of every row (the library's
    measurement entry)."""
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
    s = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    if len(s) != T:
        raise ValueError("seeds: one seed per frame")
    spacing = float(spacing)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError("spacing: a positive number")
    if half_widths is None:
        hw = np.sqrt(((x - s[:, None, :]) ** 2).sum(axis=2)).max(axis=1) if n else np.full(T, spacing)
    else:
        hw = np.broadcast_to(np.asarray(half_widths, dtype=np.float64), (T,))
    if not np.isfinite(hw).all() or (hw <= 0.0).any():
        raise ValueError("half_width: positive and finite")
    jobs = np.zeros(T, dtype=_lib.PASSAGE_JOB_DTYPE)
    cuts, at, rows = [], 0, 0
    for t in range(T):
        g = _grid(float(hw[t]), spacing)
        p = None if planes is None else planes[t]
        p = np.zeros((0, 4)) if p is None else np.asarray(p, dtype=np.float64).reshape(-1, 4)
        jobs[t] = (t * n, n, 0, at, len(p), -1, rows, s[t] - spacing * (g // 2 - 0.5), spacing, float(core2), float(cutoff2),
                   g, g, g, (g // 2 - 1,) * 3)
        cuts.append(p)
        at += len(p)
        rows += max(len(p), 1)
    counts = None if fills is None else np.zeros(rows, dtype=np.int32)
    out = engine.context(device).passage(jobs, x.reshape(-1, 3), coef, np.concatenate(cuts) if cuts else None,
                                         kernel_ms=kernel_ms, fills=counts)
    if fills is not None:
        fills.append(counts)
    shape = np.stack([jobs["nx"], jobs["ny"], jobs["nz"]], axis=1).astype(np.int64)
    return Passage(_pad(out, jobs, T), jobs["m"].copy(), jobs["origin"].copy(), shape, spacing, guest,
                   None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def _one(many: Passage) -> Passage:
    return Passage(many.raw[0], int(many.n_windows[0]), many.origin[0], many.shape[0], many.spacing, many.guest, None)


def guest_passage(xyz, elements_or_coef, guest, seed, planes=None, spacing: float = 0.5, half_width=None,
                  core2: float = 0.25, cutoff2: float = 0.0, device=None) -> Passage:
    """The barrier a one-site Lennard-Jones guest crosses at every window of the cage ``xyz`` ``(n, 3)``: see
    :class:`Passage`.  ``elements_or_coef``: the atoms' element symbols (UFF with ``guest`` a name of
    ``pywindow_amd.affinity.GUESTS`` or a ``(sigma, eps_kJ_per_mol)`` pair), or ready rows ``(A, B)`` ``(n, 2)``.  The box
    is :func:`pywindow_amd.cavity_grid`'s: centred on ``seed`` with ``2 ceil(half_width / spacing)`` voxels an axis
    (``half_width`` defaults to the largest ``|atom - seed|``; more than 64 voxels an axis: ``ValueError``).  ``planes``:
    rows ``(a, b, c, d)``, one a window; row ``k`` of the result leaves plane ``k`` out and holds the others shut
    (``None``: one row, no planes).  A voxel within ``sqrt(core2)`` of an atom is blocked.  ``xyz`` ``(T, n, 3)`` with
    ``seed`` ``(T, 3)`` is :func:`guest_passage_batch` with the same planes and half width for every frame.  ``device``:
    the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        T = len(x)
        return guest_passage_batch(x, elements_or_coef, guest, seed, None if planes is None else [planes] * T, spacing,
                                   None if half_width is None else np.full(T, half_width), core2, cutoff2, device)
    return _one(guest_passage_batch(x.reshape(1, -1, 3), elements_or_coef, guest, np.asarray(seed, dtype=np.float64).reshape(1, 3),
                                    None if planes is None else [planes], spacing,
                                    None if half_width is None else [half_width], core2, cutoff2, device))


def passage_field(field, seed_voxel, planes=None, origin=(0.0, 0.0, 0.0), spacing: float = 1.0, device=None) -> Passage:
    """:class:`Passage` of a caller's scalar ``field`` ``(nz, ny, nx)`` -- every value finite or ``+inf`` (blocked) --
    from the voxel ``seed_voxel = (i, j, l)``: the level at which the seed's basin reaches a face of the grid.  The
    negative distance to the nearest atom surface as the field gives the largest hard sphere that passes.  ``planes``
    rows ``(a, b, c, d)`` against the voxel centres ``origin + spacing * (i, j, l)``, one row of the result a plane left
    out."""
    f = np.ascontiguousarray(field, dtype=np.float64)
    if f.ndim != 3:
        raise ValueError("field: (nz, ny, nx)")
    p = np.zeros((0, 4)) if planes is None else np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    jobs = np.zeros(1, dtype=_lib.PASSAGE_JOB_DTYPE)
    nz, ny, nx = f.shape
    jobs[0] = (0, 0, 0, 0, len(p), 0, 0, np.asarray(origin, dtype=np.float64), float(spacing), 0.25, 0.0, nx, ny, nz,
               tuple(int(v) for v in seed_voxel))
    out = engine.context(device).passage(jobs, None, None, p, f.reshape(-1))
    shape = np.array([[nx, ny, nz]], dtype=np.int64)
    return _one(Passage(_pad(out, jobs, 1), jobs["m"].copy(), jobs["origin"].copy(), shape, float(spacing), None, None))
