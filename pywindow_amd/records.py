"""Columnar results of a trajectory analysis and lazy views of them.

The reference keeps ``analysis_output[frame][molecule]`` as nested dicts and writes them as JSON
(trajectory.py:251-271, io_tools.py:215-265): at a million units that is a million dicts and a
gigabyte of text.  The engine's own result is columnar -- one fixed-size record per (frame, molecule)
unit -- so that is what is kept and persisted here:

* :class:`RecordStore`: the structured record array (``_lib.UNIT_OUT_DTYPE``) of an analysis, the
  windows beyond what a record holds, and the (frame, molecule) of every unit; ``save`` / ``load``
  as ONE flat file (a JSON header and the arrays as they lie in memory; reopened as a memory map).
* :class:`LazyAnalysis`: a mapping with the reference's shape -- ``view[frame][molecule]`` is the
  dict ``Molecule.full_analysis()`` returns -- whose entries are built from the records on first
  access and cached.  Frames assigned by hand are kept as given.

``DLPOLY.analysis(lazy=True)``, ``DLPOLY.save_records`` and ``DLPOLY.load_records`` are the entry
points (pywindow_amd/trajectory.py); the JSON route (``save_analysis``) is unchanged.
"""

from __future__ import annotations

import pathlib
from collections.abc import MutableMapping

import numpy as np

from . import _lib, engine

FORMAT = "pywindow_amd.records/1"
MAGIC = b"PWREC001"
HEADER_BYTES = 4096


class RecordStore:
    """Records of one analysis in unit order.

    ``records`` (U,) ``UNIT_OUT_DTYPE``; ``extra`` ``EXTRA_WINDOW_DTYPE`` (its ``unit`` indexes
    ``records``); ``unit_frame`` (U,) the frame of every unit; ``unit_molecule`` (U,) the molecule
    index inside the frame, or all ``-1`` for a non-modular analysis (one unit per frame, key
    ``"0"`` -- a string -- in the reference's dict, trajectory.py:515-522)."""

    def __init__(self, records, unit_frame, unit_molecule=None, extra=None, stages: int = _lib.STAGE_ALL):
        def keep(a, dtype):          # (no copy of what already is such an array: memory maps stay memory maps)
            return a if isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 1 else np.ascontiguousarray(a, dtype=dtype).reshape(-1)

        self.records = keep(records, _lib.UNIT_OUT_DTYPE)
        self.unit_frame = keep(unit_frame, np.dtype(np.int64))
        n = len(self.records)
        if unit_molecule is None:
            unit_molecule = np.full(n, -1, dtype=np.int64)
        self.unit_molecule = keep(unit_molecule, np.dtype(np.int64))
        self.extra = np.zeros(0, dtype=_lib.EXTRA_WINDOW_DTYPE) if extra is None else keep(extra, _lib.EXTRA_WINDOW_DTYPE)
        self.stages = int(stages)
        if len(self.unit_frame) != n or len(self.unit_molecule) != n:
            raise ValueError("one frame / molecule index per record")
        self._more = None
        self._spans = None
        self._tracks = None

    # ---- index -----------------------------------------------------------------------------
    @property
    def modular(self) -> bool:
        return bool(len(self.unit_molecule)) and bool((self.unit_molecule >= 0).any())

    def spans(self) -> dict:
        """``{frame: (first unit, one past the last)}`` -- the units of a frame are contiguous."""
        if self._spans is None:
            uf = self.unit_frame
            spans = {}
            if len(uf):
                cut = np.flatnonzero(np.diff(uf)) + 1
                lo = np.concatenate([[0], cut])
                hi = np.concatenate([cut, [len(uf)]])
                for a, b in zip(lo.tolist(), hi.tolist()):
                    f = int(uf[a])
                    if f in spans:
                        raise ValueError(f"the units of frame {f} are not contiguous")
                    spans[f] = (a, b)
            self._spans = spans
        return self._spans

    def frame_properties(self, frame: int) -> dict:
        """The reference's ``analysis_output[frame]``: ``{"0": properties}`` or ``{0: ..., 1: ...}``."""
        lo, hi = self.spans()[frame]
        if self._more is None:
            self._more = engine.extra_by_unit([self.extra]) if len(self.extra) else {}
        out = {}
        for u in range(lo, hi):
            rec = self.records[u]
            if int(rec["status"]) != 0:
                engine.warn_like_reference(rec)
            m = int(self.unit_molecule[u])
            out["0" if m < 0 else m] = engine.record_to_properties(rec, self.stages, self._more.get(u))
        return out

    # ---- distributions ---------------------------------------------------------------------
    #: quantity (the reference's property names) -> (record field, stages of which one must have run, status
    #: bits that say the unit has no such value)
    _QUANTITIES = {
        "maximum_diameter": ("maxd", _lib.STAGE_ALL, 0),
        "pore_diameter": ("pore_d", _lib.STAGE_ALL, 0),
        "pore_volume": ("pore_vol", _lib.STAGE_ALL, 0),
        "average_diameter": ("avg_d", _lib.STAGE_AVG, _lib.ST_POINTS_OVERFLOW),
        "pore_diameter_opt": ("pore_opt_d", _lib.STAGE_OPT | _lib.STAGE_WINDOWS, _lib.ST_NEGATIVE_PORE),
        "pore_volume_opt": ("pore_vol_opt", _lib.STAGE_OPT | _lib.STAGE_WINDOWS, _lib.ST_NEGATIVE_PORE),
        "windows": (None, _lib.STAGE_WINDOWS, 0),
    }

    def _samples_by_unit(self, quantity: str):
        """``(values, unit of every value)`` of :meth:`samples`."""
        if quantity not in self._QUANTITIES:
            raise KeyError(f"unknown quantity {quantity!r}: one of {sorted(self._QUANTITIES)}")
        field, stages, missing = self._QUANTITIES[quantity]
        if not self.stages & stages:
            raise KeyError(f"{quantity!r} was not computed: the analysis ran without its stage (stages = {self.stages})")
        recs = self.records
        if field is not None:
            units = np.flatnonzero((recs["status"] & missing) == 0) if missing else np.arange(len(recs))
            return np.array(recs[field][units], dtype=np.float64), units
        held = np.clip(recs["n_windows"], 0, _lib.W_MAX)
        mask = np.arange(_lib.W_MAX)[None, :] < held[:, None]
        unit, index = np.nonzero(mask)
        values = np.array(recs["win_d"][mask], dtype=np.float64)
        if len(self.extra):              # the windows a record has no room for, each after its unit's sixteen
            unit = np.concatenate([unit, self.extra["unit"].astype(np.int64)])
            index = np.concatenate([index, self.extra["index"].astype(np.int64)])
            values = np.concatenate([values, self.extra["d"]])
            order = np.lexsort((index, unit))
            unit, values = unit[order], values[order]
        return values, unit

    def samples(self, quantity: str) -> np.ndarray:
        """Every value of ``quantity`` in the store, in unit order: ``"maximum_diameter"``, ``"pore_diameter"``,
        ``"pore_volume"``, ``"average_diameter"``, ``"pore_diameter_opt"``, ``"pore_volume_opt"``, or ``"windows"``
        -- all window diameters, unit by unit in window order, those beyond what a record holds included.  What
        the reference's examples collect from ``analysis_output`` (examples/example_7.py:53-66).  A unit that has
        no such value contributes nothing (windows ``None``; a non-porous unit has no optimised pore; a unit
        whose sampling overflowed has no average diameter); a quantity whose stage never ran is a ``KeyError``."""
        return self._samples_by_unit(quantity)[0]

    def distribution(self, quantity: str, points=1000, pad: float = 1.0, bw_method="scott", per_molecule: bool = False,
                     device=None):
        """Gaussian kernel density estimate of :meth:`samples` (pywindow_amd/distributions.py): a
        ``Distribution``.  ``points``: an int for ``np.linspace(min - pad, max + pad, points)`` as the reference's
        examples do, or the grid itself.  ``per_molecule`` (modular stores): ``{molecule: Distribution}``, every
        molecule's curve on its own grid, all from one batched call."""
        from . import distributions as D

        values, unit = self._samples_by_unit(quantity)
        if not per_molecule:
            return D.gaussian_kde_1d(values, D.grid(values, points, pad), bw_method, device)
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        mol = np.asarray(self.unit_molecule)[unit]
        keys = [int(m) for m in np.unique(mol)]
        sets = [values[mol == m] for m in keys]
        curves = D.gaussian_kde_batch(sets, [D.grid(v, points, pad) for v in sets], bw_method, device)
        return dict(zip(keys, curves))

    def distribution_band(self, quantity: str, points=1000, pad: float = 1.0, bw_method="scott", replicas: int = 200,
                          block=None, level: float = 0.95, seed=0, per_molecule: bool = False, device=None):
        """:meth:`distribution` with a pointwise error band (pywindow_amd/distributions.py): a ``DistributionBand``
        whose ``density`` is :meth:`distribution`'s, bit for bit.  The band is a circular moving-block bootstrap over
        the frame axis of :meth:`series`: ``replicas`` times, blocks of ``block`` consecutive frames are drawn until
        the series is full again, a sample weighs as often as its frame was drawn (every window of a frame with its
        frame; gap frames carry no samples), and the KDE is redone at the ORIGINAL bandwidth -- all replicas in one
        ``pw_kde_wsums`` call that computes every exponential once.  ``lower`` / ``upper`` are ``np.quantile`` over the
        replicas at ``(1 - level) / 2`` and ``1 - (1 - level) / 2``.  ``block=None``: ``max(1, ceil(2 * time))`` with
        ``time`` the correlation time of ``correlation(quantity)`` (of ``"windows_mean"`` for ``"windows"``), so that
        frames that are not independent stay together; ``block=1`` is the ordinary bootstrap, which takes every frame
        for independent.  A replica that drew no sample is left out; ``.replicas`` is the number used.
        ``per_molecule`` (modular stores): ``{molecule: DistributionBand}``, all molecules in one batched call."""
        import math

        from . import distributions as D

        replicas = int(replicas)
        if replicas < 1:
            raise ValueError("replicas must be at least 1")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie between 0 and 1")
        if block is not None and int(block) < 1:
            raise ValueError("block must be at least 1 frame")
        values, unit = self._samples_by_unit(quantity)
        if per_molecule and not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        curves = self.distribution(quantity, points, pad, bw_method, per_molecule, device)
        along = "windows_mean" if quantity == "windows" else quantity
        if per_molecule:
            mol = np.asarray(self.unit_molecule)[unit]
            keys = sorted(curves)
            picks = [np.flatnonzero(mol == m) for m in keys]
            times = None if block is not None else self.correlation(along, per_molecule=True, device=device)
        else:
            keys, picks, curves = [None], [np.arange(len(values))], {None: curves}
            times = None if block is not None else {None: self.correlation(along, device=device)}
        weights, blocks = [], []
        for m, pick in zip(keys, picks):
            frames = self.series(along, m)[0]
            length = int(block) if block is not None else max(1, math.ceil(2.0 * times[m].time))
            counts = D.block_bootstrap_counts(len(frames), length, replicas, seed)
            stride = int(frames[1] - frames[0])
            w = counts[:, (np.asarray(self.unit_frame)[unit[pick]] - int(frames[0])) // stride].astype(np.float64)
            w = w[w.sum(axis=1) > 0.0]
            if not len(w):
                raise ValueError("no replica drew a sample")
            weights.append(w)
            blocks.append(length)
        dens = D.gaussian_kde_replicas_batch([values[p] for p in picks], [curves[m].x for m in keys], weights,
                                             [curves[m].bandwidth for m in keys], device)
        lo, hi = (1.0 - float(level)) / 2.0, 1.0 - (1.0 - float(level)) / 2.0
        out = {}
        for m, d, w, length in zip(keys, dens, weights, blocks):
            c = curves[m]
            out[m] = D.DistributionBand(c.x, c.density, np.quantile(d, lo, axis=0), np.quantile(d, hi, axis=0), c.n,
                                        c.bandwidth, c.factor, len(w), length, float(level))
        return out if per_molecule else out[None]

    def _pairs_by_unit(self, quantity_x: str, quantity_y: str):
        """``(values of x, values of y, unit of every pair)`` of :meth:`sample_pairs`."""
        vx, ux = self._samples_by_unit(quantity_x)
        vy, uy = self._samples_by_unit(quantity_y)
        if quantity_x == "windows" and quantity_y == "windows":
            raise ValueError("'windows' against 'windows': the windows of a unit have no partner among themselves")
        if quantity_y == "windows":
            wy, wx, unit = self._pairs_by_unit(quantity_y, quantity_x)
            return wx, wy, unit
        # ux: the unit of every value of x (one per unit, or one per window); uy: one per unit, ascending
        at = np.minimum(np.searchsorted(uy, ux), max(len(uy) - 1, 0))
        has = uy[at] == ux if len(uy) else np.zeros(len(ux), dtype=bool)
        return vx[has], vy[at[has]], ux[has]

    def sample_pairs(self, quantity_x: str, quantity_y: str):
        """``(values of quantity_x, values of quantity_y)``, pair by pair, for a joint distribution.  Two per-unit
        quantities pair by unit over the units that have BOTH (a non-porous unit has no optimised pore, ...), in
        unit order.  ``"windows"`` against a per-unit quantity pairs EVERY window diameter with its unit's value --
        those beyond what a record holds included, in the order :meth:`samples` has.  ``"windows"`` against
        ``"windows"`` is a ``ValueError``; unknown names and stages that never ran are :meth:`samples`' ``KeyError``."""
        vx, vy, _ = self._pairs_by_unit(quantity_x, quantity_y)
        return vx, vy

    def joint_distribution(self, quantity_x: str, quantity_y: str, points=128, pad: float = 1.0, bw_method="scott",
                           per_molecule: bool = False, device=None):
        """Two-dimensional Gaussian kernel density estimate of :meth:`sample_pairs` (pywindow_amd/distributions.py):
        a ``Distribution2D`` with ``density[iy, ix]`` at ``(x[ix], y[iy])``.  ``points``: an int or a pair of ints
        for ``np.linspace(min - pad, max + pad, .)`` per axis, or the two axes themselves.  ``per_molecule``
        (modular stores): ``{molecule: Distribution2D}``, every molecule's map on its own mesh, all from one
        batched call."""
        from . import distributions as D

        vx, vy, unit = self._pairs_by_unit(quantity_x, quantity_y)
        if not per_molecule:
            return D.gaussian_kde_2d(vx, vy, points, bw_method, device, pad)
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        mol = np.asarray(self.unit_molecule)[unit]
        keys = [int(m) for m in np.unique(mol)]
        sets = [(vx[mol == m], vy[mol == m]) for m in keys]
        maps = D.gaussian_kde_2d_batch(sets, [D.grid_2d(sx, sy, points, pad) for sx, sy in sets], bw_method, device)
        return dict(zip(keys, maps))

    # ---- dynamics --------------------------------------------------------------------------
    #: per-frame reductions of a unit's window diameters, for :meth:`series`
    _WINDOW_SERIES = ("windows_min", "windows_max", "windows_mean", "n_windows")

    def attach_tracks(self, tracks) -> None:
        """Keep the ``WindowTracks`` of this store (pywindow_amd/tracks.py) so that :meth:`series` knows
        ``"window_site"``.  In memory only: tracks are not written by :meth:`save`, and the record file is unchanged."""
        if len(tracks.site_of) != len(self._samples_by_unit("windows")[0]):
            raise ValueError("the tracks are not of this store: one site per window")
        self._tracks = tracks

    def _site_series(self, quantity: str, site, molecule, guest):
        if quantity != "window_site":
            raise ValueError("site= belongs to 'window_site'")
        if self._tracks is None:
            raise ValueError("'window_site' needs window tracks: attach_tracks(track_windows(...)) first")
        if site is None:
            raise ValueError("'window_site' is one series a site: say which with site=")
        if molecule is not None or guest is not None:
            raise ValueError("'window_site' takes neither molecule= nor guest=")
        t = self._tracks
        j = int(site)
        if not 0 <= j < t.diameter.shape[1]:
            raise ValueError(f"site: 0 .. {t.diameter.shape[1] - 1}")
        return t.frames.copy(), t.diameter[:, j].copy(), t.valid[:, j].copy()

    def _value_by_unit(self, quantity: str, guest=None):
        """``(value of every unit (nan where it has none), which units have one)``."""
        n = len(self.records)
        values, has = np.full(n, np.nan), np.zeros(n, dtype=bool)
        if quantity == "windows_open":
            if guest is None or not np.isfinite(float(guest)):
                raise ValueError("'windows_open' counts the windows a guest passes: say its diameter with guest=")
            d, unit = self._samples_by_unit("windows")
            return np.bincount(unit[d >= float(guest)], minlength=n).astype(np.float64), np.ones(n, dtype=bool)
        if guest is not None:
            raise ValueError("guest= belongs to 'windows_open'")
        if quantity == "windows":
            raise ValueError("'windows' is several values a frame: a series needs one of " + ", ".join(self._WINDOW_SERIES))
        if quantity not in self._WINDOW_SERIES:
            v, unit = self._samples_by_unit(quantity)
            values[unit], has[unit] = v, True
            return values, has
        d, unit = self._samples_by_unit("windows")             # unit by unit, in window order
        count = np.bincount(unit, minlength=n)
        if quantity == "n_windows":
            return count.astype(np.float64), np.ones(n, dtype=bool)
        first = np.cumsum(count) - count
        for u in np.flatnonzero(count).tolist():
            w = d[first[u]:first[u] + count[u]]
            values[u] = w.min() if quantity == "windows_min" else w.max() if quantity == "windows_max" else np.sum(w) / len(w)
        return values, count > 0

    def series(self, quantity: str, molecule=None, guest=None, site=None):
        """``(frames, values, valid)``: ``quantity`` along the frame axis.  Every per-unit name of :meth:`samples`, or a
        per-frame reduction of the windows: ``"windows_min"``, ``"windows_max"``, ``"windows_mean"`` (``np.sum(d) /
        len(d)`` of the unit's diameters, those beyond what a record holds included) or ``"n_windows"`` (how many there
        are; 0 is a value), or ``"windows_open"`` with ``guest=d``: how many of the unit's windows have a diameter ``>= d``,
        the cooperative-gating state (0 is a value, also for a unit without windows).  ``frames = f0 + stride * arange(T)`` from the smallest frame of the store to the largest
        in steps of the gcd of their differences; units are placed by their frame index, whatever their order in the
        store.  A frame that is absent, or whose unit has no such value (non-porous, windows ``None``, ...), is a GAP:
        ``valid[t]`` is ``False`` and ``values[t]`` nan.  Modular stores: ``molecule`` selects the molecule.
        ``"window_site"`` with ``site=j``, once tracks are attached (:meth:`attach_tracks`): the diameter of the window
        at site ``j`` of the cage, a gap where the frame has no window there; ``site=`` with any other quantity, or
        ``"window_site"`` without tracks, is a ``ValueError``."""
        if site is not None or quantity == "window_site":
            return self._site_series(quantity, site, molecule, guest)
        values, has = self._value_by_unit(quantity, guest)
        if self.modular:
            if molecule is None:
                raise ValueError("a modular store holds several molecules a frame: say which with molecule=")
            units = np.flatnonzero(np.asarray(self.unit_molecule) == int(molecule))
        elif molecule is not None:
            raise ValueError("molecule= needs a modular analysis (the store has one unit per frame)")
        else:
            units = np.arange(len(self.records))
        f = np.asarray(self.unit_frame)[units]
        if len(np.unique(f)) < 2:
            raise ValueError("a series needs at least two frames")
        if len(np.unique(f)) != len(f):
            raise ValueError("a frame appears more than once")
        f0 = int(f.min())
        stride = int(np.gcd.reduce(f - f0))
        at = (f - f0) // stride
        frames = f0 + stride * np.arange(int(at.max()) + 1, dtype=np.int64)
        out, valid = np.full(len(frames), np.nan), np.zeros(len(frames), dtype=bool)
        out[at], valid[at] = values[units], has[units]
        return frames, out, valid

    def correlation(self, quantity: str, other=None, max_lag=None, per_molecule: bool = False, device=None, site=None):
        """Lagged correlation of :meth:`series` over the frames (pywindow_amd/correlations.py): a ``TimeCorrelation``
        of ``quantity`` with itself, or with ``other`` at later frames; gaps are left out pair by pair.  ``lag`` is in
        frames.  ``per_molecule`` (modular stores): ``{molecule: TimeCorrelation}``, all from one batched call.
        ``site``: passed to :meth:`series` for ``quantity`` (``"window_site"``); ``other`` may be ``("window_site", j)``,
        so that ``correlation("window_site", ("window_site", 2), site=0)`` says whether two windows open together."""
        from . import correlations as C

        def pair(molecule):
            frames, a, va = self.series(quantity, molecule, site=site)
            if isinstance(other, tuple):
                b, vb = self.series(other[0], molecule, site=other[1])[1:]
            else:
                b, vb = self.series(other, molecule)[1:] if other is not None else (None, None)
            return int(frames[1] - frames[0]), (a, b, va, vb)

        if not per_molecule:
            stride, p = pair(None)
            return C.time_correlation_batch([p], max_lag, device, stride)[0]
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        keys = [int(m) for m in np.unique(self.unit_molecule)]
        pairs = [pair(m) for m in keys]
        return dict(zip(keys, C.time_correlation_batch([p for _, p in pairs], max_lag, device, [s for s, _ in pairs])))

    def spectrum(self, quantity: str, molecule=None, per_molecule: bool = False, oversample: int = 4,
                 max_frequency: float = 0.5, dt: float = 1.0, device=None, site=None):
        """Generalised Lomb-Scargle periodogram of :meth:`series` over the frames (pywindow_amd/spectra.py): a
        ``Spectrum`` whose ``peak_frequency`` says at which frequency ``quantity`` oscillates; gaps are left out
        exactly.  ``frequency`` is in cycles per ``dt`` (the time of one frame; the stride of the frame axis is taken
        from the series), ``max_frequency`` in cycles per sample.  ``per_molecule`` (modular stores): ``{molecule:
        Spectrum}``, all from one batched call.  ``site``: passed to :meth:`series` (``"window_site"``)."""
        from . import spectra as S

        def one(mol):
            frames, a, valid = self.series(quantity, mol, site=site)
            return int(frames[1] - frames[0]), (a, valid)

        if not per_molecule:
            stride, p = one(molecule)
            return S.lomb_scargle_batch([p], oversample, max_frequency, stride, dt, device)[0]
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        keys = [int(m) for m in np.unique(self.unit_molecule)]
        each = [one(m) for m in keys]
        return dict(zip(keys, S.lomb_scargle_batch([p for _, p in each], oversample, max_frequency, [s for s, _ in each],
                                                   dt, device)))

    def gating(self, quantity: str = "windows_max", thresholds=200, molecule=None, per_molecule: bool = False,
               n_bins: int = 64, device=None, site=None):
        """Gating statistics of :meth:`series` over the frames (pywindow_amd/gating.py): a ``Gating`` that says, for a
        guest of every diameter of ``thresholds``, what fraction of the time ``quantity`` admits it (``windows_max``: the
        largest window does; ``windows_min``: every window does), how often it opens and closes and how long the
        openings and closures last; gaps end a run and censor it.  ``thresholds``: an int for ``np.linspace(min, max,
        thresholds)`` over the valid values of the series, or the thresholds themselves.  Lengths are in frames (the
        stride of the frame axis is taken from the series).  ``per_molecule`` (modular stores): ``{molecule: Gating}``,
        all from one batched call.  ``site``: passed to :meth:`series` (``"window_site"``: the gating of ONE window)."""
        from . import gating as G

        def one(mol):
            frames, a, valid = self.series(quantity, mol, site=site)
            if isinstance(thresholds, (bool, np.bool_)):
                raise ValueError("thresholds: a number of thresholds or the thresholds themselves, not a bool")
            if isinstance(thresholds, (int, np.integer)):
                if thresholds < 1 or not valid.any():
                    raise ValueError("thresholds: at least one, over a series with a valid entry")
                d = np.linspace(a[valid].min(), a[valid].max(), int(thresholds))
            else:
                d = np.asarray(thresholds, dtype=np.float64)
            return int(frames[1] - frames[0]), (a, d, valid)

        if not per_molecule:
            stride, item = one(molecule)
            return G.gate_statistics_batch([item], n_bins, stride, device)[0]
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        keys = [int(m) for m in np.unique(self.unit_molecule)]
        each = [one(m) for m in keys]
        return dict(zip(keys, G.gate_statistics_batch([i for _, i in each], n_bins, [s for s, _ in each], device)))

    def kinetics(self, quantity: str = "windows_max", edges=None, max_lag=None, lag_step: int = 1, molecule=None,
                 per_molecule: bool = False, guest=None, device=None, site=None):
        """Lagged state-transition counts of :meth:`series` over the frames (pywindow_amd/kinetics.py): a ``Kinetics``
        with the count matrices ``C_k[i][j] = #{t : s[t] = i, s[t + k] = j}``, the transition matrices, the populations
        and the implied timescales; a pair with a gap at either end is counted nowhere.  ``edges`` cut the value axis
        into states (a value equal to an edge is in the upper one).  ``quantity="windows_open"`` with ``guest=d`` is the
        number of windows open to a guest of diameter ``d``; its ``edges`` default to ``0.5, 1.5, ...`` up to the largest
        count seen, one state per count.  The lags are ``0, lag_step, 2 * lag_step, ...`` up to ``max_lag`` (default
        ``T // 2``), both in samples of the series; ``Kinetics.lag`` is in frames (the stride of the frame axis is taken
        from the series).  ``per_molecule`` (modular stores): ``{molecule: Kinetics}``, all from one batched call.
        ``site``: passed to :meth:`series` (``"window_site"``)."""
        from . import kinetics as K

        lag_step = int(lag_step)
        if lag_step < 1:
            raise ValueError("lag_step: at least 1")

        def one(mol):
            frames, a, valid = self.series(quantity, mol, guest, site)
            if edges is not None:
                e = np.asarray(edges, dtype=np.float64)
            elif quantity == "windows_open":
                e = 0.5 + np.arange(int(a[valid].max()) if valid.any() else 0)
            else:
                raise ValueError("edges: the values that separate the states (only 'windows_open' has a default)")
            top = len(a) // 2 if max_lag is None else int(max_lag)
            if top < 0:
                raise ValueError("max_lag is negative")
            return int(frames[1] - frames[0]), (a, e, valid), (0, lag_step, top // lag_step + 1)

        if not per_molecule:
            stride, item, grid = one(molecule)
            return K.transition_counts_batch([item], grid, stride, device)[0]
        if not self.modular:
            raise ValueError("per_molecule needs a modular analysis (the store has one unit per frame)")
        keys = [int(m) for m in np.unique(self.unit_molecule)]
        each = [one(m) for m in keys]
        return dict(zip(keys, K.transition_counts_batch([i for _, i, _ in each], [g for _, _, g in each],
                                                        [s for s, _, _ in each], device)))

    # ---- persistence -----------------------------------------------------------------------
    # One file: a 4096-byte header (magic, then JSON: format, stages, record layout, and for every array its
    # dtype, length and byte offset), then the arrays as they lie in memory, each at a 4096-byte boundary.
    # Written with plain sequential writes and reopened as a memory map, so a result of any size is "open" as
    # soon as its header has been read and only the frames that are looked at are ever paged in.
    _ARRAYS = ("records", "extra", "unit_frame", "unit_molecule")

    def save(self, path) -> pathlib.Path:
        """Write the store to ``path`` (``.pwrec`` is appended when the name has no suffix)."""
        import json

        path = pathlib.Path(path)
        if path.suffix == "":
            path = path.with_suffix(".pwrec")
        arrays = {k: np.ascontiguousarray(getattr(self, k)) for k in self._ARRAYS}
        meta = {"format": FORMAT, "stages": self.stages, "record_dtype": repr(_lib.UNIT_OUT_DTYPE.descr),
                "extra_dtype": repr(_lib.EXTRA_WINDOW_DTYPE.descr), "arrays": {}}
        at = HEADER_BYTES
        for k, a in arrays.items():
            meta["arrays"][k] = {"count": int(len(a)), "itemsize": int(a.dtype.itemsize), "offset": at}
            at += -(-a.nbytes // HEADER_BYTES) * HEADER_BYTES
        head = MAGIC + json.dumps(meta).encode()
        if len(head) > HEADER_BYTES:
            raise ValueError("header too large")
        # the arrays go out with one sequential write() each, at their offsets (the gaps are holes that read as zeros,
        # the end is sized afterwards): what a plain dump of the records costs, on any disk.  (Filling the file through
        # a memory map and flushing it waits for the disk itself and took 2.8x a plain write on a slow one.)
        # ... into a temporary file beside the target, moved over it at the end: the arrays of a store that was LOADED
        # from `path` are read-only memory maps of that very file, and truncating it first would pull the pages from
        # under them (load, then save to the same name); a reader also never sees a half-written file
        import os
        import tempfile

        fd, tmp = tempfile.mkstemp(prefix=path.name + ".", suffix=".tmp", dir=str(path.parent))
        try:
            with os.fdopen(fd, "wb") as fh:
                fh.write(head)
                for k, a in arrays.items():
                    if a.nbytes:
                        fh.seek(meta["arrays"][k]["offset"])
                        fh.write(a.view(np.uint8).reshape(-1).data)
                fh.truncate(at)
            # mkstemp creates the file 0600: give it what open(path, "wb") would have given -- the mode of the file it
            # replaces, else 0666 less the umask
            try:
                mode = os.stat(path).st_mode & 0o7777
            except OSError:
                um = os.umask(0)
                os.umask(um)
                mode = 0o666 & ~um
            os.chmod(tmp, mode)
            os.replace(tmp, path)
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise
        return path

    @classmethod
    def load(cls, path, mmap: bool = True) -> "RecordStore":
        """Reopen a file written by :meth:`save`; ``mmap`` (default): the arrays are read-only memory maps."""
        import json

        path = pathlib.Path(path)
        if not path.exists() and path.suffix == "":
            path = path.with_suffix(".pwrec")
        with open(path, "rb") as fh:
            head = fh.read(HEADER_BYTES)
        if not head.startswith(MAGIC):
            raise ValueError(f"{path}: not a {FORMAT} file")
        meta = json.loads(head[len(MAGIC):].rstrip(b"\0").decode())
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a {FORMAT} file")
        if meta["record_dtype"] != repr(_lib.UNIT_OUT_DTYPE.descr) or meta["extra_dtype"] != repr(_lib.EXTRA_WINDOW_DTYPE.descr):
            raise ValueError(f"{path}: written with another record layout")
        dtypes = {"records": _lib.UNIT_OUT_DTYPE, "extra": _lib.EXTRA_WINDOW_DTYPE, "unit_frame": np.dtype(np.int64),
                  "unit_molecule": np.dtype(np.int64)}
        got = {}
        for k in cls._ARRAYS:
            info = meta["arrays"][k]
            if info["itemsize"] != dtypes[k].itemsize:
                raise ValueError(f"{path}: array {k} has another item size")
            if info["count"] == 0:
                got[k] = np.zeros(0, dtype=dtypes[k])
            elif mmap:
                got[k] = np.memmap(path, dtype=dtypes[k], mode="r", offset=info["offset"], shape=(info["count"],))
            else:
                got[k] = np.fromfile(path, dtype=dtypes[k], count=info["count"], offset=info["offset"])
        return cls(got["records"], got["unit_frame"], got["unit_molecule"], got["extra"], int(meta["stages"]))

    @classmethod
    def concatenate(cls, stores) -> "RecordStore":
        stores = list(stores)
        if not stores:
            return cls(np.zeros(0, dtype=_lib.UNIT_OUT_DTYPE), np.zeros(0, np.int64))
        extras, first = [], 0
        for s in stores:
            extras.append(engine.offset_extra(s.extra, first))
            first += len(s.records)
        return cls(np.concatenate([s.records for s in stores]), np.concatenate([s.unit_frame for s in stores]),
                   np.concatenate([s.unit_molecule for s in stores]), np.concatenate(extras), stores[0].stages)

    def select(self, frames) -> "RecordStore":
        """The store of a subset of frames (in the given order)."""
        spans = self.spans()
        idx = np.concatenate([np.arange(*spans[f]) for f in frames]) if len(frames) else np.zeros(0, np.int64)
        extra = self.extra
        if len(extra):
            pos = {int(u): k for k, u in enumerate(idx.tolist())}
            keep = [e for e in extra if int(e["unit"]) in pos]
            extra = np.array(keep, dtype=_lib.EXTRA_WINDOW_DTYPE)
            for e in extra:
                e["unit"] = pos[int(e["unit"])]
        return RecordStore(self.records[idx], self.unit_frame[idx], self.unit_molecule[idx], extra, self.stages)


class LazyAnalysis(MutableMapping):
    """``analysis_output`` backed by records: a frame's nested dict is built when it is first asked for.

    Keys keep the order in which frames were analysed or assigned.  ``dict(view)`` (or
    :meth:`materialise`) gives the plain dict the reference builds."""

    def __init__(self, initial=None):
        self._order: dict = {}          # frame -> None (insertion order)
        self._built: dict = {}          # frame -> dict (built, or assigned by hand)
        self._source: dict = {}         # frame -> RecordStore holding its records
        if initial:
            for k, v in dict(initial).items():
                self[k] = v

    def attach(self, store: RecordStore, frames=None) -> None:
        """Frames of ``store`` (all of them, or ``frames``) become entries of the view, replacing older ones."""
        for f in (store.spans().keys() if frames is None else frames):
            self._order.setdefault(f, None)
            self._built.pop(f, None)
            self._source[f] = store

    def record_store(self) -> RecordStore:
        """ONE store with the records of every record-backed frame of the view, in the view's order (frames
        assigned by hand have no records and are left out)."""
        groups: list = []
        for f in self._order:
            s = self._source.get(f)
            if s is None:
                continue
            if groups and groups[-1][0] is s:
                groups[-1][1].append(f)
            else:
                groups.append((s, [f]))
        if len(groups) == 1 and groups[0][1] == list(groups[0][0].spans()):
            return groups[0][0]                      # the whole of one analysis: no copy
        return RecordStore.concatenate(s.select(fr) for s, fr in groups)

    def __getitem__(self, frame):
        if frame in self._built:
            return self._built[frame]
        store = self._source.get(frame)
        if store is None:
            raise KeyError(frame)
        props = store.frame_properties(frame)
        self._built[frame] = props
        return props

    def __setitem__(self, frame, value) -> None:
        self._order.setdefault(frame, None)
        self._built[frame] = value
        self._source.pop(frame, None)

    def __delitem__(self, frame) -> None:
        if frame not in self._order:
            raise KeyError(frame)
        del self._order[frame]
        self._built.pop(frame, None)
        self._source.pop(frame, None)

    def __iter__(self):
        return iter(self._order)

    def __len__(self) -> int:
        return len(self._order)

    def __contains__(self, frame) -> bool:
        return frame in self._order

    def materialise(self) -> dict:
        return {f: self[f] for f in self._order}

    def __repr__(self) -> str:
        return f"LazyAnalysis({len(self._order)} frames, {len(self._built)} built)"
