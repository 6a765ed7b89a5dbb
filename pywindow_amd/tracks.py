"""Window identity: which window of a frame is which site of the cage.

A record holds its windows in the order the search found them, and the cage tumbles from frame to frame.  Once every
frame has been brought into one orientation (pywindow_amd/superposition.py), the direction of a window from the
centre of the cage says which opening it is.  Host side, numpy; every result is an integer or a copy of a record value.

ASSIGNMENT, defined exactly.  For unit ``u`` the direction of window ``w`` is ``rotation[u] @ (win_c[u, w] - centre[u])``
divided by its length (the windows beyond what a record holds included).  All cosines of the unit's windows against the
``sites`` are computed; repeatedly the largest remaining cosine is taken -- ties go to the lower window index, then to
the lower site index --; if it is ``>= min_cosine`` the pair is assigned and the window and the site are struck,
otherwise the unit is done.  Windows left over get ``-1``.  (Greedy, not the optimal assignment.)
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass(frozen=True)
class WindowTracks:
    """``site_of``: the site of every window in ``samples("windows")`` order, ``-1`` for none.  ``diameter`` (T, S):
    the diameter of the window at site ``j`` along the frame axis ``frames`` (that of :meth:`RecordStore.series`), NaN
    where ``valid`` (T, S) is false -- the frame is absent or no window of it was assigned to the site.
    ``n_unassigned``: the windows with ``-1``; ``occupancy[j]``: the fraction of the present frames in which site ``j``
    has a window.  ``sites`` (S, 3) and ``min_cosine`` as used."""

    site_of: np.ndarray
    diameter: np.ndarray
    valid: np.ndarray
    frames: np.ndarray
    n_unassigned: int
    occupancy: np.ndarray
    sites: np.ndarray
    min_cosine: float


def default_min_cosine(sites) -> float:
    """``cos(half the smallest angle between two sites)``: a window nearer a midpoint than any site belongs to no
    site.  One site: 0."""
    s = np.asarray(sites, dtype=np.float64)
    if len(s) < 2:
        return 0.0
    c = np.clip(s @ s.T, -1.0, 1.0)
    largest = float(c[np.triu_indices(len(s), 1)].max())
    return float(np.cos(0.5 * np.arccos(largest)))


def assign(cosines, min_cosine: float) -> np.ndarray:
    """The rule of the module docstring on a (windows, sites) matrix of cosines: the site of every window or ``-1``."""
    c = np.array(cosines, dtype=np.float64)
    out = np.full(c.shape[0], -1, dtype=np.int64)
    if c.size == 0:
        return out
    for _ in range(min(c.shape)):
        k = int(np.argmax(c))                  # (the first maximum in row-major order: lower window, then lower site)
        w, s = divmod(k, c.shape[1])
        if not c[w, s] >= min_cosine:
            break
        out[w] = s
        c[w, :] = -np.inf
        c[:, s] = -np.inf
    return out


def _unit(v):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v / np.where(n > 0.0, n, 1.0)


def window_directions(store, rotation, centre):
    """``(unit directions (K, 3), diameters (K), unit of every window (K))`` in ``samples("windows")`` order."""
    recs = store.records
    n = len(recs)
    rotation = np.asarray(rotation, dtype=np.float64).reshape(-1, 3, 3)
    centre = np.asarray(centre, dtype=np.float64).reshape(-1, 3)
    if len(rotation) != n or len(centre) != n:
        raise ValueError("one rotation and one centre per unit of the store")
    d, unit = store._samples_by_unit("windows")
    held = np.clip(recs["n_windows"], 0, _lib.W_MAX)
    mask = np.arange(_lib.W_MAX)[None, :] < held[:, None]
    u, index = np.nonzero(mask)
    c = np.array(recs["win_c"][mask], dtype=np.float64).reshape(-1, 3)
    if len(store.extra):
        u = np.concatenate([u, store.extra["unit"].astype(np.int64)])
        index = np.concatenate([index, store.extra["index"].astype(np.int64)])
        c = np.concatenate([c, np.asarray(store.extra["c"], dtype=np.float64).reshape(-1, 3)])
        order = np.lexsort((index, u))
        u, c = u[order], c[order]
    assert np.array_equal(u, unit)
    v = np.einsum("kab,kb->ka", rotation[unit], c - centre[unit])
    return _unit(v), d, unit


def track_windows(store, rotation, centre, sites=None, min_cosine=None, reference_unit: int = 0) -> WindowTracks:
    """Follow every window of a non-modular ``store`` through the frames: see the module docstring.  ``rotation`` (U,
    3, 3) and ``centre`` (U, 3) bring unit ``u`` into the reference orientation (``DLPOLY.superposition``).  ``sites``
    (S, 3): unit vectors in that orientation; by default the directions of the windows of unit ``reference_unit``.
    ``min_cosine``: by default :func:`default_min_cosine` of the sites."""
    if store.modular:
        raise ValueError("window tracks need one unit per frame (a modular store holds several molecules a frame)")
    dirs, d, unit = window_directions(store, rotation, centre)
    if sites is None:
        sites = dirs[unit == int(reference_unit)]
        if not len(sites):
            raise ValueError("the reference unit has no windows: give the sites")
    sites = _unit(np.asarray(sites, dtype=np.float64).reshape(-1, 3))
    S = len(sites)
    if S < 1:
        raise ValueError("sites: at least one")
    cut = default_min_cosine(sites) if min_cosine is None else float(min_cosine)
    site_of = np.full(len(d), -1, dtype=np.int64)
    count = np.bincount(unit, minlength=len(store.records))
    first = np.cumsum(count) - count
    cos = dirs @ sites.T
    for u in np.flatnonzero(count).tolist():
        site_of[first[u]:first[u] + count[u]] = assign(cos[first[u]:first[u] + count[u]], cut)
    # the frame axis of RecordStore.series
    f = np.asarray(store.unit_frame)
    if len(np.unique(f)) < 2:
        raise ValueError("a series needs at least two frames")
    if len(np.unique(f)) != len(f):
        raise ValueError("a frame appears more than once")
    f0 = int(f.min())
    stride = int(np.gcd.reduce(f - f0))
    at = (f - f0) // stride
    frames = f0 + stride * np.arange(int(at.max()) + 1, dtype=np.int64)
    diameter = np.full((len(frames), S), np.nan)
    valid = np.zeros((len(frames), S), dtype=bool)
    has = site_of >= 0
    diameter[at[unit[has]], site_of[has]] = d[has]
    valid[at[unit[has]], site_of[has]] = True
    return WindowTracks(site_of, diameter, valid, frames, int((~has).sum()), valid.sum(axis=0) / float(len(f)), sites, cut)
