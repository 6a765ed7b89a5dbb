"""Conformational clustering of frames on the GPU (``pw_cluster_gromos``, include/pywindow_amd.h).

A matrix of pairwise RMSDs (:func:`pywindow_amd.rmsd_matrix`) answers nothing by itself; the questions are which
conformations a cage visits, which frame stands for each of them and in which conformation a given frame is.  The method
is GROMACS's ``gromos`` (Daura et al. 1999), the usual choice for MD trajectories: count every frame's neighbours within
a cutoff, take the frame with the most as the centre of a cluster with all its neighbours, remove them, repeat.  Ties go
to the smallest index, so the result is defined: every output is an integer, the same on the device and on the explicit
host path (``device=-1``).  The reference has no counterpart.

A label per frame is a state series: :meth:`Clusters.state_series` goes straight into
:func:`pywindow_amd.transition_counts`, which makes a conformational Markov model of it.

* :func:`cluster_frames` -- one cutoff; :func:`cluster_frames_scan` -- many cutoffs over one matrix, one call.
* ``DLPOLY.conformations`` (trajectory.py) takes the matrix from the frames of a trajectory.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine

__all__ = ["Clusters", "cluster_frames", "cluster_frames_scan"]


@dataclasses.dataclass(frozen=True)
class Clusters:
    """``labels[i]`` is the cluster of row ``i`` of the matrix, ``centres[k]`` the row that stands for cluster ``k`` and
    ``sizes[k]`` its number of members; clusters are numbered in the order found, so ``sizes`` does not increase.
    ``frames`` is ``None`` or the frame number of every row (``DLPOLY.conformations``)."""

    labels: np.ndarray          # (n,) int32
    centres: np.ndarray         # (n_clusters,) int32
    sizes: np.ndarray           # (n_clusters,) int32
    cutoff: float
    frames: np.ndarray | None = None

    @property
    def n_clusters(self) -> int:
        return len(self.centres)

    def members(self, k: int) -> np.ndarray:
        """The rows of cluster ``k``, ascending (``frames[members(k)]`` are their frame numbers)."""
        k = int(k)
        if not 0 <= k < self.n_clusters:
            raise IndexError("members: not a cluster")
        return np.flatnonzero(self.labels == k)

    def state_series(self, max_states: int = 16):
        """``(series, edges)`` for :func:`pywindow_amd.transition_counts`: the labels as float64 with the clusters
        ``>= max_states - 1`` merged into the last state, and ``edges = 0.5 + arange(states - 1)`` with ``states =
        min(n_clusters, max_states)``, which cut that series back into its states."""
        max_states = int(max_states)
        if not 1 <= max_states <= _lib.TRANS_MAX_STATES:
            raise ValueError(f"max_states: 1 .. {_lib.TRANS_MAX_STATES}")
        states = max(min(self.n_clusters, max_states), 1)
        return np.minimum(self.labels, states - 1).astype(np.float64), 0.5 + np.arange(states - 1, dtype=np.float64)


def _matrix(dist) -> np.ndarray:
    d = np.ascontiguousarray(dist, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("dist: a square (n, n) matrix")
    if len(d) > _lib.CLUSTER_MAX_N:
        raise ValueError(f"dist: at most {_lib.CLUSTER_MAX_N} frames")
    return d


def cluster_frames_scan(dist, cutoffs, device=None, frames=None) -> list:
    """One :class:`Clusters` per cutoff of ``cutoffs`` over the ``(n, n)`` matrix ``dist``, all from ONE
    ``pw_cluster_gromos`` call: the matrix goes to the device once.  Only the strict upper triangle of ``dist`` is
    read; a NaN there or a NaN cutoff: ``ValueError``.  ``device``: the HIP ordinal (``None``: the process's); ``-1``
    the explicit host path."""
    d = _matrix(dist)
    cut = np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
    if np.isnan(cut).any():
        raise ValueError("cutoffs: a cutoff is NaN")
    n = len(d)
    if frames is not None:
        frames = np.array(frames, dtype=np.int64).reshape(-1)
        if len(frames) != n:
            raise ValueError("frames: one frame number per row of dist")
    if not len(cut):
        return []
    jobs = np.zeros(len(cut), dtype=_lib.CLUSTER_JOB_DTYPE)
    jobs["n"] = n
    jobs["cutoff"] = cut
    jobs["out_first"] = np.arange(len(cut), dtype=np.int64) * n
    labels, centres, sizes, found = engine.context(device).cluster_gromos(jobs, d)
    out = []
    for q, c in enumerate(cut.tolist()):
        k = int(found[q])
        out.append(Clusters(labels[q * n:(q + 1) * n].copy(), centres[q * n:q * n + k].copy(), sizes[q * n:q * n + k].copy(),
                            c, frames))
    return out


def cluster_frames(dist, cutoff, device=None, frames=None) -> Clusters:
    """The gromos clustering of the frames behind the ``(n, n)`` distance matrix ``dist`` at ``cutoff``: see
    :class:`Clusters`.  Frames ``i != j`` are neighbours iff ``dist[min(i, j), max(i, j)] <= cutoff``."""
    return cluster_frames_scan(dist, [float(cutoff)], device, frames)[0]
