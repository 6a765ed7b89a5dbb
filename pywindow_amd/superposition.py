"""Least-squares superposition of point sets on the GPU (``pw_superpose``, include/pywindow_amd.h).

Bringing a frame into the orientation of a reference is the first step of every question about ONE window of a
tumbling cage (pywindow_amd/tracks.py), the per-frame RMSD to a reference the first plot anyone makes of a trajectory,
and the pairwise RMSD matrix the input of every conformational clustering.  The rotation is Horn's: the eigenvector of
the largest eigenvalue of a symmetric 4 x 4 built from the weighted covariance of the centred sets, taken by a cyclic
Jacobi iteration; always a proper rotation (det +1), also for a mirror-image target and for degenerate sets, where it
is *a* minimiser and ``eigenvalues[0] - eigenvalues[1]`` is small and says so.  The RMSD is a direct sum of residuals.
The result is defined to the bit (pywindow_amd/csrc/pw_superpose.hpp): the device and the explicit host path
(``device=-1``) return the same bytes.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib, engine

#: jobs of one ``pw_superpose`` call of :func:`rmsd_matrix`: 152 bytes a result row, 40 a job
MATRIX_SLAB = 1 << 20


@dataclass(frozen=True)
class Superposition:
    """``rotation @ (x - centre_mobile) + centre_target`` lies on the target in the least-squares sense."""

    rotation: np.ndarray        # (3, 3), det +1
    centre_mobile: np.ndarray   # (3,) weighted centroid of the mobile set
    centre_target: np.ndarray   # (3,)
    rmsd: float                 # sqrt(sum w |R (x - cx) - (y - cy)|^2 / sum w)
    eigenvalues: np.ndarray     # (2,) the two largest eigenvalues of Horn's matrix, descending
    sweeps: int                 # Jacobi sweeps taken

    def apply(self, xyz) -> np.ndarray:
        """``xyz`` (..., 3) moved as the mobile set was."""
        x = np.asarray(xyz, dtype=np.float64)
        return (x - self.centre_mobile) @ self.rotation.T + self.centre_target

    @classmethod
    def from_row(cls, row) -> "Superposition":
        return cls(np.array(row["rotation"]), np.array(row["centre_mobile"]), np.array(row["centre_target"]),
                   float(row["rmsd"]), np.array(row["lambda"]), int(row["sweeps"]))


def _points(a, what: str) -> np.ndarray:
    x = np.ascontiguousarray(a, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 3 or len(x) < 1:
        raise ValueError(f"{what}: (n, 3) coordinates, n >= 1")
    return x


def superpose_rows(items, device=None) -> np.ndarray:
    """The raw ``SUPERPOSE_OUT_DTYPE`` rows, one per ``(mobile, target, weights | None)`` of ``items``, from ONE
    ``pw_superpose`` call."""
    xyz, wts, jobs = [], [], []
    at = 0
    weighted = False
    for k, (mobile, target, weights) in enumerate(items):
        m, t = _points(mobile, "mobile"), _points(target, "target")
        if m.shape != t.shape:
            raise ValueError("mobile and target: the same number of points")
        n = len(m)
        if weights is None:
            w, first = np.zeros(2 * n), -1
        else:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if len(w) != n:
                raise ValueError("weights: one per point")
            w, first, weighted = np.concatenate([w, np.zeros(n)]), at, True
        jobs.append((at, at + n, first, n, k))
        xyz += [m, t]
        wts.append(w)
        at += 2 * n
    if not jobs:
        return np.zeros(0, dtype=_lib.SUPERPOSE_OUT_DTYPE)
    rec = np.array(jobs, dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    return engine.context(device).superpose(rec, np.concatenate(xyz), np.concatenate(wts) if weighted else None)


def superpose_batch(items, device=None) -> list:
    """One :class:`Superposition` per ``(mobile, target, weights | None)`` of ``items`` -- ``mobile`` and ``target``
    (n, 3), ``weights`` (n) not negative and not all zero -- all from ONE ``pw_superpose`` call.  ``device``: the HIP
    ordinal (``None``: the process's); ``-1`` the explicit host path."""
    return [Superposition.from_row(r) for r in superpose_rows(list(items), device)]


def superpose(mobile, target, weights=None, device=None) -> Superposition:
    """The rotation and translation that bring ``mobile`` (n, 3) onto ``target`` (n, 3) with the least weighted sum of
    squared distances, and the RMSD left: see :class:`Superposition`.  A coordinate that is not finite, a weight that
    is negative or not finite, or weights that sum to 0: ``ValueError``."""
    return superpose_batch([(mobile, target, weights)], device)[0]


def _frames(coords, weights):
    x = np.ascontiguousarray(coords, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3 or x.shape[1] < 1:
        raise ValueError("coords: (F, n, 3) coordinates, n >= 1")
    F, n = x.shape[:2]
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if len(w) != n:
            raise ValueError("weights: one per atom")
        w = np.concatenate([w, np.zeros(max(F * n - n, 0))])      # (one entry per row of xyz; every job reads the first n)
    return x, w, F, n


def superpose_onto(coords, reference: int = 0, weights=None, device=None) -> np.ndarray:
    """Every frame of ``coords`` (F, n, 3) onto frame ``reference``: the raw ``SUPERPOSE_OUT_DTYPE`` rows, one per
    frame, from one ``pw_superpose`` call over one upload of the coordinates."""
    x, w, F, n = _frames(coords, weights)
    if not 0 <= int(reference) < F:
        raise ValueError("reference: not a frame of coords")
    jobs = np.zeros(F, dtype=_lib.SUPERPOSE_JOB_DTYPE)
    jobs["mobile_first"] = np.arange(F, dtype=np.int64) * n
    jobs["target_first"] = int(reference) * n
    jobs["weight_first"] = -1 if w is None else 0
    jobs["n"] = n
    jobs["out"] = np.arange(F)
    return engine.context(device).superpose(jobs, x.reshape(-1, 3), w)


def rmsd_matrix(coords, weights=None, device=None) -> np.ndarray:
    """The symmetric (F, F) matrix of the least-squares RMSD between every two frames of ``coords`` (F, n, 3): the
    ``F (F - 1) / 2`` jobs ``i < j`` (frame ``i`` onto frame ``j``) over the coordinates as ONE array that every job
    indexes, in slabs of ``MATRIX_SLAB`` jobs so that the result rows of a call stay bounded; the diagonal is exactly
    0 and ``[j, i]`` is a copy of ``[i, j]``."""
    x, w, F, n = _frames(coords, weights)
    out = np.zeros((F, F))
    i, j = np.triu_indices(F, 1)
    ctx = engine.context(device)
    flat = x.reshape(-1, 3)
    for lo in range(0, len(i), MATRIX_SLAB):
        a, b = i[lo:lo + MATRIX_SLAB], j[lo:lo + MATRIX_SLAB]
        jobs = np.zeros(len(a), dtype=_lib.SUPERPOSE_JOB_DTYPE)
        jobs["mobile_first"], jobs["target_first"] = a * n, b * n
        jobs["weight_first"] = -1 if w is None else 0
        jobs["n"] = n
        jobs["out"] = np.arange(len(a))
        rows = ctx.superpose(jobs, flat, w)
        out[a, b] = out[b, a] = rows["rmsd"]
    return out
