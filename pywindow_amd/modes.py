"""Essential dynamics on the GPU: the covariance of superposed frames and its modes (``pw_covariance``,
``pw_project``, include/pywindow_amd.h).

After an RMSD plot and a clustering the next question about a trajectory is which collective motion of the atoms lies
behind them: which few modes carry the cage's flexibility, which atoms move, whether a window's diameter follows mode 1.
The tool is principal component analysis of the superposed Cartesian coordinates (Amadei et al. 1993; GROMACS's
``covar`` and ``anaeig``); its by-products are the per-atom RMSF and the atom-by-atom cross-correlation map.  The part
that scales with the trajectory -- the ``3n x 3n`` scatter matrix of ``F`` aligned frames, ``F (3n)^2`` FP64
multiply-adds -- runs on the GPU with the rotation of ``pw_superpose`` applied as the frames are loaded, and so do the
projections.  The mean, the scatter matrix and the projections given the vectors are defined to the bit
(pywindow_amd/csrc/pw_cov.hpp): the device and the explicit host path (``device=-1``) return the same bytes.  The eigen
decomposition of the ``3n x 3n`` covariance is ``numpy.linalg.eigh`` on the host -- a ``504 x 504`` solve is not where
the time goes -- so eigenvalues and modes are LAPACK's and NOT defined to the bit.  The reference has no counterpart.

* :func:`covariance`, :func:`project` -- any matrix, with or without transforms.
* :func:`principal_modes` -- frames ``(F, n, 3)`` to a :class:`Modes`.
* ``DLPOLY.essential_dynamics`` (trajectory.py) takes the frames from a trajectory.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib, engine
from . import superposition as SP

__all__ = ["Modes", "covariance", "project", "principal_modes"]

#: ``reference="mean"``: the iteration ends when the mean structure moves by less than this times its radius of
#: gyration (root mean square over the atoms), or after ``MEAN_ROUNDS`` superpositions onto a mean
MEAN_TOLERANCE = 1e-10
MEAN_ROUNDS = 5


def _matrix(X) -> np.ndarray:
    x = np.ascontiguousarray(X, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("X: a (T, D) matrix, T >= 1 and D >= 1")
    return x


def _rows(transforms, T: int):
    if transforms is None:
        return None
    tr = np.ascontiguousarray(transforms, dtype=_lib.SUPERPOSE_OUT_DTYPE).reshape(-1)
    if len(tr) != T:
        raise ValueError("transforms: one row of pw_superpose per row of X")
    return tr


def covariance(X, transforms=None, device=None, scatter: bool = True):
    """``(mean, scatter)`` of the rows of ``X`` (T, D): ``mean`` (D) the column mean and ``scatter`` (D, D) the sums
    ``sum_t (y_ta - mean_a)(y_tb - mean_b)`` -- NOT divided by ``T - 1``; the covariance is ``scatter / (T - 1)``.
    ``transforms``: ``None``, or T rows of ``pw_superpose`` (``SUPERPOSE_OUT_DTYPE``); then D is a multiple of 3, a row
    is D / 3 points and each point is taken as ``R (x - centre_mobile) + centre_target``.  ``scatter=False``: the mean
    only, and ``None`` in place of the matrix.  Defined to the bit (module docstring).  ``device``: the HIP ordinal
    (``None``: the process's); ``-1`` the explicit host path.  A value that is not finite or D above
    ``_lib.COV_MAX_D``: ``ValueError``."""
    x = _matrix(X)
    T, D = x.shape
    jobs = np.zeros(1, dtype=_lib.COV_JOB_DTYPE)
    jobs["T"], jobs["D"] = T, D
    jobs["transform_first"] = -1 if transforms is None else 0
    jobs["s_first"] = 0 if scatter else -1
    mean, s = engine.context(device).covariance(jobs, x, _rows(transforms, T))
    return mean, (s.reshape(D, D) if scatter else None)


def project(X, mean, vectors, transforms=None, device=None) -> np.ndarray:
    """``P`` (T, k) with ``P[t, j] = sum_a (y_ta - mean_a) vectors[j, a]`` for the rows of ``X`` (T, D), ``mean`` (D)
    and ``vectors`` (k, D), ``k >= 1``; ``transforms`` and ``device`` as for :func:`covariance`.  Defined to the bit."""
    x = _matrix(X)
    T, D = x.shape
    m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(vectors, dtype=np.float64)
    v = v.reshape(1, -1) if v.ndim == 1 else v.reshape(len(v), -1)
    if len(m) != D or v.shape[1] != D or len(v) < 1:
        raise ValueError("mean: D entries; vectors: (k, D), k >= 1")
    jobs = np.zeros(1, dtype=_lib.PROJECT_JOB_DTYPE)
    jobs["T"], jobs["D"], jobs["k"] = T, D, len(v)
    jobs["transform_first"] = -1 if transforms is None else 0
    return engine.context(device).project(jobs, x, m, v, _rows(transforms, T)).reshape(T, len(v))


@dataclasses.dataclass(frozen=True)
class Modes:
    """The essential dynamics of ``F`` frames of ``n`` atoms.  ``mean_structure``, ``scatter`` and ``projection`` (given
    ``vectors``) are defined to the bit; ``eigenvalues``, ``explained`` and ``vectors`` come from LAPACK."""

    mean_structure: np.ndarray      # (n, 3) the mean of the superposed frames
    eigenvalues: np.ndarray         # (3n,) of scatter / (F - 1), descending
    explained: np.ndarray           # (3n,) eigenvalues / their sum (the trace); zeros when nothing moves
    vectors: np.ndarray             # (n_modes, n, 3) orthonormal; the component of largest magnitude is positive
    projection: np.ndarray          # (F, n_modes) of the centred, superposed frames on the modes
    rmsf: np.ndarray                # (n,) sqrt(trace of the atom's 3 x 3 diagonal block of scatter / F)
    cross_correlation: np.ndarray   # (n, n) trace of block (i, j) / sqrt(trace (i, i) trace (j, j)); 0 for a frozen atom
    scatter: np.ndarray             # (3n, 3n)
    transforms: np.ndarray          # (F,) SUPERPOSE_OUT_DTYPE: the superposition the scatter matrix was taken with
    frames: np.ndarray              # (F,) the frame number of every row
    rounds: int                     # superpositions onto a mean structure (reference="mean"); 0 for a frame

    @property
    def n_modes(self) -> int:
        return len(self.vectors)

    def series(self, j: int):
        """``(values, valid)`` of mode ``j`` over the frames -- its projection and an all-true mask -- ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle` and
        :func:`pywindow_amd.transition_counts`."""
        j = int(j)
        if not 0 <= j < self.n_modes:
            raise IndexError("series: not a mode")
        return self.projection[:, j].copy(), np.ones(len(self.projection), dtype=bool)


def _sign_rule(v: np.ndarray) -> np.ndarray:
    """``v`` or ``-v``: the component of largest magnitude, the lowest index among equals, is positive."""
    flat = v.reshape(-1)
    return -v if flat[int(np.argmax(np.abs(flat)))] < 0.0 else v


def _atom_blocks(scatter: np.ndarray, n: int) -> np.ndarray:
    """``(n, n)``: the trace of every 3 x 3 block of ``scatter``, summed ``xx + yy + zz`` in that order."""
    s = scatter.reshape(n, 3, n, 3)
    return (s[:, 0, :, 0] + s[:, 1, :, 1]) + s[:, 2, :, 2]


def principal_modes(coords, weights=None, reference="mean", n_modes: int = 10, device=None, frames=None,
                    vectors=None) -> Modes:
    """The essential dynamics of the frames ``coords`` (F, n, 3), F >= 2: every frame is superposed by
    ``pywindow_amd.superposition.superpose_onto`` (``weights``: ``None`` or one per atom; they weigh the superposition
    only, the covariance is the plain Cartesian one), the scatter matrix of the superposed coordinates is taken by
    ``pw_covariance`` with those rotations applied on the fly, the covariance ``scatter / (F - 1)`` is decomposed by
    ``numpy.linalg.eigh`` on the host, and the frames are projected on the ``n_modes`` leading modes by ``pw_project``.

    ``reference="mean"`` iterates: superpose onto frame 0 and take the mean structure; superpose onto the mean and take
    it again; repeat until the mean moves by less than ``MEAN_TOLERANCE`` times its radius of gyration or
    ``MEAN_ROUNDS`` rounds have passed.  ``Modes.rounds`` is the number of rounds taken.  ``reference=<int>`` is one
    pass onto that frame.

    The mean structure, the scatter matrix and the projections given the vectors are defined to the bit; the
    eigenvalues and the modes are LAPACK's and are not.  ``vectors`` (n_modes, n, 3), when given, are taken as the
    modes as they are (no sign rule, ``n_modes`` is their number): for comparing two paths without LAPACK in between.
    ``frames``: the frame number of every row (default ``arange(F)``)."""
    x = np.ascontiguousarray(coords, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3 or x.shape[1] < 1 or x.shape[0] < 2:
        raise ValueError("coords: (F, n, 3) coordinates, F >= 2 and n >= 1")
    F, n = x.shape[:2]
    D = 3 * n
    if D > _lib.COV_MAX_D:
        raise ValueError(f"coords: at most {_lib.COV_MAX_D // 3} atoms")
    if vectors is not None:
        vectors = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, n, 3)
        n_modes = len(vectors)
    n_modes = int(n_modes)
    if not 1 <= n_modes <= D:
        raise ValueError("n_modes: 1 .. 3 n")
    frames = np.arange(F, dtype=np.int64) if frames is None else np.array(frames, dtype=np.int64).reshape(-1)
    if len(frames) != F:
        raise ValueError("frames: one frame number per frame of coords")
    X = x.reshape(F, D)

    rounds = 0
    if isinstance(reference, str):
        if reference != "mean":
            raise ValueError('reference: "mean" or a frame of coords')
        rows = SP.superpose_onto(x, 0, weights, device)
        mean, _ = covariance(X, rows, device, scatter=False)
        while rounds < MEAN_ROUNDS:
            target = mean.reshape(1, n, 3)
            rows = SP.superpose_onto(np.concatenate([x, target]), F, weights, device)[:F]
            new, _ = covariance(X, rows, device, scatter=False)
            rounds += 1
            centred = new.reshape(n, 3) - new.reshape(n, 3).mean(axis=0)
            gyration = float(np.sqrt((centred ** 2).sum() / n))
            moved = float(np.sqrt(((new - mean) ** 2).sum() / n))
            mean = new
            if moved < MEAN_TOLERANCE * gyration or moved == 0.0:
                break
    else:
        rows = SP.superpose_onto(x, int(reference), weights, device)
    rows = np.ascontiguousarray(rows)
    mean, scatter = covariance(X, rows, device)

    values, columns = np.linalg.eigh(scatter / (F - 1))
    order = np.argsort(-values, kind="stable")
    values = values[order]
    if vectors is None:
        vectors = np.stack([_sign_rule(columns[:, j]) for j in order[:n_modes]]).reshape(n_modes, n, 3)
    total = float(values.sum())
    explained = values / total if total > 0.0 else np.zeros_like(values)
    projection = project(X, mean, vectors.reshape(n_modes, D), rows, device)

    blocks = _atom_blocks(scatter, n)
    diagonal = np.diagonal(blocks).copy()
    rmsf = np.sqrt(diagonal / F)
    scale = np.sqrt(np.outer(diagonal, diagonal))
    cross = np.divide(blocks, scale, out=np.zeros_like(blocks), where=scale > 0.0)
    return Modes(mean.reshape(n, 3), values, explained, vectors, projection, rmsf, cross, scatter, rows, frames, rounds)
