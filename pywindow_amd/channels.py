"""The pore network of a crystal cell on the GPU: the periodic components of its void and in how many dimensions each
of them percolates (``pw_channels``, include/pywindow_amd.h; the definition and its proofs in
pywindow_amd/csrc/pw_channels.hpp).

Every other grid analysis here looks at one cage cut out of its surroundings.  What makes a porous molecular crystal
porous is the network: are the cavities connected, in how many dimensions, for a guest of which size, and how much of the
void is accessible through that network rather than locked in pockets.  The cell is cut into at most 64 voxels along each
of its vectors; a voxel is open when a probe's centre fits there; the open voxels fall into components under periodic
neighbours, and a component is a pocket (rank 0), a channel (1), a layer (2) or a network (3) according to how it connects
to its own periodic images.  Every output of the kernel is an integer, so the device and the explicit host path
(``device=-1``) return the same bytes.  One limit is part of the definition: a component all of whose windings through the
cell are even (a double helix of pitch two cells) reads as a pocket.  The reference has no counterpart.

* :func:`channel_network` -- one cell; :func:`channel_network_batch` -- frames x probes in ONE call; :class:`Channels` --
  the result, whose :meth:`Channels.series` goes into :func:`pywindow_amd.time_correlation` and the other statistical
  entries, and whose ``accessible_words`` are a region for :func:`pywindow_amd.guest_affinity` and
  :func:`pywindow_amd.surface_area`.
* ``MolecularSystem.calculate_channels`` (molecular.py) for a loaded cell and ``DLPOLY.channels`` (trajectory.py) for a
  periodic trajectory.
"""

from __future__ import annotations

import dataclasses
import itertools
import math

import numpy as np

from . import _lib, engine
from .cavity import unpack_mask

__all__ = ["Channels", "channel_network", "channel_network_batch"]

_SERIES = ("accessible_volume", "void_fraction", "dimensionality", "limiting_probe")
#: an image of an atom is kept iff it lies within the cell grown by IMAGE_SAFETY times the atom's reach (in fractional
#: units of every cell vector) and a hair: the product and the division that make the margin round, the cull may not
IMAGE_SAFETY = 1.001
#: the 27 cell shifts of the images, in the order in which the images of an atom are listed
SHIFTS = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))


def triangular_lattice(lattice):
    """``(R, Q)``: the lattice (columns as vectors, the convention of ``system["lattice"]``) in the triangular form the
    kernel takes -- first vector along x, second in the xy plane, positive diagonal -- and the orthogonal ``Q`` with
    ``lattice = Q @ R``.  A lattice already in that form is returned as it is with ``Q = 1``; any other is rotated by
    the QR factorisation of numpy with the signs fixed so that the diagonal is positive (a left-handed cell is
    mirrored, which changes no distance)."""
    L = np.asarray(lattice, dtype=np.float64)
    if L.shape != (3, 3) or not np.isfinite(L).all():
        raise ValueError("lattice: a finite (3, 3) array, columns as vectors")
    if L[1, 0] == 0.0 and L[2, 0] == 0.0 and L[2, 1] == 0.0 and (np.diag(L) > 0.0).all():
        return L.copy(), np.eye(3)
    Q, R = np.linalg.qr(L)
    sign = np.where(np.diag(R) < 0.0, -1.0, 1.0)
    Q, R = Q * sign[None, :], R * sign[:, None]
    if not (np.diag(R) > 0.0).all():
        raise ValueError("lattice: the three vectors do not span a cell")
    return np.triu(R), Q


def cell_grid(R, spacing: float):
    """``((nx, ny, nz), origin, step)`` of the cell ``R`` (triangular) at ``spacing``: ``n_k = ceil(|v_k| / spacing)``
    voxels along vector ``k``, a step of ``v_k / n_k``, and the centre of voxel (0, 0, 0) half a step along each
    vector from the cell's corner.  More than 64 voxels along a vector: ``ValueError`` that names the smallest spacing
    that fits -- the grid is never coarsened silently."""
    lengths = np.sqrt((R * R).sum(axis=0))
    n = np.maximum(np.ceil(lengths / spacing).astype(np.int64), 1)
    if (n > _lib.CAVITY_MAX_G).any():
        need = float(lengths.max()) / _lib.CAVITY_MAX_G
        raise ValueError(f"channel_network: a cell vector of length {float(lengths.max()):.6g} needs {int(n.max())} voxels at "
                         f"spacing {spacing:.6g}, more than {_lib.CAVITY_MAX_G}: the smallest spacing that fits is {need:.6g}")
    S = R / n[None, :].astype(np.float64)
    step = np.array([S[0, 0], S[0, 1], S[1, 1], S[0, 2], S[1, 2], S[2, 2]])
    return tuple(int(v) for v in n), 0.5 * S.sum(axis=1), step


def cell_images_many(xyz, radii, cells, probe: float, cull: bool = True, chunk: int = 32, sources: bool = False):
    """:func:`cell_images` for ``T`` frames ``xyz`` ``(T, n, 3)`` in their cells ``cells`` ``(T, 3, 3)``:
    ``(xyz, radii, counts)``, the images of frame after frame and how many each frame has.  The same expression for
    every frame, evaluated ``chunk`` frames at a time.  ``sources=True``: a fourth array, for every image the index
    ``0 .. n - 1`` of the atom it is an image of (what an entry with other per-atom rows than radii repeats them by)."""
    x = np.asarray(xyz, dtype=np.float64)
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    R = np.asarray(cells, dtype=np.float64)
    inv = np.linalg.inv(R)
    width = 1.0 / np.sqrt((inv * inv).sum(axis=2))                   # (T, 3): between the faces k, 1 / |row k of the inverse|
    reach = r + probe
    if len(r) and len(R) and float(reach.max()) > float(width.min()):
        raise ValueError(f"channel_network: a reach of {float(reach.max()):.6g} (radius + probe) is above the cell's smallest "
                         f"perpendicular width {float(width.min()):.6g}: a thin cell, more than 27 images would matter")
    steps = np.array([-1.0, 0.0, 1.0])
    atoms, kept, counts, source = [], [], [], []
    for lo in range(0, len(x), chunk):
        hi = min(lo + chunk, len(x))
        frac = np.matmul(x[lo:hi], inv[lo:hi].transpose(0, 2, 1))
        frac = frac - np.floor(frac)
        if cull:
            # images = frac + SHIFTS and the test, axis by axis: shift s = 9 sa + 3 sb + sc is kept iff all three are
            margin = (IMAGE_SAFETY * reach[None, :, None] / width[lo:hi, None, :] + 1e-9)[:, :, None, :]
            moved = frac[:, :, None, :] + steps[None, None, :, None]                 # (t, n, 3 shifts, 3 axes)
            ok = (moved >= -margin) & (moved <= 1.0 + margin)
            keep = (ok[:, :, :, None, None, 0] & ok[:, :, None, :, None, 1] & ok[:, :, None, None, :, 2]).reshape(hi - lo, -1, 27)
        else:
            keep = np.ones(frac.shape[:2] + (27,), dtype=bool)
        t, n, shift = np.nonzero(keep)
        cells_t = R[lo:hi].transpose(0, 2, 1)
        atoms.append(np.matmul(frac, cells_t)[t, n] + np.matmul(SHIFTS[None], cells_t)[t, shift])
        kept.append(r[n])
        source.append(n)
        counts.append(keep.sum(axis=(1, 2)))
    if not atoms:
        none = (np.zeros((0, 3)), np.zeros(0), np.zeros(0, dtype=np.int64))
        return none + (np.zeros(0, dtype=np.int64),) if sources else none
    made = (np.ascontiguousarray(np.concatenate(atoms)), np.ascontiguousarray(np.concatenate(kept)), np.concatenate(counts))
    return made + (np.concatenate(source).astype(np.int64),) if sources else made


def cell_images(xyz, radii, R, probe: float, cull: bool = True):
    """``(xyz, radii)`` of the periodic images of the atoms (already in the frame of the triangular cell ``R``) that a
    voxel of the cell can feel: every atom is wrapped into the cell, its 27 images
    ``wrapped + SHIFTS @ cell`` are listed in the order of ``SHIFTS``, and an image is kept iff every fractional coordinate ``f_k`` has
    ``-m_k <= f_k <= 1 + m_k`` with ``m_k = IMAGE_SAFETY * (radius + probe) / w_k + 1e-9`` and ``w_k`` the
    perpendicular width of the cell along vector ``k`` (a voxel centre lies inside the cell, and a point further than
    the reach from a face's plane is further than that from everything behind it).  ``cull=False`` keeps all 27.  A
    reach above the smallest width raises: images beyond the 27 would matter (a thin cell)."""
    x = np.asarray(xyz, dtype=np.float64).reshape(1, -1, 3)
    return cell_images_many(x, radii, np.asarray(R, dtype=np.float64).reshape(1, 3, 3), probe, cull)[:2]


@dataclasses.dataclass(frozen=True)
class Channels:
    """The pore network of one cell at one probe (scalars), of one cell on a ladder of probes (arrays over the probes)
    or of many frames (arrays ``(frames, probes)``).  ``raw`` holds the integers of ``pw_channels``
    (``_lib.CHANNELS_OUT_DTYPE``) and ``components`` the table (``_lib.CHANNELS_COMP_DTYPE``, a last axis of ``c_max``
    rows of which the first ``raw["n_recorded"]`` are components, in the order of their first voxels); ``shape`` the
    grid ``(nx, ny, nz)`` and ``cell_volume`` the cell's volume, per frame; ``probes`` the ladder.  With ``mask``:
    ``accessible`` ``(nz, ny, nx)`` bool arrays and ``accessible_words`` the same voxels as the kernel wrote them
    (``ny * nz`` uint64, row ``(j, l)`` at ``l * ny + j``, the layout of ``pw_cavity``'s mask); with ``labels``:
    ``labels`` ``(nz, ny, nx)`` uint8 arrays -- a component's row of the table, 254 beyond ``c_max``, 255 not open.
    Lists over the jobs, frame after frame, for anything but one cell at one probe."""

    raw: np.ndarray
    components: np.ndarray
    shape: np.ndarray
    cell_volume: np.ndarray
    probes: np.ndarray
    spacing: float
    lattice: np.ndarray                  # the triangular cells, (..., 3, 3)
    rotation: np.ndarray                 # Q of triangular_lattice, (..., 3, 3)
    accessible: object = None
    accessible_words: object = None
    labels: object = None
    frames: np.ndarray | None = None

    def _voxel_volume(self):
        n = np.prod(np.asarray(self.shape, dtype=np.float64), axis=-1)
        v = np.asarray(self.cell_volume, dtype=np.float64) / n
        return v[..., None] if self.raw.ndim == v.ndim + 1 else v, n[..., None] if self.raw.ndim == n.ndim + 1 else n

    @property
    def n_open(self):
        return self.raw["n_open"]

    @property
    def n_components(self):
        return self.raw["n_components"]

    @property
    def truncated(self):
        return (self.raw["flags"] & _lib.CHAN_TRUNCATED) != 0

    @property
    def void_fraction(self):
        """Open voxels over voxels."""
        return self.raw["n_open"] / self._voxel_volume()[1]

    @property
    def accessible_volume(self):
        """The voxels of the components of rank >= 1 times the volume of a voxel (cell volume over voxels): exact
        whatever ``c_max`` is."""
        return self.raw["n_voxels_by_rank"][..., 1:].sum(axis=-1) * self._voxel_volume()[0]

    @property
    def inaccessible_volume(self):
        """The voxels of the pockets times the volume of a voxel."""
        return self.raw["n_voxels_by_rank"][..., 0] * self._voxel_volume()[0]

    @property
    def dimensionality(self):
        """The largest rank of a component: 0 when nothing percolates (or nothing is open)."""
        has = self.raw["n_components_by_rank"] > 0
        return np.where(has, np.arange(4), 0).max(axis=-1)

    @property
    def limiting_probe(self):
        """The largest probe of the ladder with a component of rank >= 1, per frame; NaN when none has one."""
        d = np.asarray(self.dimensionality)
        p = np.broadcast_to(np.asarray(self.probes, dtype=np.float64), d.shape) if d.ndim else np.asarray(self.probes, dtype=np.float64)
        best = np.where(d >= 1, p, -np.inf)
        best = best.max(axis=-1) if d.ndim else best
        return np.where(np.isfinite(best), best, np.nan)[()]

    def series(self, name: str = "accessible_volume", probe: int = 0):
        """``(values, valid)`` of a quantity over the frames at probe number ``probe`` of the ladder (``limiting_probe``
        is of the whole ladder; its ``valid`` says that some probe percolates; for one cell, not a batch of frames, the
        values run over its probes) -- float64 values ready for
        :func:`pywindow_amd.time_correlation`, :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`,
        :func:`pywindow_amd.gate_statistics` and :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        v = np.asarray(getattr(self, name), dtype=np.float64)
        if name != "limiting_probe" and self.raw.ndim == 2:
            v = v[:, probe]
        v = np.atleast_1d(v).copy()
        return v, np.isfinite(v)

    def component_of(self, points, job: int = 0):
        """The label of the voxel that holds each of ``points`` ``(m, 3)`` (in the coordinates the atoms were given in;
        wrapped into the cell): a row of ``components``, 254 or 255.  Two cage centres with one label below 254 are in
        one component -- the cages are connected.  Needs ``labels=True``; ``job``: which cell of a batch, frame after
        frame and probe after probe."""
        if self.labels is None:
            raise ValueError("component_of: the result was made without labels=True")
        single = isinstance(self.labels, np.ndarray)
        lab = self.labels if single else self.labels[job]
        n_probes = 1 if self.raw.ndim < 2 else self.raw.shape[1]
        t = 0 if single else job // n_probes
        R = self.lattice.reshape(-1, 3, 3)[t if self.lattice.ndim == 3 else 0]
        Q = self.rotation.reshape(-1, 3, 3)[t if self.rotation.ndim == 3 else 0]
        frac = (np.asarray(points, dtype=np.float64).reshape(-1, 3) @ Q) @ np.linalg.inv(R).T
        frac = frac - np.floor(frac)
        nz, ny, nx = lab.shape
        idx = np.minimum((frac * np.array([nx, ny, nz])).astype(np.int64), np.array([nx, ny, nz]) - 1)
        return lab[idx[:, 2], idx[:, 1], idx[:, 0]]


def _radii(radii_or_elements, n: int) -> np.ndarray:
    a = np.asarray(radii_or_elements)
    if a.dtype.kind in "US" or a.dtype == object:
        from .element_data import VDW, element_ids

        a = VDW[element_ids(a)]
    r = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if len(r) != n:
        raise ValueError("radii_or_elements: one radius or element per atom")
    return r


def plan_jobs(xyz, radii_or_elements, lattice, probe=0.0, spacing: float = 0.5, c_max: int = 64, mask: bool = False,
              labels: bool = False):
    """What :func:`channel_network_batch` hands to ``Context.channels``, and what it keeps for the result:
    ``(jobs, atoms, radii, probes, cells (T, 3, 3), rotations (T, 3, 3), shapes (T, 3))`` -- job ``t * P + p`` is frame
    ``t`` at probe ``p``; the images of a frame are made once, for the largest probe, and shared by its jobs."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("xyz: (T, n, 3)")
    T, n = x.shape[:2]
    r = _radii(radii_or_elements, n)
    probes = np.atleast_1d(np.asarray(probe, dtype=np.float64)).reshape(-1)
    spacing, c_max = float(spacing), int(c_max)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError("spacing: a positive number")
    if len(probes) == 0 or not np.isfinite(probes).all() or (probes < 0.0).any():
        raise ValueError("probe: finite and not negative")
    if not np.isfinite(x).all() or not np.isfinite(r).all() or (r < 0.0).any():
        raise ValueError("xyz and radii: finite, and no negative radius")
    if not 0 <= c_max <= _lib.CHAN_MAX_COMPONENTS:
        raise ValueError(f"c_max: 0 .. {_lib.CHAN_MAX_COMPONENTS}")
    lat = np.asarray(lattice, dtype=np.float64)
    lat = np.broadcast_to(lat, (T, 3, 3)) if lat.ndim == 2 else lat
    if lat.shape != (T, 3, 3):
        raise ValueError("lattice: (3, 3) or one (3, 3) per frame")
    P = len(probes)
    jobs = np.zeros(T * P, dtype=_lib.CHANNELS_JOB_DTYPE)
    Rs, Qs = np.zeros((T, 3, 3)), np.zeros((T, 3, 3))
    for t in range(T):
        Rs[t], Qs[t] = triangular_lattice(lat[t])
    atoms, reach, counts = cell_images_many(np.matmul(x, Qs), r, Rs, float(probes.max()))
    shapes = np.zeros((T, 3), dtype=np.int64)
    at = words = voxels = 0
    for t in range(T):
        dims, origin, step = cell_grid(Rs[t], spacing)
        shapes[t] = dims
        for p in range(P):
            k = t * P + p
            jobs[k] = (at, counts[t], at, k * c_max, words if mask else -1, voxels if labels else -1, k, origin, step,
                       probes[p], *dims, c_max)
            words += dims[1] * dims[2] if mask else 0
            voxels += dims[0] * dims[1] * dims[2] if labels else 0
        at += int(counts[t])
    return jobs, atoms, reach, probes, Rs, Qs, shapes


def channel_network_batch(xyz, radii_or_elements, lattice, probe=0.0, spacing: float = 0.5, c_max: int = 64,
                          mask: bool = False, labels: bool = False, device=None, frames=None, kernel_ms=None) -> Channels:
    """:func:`channel_network` for ``T`` frames of the same ``n`` atoms on a ladder of ``P`` probes, all ``T * P`` jobs
    in ONE ``pw_channels`` call: ``xyz`` ``(T, n, 3)``, ``lattice`` ``(3, 3)`` or ``(T, 3, 3)``, ``probe`` a number or
    a sequence.  The fields of the result are ``(T, P)`` arrays (:func:`plan_jobs`).  ``kernel_ms``: a list that
    receives the time of the device work by HIP events."""
    jobs, atoms, reach, probes, Rs, Qs, shapes = plan_jobs(xyz, radii_or_elements, lattice, probe, spacing, c_max, mask, labels)
    T, P, c_max = len(Rs), len(probes), int(c_max)
    out, comps, bits, lab = engine.context(device).channels(jobs, atoms, reach, kernel_ms=kernel_ms)
    comps = np.zeros(0, dtype=_lib.CHANNELS_COMP_DTYPE) if comps is None else comps
    masks = wordlist = labellist = None
    if mask:
        wordlist = [bits[int(j["mask_first"]):int(j["mask_first"]) + int(j["ny"]) * int(j["nz"])] for j in jobs]
        masks = [unpack_mask(w, int(j["nx"]), int(j["ny"]), int(j["nz"])) for w, j in zip(wordlist, jobs)]
    if labels:
        labellist = [lab[int(j["label_first"]):int(j["label_first"]) + int(j["nx"]) * int(j["ny"]) * int(j["nz"])]
                     .reshape(int(j["nz"]), int(j["ny"]), int(j["nx"])) for j in jobs]
    volume = Rs[:, 0, 0] * Rs[:, 1, 1] * Rs[:, 2, 2]
    return Channels(out.reshape(T, P), comps.reshape(T, P, c_max), shapes, volume, probes, float(spacing), Rs, Qs, masks,
                    wordlist, labellist, None if frames is None else np.array(frames, dtype=np.int64).reshape(-1))


def channel_network(xyz, radii_or_elements, lattice, probe=0.0, spacing: float = 0.5, c_max: int = 64, mask: bool = False,
                    labels: bool = False, device=None) -> Channels:
    """The pore network of the cell ``lattice`` (columns as vectors, the convention of ``system["lattice"]``) filled with
    the atoms ``xyz`` ``(n, 3)`` of radii ``radii_or_elements`` (numbers, or element symbols for the van der Waals radii of
    ``element_data.VDW``) for a probe of radius ``probe``: see :class:`Channels`.

    The grid has ``n_k = ceil(|v_k| / spacing)`` voxels along cell vector ``k`` (more than 64: ``ValueError`` naming the
    smallest spacing that fits), so its voxels are parallelepipeds of the cell's shape.  A lattice that is not in the
    triangular form of ``rebuild.unit_cell_to_lattice_array`` (first vector along x, second in the xy plane) is rotated
    into it on the host by a QR factorisation (:func:`triangular_lattice`), the atoms with it.  The atoms are wrapped
    into the cell and each contributes those of its 27 images that lie within the cell grown by its reach
    (:func:`cell_images`); a reach above the cell's smallest perpendicular width raises.  ``c_max``: rows of the
    component table (the totals, and so the volumes, count every component).  ``probe`` a sequence: a ladder, and the
    fields are arrays over it.  ``xyz`` ``(T, n, 3)`` is :func:`channel_network_batch`.  ``device``: the HIP ordinal
    (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    if x.ndim == 3:
        return channel_network_batch(x, radii_or_elements, lattice, probe, spacing, c_max, mask, labels, device)
    many = channel_network_batch(x.reshape(1, -1, 3), radii_or_elements, lattice, probe, spacing, c_max, mask, labels, device)
    one = np.ndim(probe) == 0

    def pick(v):
        return None if v is None else (v[0] if one else v)

    return Channels(many.raw[0, 0] if one else many.raw[0], many.components[0, 0] if one else many.components[0],
                    many.shape[0], many.cell_volume[0], many.probes[0] if one else many.probes, many.spacing, many.lattice[0],
                    many.rotation[0], pick(many.accessible), pick(many.accessible_words), pick(many.labels), None)
