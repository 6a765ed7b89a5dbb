"""Crystal diffusion on the GPU: the self-diffusion tensor of a guest through a periodic cell from the energy basins of
its landscape (``pw_basins``, include/pywindow_amd.h; the definition and its proofs in pywindow_amd/csrc/pw_basins.hpp).

:func:`pywindow_amd.guest_percolation` gives the level at which the landscape connects; an activation energy alone
cannot give a rate.  Here the periodic Lennard-Jones landscape of one guest is cut into the basins of steepest descent on
the cell's own grid; the library returns the Boltzmann sum over every basin and over every dividing surface between two
basins with the INTEGER cell offset between them.  What follows is plain numpy on those rows, the same for the device and
the explicit host path (``device=-1``): shallow basins are merged into sites, every dividing surface becomes a hop with
the transition-state-theory rate ``k(i -> j) = sqrt(k_B T / 2 pi m) * sum_k a_k S_k / (v Z_i)`` (``v`` the voxel's
volume, ``a_k`` the area of its face across ``e_k``), and the diffusion tensor of the periodic hop network is

    ``D = 1/2 sum_i pi_i sum_j k_ij (Delta_ij + chi_j - chi_i)(Delta_ij + chi_j - chi_i)^T``

with the corrector ``chi`` of ``sum_j k_ij (chi_j - chi_i) = -sum_j k_ij Delta_ij``: symmetric and positive
semi-definite by construction, ``1/2 sum k Delta Delta^T`` on a Bravais lattice.  Lengths in Angstrom, times in seconds
(``D`` in Angstrom^2 / s, the units of :meth:`pywindow_amd.Hopping.diffusion`), energies in kJ/mol.  Limits that are
part of the definition: a dividing surface is a staircase of voxel faces, whose area exceeds a smooth surface's by up to
``sqrt(3)``; transition-state theory without recrossing at infinite dilution (one guest, no charges), with ``merge`` a
model parameter; the bottleneck is that of the grid at its spacing.  The reference has no counterpart.

* :func:`guest_diffusion` -- one cell; :func:`guest_diffusion_batch` -- frames in ONE call; :func:`diffusion_field` --
  any periodic scalar field; :class:`Diffusion` -- the result; :func:`hop_network` and :func:`network_tensor` -- the
  two numpy steps on their own.
* ``MolecularSystem.calculate_guest_diffusion`` (molecular.py) and ``DLPOLY.diffusion`` (trajectory.py).
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import _lib, engine
from .affinity import R
from .channels import triangular_lattice
from .hopping import _AMU, _KB, GUEST_MASSES
from .percolation import plan_jobs

__all__ = ["Diffusion", "guest_diffusion", "guest_diffusion_batch", "diffusion_field", "hop_network", "network_tensor"]

_SERIES = ("coefficient", "axis_coefficient", "trapped_fraction")
B_CAP, E_CAP = 1024, 8192

SITE_DTYPE = np.dtype([("position", np.float64, (3,)), ("u_min", np.float64), ("root", np.int64), ("n_basins", np.int64)])
HOP_DTYPE = np.dtype([("i", np.int64), ("j", np.int64), ("cell", np.int64, (3,)), ("saddle", np.float64),
                      ("vector", np.float64, (3,))])


def _key(values):
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
    bits[bits == np.uint64(0x8000000000000000)] = 0
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(0x8000000000000000))


class _Offsets:
    """A union-find whose members carry their integer cell offset to their set's representative:
    ``position(b) = position(find(b)) + g(b) . cell``."""

    def __init__(self, n):
        self.parent = list(range(n))
        self.g = np.zeros((n, 3), dtype=np.int64)

    def find(self, a):
        path = []
        while self.parent[a] != a:
            path.append(a)
            a = self.parent[a]
        acc = np.zeros(3, dtype=np.int64)
        for u in reversed(path):
            acc = acc + self.g[u]
            self.g[u] = acc
            self.parent[u] = a
        return a

    def net(self, a, b, d):
        """The offset of b's representative to a's through the edge (a, b, d): with one representative, the net offset
        of the closed walk the edge closes."""
        ra, rb = self.find(a), self.find(b)
        return ra, rb, self.g[a] + np.asarray(d, dtype=np.int64) - self.g[b]

    def join(self, ra, rb, net):
        self.parent[rb] = ra
        self.g[rb] = net


def hop_network(basins, edges, merge: float):
    """The merge of the basins into sites and of the edges into hops (plain numpy on ``pw_basins``' rows).  A Kruskal
    pass over the edges in ascending (saddle key, edge order): an edge joins two sets when ``saddle - max(u_min of the two
    sets) <= merge``; an edge inside one set with zero net offset is dropped into the set; one with a non-zero net
    offset and ``saddle - u_min(set) <= merge`` means the guest runs free along that direction (``barrierless``).
    Returns ``(site_of (B,), offset (B, 3), roots (n_sites,), hops, barrierless)``: the site of every basin, the cell
    offset of the basin's root to the site's root basin (the member with the lowest (u_min key, number)), the root basin
    of every site, and ``hops`` a list of ``(i, j, cell (3,), saddle, rows)`` with ``i <= j`` in canonical form, ``rows``
    the numbers of the parallel edges in edge order, ascending in ``(i, j, cell)``."""
    B = len(basins)
    uf = _Offsets(B)
    low = np.asarray(basins["u_min"], dtype=np.float64).copy()       # per representative: the set's u_min
    keys = _key(edges["saddle"]) if len(edges) else np.zeros(0, dtype=np.uint64)
    barrierless = False
    kept = []
    for q in np.lexsort((np.arange(len(edges)), keys)).tolist():
        e = edges[q]
        ra, rb, net = uf.net(int(e["a"]), int(e["b"]), e["d"])
        saddle = float(e["saddle"])
        if ra != rb:
            if saddle - max(low[ra], low[rb]) <= merge:
                uf.join(ra, rb, net)
                low[ra] = min(low[ra], low[rb])
            else:
                kept.append(q)
        elif net.any():
            if saddle - low[ra] <= merge:
                barrierless = True
            kept.append(q)
    rep = np.array([uf.find(b) for b in range(B)], dtype=np.int64)
    ukey = _key(basins["u_min"]) if B else np.zeros(0, dtype=np.uint64)
    order = np.lexsort((np.arange(B), ukey))
    root_of = {}
    for b in order.tolist():                                         # the first member in (u_min key, number) is the root
        root_of.setdefault(int(rep[b]), b)
    roots = np.array(sorted(root_of.values()), dtype=np.int64)
    number = {int(b): s for s, b in enumerate(roots)}
    site_of = np.array([number[root_of[int(r)]] for r in rep], dtype=np.int64)
    offset = np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        offset[b] = uf.g[b] - uf.g[root_of[int(rep[b])]]
    grouped = {}
    for q in kept:
        e = edges[q]
        a, b = int(e["a"]), int(e["b"])
        i, j = int(site_of[a]), int(site_of[b])
        cell = offset[a] + np.asarray(e["d"], dtype=np.int64) - offset[b]
        lead = next((int(x) for x in cell if x), 0)
        if i > j or (i == j and lead < 0):
            i, j, cell = j, i, -cell
        if i == j and not cell.any():
            continue                                                 # (a barrier inside a site between two of its own basins)
        grouped.setdefault((i, j) + tuple(int(x) for x in cell), []).append(q)
    hops = []
    for name in sorted(grouped):
        rows = sorted(grouped[name])
        k = _key(edges["saddle"][rows])
        hops.append((name[0], name[1], np.array(name[2:], dtype=np.int64), float(edges["saddle"][rows[int(np.argmin(k))]]), rows))
    return site_of, offset, roots, hops, barrierless


def winding_vectors(n_sites, i, j, cells):
    """``(component (n_sites,), vectors)``: the connected components of the hop graph and the net offsets of the closed
    walks that its edges close against a spanning forest (they generate every closed walk's)."""
    uf = _Offsets(n_sites)
    vectors = []
    for a, b, d in zip(i, j, cells):
        ra, rb, net = uf.net(int(a), int(b), d)
        if ra != rb:
            uf.join(ra, rb, net)
        elif net.any():
            vectors.append((ra, net.copy()))
    comp = np.array([uf.find(s) for s in range(n_sites)], dtype=np.int64)
    return comp, [(int(comp[r]), v) for r, v in vectors]


def network_tensor(populations, i, j, vectors, k_forward, k_backward, cells):
    """``(D (3, 3), trapped_fraction, winding_rank)`` of a periodic hop network: sites with the populations ``Z`` and
    hops ``i -> j`` with the jump vector ``vectors`` and the integer cell offset ``cells``, forward rate ``k_forward``
    (``i -> j``) and backward rate ``k_backward`` (``j -> i`` along ``-vector``); a hop with ``i == j`` is a jump of a
    site to its own image and counts in both directions.  The tensor is computed on the union ``N`` of the components
    that hold a closed walk with non-zero net offset; ``trapped_fraction = 1 - Z(N) / Z(all)``."""
    Z = np.asarray(populations, dtype=np.float64)
    n = len(Z)
    i, j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
    vectors = np.asarray(vectors, dtype=np.float64).reshape(-1, 3)
    kf, kb = np.asarray(k_forward, dtype=np.float64).reshape(-1), np.asarray(k_backward, dtype=np.float64).reshape(-1)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    comp, wind = winding_vectors(n, i, j, cells)
    rank = int(np.linalg.matrix_rank(np.array([v for _, v in wind], dtype=np.float64))) if wind else 0
    moving = sorted({c for c, _ in wind})
    D = np.zeros((3, 3))
    total = float(Z.sum())
    if not moving or total <= 0.0:
        return D, 1.0 if total > 0.0 else 0.0, rank
    inside = np.isin(comp, moving)
    ZN = float(Z[inside].sum())
    pi = np.where(inside, Z / ZN, 0.0)
    # directed jumps: source, target, vector, rate
    src = np.concatenate([i, j])
    dst = np.concatenate([j, i])
    vec = np.concatenate([vectors, -vectors])
    rate = np.concatenate([kf, kb])
    for c in moving:
        sites = np.flatnonzero(comp == c)
        local = {int(s): q for q, s in enumerate(sites)}
        use = np.flatnonzero(comp[src] == c)
        s = np.array([local[int(a)] for a in src[use]], dtype=np.int64)
        t = np.array([local[int(a)] for a in dst[use]], dtype=np.int64)
        w = pi[src[use]] * rate[use]                                 # pi_i k_ij: symmetric under i <-> j (detailed balance)
        M = np.zeros((len(sites), len(sites)))
        np.add.at(M, (s, t), w)
        np.add.at(M, (s, s), -w)
        drift = np.zeros((len(sites), 3))
        np.add.at(drift, s, w[:, None] * vec[use])
        chi = np.linalg.lstsq(M, -drift, rcond=None)[0]              # (the constant mode is left out: minimum norm)
        step = vec[use] + chi[t] - chi[s]
        D += 0.5 * np.einsum("h,ha,hb->ab", w, step, step)
    return D, 1.0 - ZN / total, rank


@dataclasses.dataclass(frozen=True)
class Diffusion:
    """The diffusion of a guest through one cell (``tensor`` ``(L, 3, 3)``) or through ``T`` frames (``(T, L, 3, 3)``),
    ``L`` the number of temperatures.  ``tensor`` in Angstrom^2 / s in the coordinates the atoms were given in;
    ``sites`` (per frame a record array: position of the site's root voxel, ``u_min``, root basin, members;
    ``populations`` ``(n_sites, L)`` the Boltzmann sums ``Z``, ``free_energy`` ``-RT ln(Z v)``) and ``hops`` (per frame a
    record array: ``i``, ``j``, cell offset, saddle, jump vector; ``rates`` ``(n_hops, L, 2)`` forward and backward per
    second); ``raw`` the job's row of ``pw_basins``; ``barrierless``: a closed walk with a non-zero cell offset lies
    below the merge threshold (the guest runs free and the hop model does not hold); ``valid``: nothing overflowed,
    nothing was clamped, no offset left its range and the frame is not barrierless."""

    tensor: np.ndarray
    temperatures: np.ndarray
    raw: np.ndarray
    n_basins: np.ndarray
    n_sites: np.ndarray
    trapped_fraction: np.ndarray
    barrierless: np.ndarray
    winding_rank: np.ndarray
    valid: np.ndarray
    sites: object
    populations: object
    hops: object
    rates: object
    lattice: np.ndarray
    rotation: np.ndarray
    shape: np.ndarray
    spacing: float
    merge: float
    mass: float
    guest: object = None
    maps: object = None
    labels: object = None
    frames: np.ndarray | None = None
    voxel_volume: object = None
    charges_converged: object = None      # of a rigid guest with charges="qeq-cell": whether the frame's charges converged (part of valid)

    @property
    def coefficient(self):
        """``trace(tensor) / 3``: ``(..., L)``."""
        return np.trace(self.tensor, axis1=-2, axis2=-1) / 3.0

    @property
    def principal(self):
        """``(values (..., L, 3) ascending, axes (..., L, 3, 3) as columns)`` of the symmetric tensor."""
        return np.linalg.eigh(self.tensor)

    @property
    def axis_coefficient(self):
        """``(..., L, 3)``: ``u^T D u`` along the unit vectors of the cell vectors a, b, c."""
        u = np.asarray(self.lattice, dtype=np.float64)               # columns as vectors
        u = u / np.sqrt((u * u).sum(axis=-2, keepdims=True))
        return np.einsum("...ak,...lab,...bk->...lk", u, self.tensor, u)

    @property
    def free_energy(self):
        """Per frame ``(n_sites, L)``: ``-RT ln(Z v)`` of every site, kJ/mol."""
        def one(Z, v):
            with np.errstate(divide="ignore"):
                return -(R * self.temperatures)[None, :] * np.log(Z * v)
        if isinstance(self.populations, list):
            return [one(Z, v) for Z, v in zip(self.populations, self.voxel_volume)]
        return one(self.populations, self.voxel_volume)

    def activation_energy(self):
        """``-d ln D / d beta`` of ``coefficient`` by least squares over the temperatures given (at least two), kJ/mol;
        NaN where a coefficient is not positive."""
        if len(self.temperatures) < 2:
            raise ValueError("activation_energy: at least two temperatures")
        beta = 1.0 / (R * self.temperatures)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.log(np.atleast_2d(self.coefficient))
        x = beta - beta.mean()
        slope = (y - y.mean(axis=1, keepdims=True)) @ x / float(x @ x)
        slope = np.where(np.isfinite(y).all(axis=1), -slope, np.nan)
        return slope if np.ndim(self.coefficient) == 2 else float(slope[0])

    def series(self, name: str = "coefficient", level: int = 0, axis: int | None = None):
        """``(values, valid)`` over the frames: ``"coefficient"`` or ``"trapped_fraction"`` at temperature ``level``, or
        ``"axis_coefficient"`` along cell vector ``axis``.  Ready for :func:`pywindow_amd.time_correlation`,
        :func:`pywindow_amd.lomb_scargle`, :func:`pywindow_amd.gaussian_kde_1d`, :func:`pywindow_amd.gate_statistics` and
        :func:`pywindow_amd.transition_counts`."""
        if name not in _SERIES:
            raise KeyError(f"series: one of {_SERIES}")
        if not 0 <= int(level) < len(self.temperatures):
            raise ValueError("series: level 0 .. L - 1")
        many = np.ndim(self.valid) == 1
        v = np.asarray(getattr(self, name), dtype=np.float64)
        v = v if many else v[None]
        if name == "axis_coefficient":
            if axis not in (0, 1, 2):
                raise ValueError("series: axis 0, 1 or 2 for axis_coefficient")
            v = v[:, int(level), int(axis)]
        else:
            v = v[:, int(level)]
        return v.copy(), np.atleast_1d(self.valid).copy()


def _speed(temperatures, mass):
    return np.sqrt(_KB * temperatures / (2.0 * math.pi * mass * _AMU)) * 1e10      # Angstrom / s


def _frame(J, out, basins, edges, temperatures, mass, merge):
    """One frame's sites, hops, rates and tensors (in the triangular frame) from its rows."""
    L = len(temperatures)
    nx, ny, nz = int(J["nx"]), int(J["ny"]), int(J["nz"])
    ax, bx, by, cx, cy, cz = (float(s) for s in J["step"])
    sa, sb, sc = np.array([ax, 0.0, 0.0]), np.array([bx, by, 0.0]), np.array([cx, cy, cz])
    cell = np.stack([nx * sa, ny * sb, nz * sc])                     # rows: the cell vectors
    volume = ax * by * cz
    area = np.array([np.linalg.norm(np.cross(sb, sc)), np.linalg.norm(np.cross(sc, sa)), np.linalg.norm(np.cross(sa, sb))])
    site_of, offset, roots, hops, barrierless = hop_network(basins, edges, merge)
    n = len(roots)
    Z = np.zeros((n, L))
    members = np.zeros(n, dtype=np.int64)
    for b in range(len(basins)):                                     # (the members' sums added in basin order)
        Z[site_of[b]] = Z[site_of[b]] + basins["z"][b][:L]
        members[site_of[b]] += 1
    sites = np.zeros(n, dtype=SITE_DTYPE)
    rank = basins["root"][roots]
    i, row = rank % nx, rank // nx
    origin = np.asarray(J["origin"], dtype=np.float64)
    sites["position"] = origin[None, :] + i[:, None] * sa + (row % ny)[:, None] * sb + (row // ny)[:, None] * sc
    sites["u_min"], sites["root"], sites["n_basins"] = basins["u_min"][roots], roots, members
    rows = np.zeros(len(hops), dtype=HOP_DTYPE)
    rates = np.zeros((len(hops), L, 2))
    speed = _speed(temperatures, mass)
    for h, (a, b, d, saddle, parallel) in enumerate(hops):
        S = np.zeros((L, 3))
        for q in parallel:                                           # (parallel edges add their S in edge order)
            S = S + edges["s"][q][:L]
        flux = speed * (S @ area) / volume
        with np.errstate(divide="ignore", invalid="ignore"):
            rates[h, :, 0], rates[h, :, 1] = flux / Z[a], flux / Z[b]
        rows[h] = (a, b, d, saddle, sites["position"][b] + d @ cell - sites["position"][a])
    tensor = np.zeros((L, 3, 3))
    trapped = np.zeros(L)
    rank_w = 0
    for l in range(L):
        tensor[l], trapped[l], rank_w = network_tensor(Z[:, l], rows["i"], rows["j"], rows["vector"], rates[:, l, 0], rates[:, l, 1],
                                                       rows["cell"])
    flags = int(out["flags"])
    valid = not (flags & (_lib.BAS_OVERFLOW | _lib.BAS_CLAMPED | _lib.BAS_RANGE)) and not barrierless
    return dict(tensor=tensor, trapped=trapped, rank=rank_w, barrierless=barrierless, valid=valid, sites=sites, Z=Z, hops=rows,
                rates=rates, volume=volume)


def _run(ctx, jobs, atoms, coef, field):
    """``Context.basins`` with the capacities of the jobs; a job that overflows is run once more with the counts it
    returned.  Returns ``(out, [basins], [edges], maps, labels)``, the rows per job."""
    out, basins, edges, maps, labels = ctx.basins(jobs, atoms, coef, field)
    per_b = [basins[int(J["basin_first"]):int(J["basin_first"]) + int(o["n_basins_written"])] for J, o in zip(jobs, out)]
    per_e = [edges[int(J["edge_first"]):int(J["edge_first"]) + int(o["n_edges_written"])] for J, o in zip(jobs, out)]
    again = np.flatnonzero((out["flags"] & _lib.BAS_OVERFLOW) != 0)
    if len(again):
        more = jobs[again].copy()
        more["b_cap"], more["e_cap"] = out["n_basins"][again], out["n_edges"][again]
        more["basin_first"] = np.cumsum(more["b_cap"]) - more["b_cap"]
        more["edge_first"] = np.cumsum(more["e_cap"]) - more["e_cap"]
        more["out"] = np.arange(len(again))
        more["map_first"] = more["label_first"] = -1                 # (written by the first call)
        o2, b2, e2, _, _ = ctx.basins(more, atoms, coef, field)
        for q, k in enumerate(again.tolist()):
            out[k] = o2[q]
            per_b[k] = b2[int(more["basin_first"][q]):int(more["basin_first"][q]) + int(o2[q]["n_basins_written"])]
            per_e[k] = e2[int(more["edge_first"][q]):int(more["edge_first"][q]) + int(o2[q]["n_edges_written"])]
    return out, per_b, per_e, maps, labels


def _basins_jobs(perc_jobs, temperatures, cap, maps, labels):
    T = len(perc_jobs)
    jobs = np.zeros(T, dtype=_lib.BASINS_JOB_DTYPE)
    for name in ("atom_first", "n", "coef_first", "field_first", "origin", "step", "core2", "cutoff2", "nx", "ny", "nz"):
        jobs[name] = perc_jobs[name]
    voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
    first = np.cumsum(voxels) - voxels
    jobs["map_first"] = first if maps else -1
    jobs["label_first"] = first if labels else -1
    jobs["out"] = np.arange(T)
    jobs["b_cap"], jobs["e_cap"] = B_CAP, E_CAP
    jobs["basin_first"], jobs["edge_first"] = B_CAP * np.arange(T), E_CAP * np.arange(T)
    jobs["cap"] = cap
    jobs["n_betas"] = len(temperatures)
    jobs["betas"][:, :len(temperatures)] = 1.0 / (R * temperatures)
    return jobs


def _temperatures(temperatures, mass, guest):
    temps = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=np.float64)))
    if mass is None:
        if not isinstance(guest, str) or guest not in GUEST_MASSES:
            raise ValueError("mass: the guest's molar mass in g/mol (built in for the names of affinity.GUESTS only)")
        mass = GUEST_MASSES[guest]
    mass = float(mass)
    if not (1 <= len(temps) <= _lib.BAS_MAX_BETAS) or not np.isfinite(temps).all() or (temps <= 0.0).any() or not mass > 0.0:
        raise ValueError("temperatures: 1 to 8 positive numbers; mass: positive")
    return temps, mass


def _result(jobs, ran, temps, mass, merge, Rs, Qs, shapes, spacing, guest, maps, labels, frames) -> Diffusion:
    out, per_b, per_e, fields, labelled = ran
    made = [_frame(J, o, b, e, temps, mass, merge) for J, o, b, e in zip(jobs, out, per_b, per_e)]
    tensor = np.stack([np.einsum("ab,lbc,dc->lad", Q, m["tensor"], Q) for Q, m in zip(Qs, made)])
    for Q, m in zip(Qs, made):                                       # (the positions come back in the caller's frame)
        m["sites"]["position"] = m["sites"]["position"] @ Q.T
        m["hops"]["vector"] = m["hops"]["vector"] @ Q.T

    def cut(array, name):
        if array is None:
            return None
        return [array[int(J[name]):int(J[name]) + int(J["nx"]) * int(J["ny"]) * int(J["nz"])]
                .reshape(int(J["nz"]), int(J["ny"]), int(J["nx"])) for J in jobs]

    lattice = np.matmul(Qs, Rs)
    return Diffusion(tensor, temps, out, out["n_basins"].copy(), np.array([len(m["sites"]) for m in made]),
                     np.stack([m["trapped"] for m in made]), np.array([m["barrierless"] for m in made]),
                     np.array([m["rank"] for m in made]), np.array([m["valid"] for m in made]), [m["sites"] for m in made],
                     [m["Z"] for m in made], [m["hops"] for m in made], [m["rates"] for m in made], lattice, Qs, shapes,
                     float(spacing), float(merge), mass, guest, cut(fields, "map_first") if maps else None,
                     cut(labelled, "label_first") if labels else None,
                     None if frames is None else np.array(frames, dtype=np.int64).reshape(-1), [m["volume"] for m in made])


def _one(many: Diffusion) -> Diffusion:
    first = lambda v: None if v is None else v[0]
    return dataclasses.replace(many, tensor=many.tensor[0], raw=many.raw[0], n_basins=many.n_basins[0], n_sites=many.n_sites[0],
                               trapped_fraction=many.trapped_fraction[0], barrierless=many.barrierless[0],
                               winding_rank=many.winding_rank[0], valid=many.valid[0], sites=many.sites[0],
                               populations=many.populations[0], hops=many.hops[0], rates=many.rates[0], lattice=many.lattice[0],
                               rotation=many.rotation[0], shape=many.shape[0], maps=first(many.maps), labels=first(many.labels),
                               frames=None, voxel_volume=many.voxel_volume[0])


def guest_diffusion_batch(xyz, elements_or_coef, lattice, guest="Xe", temperatures=298.0, spacing: float = 0.5,
                          cutoff: float = 12.0, core2: float = 0.25, cap: float = 100.0, merge=None, mass=None,
                          maps: bool = False, labels: bool = False, device=None, frames=None) -> Diffusion:
    """:func:`guest_diffusion` for ``T`` frames of the same ``n`` atoms, all jobs in ONE ``pw_basins`` call (and one more
    for the frames whose basins or edges overflowed the first capacities): ``xyz`` ``(T, n, 3)``, ``lattice`` ``(3, 3)``
    or ``(T, 3, 3)``.  The fields of the result are arrays, or lists, over the frames."""
    temps, mass = _temperatures(temperatures, mass, guest)
    merge = float(R * temps.min()) if merge is None else float(merge)
    cap = float(cap)
    if math.isnan(cap) or math.isnan(merge) or merge < 0.0:
        raise ValueError("cap: a number; merge: >= 0")
    perc_jobs, atoms, coef, Rs, Qs, shapes = plan_jobs(xyz, elements_or_coef, lattice, guest, spacing, cutoff, core2, False)
    jobs = _basins_jobs(perc_jobs, temps, cap, maps, labels)
    ran = _run(engine.context(device), jobs, atoms, coef, None)
    return _result(jobs, ran, temps, mass, merge, Rs, Qs, shapes, spacing, guest, maps, labels, frames)


def guest_diffusion(xyz, elements_or_coef, lattice, guest="Xe", temperatures=298.0, spacing: float = 0.5, cutoff: float = 12.0,
                    core2: float = 0.25, cap: float = 100.0, merge=None, mass=None, maps: bool = False, labels: bool = False,
                    device=None) -> Diffusion:
    """The self-diffusion tensor of the one-site Lennard-Jones guest ``guest`` (a name of ``affinity.GUESTS`` or ``(sigma,
    eps_kJ_per_mol)`` with ``mass`` in g/mol) through the crystal of the cell ``lattice`` (columns as vectors) filled
    with the atoms ``xyz`` ``(n, 3)``, at every temperature of ``temperatures`` (1 to 8, in K): see :class:`Diffusion`
    and the module's text for the model and its limits.

    The grid, the rotation into the triangular cell, the periodic images and the cutoff check are those of
    :func:`pywindow_amd.guest_percolation`.  ``cap``: voxels above this energy (kJ/mol) take no part.  ``merge``: basins
    separated by less than this (kJ/mol) are one site; the default is ``R * min(temperatures)``.  ``maps`` / ``labels``
    keep the energy and the basin with its cell offset of every voxel.  ``xyz`` ``(T, n, 3)`` is
    :func:`guest_diffusion_batch`.  ``device``: the HIP ordinal (``None``: the process's); ``-1`` the explicit host path."""
    x = np.asarray(xyz, dtype=np.float64)
    args = (elements_or_coef, lattice, guest, temperatures, spacing, cutoff, core2, cap, merge, mass, maps, labels, device)
    if x.ndim == 3:
        return guest_diffusion_batch(x, *args)
    return _one(guest_diffusion_batch(x.reshape(1, -1, 3), *args))


def diffusion_field(field, lattice, temperatures, mass, cap: float = np.inf, merge=None, labels: bool = False,
                    device=None) -> Diffusion:
    """:func:`guest_diffusion` of any periodic scalar field ``(nz, ny, nx)`` in kJ/mol (finite values or ``+inf`` for a
    blocked voxel) on the grid that divides the cell ``lattice`` (columns as vectors) into ``nx x ny x nz`` voxels."""
    f = np.ascontiguousarray(field, dtype=np.float64)
    if f.ndim != 3 or f.size == 0:
        raise ValueError("field: (nz, ny, nx)")
    temps, mass = _temperatures(temperatures, mass, None)
    merge = float(R * temps.min()) if merge is None else float(merge)
    if math.isnan(float(cap)) or math.isnan(merge) or merge < 0.0:
        raise ValueError("cap: a number; merge: >= 0")
    nz, ny, nx = f.shape
    Rt, Q = triangular_lattice(lattice)
    S = Rt / np.array([nx, ny, nz], dtype=np.float64)[None, :]
    perc = np.zeros(1, dtype=_lib.PERCOLATION_JOB_DTYPE)
    perc[0] = (0, 0, 0, 0, -1, 0, 0, 0.5 * S.sum(axis=1), (S[0, 0], S[0, 1], S[1, 1], S[0, 2], S[1, 2], S[2, 2]), 0.25, 0.0,
               nx, ny, nz, 0)
    jobs = _basins_jobs(perc, temps, float(cap), False, labels)
    ran = _run(engine.context(device), jobs, None, None, f.reshape(-1))
    spacing = float(np.sqrt((S * S).sum(axis=0)).max())
    return _one(_result(jobs, ran, temps, mass, merge, Rt[None], Q[None], np.array([[nx, ny, nz]]), spacing, None, False, labels, None))
