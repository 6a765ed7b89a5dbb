"""Inputs shared by tests/test_ewald_host.py (host path against pw_rigid_cell, pw_rigid_affinity and a numpy restatement)
and tests/test_ewald_gpu.py (device against the host path, as bytes): pw_rigid_cell_ewald, the field of a rigid linear
guest over a periodic cell with the Ewald sum of the framework's point charges.  numpy and math only, seeded.  The jobs
are built on tests/_rigid_cell_cases.py's Case, atoms and directions; `reference` restates the definition of
include/pywindow_amd.h plainly -- complex exponentials at the voxel centres, math.erfc, every atom and no skip."""
import math

import numpy as np

import _rigid_cell_cases as C

SENTINEL = C.SENTINEL
SKEW = C.SKEW
MAX_K = 4096
MAX_INDEX = 64


class Inputs:
    """What jobs may share: listed atoms (n, 3), rows (A, B, C) (S, n, 3), offsets (S,), directions (M, 3), site charges
    (S,), cell atoms (n_cell, 4) and rows (h, k, l, w) (K, 4)."""

    def __init__(self, xyz, coef, offsets, dirs, site_q, cell, kvecs):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        S = len(self.offsets)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(S, -1, 3)
        self.dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        self.site_q = np.ascontiguousarray(site_q, dtype=np.float64).reshape(-1)
        self.cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(-1, 4)
        self.kvecs = np.ascontiguousarray(kvecs, dtype=np.float64).reshape(-1, 4)
        assert self.coef.shape[1] == len(self.xyz) and len(self.site_q) == S


class Job:
    def __init__(self, name, inputs, dims, origin=(0.0, 0.0, 0.0), step=C.ortho(1.0), core2=0.25, cutoff2=9.0, betas=(0.4,),
                 alpha=0.4, charged=1, map=True):
        self.name, self.inputs, self.dims = name, inputs, tuple(int(d) for d in dims)
        self.origin, self.step = np.asarray(origin, dtype=np.float64), np.asarray(step, dtype=np.float64)
        self.core2, self.cutoff2 = float(core2), float(cutoff2)
        self.betas = np.asarray(betas, dtype=np.float64).reshape(-1)
        self.alpha, self.charged, self.map = float(alpha), int(charged), bool(map)

    @property
    def voxels(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def uncharged_case(self):
        """The pw_rigid_cell job of the same grid, atoms and rows (A, B)."""
        i = self.inputs
        return C.Case(self.name, self.dims, i.xyz, i.coef[:, :, :2], i.offsets, i.dirs, self.origin, self.step, self.core2,
                      self.cutoff2, self.betas, self.map)

    def replace(self, **kw):
        new = Job(self.name, self.inputs, self.dims, self.origin, self.step, self.core2, self.cutoff2, self.betas, self.alpha,
                  self.charged, self.map)
        for k, v in kw.items():
            setattr(new, k, v)
        return new


def half_rows(K, top, seed):
    """K distinct rows (h, k, l, w) of the half space with |index| <= top, in a seeded order, weights within 0.05 .. 1."""
    rng = np.random.default_rng(seed)
    rows = [(h, k, l) for h in range(0, top + 1) for k in range(-top, top + 1) for l in range(-top, top + 1)
            if h > 0 or (h == 0 and k > 0) or (h == 0 and k == 0 and l > 0)]
    pick = rng.permutation(len(rows))[:K]
    assert len(pick) == K
    return np.array([[*rows[p], rng.uniform(0.05, 1.0)] for p in pick], dtype=np.float64)


def make_inputs(n, S, M, dims, step, seed, n_cell=10, K=20, pad=2.0, origin=(0.0, 0.0, 0.0), top=2):
    rng = np.random.default_rng(seed + 1000)
    xyz, ab = C.box_atoms(n, S, dims, step, seed, pad=pad, origin=origin)
    coef = np.concatenate([ab, rng.uniform(-40.0, 40.0, (S, n, 1))], axis=2)
    cell_xyz, _ = C.box_atoms(n_cell, 1, dims, step, seed + 1, pad=0.0, origin=origin)
    q = rng.uniform(-1.0, 1.0, n_cell)
    return Inputs(xyz, coef, C.line(S, 0.3), C.dirs_of(M, seed + 2), rng.uniform(-0.7, 0.7, S),
                  np.concatenate([cell_xyz, (q - q.mean())[:, None]], axis=1), half_rows(K, top, seed + 3))


_made = {}


def once(f):
    def g():
        if f.__name__ not in _made:
            _made[f.__name__] = f()
        return _made[f.__name__]
    return g


@once
def skew_job():
    """Tests 1 and 3: a skewed cell, a 5 x 6 x 7 grid (every group cut at an edge, a short last chunk), 3 sites, 3 directions,
    2 betas, 40 listed atoms of which some lie beyond every reach, 10 cell atoms, 20 rows."""
    d = (5, 6, 7)
    return Job("skew", make_inputs(40, 3, 3, d, SKEW, 7, origin=(0.1, -0.2, 0.3)), d, origin=(0.1, -0.2, 0.3), step=SKEW, core2=0.04,
               cutoff2=4.0, betas=(0.4, 1.0), alpha=0.6)


@once
def skip_job():
    """Test 6: listed atoms spread 5 beyond the cell at a cutoff of 1.5: most are beyond the reach of most groups."""
    d = (9, 6, 5)
    return Job("skip", make_inputs(70, 2, 4, d, SKEW, 17, pad=5.0), d, step=SKEW, core2=0.04, cutoff2=2.25, betas=(0.7,), alpha=0.8)


@once
def wide_job():
    """K = 65 (a wave of rows and one more), M = 5 (an orientation tile and one more), n_cell = 67 (the 64 strided
    accumulators and three that take a second atom)."""
    d = (6, 5, 3)
    return Job("wide", make_inputs(20, 1, 5, d, C.ortho(0.7), 27, n_cell=67, K=65, top=3), d, step=C.ortho(0.7), core2=0.04,
               cutoff2=6.25, betas=(0.5,), alpha=0.5)


@once
def shared_jobs():
    """Test 11: six jobs on one set of inputs -- charged and not, 1 .. 3 rows of betas, with and without maps, three
    grids."""
    inputs = make_inputs(30, 2, 6, (8, 8, 8), C.ortho(0.5), 37, K=12)
    grids = ((8, 8, 8), (5, 3, 2), (1, 9, 4), (4, 4, 4), (7, 2, 3), (3, 3, 3))
    return [Job(f"shared-{q}", inputs, d, step=C.ortho(0.5), core2=0.01, cutoff2=4.0, betas=(0.2 + q, 0.4)[:1 + q % 2],
                alpha=0.3 + 0.1 * q, charged=int(q != 2), map=q != 1) for q, d in enumerate(grids)]


def pack(jobs, hole=0):
    """The arrays of one call: (rec, xyz, coef, offsets, dirs, betas, site_q, cell, kvecs, n_maps, n_levels, n_out); inputs
    that jobs share are stored once; `hole` rows and entries nobody owns in front of each job's outputs."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.RIGID_CELL_EWALD_JOB_DTYPE)
    stored, order = {}, []
    at = dict(xyz=0, rows=0, sites=0, dirs=0, cell=0, k=0)
    for j in jobs:
        if id(j.inputs) not in stored:
            stored[id(j.inputs)] = dict(at)
            order.append(j.inputs)
            i = j.inputs
            at["xyz"] += len(i.xyz)
            at["rows"] += i.coef.shape[0] * i.coef.shape[1]
            at["sites"] += len(i.offsets)
            at["dirs"] += len(i.dirs)
            at["cell"] += len(i.cell)
            at["k"] += len(i.kvecs)
    n_maps = n_levels = n_out = n_betas = 0
    betas = []
    for k, j in enumerate(jobs):
        a, i = stored[id(j.inputs)], j.inputs
        n_out, n_levels = n_out + hole, n_levels + hole
        n_maps += hole if j.map else 0
        rec["cell"][k] = (a["xyz"], len(i.xyz), a["rows"], n_betas, len(j.betas), a["sites"], len(i.offsets), a["dirs"], len(i.dirs),
                          n_levels, n_maps if j.map else -1, n_out, j.origin, j.step, j.core2, j.cutoff2, *j.dims, 0)
        rec[k]["charge_first"], rec[k]["cell_first"], rec[k]["n_cell"] = a["sites"], a["cell"], len(i.cell)
        rec[k]["k_first"], rec[k]["n_k"], rec[k]["alpha"], rec[k]["charged"] = a["k"], len(i.kvecs), j.alpha, j.charged
        betas.append(j.betas)
        n_betas += len(j.betas)
        n_out += 1
        n_levels += len(j.betas)
        n_maps += (len(j.betas) + 1) * j.voxels if j.map else 0

    def cat(parts, width):
        return np.concatenate([np.zeros((0, width))] + parts) if width else np.concatenate([np.zeros(0)] + parts)

    return (rec, cat([i.xyz for i in order], 3), cat([i.coef.reshape(-1, 3) for i in order], 3), cat([i.offsets for i in order], 0),
            cat([i.dirs for i in order], 3), cat(betas, 0), cat([i.site_q for i in order], 0), cat([i.cell for i in order], 4),
            cat([i.kvecs for i in order], 4), n_maps, n_levels, n_out)


def run(ctx, packed, **kw):
    """pw_rigid_cell_ewald into SENTINEL-filled arrays: (out, levels, maps).  kw: workspace_bytes, diagnostics, skip."""
    rec, xyz, coef, offsets, dirs, betas, site_q, cell, kvecs, n_maps, n_levels, n_out = packed
    out, levels, maps = C.blank(n_out, n_levels, n_maps)
    return ctx.rigid_cell_ewald(rec, xyz, coef, offsets, dirs, betas, site_q, cell, kvecs, out=out, levels=levels, maps=maps, **kw)


def same(got, want):
    return C.same(got, want)


def kvectors(j: Job):
    """(K, 3): 2 pi (h a* + k b* + l c*) of the job's cell."""
    nx, ny, nz = j.dims
    ax, bx, by, cx, cy, cz = j.step
    cell = np.array([[nx * ax, ny * bx, nz * cx], [0.0, ny * by, nz * cy], [0.0, 0.0, nz * cz]])   # columns as vectors
    return 2.0 * math.pi * j.inputs.kvecs[:, :3] @ np.linalg.inv(cell)


def reference(j: Job):
    """(planes (L + 1, V): zbar_0 .. zbar_{L-1} and umin_v; blocked poses; dead voxels; the pair terms a pose) of a charged
    job by the definition, plainly: every atom, math.erfc, the reciprocal sum by complex exponentials."""
    i = j.inputs
    c = j.uncharged_case()
    x, y, z = C.centres(c)
    V, M, S = len(x), len(i.dirs), len(i.offsets)
    erfc = np.vectorize(math.erfc)
    U = np.zeros((V, M))
    blocked = np.zeros((V, M), dtype=bool)
    for s, t in enumerate(i.offsets):
        px, py, pz = (p[:, None] + (t * i.dirs[:, a])[None, :] for a, p in enumerate((x, y, z)))
        for (X, Y, Z), (a, b, cc) in zip(i.xyz, i.coef[s]):
            dx, dy, dz = px - X, py - Y, pz - Z
            r2 = (dx * dx + dy * dy) + dz * dz
            blocked |= r2 <= j.core2
            r = np.sqrt(r2)
            s6 = 1.0 / r2 ** 3
            u = s6 * (a * s6 - b) + cc * erfc(j.alpha * r) / r
            U += np.where(r2 <= j.cutoff2, u, 0.0)
    kv = kvectors(j)
    w = i.kvecs[:, 3]
    rho = (i.cell[:, 3][None, :] * np.exp(1j * (kv @ i.cell[:, :3].T))).sum(axis=1)                      # (K,)
    centre = np.exp(1j * (np.stack([x, y, z], axis=1) @ kv.T))                                             # (V, K)
    for o, d in enumerate(i.dirs):
        form = (i.site_q[None, :] * np.exp(1j * (kv @ d)[:, None] * i.offsets[None, :])).sum(axis=1)      # (K,)
        U[:, o] += (w[None, :] * (rho * np.conj(form))[None, :] * np.conj(centre)).real.sum(axis=1)
    live = ~blocked
    planes = np.zeros((len(j.betas) + 1, V))
    planes[-1] = np.where(live, U, np.inf).min(axis=1)
    for b, beta in enumerate(j.betas):
        planes[b] = np.where(live, np.exp(-beta * np.where(live, U, 0.0)), 0.0).sum(axis=1) / M
    return planes, int(blocked.sum()), int((~live.any(axis=1)).sum()), S * len(i.xyz)


def erfc_sweep():
    """The arguments of the pw_erfc tests: 0, every piece boundary of pw_math.hpp with both neighbours, the onset of the
    denormals with both neighbours, 2^21, and 10^5 log-spaced points from 2^-60 to 30, ascending."""
    lo, hi = 26.0, 27.0
    while np.nextafter(lo, hi) < hi:                                 # the first argument whose erfc is below the normals
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if math.erfc(mid) < 2.2250738585072014e-308 else (mid, hi)
    points = [0.0, 2.0 ** 21]
    for b in (2.0 ** -56, 0.25, 0.84375, 1.25, 2.857142857142857, 28.0, hi):
        points += [np.nextafter(b, 0.0), b, np.nextafter(b, 100.0)]
    return np.unique(np.concatenate([points, np.exp(np.linspace(math.log(2.0 ** -60), math.log(30.0), 100000))]))


def erfc_ulps(got, x):
    """(the largest error in ulps of the C library's value over the arguments whose value is a normal number, the
    arguments beyond them)."""
    want = np.array([math.erfc(v) for v in x])
    normal = want >= 2.2250738585072014e-308
    ulp = np.array([math.ulp(v) for v in want[normal]])
    return float((np.abs(got[normal] - want[normal]) / ulp).max()), ~normal
