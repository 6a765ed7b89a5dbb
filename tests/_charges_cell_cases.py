"""Case list, restatement and independent model of the periodic charge equilibration tests (tests/test_charges_cell.py,
tests/test_gpu_charges_cell.py).  numpy only, seeded.

`restate` is the definition of pywindow_amd/csrc/pw_charges_cell.hpp written again, operation by operation: the lists of
R by the formulas, the phase tables and their combination, every sum by 64 strided accumulators folded pairwise, every
fused multiply-add exact (tests/_charges_cases.py: fma).  The two elementary functions the definition names, pw_erfc and
pw_sincos, are the library's own through its test hooks (Context.erfc, Context.sincos); tests/test_ewald_host.py and
tests/test_math.py hold those to the C library.  Everything else owes nothing to the library.

`dense_model` is the other reference: the matrix as a dense array straight from the formulas -- math.erfc, G as an explicit
cosine matrix over the rows -- and the constrained minimum by numpy.linalg.solve of the bordered system."""
import dataclasses
import functools
import math

import numpy as np

import _charges_cases as Q

HCNO = Q.HCNO
K_EV = Q.K_EV
ACC = Q.ACC
NAN = Q.NAN
SENTINEL = Q.SENTINEL
NOT_CONVERGED, BREAKDOWN, NO_SUM = 1, 2, 4
TWO_OVER_SQRT_PI = 1.1283791670955126
TWO_PI = 6.283185307179586
MAX_INDEX = 64
f8 = np.float64


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    xyz: np.ndarray               # in the triangular frame of `edges`, as the entry takes them
    params: np.ndarray
    edges: np.ndarray             # a1, b1, b2, c1, c2, c3
    cutoff2: float
    on2: float
    off2: float
    alpha: float = 0.0
    kvecs: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 4)))
    K: float = K_EV
    tol: float = 1e-10
    max_iter: int = 1000
    converges: bool = True        # meant to converge: the restatement ends with no flag

    def but(self, name, **changes):
        return dataclasses.replace(self, name=name, **changes)

    @property
    def cell(self):
        """The lattice, columns as vectors."""
        a1, b1, b2, c1, c2, c3 = (float(v) for v in self.edges)
        return np.array([[a1, b1, c1], [0.0, b2, c2], [0.0, 0.0, c3]])


# ---- the definition ------------------------------------------------------------------------------------------------
def _hooks():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=1)


def shifts(edges):
    e = [f8(v) for v in edges]
    m = np.arange(27)
    la, lb, lc = (m // 9 - 1).astype(f8), ((m // 3) % 3 - 1).astype(f8), (m % 3 - 1).astype(f8)
    return (la * e[0] + lb * e[1]) + lc * e[3], lb * e[2] + lc * e[4], lc * e[5]


def candidates(case):
    """(r2 (n, n, 27), counts (n, n, 27)): row i, column j, image m."""
    x = np.asarray(case.xyz, dtype=f8)
    tx, ty, tz = shifts(case.edges)
    d = [(x[:, None, None, a] - x[None, :, None, a]) + t[None, None, :] for a, t in enumerate((tx, ty, tz))]
    r2 = Q.fma(d[2], d[2], Q.fma(d[1], d[1], d[0] * d[0]))
    counts = r2 <= f8(case.cutoff2)
    i = np.arange(len(x))
    counts[i, i, 13] = False
    return r2, counts


def switch(r2, on2, off2):
    u = (r2 - f8(on2)) / (f8(off2) - f8(on2))
    u = np.where(u < 0.0, 0.0, np.where(u > 1.0, 1.0, u))
    return 1.0 - ((u * u) * u) * ((10.0 - 15.0 * u) + (6.0 * u) * u)


def terms(case, r2, Ji, Jj, erfc):
    """chc_term of the candidates r2 (any shape) with the hardness of row and column."""
    K, alpha = f8(case.K), f8(case.alpha)
    with np.errstate(all="ignore"):
        s = switch(r2, case.on2, case.off2)
        r = np.sqrt(r2)
        a = (2.0 * K) / (Ji + Jj)
        shielded = K / np.sqrt(r2 + a * a)
        point = K / r
        e = erfc(alpha * r).reshape(r.shape)
        away = s * (shielded - point) + (K * e) / r
        at = s * ((Ji + Jj) / 2.0) - (K * alpha) * TWO_OVER_SQRT_PI
    return np.where(r2 == 0.0, at, away)


def rows_of_R(case, erfc):
    """Row i's list as padded arrays: (values (n, width), columns (n, width), lengths (n,))."""
    J = np.ascontiguousarray(case.params[:, 1], dtype=f8)
    n = len(J)
    r2, counts = candidates(case)
    i, j, m = np.nonzero(counts)                                     # (C order: row, then column, then image)
    v = terms(case, r2[i, j, m], J[i], J[j], erfc)
    lengths = counts.reshape(n, -1).sum(axis=1)
    width = max(int(lengths.max()) if n else 0, 1)
    width += (-width) % ACC
    first = np.concatenate([[0], np.cumsum(lengths)])
    at = np.arange(len(i)) - first[i]
    values, columns = np.zeros((n, width)), np.zeros((n, width), dtype=np.int64)
    values[i, at], columns[i, at] = v, j
    return values, columns, lengths


def kvec(edges, h, k, l):
    a1, b1, b2, c1, c2, c3 = (f8(1.0) * f8(v) for v in edges)
    h, k, l = f8(h), f8(k), f8(l)
    with np.errstate(all="ignore"):
        ax, ay, az = 1.0 / a1, -(b1 / (a1 * b2)), (b1 * c2 - b2 * c1) / ((a1 * b2) * c3)
        by, bz, cz = 1.0 / b2, -(c2 / (b2 * c3)), 1.0 / c3
        return f8(TWO_PI) * (h * ax), f8(TWO_PI) * (h * ay + k * by), f8(TWO_PI) * ((h * az + k * bz) + l * cz)


def phases(case, sincos):
    """(cos (n_k, n), sin (n_k, n)) of chc_phase, from the per-atom per-axis tables."""
    x = np.asarray(case.xyz, dtype=f8)
    kv = np.asarray(case.kvecs, dtype=f8).reshape(-1, 4)
    idx = kv[:, :3].astype(np.int64)
    picked = []
    for a in range(3):
        top = int(np.abs(idx[:, a]).max()) if len(idx) else 0
        cos, sin = np.zeros((top + 1, len(x))), np.zeros((top + 1, len(x)))
        for m in range(top + 1):
            kx, ky, kz = kvec(case.edges, *(m if b == a else 0 for b in range(3)))
            sin[m], cos[m] = sincos((kx * x[:, 0] + ky * x[:, 1]) + kz * x[:, 2])
        mag = np.abs(idx[:, a])
        picked.append((cos[mag], np.where((idx[:, a] < 0)[:, None], -sin[mag], sin[mag])))

    def add(p, q):
        return p[0] * q[0] - p[1] * q[1], p[1] * q[0] + p[0] * q[1]

    return add(add(picked[0], picked[1]), picked[2])


def _row_sums(values, columns, lengths, p):
    """The rule of the sums over every row's list."""
    n, width = values.shape
    acc = np.zeros((n, ACC))
    lane = np.arange(ACC)
    for c0 in range(0, width, ACC):
        live = (c0 + lane)[None, :] < lengths[:, None]
        new = Q.fma(values[:, c0:c0 + ACC], p[columns[:, c0:c0 + ACC]], acc)
        acc = np.where(live, new, acc)
    return Q._fold(acc)


def restate(case):
    """(charges (n,), row): the row a dict with the fields of pw_charges_cell_out."""
    hooks = _hooks()
    chi, J = (np.ascontiguousarray(np.asarray(case.params, dtype=f8).reshape(-1, 2)[:, c]) for c in (0, 1))
    n = len(J)
    kv = np.asarray(case.kvecs, dtype=f8).reshape(-1, 4)
    nk = len(kv)
    values, columns, lengths = rows_of_R(case, hooks.erfc)
    pc, ps = phases(case, hooks.sincos)
    w = np.ascontiguousarray(kv[:, 3])
    own = (f8(case.K) * f8(case.alpha)) * TWO_OVER_SQRT_PI
    tol2 = f8(case.tol) * f8(case.tol)

    def product(p):
        real = _row_sums(values, columns, lengths, p)
        if nk:
            Sc, Ss = Q.dots(np.broadcast_to(p, (nk, n)), pc), Q.dots(np.broadcast_to(p, (nk, n)), ps)
            rec = Q.dots(np.broadcast_to(w, (n, nk)), pc.T * Sc[None, :] + ps.T * Ss[None, :])
        else:
            rec = np.zeros(n)
        return ((J - own) * p + real) + rec

    with np.errstate(all="ignore"):
        sJ = Q.sums(1.0 / J)[0]

        def precondition(r):
            u = r / J
            lam = Q.sums(u)[0] / sJ
            return u - lam / J, lam

        q, r = np.zeros(n), -chi
        z, lam = precondition(r)
        p = z.copy()
        rz = rz0 = Q.dots(r - lam, z)[0]
        ran_out = broke = False
        k = 0
        while True:
            if rz <= tol2 * rz0:
                break
            if k == case.max_iter:
                ran_out = True
                break
            y = product(p)
            pAp = Q.dots(p, y)[0]
            if not pAp > 0.0:
                broke = True
                break
            al = rz / pAp
            q = Q.fma(al, p, q)
            r = Q.fma(-al, y, r)
            z, lam = precondition(r)
            rz_new = Q.dots(r - lam, z)[0]
            beta = rz_new / rz
            p = Q.fma(beta, p, z)
            rz = rz_new
            k += 1
        flags = (NOT_CONVERGED if ran_out else 0) | (BREAKDOWN if broke else 0) | (0 if sJ > 0.0 else NO_SUM)
        lost = bool(flags & (BREAKDOWN | NO_SUM))
        pad = (-n) % ACC
        grid = lambda v, fill: np.concatenate([v, np.full(pad, fill)]).reshape(-1, ACC)
        lo, hi = np.full(ACC, np.inf), np.full(ACC, -np.inf)
        for row_lo, row_hi in zip(grid(q, np.inf), grid(q, -np.inf)):
            lo = np.where(row_lo < lo, row_lo, lo)
            hi = np.where(row_hi > hi, row_hi, hi)
        q_min = Q._fold(lo, lambda b, a: np.where(b < a, b, a))
        q_max = Q._fold(hi, lambda b, a: np.where(b > a, b, a))
        energy = f8(0.5) * Q.dots(chi, q)[0]
    gone = lambda v: Q._canon(np.full(np.shape(v), NAN) if lost else v)
    row = dict(mu=gone(-lam), energy=gone(energy), q_min=gone(q_min), q_max=gone(q_max), iterations=k, flags=flags)
    return gone(q), row


# ---- the independent model -----------------------------------------------------------------------------------------
def dense_matrix(xyz, params, cell, cutoff, shield, alpha, kvecs, K=K_EV, images=1):
    """A = D + R + G as a dense array straight from the formulas: the atoms wrapped into `cell` (columns as vectors), the
    images {-images .. images}^3, math.erfc, G as an explicit cosine matrix over the rows (h, k, l, w) of `kvecs`."""
    x = np.asarray(xyz, dtype=f8)
    J = np.asarray(params, dtype=f8)[:, 1]
    n = len(x)
    cell = np.asarray(cell, dtype=f8)
    frac = x @ np.linalg.inv(cell).T
    x = (frac - np.floor(frac)) @ cell.T
    span = np.arange(-images, images + 1)
    L = np.array([(a, b, c) for a in span for b in span for c in span], dtype=f8) @ cell.T
    d = x[:, None, None, :] - x[None, :, None, :] + L[None, None, :, :]
    r2 = (d * d).sum(axis=3)
    inside = r2 <= cutoff * cutoff
    inside[np.arange(n), np.arange(n), len(L) // 2] = False
    on2, off2 = shield[0] ** 2, shield[1] ** 2
    u = np.clip((r2 - on2) / (off2 - on2), 0.0, 1.0)
    s = 1.0 - u ** 3 * (10.0 - 15.0 * u + 6.0 * u * u)
    Jm = 0.5 * (J[:, None, None] + J[None, :, None])
    a = K / Jm
    erfc = np.vectorize(math.erfc, otypes=[f8])
    with np.errstate(all="ignore"):
        r = np.sqrt(r2)
        away = s * (K / np.sqrt(r2 + a * a) - K / r) + K * erfc(alpha * r) / r
    at = s * Jm - K * 2.0 * alpha / math.sqrt(math.pi)
    R = np.where(inside, np.where(r2 == 0.0, at, away), 0.0).sum(axis=2)
    A = R + np.diag(J - K * 2.0 * alpha / math.sqrt(math.pi))
    kv = np.asarray(kvecs, dtype=f8).reshape(-1, 4)
    if len(kv):
        k = 2.0 * math.pi * kv[:, :3] @ np.linalg.inv(cell)          # rows: h a* + k b* + l c*
        ph = x @ k.T
        A = A + (np.cos(ph) * kv[:, 3]) @ np.cos(ph).T + (np.sin(ph) * kv[:, 3]) @ np.sin(ph).T
    return A


def bordered(A, chi, Q_total=0.0):
    """(q, mu): the minimum of chi.q + q.A.q / 2 at sum q = Q_total through numpy.linalg.solve."""
    n = len(A)
    B = np.zeros((n + 1, n + 1))
    B[:n, :n] = A
    B[:n, n] = B[n, :n] = 1.0
    sol = np.linalg.solve(B, np.concatenate([-np.asarray(chi, dtype=f8), [Q_total]]))
    return sol[:n], -sol[n]


def dense_model(case):
    """(q, mu, A) of a case."""
    cutoff, shield = math.sqrt(case.cutoff2), (math.sqrt(case.on2), math.sqrt(case.off2))
    A = dense_matrix(case.xyz, case.params, case.cell, cutoff, shield, case.alpha, case.kvecs, case.K)
    q, mu = bordered(A, case.params[:, 0])
    return q, mu, A


def public_model(xyz, elements, lattice, cutoff=12.0, tolerance=1e-6, shield=(4.0, 6.0), images=1):
    """(q, mu) of the dense model for the arguments of pw.equilibrate_cell_charges: the lattice as the caller gives it,
    alpha and the rows by pw.ewald_parameters with the weights in eV."""
    import pywindow_amd as pw
    from pywindow_amd.charges import COULOMB_EV, qeq_parameters
    from pywindow_amd.rigid import COULOMB

    alpha, kv = pw.ewald_parameters(lattice, cutoff, tolerance)
    kv = kv.copy()
    kv[:, 3] *= COULOMB_EV / COULOMB
    p = qeq_parameters(elements)
    return bordered(dense_matrix(xyz, p, lattice, cutoff, shield, alpha, kv, COULOMB_EV, images), p[:, 0])


def vacuum_model(xyz, elements):
    """(q, mu) of pw_charges' model by the same route: A_ii = J_i, A_ij = K / sqrt(r^2 + a^2)."""
    from pywindow_amd.charges import COULOMB_EV, qeq_parameters

    p = qeq_parameters(elements)
    return bordered(Q.matrix(np.asarray(xyz, dtype=f8), np.ascontiguousarray(p[:, 1]), COULOMB_EV), p[:, 0])


# ---- the cases -----------------------------------------------------------------------------------------------------
SKEWED = np.array([1.0, 0.31, 0.94, -0.23, 0.17, 0.89])              # edges of a unit skewed cell
ORTHO = np.array([1.0, 0.0, 1.13, 0.0, 0.0, 0.91])


def widths(edges):
    a1, b1, b2, c1, c2, c3 = (float(v) for v in edges)
    inv = np.linalg.inv(np.array([[a1, b1, c1], [0.0, b2, c2], [0.0, 0.0, c3]]))
    return 1.0 / np.sqrt((inv * inv).sum(axis=1))


def rows_for(edges, cutoff, tolerance, K=K_EV):
    """(alpha, rows) of pw.ewald_parameters on the cell, the weights in eV per squared charge for the constant K."""
    import pywindow_amd as pw
    from pywindow_amd.rigid import COULOMB

    case = Case("", None, None, np.asarray(edges, dtype=f8), 0.0, 0.0, 0.0)
    alpha, kv = pw.ewald_parameters(case.cell, cutoff, tolerance)
    kv = kv.copy()
    kv[:, 3] *= K / COULOMB
    return float(alpha), np.ascontiguousarray(kv)


def lattice_gas(n, seed, edges, spread=0.25):
    """n atoms of H, C, N, O on the sites of the smallest cubic sublattice of the cell that holds them, each moved by up to
    `spread` of the site spacing, in the triangular frame: no two atoms on top of each other."""
    rng = np.random.default_rng(seed)
    g = 1
    while g ** 3 < n:
        g += 1
    sites = rng.permutation(g ** 3)[:n]
    frac = (np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) + 0.5 + rng.uniform(-spread, spread, (n, 3))) / g
    case = Case("", None, None, np.asarray(edges, dtype=f8), 0.0, 0.0, 0.0)
    return frac @ case.cell.T, Q.rows_of(rng.choice(list(HCNO), n))


def gas_system(n, seed, lattice, spread=0.25):
    """(elements, xyz, lattice) for the public layer: the lattice gas of `lattice_gas` in a caller's cell (columns as
    vectors), element symbols in place of rows."""
    rng = np.random.default_rng(seed)
    g = 1
    while g ** 3 < n:
        g += 1
    sites = rng.permutation(g ** 3)[:n]
    frac = (np.stack([sites // (g * g), (sites // g) % g, sites % g], axis=1) + 0.5 + rng.uniform(-spread, spread, (n, 3))) / g
    lattice = np.asarray(lattice, dtype=f8)
    return [str(e) for e in rng.choice(list(HCNO), n)], frac @ lattice.T, lattice


@functools.lru_cache(maxsize=None)
def solved(case):
    """The restatement of a case, once a process."""
    return restate(case)


def gas_case(n, seed, shape=SKEWED, cutoff=None, shield=(1.6, 2.6), tolerance=1e-4, density=0.08, **settings):
    """A lattice gas of n atoms at `density` atoms per cubic Angstrom (CC3: 0.088) in a cell of the given shape, at least 6
    Angstrom wide; the cutoff defaults to 0.8 of the smallest perpendicular width.  A case meant to converge that does
    not is replaced by the next seed, never skipped."""
    shape = np.asarray(shape, dtype=f8)
    unit = abs(shape[0] * shape[2] * shape[5])
    scale = max((n / density / unit) ** (1.0 / 3.0), 6.0 / float(widths(shape).min()))
    edges = scale * shape
    rc = 0.8 * float(widths(edges).min()) if cutoff is None else float(cutoff)
    alpha, kv = rows_for(edges, rc, tolerance)
    for attempt in range(20):
        x, p = lattice_gas(n, seed + 1000 * attempt, edges)
        case = Case(f"gas n={n}", x, p, edges, rc * rc, shield[0] ** 2, shield[1] ** 2, alpha, kv, **settings)
        if not case.converges or solved(case)[1]["flags"] == 0:
            return case
    raise AssertionError(f"no converging gas of {n} atoms in 20 seeds")


SIZES = (1, 2, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def cases():
    out = [gas_case(n, 100 + n, SKEWED if k % 2 == 0 else ORTHO).but(f"gas n={n}, {'skewed' if k % 2 == 0 else 'orthorhombic'}")
           for k, n in enumerate(SIZES)]
    base = out[SIZES.index(65)]
    small = gas_case(12, 7, SKEWED)
    # the cutoff IS the smallest perpendicular width (of an orthorhombic cell: its shortest edge, so an atom's own image
    # along it sits at r2 == cutoff2 exactly): a pair counts through several images, an atom sees its own
    brick = gas_case(12, 8, ORTHO)
    wide = float(brick.edges[5])
    assert abs(wide - float(widths(brick.edges).min())) < 1e-12
    alpha, kv = rows_for(brick.edges, wide, 1e-4)
    at_width = brick.but("cutoff == the smallest width", cutoff2=wide * wide, alpha=alpha, kvecs=kv, converges=False)
    r2, counts = candidates(at_width)
    assert (counts.sum(axis=2) > 1).any() and counts[np.arange(12), np.arange(12)].sum(axis=1).min() == 2
    out.append(at_width)
    # no pair at all: the charges follow from chi and J alone
    lonely = small.but("no pair within the cutoff", cutoff2=0.01, on2=0.0025, off2=0.01, alpha=0.0, kvecs=np.zeros((0, 4)))
    assert not candidates(lonely)[1].any()
    out.append(lonely)
    # an atom exactly on a cell face (the origin: on three)
    x = small.xyz.copy()
    x[0] = 0.0
    out.append(small.but("an atom on a face", xyz=x))
    # two coincident atoms of different elements
    x = small.xyz.copy()
    x[1] = x[0]
    p = small.params.copy()
    p[0], p[1] = HCNO["H"], HCNO["O"]
    out.append(small.but("coincident, two elements", xyz=x, params=p, converges=False))
    # a pair exactly at r2 == cutoff2, == shield_on2, == shield_off2: dx = 3 exactly in a 9 x 10.17 x 8.19 cell
    edges = 9.0 * ORTHO
    x = np.array([[1.0, 1.0, 1.0], [4.0, 1.0, 1.0], [2.5, 6.0, 4.5], [7.0, 3.0, 6.0]])
    p = Q.rows_of(["C", "N", "O", "H"])
    alpha, kv = rows_for(edges, 3.0, 1e-4)
    exact = Case("a pair at r2 == cutoff2", x, p, edges, 9.0, 1.0, 4.0, alpha, kv, converges=False)
    r2, counts = candidates(exact)
    assert r2[0, 1, 13] == 9.0 and counts[0, 1, 13] and counts[1, 0, 13]
    alpha, kv = rows_for(edges, 5.0, 1e-4)
    out += [exact, exact.but("a pair at r2 == shield_on2", cutoff2=25.0, on2=9.0, off2=16.0, alpha=alpha, kvecs=kv),
            exact.but("a pair at r2 == shield_off2", cutoff2=25.0, on2=4.0, off2=9.0, alpha=alpha, kvecs=kv)]
    # alpha = 0 with no rows: the purely truncated sum
    out.append(base.but("alpha = 0, n_k = 0", alpha=0.0, kvecs=np.zeros((0, 4)), converges=False))
    # 64 and 65 rows; an index at the cap
    assert len(base.kvecs) > 65
    out += [base.but("n_k = 64", kvecs=base.kvecs[:64].copy(), converges=False),
            base.but("n_k = 65", kvecs=base.kvecs[:65].copy(), converges=False)]
    capped = np.concatenate([small.kvecs, [[MAX_INDEX, 0.0, 0.0, 1e-3], [0.0, -MAX_INDEX, 0.0, 1e-3], [0.0, 1.0, MAX_INDEX, 1e-3]]])
    out.append(small.but("indices at the cap", kvecs=capped, converges=False))
    # tol at both ends
    out += [base.but("tol 1e-14", tol=1e-14, converges=False), base.but("tol 1e-2", tol=1e-2)]
    # max_iter = 1: not converged, the charges of the last step
    short = base.but("max_iter 1", max_iter=1, converges=False)
    assert solved(short)[1]["flags"] == NOT_CONVERGED and np.isfinite(solved(short)[0]).all() and solved(short)[0].any()
    out.append(short)
    for c in out:
        if c.converges:
            assert solved(c)[1]["flags"] == 0, c.name
    return tuple(out)


@functools.lru_cache(maxsize=None)
def breakdown_case():
    """J tiny against the couplings: four atoms 0.5 Angstrom apart with J = 1e-3 eV.  The matrix is indefinite on the neutral
    subspace and the restatement finds !(pAp > 0) within a few steps."""
    edges = 8.0 * ORTHO
    x = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [1.0, 1.5, 1.0], [1.0, 1.0, 1.5]])
    p = np.array([[1.0, 1e-3], [2.0, 1e-3], [3.0, 1e-3], [5.0, 1e-3]])
    alpha, kv = rows_for(edges, 4.0, 1e-4)
    c = Case("breakdown", x, p, edges, 16.0, 1.0, 4.0, alpha, kv, converges=False)
    q, row = solved(c)
    assert row["flags"] & BREAKDOWN and np.isnan(q).all() and row["iterations"] <= len(x)
    return c


def cc3_cell():
    """(elements, coordinates, lattice) of the 1344-atom CC3 cell of the golden file."""
    import pathlib

    with np.load(pathlib.Path(__file__).parent / "golden" / "rebuild.npz", allow_pickle=True) as d:
        return [str(e) for e in d["cc3_cell__in_elements"]], d["cc3_cell__in_coordinates"], d["cc3_cell__in_lattice"]


def other_shapes():
    """What a call before the call under test holds: other sizes, other values."""
    return [gas_case(40, 31, ORTHO, tol=1e-4, converges=False), gas_case(131, 32, SKEWED, tol=1e-3, converges=False)]


# ---- calls ---------------------------------------------------------------------------------------------------------
def pack(jobs, hole=0, reverse=False, pad=0):
    """(records, xyz, params, kvecs, n_points, rows of out, entries of charges): the jobs' atoms, parameters and rows one
    after another behind `pad` rows nobody reads; `hole` rows of out and entries of charges nobody owns in front of every
    job's; with `reverse` the outputs go from the back to the front."""
    from pywindow_amd import _lib

    xyz, prm, kvs, rec = [np.full((pad, 3), 1e3)], [np.full((pad, 2), 7.0)], [np.full((pad, 4), 3.0)], []
    at, k_at = pad, pad
    N = len(jobs)
    sizes = np.array([len(c.xyz) for c in jobs], dtype=np.int64)
    before = np.concatenate([[0], np.cumsum(sizes + hole)[:-1]])
    total = int((sizes + hole).sum())
    q_first = total - before - sizes if reverse else before + hole
    for k, c in enumerate(jobs):
        n, nk = len(c.xyz), len(c.kvecs)
        slot = N - 1 - k if reverse else k
        rec.append((at, at, n, k_at, nk, c.edges, c.K, c.alpha, c.cutoff2, c.on2, c.off2, c.tol, c.max_iter, int(q_first[k]),
                    slot * (hole + 1) + hole))
        xyz.append(c.xyz)
        prm.append(c.params)
        kvs.append(np.asarray(c.kvecs, dtype=f8).reshape(-1, 4))
        at += n
        k_at += nk
    rec = np.array(rec, dtype=_lib.CHARGES_CELL_JOB_DTYPE)
    return rec, np.concatenate(xyz), np.concatenate(prm), np.concatenate(kvs), max(at, total), N * (hole + 1), total


def blank(packed):
    from pywindow_amd import _lib

    dt = _lib.CHARGES_CELL_OUT_DTYPE
    rows = np.frombuffer(bytearray([SENTINEL]) * (packed[5] * dt.itemsize), dtype=dt).copy()
    q = np.frombuffer(bytearray([SENTINEL]) * (8 * packed[4]), dtype=f8).copy()
    return q, rows


def raw(ctx, packed, workspace_bytes=None, n_points=None, n_kvecs=None):
    """pw_charges_cell through ctypes into sentinel-filled outputs (through the library's test entry when
    `workspace_bytes` is given): (rc, (charges, rows))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, prm, kvs, points = packed[:5]
    rec = np.ascontiguousarray(rec, dtype=_lib.CHARGES_CELL_JOB_DTYPE)
    x = np.zeros((points, 3))
    x[:len(xyz)] = xyz
    p = np.zeros((points, 2))
    p[:len(prm)] = prm
    kvs = np.ascontiguousarray(kvs)
    q, rows = blank(packed)
    args = [ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, p.ctypes.data, points if n_points is None else n_points,
            kvs.ctypes.data, len(kvs) if n_kvecs is None else n_kvecs, q.ctypes.data, rows.ctypes.data]
    if workspace_bytes is None:
        rc = L.pw_charges_cell(*args)
    else:
        rc = L.pw_internal_charges_cell(*args, int(workspace_bytes), None)
    return rc, (q, rows)


def expected(jobs, packed):
    """What `raw` returns for the packed jobs, from the restatement."""
    q, rows = blank(packed)
    for c, r in zip(jobs, packed[0]):
        charges, row = solved(c)
        q[r["charge_first"]:r["charge_first"] + r["n"]] = charges
        for name, value in row.items():
            rows[r["out"]][name] = value
    return q, rows


same = Q.same
first_difference = Q.first_difference


# ---- refusals ------------------------------------------------------------------------------------------------------
def bad_batches():
    """(packed, n_points or None, n_kvecs or None, what): two-job calls whose job 1 is refused for `what`."""
    good = [gas_case(5, 61, ORTHO, converges=False), gas_case(7, 62, SKEWED, converges=False)]
    k0 = len(good[0].kvecs)

    def with_job(change):
        packed = list(pack(good))
        packed[0] = packed[0].copy()
        change(packed)
        return tuple(packed)

    def setter(name, value, index=None):
        def change(packed):
            if index is None:
                packed[0][name][1] = value
            else:
                packed[0][name][1][index] = value
        return change

    def value_at(which, row, column, value):
        def change(packed):
            packed[which] = packed[which].copy()
            packed[which][row, column] = value
        return change

    atom, krow = 5 + 3, k0 + 2                                       # atom 3 and row 2 of job 1
    on2, off2, cut2 = (float(good[1].on2), float(good[1].off2), float(good[1].cutoff2))
    out = [(setter("n", 0), "n < 1"),
           (setter("xyz_first", -1), "atoms outside xyz"),
           (setter("xyz_first", 6), "atoms outside xyz"),
           (setter("param_first", 6), "parameters outside params"),
           (setter("charge_first", 6), "outside charges"),
           (setter("k_first", -1), "rows outside kvecs"),
           (setter("k_first", k0 + 1), "rows outside kvecs"),
           (setter("n_k", -1), "n_k outside"),
           (setter("n_k", 4097), "n_k outside"),
           (setter("out", -1), "a negative row"),
           (setter("out", 0), "shares its row of out"),
           (setter("charge_first", 4), "shares entries of charges"),
           (setter("edges", np.nan, 1), "an edge is not finite"),
           (setter("edges", 0.0, 0), "a1, b2 or c3 is not positive"),
           (setter("edges", -1.0, 2), "a1, b2 or c3 is not positive"),
           (setter("edges", 0.0, 5), "a1, b2 or c3 is not positive"),
           (setter("coulomb", np.nan), "coulomb is not finite"),
           (setter("coulomb", 0.0), "coulomb <= 0"),
           (setter("alpha", np.inf), "alpha is not finite"),
           (setter("alpha", -0.1), "alpha < 0"),
           (setter("cutoff2", np.nan), "cutoff2 is not finite"),
           (setter("cutoff2", 0.0), "cutoff2 <= 0"),
           (setter("shield_on2", np.nan), "the switch is not finite"),
           (setter("shield_off2", np.inf), "the switch is not finite"),
           (setter("shield_on2", -1.0), "shield_on2 < 0"),
           (setter("shield_on2", off2), "shield_on2 >= shield_off2"),
           (setter("shield_off2", 0.5 * on2), "shield_on2 >= shield_off2"),
           (setter("shield_off2", 2.0 * cut2), "shield_off2 > cutoff2"),
           (setter("tol", 1e-15), "tol outside"),
           (setter("tol", 2e-2), "tol outside"),
           (setter("tol", np.nan), "tol outside"),
           (setter("max_iter", 0), "max_iter outside"),
           (setter("max_iter", 100001), "max_iter outside"),
           (value_at(1, atom, 2, np.nan), "a coordinate is not finite"),
           (value_at(1, atom, 0, np.inf), "a coordinate is not finite"),
           (value_at(2, atom, 0, np.nan), "chi is not finite"),
           (value_at(2, atom, 1, np.inf), "J is not finite"),
           (value_at(2, atom, 1, 0.0), "J <= 0"),
           (value_at(2, atom, 1, -3.0), "J <= 0"),
           (value_at(3, krow, 0, 0.5), "an index of a row is not an integer"),
           (value_at(3, krow, 1, 65.0), "an index of a row is not an integer"),
           (value_at(3, krow, 2, np.nan), "an index of a row is not an integer"),
           (value_at(3, krow, 3, np.inf), "a weight is not finite")]
    return [(with_job(change), None, None, what) for change, what in out]
