"""Case list and restatement of the charge equilibration tests (tests/test_charges.py, tests/test_gpu_charges.py).
numpy only, seeded.  `restate` is the definition of pywindow_amd/csrc/pw_charges.hpp written again, operation by operation:
the matrix by the formula, every sum by 64 strided accumulators (a reshape) folded pairwise, every fused multiply-add
exact (`fma`: two error-free transformations and a rounding to odd, Boldo and Melquiond 2008; checked against exact
rationals in tests/test_charges.py).  It owes nothing to the library.  `numpy_solution` is the other reference: the
bordered (n + 1) system through numpy.linalg.solve.

When a case is built it is checked, on the CPU, to be fit for its purpose: a case meant to converge has a positive
definite matrix and its restatement converges within max_iter; a case that fails is replaced by the next seed, never
skipped."""
import ctypes
import dataclasses
import functools

import numpy as np

#: (chi, J) in eV of the four elements of the cases; a copy of rows of pywindow_amd.QEQ_PARAMETERS, no test needs them equal
HCNO = {"H": (4.528, 13.8904), "C": (5.343, 10.126), "N": (6.899, 11.760), "O": (8.741, 13.364)}
#: e^2 / (4 pi eps_0) in eV Angstrom, as pywindow_amd passes it
K_EV = 1389.35457644382 / 96.4853321233
SIZES = (1, 2, 3, 63, 64, 65, 129, 257)
SENTINEL = 0x5A
ACC = 64
NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
NOT_CONVERGED, BREAKDOWN, NO_SUM = 1, 2, 4


# ---- exact fused multiply-add over arrays --------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, element by element: a * b = uh + ul and c + uh = th + tl exactly, v = tl + ul
    rounded to odd, th + v rounded to nearest.  Finite operands whose product neither overflows nor falls below 1e-290."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        v, e = _two_sum(tl, ul)
        v = np.ascontiguousarray(v)
        odd = (v.view(np.int64) & 1) != 0
        v = np.where((e != 0.0) & ~odd, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)
        return np.where(uh == 0.0, c + uh, th + v)        # (a product of exactly 0 keeps IEEE's rule for the sign)


# ---- the definition ------------------------------------------------------------------------------------------------
def matrix(xyz, J, K):
    x = np.asarray(xyz, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    r2 = fma(d[..., 2], d[..., 2], fma(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
    a = (2.0 * K) / (J[:, None] + J[None, :])
    A = K / np.sqrt(r2 + a * a)
    A[np.diag_indices(len(x))] = J
    return A


def _fold(acc, op=None):
    s = ACC // 2
    while s >= 1:
        lo, hi = acc[..., :s], acc[..., s:2 * s]
        acc = lo + hi if op is None else op(hi, lo)
        s //= 2
    return acc[..., 0]


def dots(U, V):
    """The sums of U[m, i] * V[m, i] over i by the rule of the sums, for every row m."""
    U, V = np.atleast_2d(U), np.atleast_2d(V)
    acc = np.zeros((U.shape[0], ACC))
    for c0 in range(0, U.shape[1], ACC):
        w = min(ACC, U.shape[1] - c0)
        acc[:, :w] = fma(U[:, c0:c0 + w], V[:, c0:c0 + w], acc[:, :w])
    return _fold(acc)


def sums(V):
    V = np.atleast_2d(V)
    acc = np.zeros((V.shape[0], ACC))
    for c0 in range(0, V.shape[1], ACC):
        w = min(ACC, V.shape[1] - c0)
        acc[:, :w] = acc[:, :w] + V[:, c0:c0 + w]
    return _fold(acc)


def products(A, P):
    """A p for every row p of P (m, n): (m, n)."""
    n = A.shape[0]
    acc = np.zeros((P.shape[0], n, ACC))
    for c0 in range(0, n, ACC):
        w = min(ACC, n - c0)
        acc[:, :, :w] = fma(A[None, :, c0:c0 + w], P[:, None, c0:c0 + w], acc[:, :, :w])
    return _fold(acc)


def _canon(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), NAN, v)


def restate(xyz, params, Q=0.0, K=K_EV, tol=1e-10, max_iter=1000, A=None):
    """(charges (n,), row): the row a dict with the fields of pw_charges_out."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    chi, J = (np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, 2)[:, c]) for c in (0, 1))
    n = len(xyz)
    A = matrix(xyz, J, K) if A is None else A
    f8 = np.float64
    Q, tol2 = f8(Q), f8(tol) * f8(tol)
    with np.errstate(all="ignore"):
        r = np.stack([-chi, np.ones(n)])
        x = np.zeros((2, n))
        z = r / J
        p = z.copy()
        rz = dots(r, z)
        bb = dots(r, r)
        rr = bb.copy()
        frozen, broke, its = [False, False], [False, False], [0, 0]
        ran_out = False
        k = 0
        while True:
            for s in (0, 1):
                if not frozen[s] and rr[s] <= tol2 * bb[s]:
                    frozen[s], its[s] = True, k
            if all(frozen):
                break
            if k == max_iter:
                ran_out = True
                for s in (0, 1):
                    if not frozen[s]:
                        its[s] = k
                break
            on = [s for s in (0, 1) if not frozen[s]]
            Ap = products(A, p[on])
            pAp = dots(p[on], Ap)
            keep = []
            for m, s in enumerate(on):
                if pAp[m] > 0.0:
                    keep.append(m)
                else:
                    frozen[s], broke[s], its[s] = True, True, k
            on = [on[m] for m in keep]
            if on:
                Ap, pAp = Ap[keep], pAp[keep]
                alpha = (rz[on] / pAp)[:, None]
                x[on] = fma(alpha, p[on], x[on])
                r[on] = fma(-alpha, Ap, r[on])
                z[on] = r[on] / J
                both = dots(np.concatenate([r[on], r[on]]), np.concatenate([z[on], r[on]]))
                rz_new, rr[on] = both[:len(on)], both[len(on):]
                beta = (rz_new / rz[on])[:, None]
                p[on] = fma(beta, p[on], z[on])
                rz[on] = rz_new
            k += 1
        S, T = sums(x)
        flags = (NOT_CONVERGED if ran_out else 0) | (BREAKDOWN if any(broke) else 0) | (0 if T > 0.0 else NO_SUM)
        lost = bool(flags & (BREAKDOWN | NO_SUM))
        mu = (Q - S) / T
        q = fma(mu, x[1], x[0])
        pad = (-n) % ACC
        grid = lambda v, fill: np.concatenate([v, np.full(pad, fill)]).reshape(-1, ACC)
        lo, hi = np.full(ACC, np.inf), np.full(ACC, -np.inf)
        for row_lo, row_hi in zip(grid(q, np.inf), grid(q, -np.inf)):
            lo = np.where(row_lo < lo, row_lo, lo)
            hi = np.where(row_hi > hi, row_hi, hi)
        q_min = _fold(lo, lambda b, a: np.where(b < a, b, a))
        q_max = _fold(hi, lambda b, a: np.where(b > a, b, a))
        energy = f8(0.5) * (dots(chi, q)[0] + mu * Q)
        dipole = dots(np.stack([q, q, q]), np.ascontiguousarray(xyz.T))
    gone = lambda v: _canon(np.full(np.shape(v), NAN) if lost else v)
    row = dict(mu=gone(mu), sum_s=_canon(S), sum_t=_canon(T), energy=gone(energy), dipole=gone(dipole), q_min=gone(q_min),
               q_max=gone(q_max), iterations=its, flags=flags, reserved=0)
    return gone(q), row


def numpy_solution(xyz, params, Q=0.0, K=K_EV):
    """(q, mu, A, lowest eigenvalue of A) through numpy.linalg.solve of [[A, 1], [1^T, 0]] [q, -mu] = [-chi, Q]."""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 2)
    n = len(p)
    A = matrix(xyz, np.ascontiguousarray(p[:, 1]), K)
    B = np.zeros((n + 1, n + 1))
    B[:n, :n] = A
    B[:n, n] = B[n, :n] = 1.0
    sol = np.linalg.solve(B, np.concatenate([-p[:, 0], [Q]]))
    return sol[:n], -sol[n], A, float(np.linalg.eigvalsh(A)[0])


# ---- the cases -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    xyz: np.ndarray
    params: np.ndarray
    Q: float = 0.0
    K: float = K_EV
    tol: float = 1e-10
    max_iter: int = 1000
    converges: bool = True        # meant to converge: positive definite, and the restatement gets there

    def but(self, name, **changes):
        return dataclasses.replace(self, name=name, **changes)


def rows_of(elements):
    return np.array([HCNO[str(e)] for e in elements], dtype=np.float64)


def cluster(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 12.0, (n, 3)), rows_of(rng.choice(list(HCNO), n))


@functools.lru_cache(maxsize=None)
def solved(case):
    """The restatement of a case, once a process."""
    return restate(case.xyz, case.params, case.Q, case.K, case.tol, case.max_iter)


def fit(case):
    """Whether a case meant to converge does: positive definite, no flag."""
    J = np.ascontiguousarray(case.params[:, 1])
    return np.linalg.eigvalsh(matrix(case.xyz, J, case.K))[0] > 0.0 and solved(case)[1]["flags"] == 0


def converging_cluster(n, seed, **settings):
    """A random H/C/N/O cluster in a 12 Angstrom box that is fit; an unfit one is replaced by the next seed."""
    for attempt in range(20):
        case = Case(f"cluster n={n}", *cluster(n, seed + 1000 * attempt), **settings)
        if fit(case):
            return case
    raise AssertionError(f"no fit cluster of {n} atoms in 20 seeds")


@functools.lru_cache(maxsize=None)
def cc3_frames():
    """(elements, the bundled CC3 and four frames jittered by 0.12 Angstrom)."""
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    return [str(e) for e in elements], [base] + [synth.noisy_frame(base, 4100 + t, sigma=0.12) for t in range(4)]


@functools.lru_cache(maxsize=None)
def cases():
    out = [converging_cluster(n, 100 + n) for n in SIZES]
    elements, frames = cc3_frames()
    rows = rows_of(elements)
    cc3 = [Case(f"CC3 frame {t}", np.ascontiguousarray(f), rows) for t, f in enumerate(frames)]
    for c in cc3:
        assert fit(c), c.name
    out += cc3
    c65 = out[SIZES.index(65)]
    out += [c65.but("Q = +1", Q=1.0), c65.but("Q = -2", Q=-2.0)]
    for c in out[-2:]:
        assert fit(c), c.name
    # two coincident atoms: of one element the matrix is singular but both systems are consistent; of two elements it is
    # indefinite ((J1 + J2) / 2 > sqrt(J1 J2)).  Bytes only
    x, p = cluster(6, 7)
    x[1] = x[0]
    same = p.copy()
    same[1] = same[0]
    other = p.copy()
    other[0], other[1] = HCNO["H"], HCNO["C"]
    out += [Case("coincident, one element", x, same, converges=False),
            Case("coincident, two elements", x, other, converges=False)]
    # tol = 1e-2: the systems freeze at different steps
    loose = [c.but(c.name + ", tol 1e-2", tol=1e-2) for c in (cc3[0], cc3[1], out[SIZES.index(129)], c65)]
    assert any(solved(c)[1]["iterations"][0] != solved(c)[1]["iterations"][1] for c in loose)
    out += loose
    # max_iter = 1 and 3: not converged, the charges of the last step
    short = [c65.but("max_iter 1", max_iter=1, converges=False), cc3[2].but("CC3, max_iter 3", max_iter=3, converges=False)]
    for c in short:
        assert solved(c)[1]["flags"] == NOT_CONVERGED and np.isfinite(solved(c)[0]).all()
    out += short
    c64 = out[SIZES.index(64)]
    flat = c64.but("chi all zero", params=np.column_stack([np.zeros(64), c64.params[:, 1]]))
    assert solved(flat)[1]["iterations"][0] == 0 and not solved(flat)[0].any()
    out.append(flat)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def breakdown_case():
    """Two atoms with J = 1e-3 at r = 1e-3 Angstrom and a large K: the off-diagonal element exceeds the diagonal, the
    matrix is indefinite and the restatement finds !(pAp > 0)."""
    c = Case("breakdown", np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0]]), np.array([[1.0, 1e-3], [2.0, 1e-3]]), K=1e3,
             converges=False)
    q, row = solved(c)
    assert row["flags"] & BREAKDOWN and np.isnan(q).all()
    return c


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """64 jobs of 1 .. 70 atoms over 16 parameter sets, four jobs a set with coordinates of their own, and tolerances,
    total charges and bounds of several kinds."""
    sizes = (1, 2, 3, 4, 5, 7, 9, 12, 16, 20, 33, 63, 64, 65, 66, 70)
    out = []
    for g, n in enumerate(sizes):
        _, p = cluster(n, 900 + g)
        for m in range(4):
            x = np.random.default_rng(5000 + 4 * g + m).uniform(0.0, 9.0, (n, 3))
            out.append(Case(f"mixed {g}.{m}", x, p, Q=(0.0, 1.0, -1.0, 0.5)[m], tol=(1e-10, 1e-6, 1e-3, 1e-8)[(g + m) % 4],
                            max_iter=(1000, 5, 1000, 50)[(g + 2 * m) % 4], converges=False))
    return tuple(out)


def other_shapes():
    """What a call before the call under test holds: other sizes, other values."""
    return [Case("other 0", *cluster(40, 31), tol=1e-4), Case("other 1", *cluster(131, 32), Q=2.0, tol=1e-3)]


# ---- calls ---------------------------------------------------------------------------------------------------------
def pack(jobs, hole=0, reverse=False, share=True, pad=0):
    """(records, xyz, params, n_points, rows of out, entries of charges): the jobs' atoms one after another behind `pad`
    rows nobody reads; jobs whose `params` are the same array share its rows when `share`; `hole` rows of out and
    entries of charges nobody owns in front of every job's; with `reverse` the outputs go from the back to the front."""
    from pywindow_amd import _lib

    xyz, prm, rec = [np.full((pad, 3), 1e3)], [np.full((pad, 2), 7.0)], []
    at, p_at, seen = pad, pad, {}
    N = len(jobs)
    sizes = np.array([len(c.xyz) for c in jobs], dtype=np.int64)
    before = np.concatenate([[0], np.cumsum(sizes + hole)[:-1]])
    total = int((sizes + hole).sum())
    q_first = total - before - sizes if reverse else before + hole
    for k, c in enumerate(jobs):
        n = len(c.xyz)
        key = id(c.params)
        if not share or key not in seen:
            seen[key] = p_at
            prm.append(c.params)
            p_at += n
        slot = N - 1 - k if reverse else k
        rec.append((at, seen[key], n, c.Q, c.K, c.tol, c.max_iter, int(q_first[k]), slot * (hole + 1) + hole))
        xyz.append(c.xyz)
        at += n
    rec = np.array(rec, dtype=_lib.CHARGES_JOB_DTYPE)
    return rec, np.concatenate(xyz), np.concatenate(prm), max(at, p_at, total), N * (hole + 1), total


def blank(packed):
    from pywindow_amd import _lib

    rows = np.frombuffer(bytearray([SENTINEL]) * (packed[4] * _lib.CHARGES_OUT_DTYPE.itemsize), dtype=_lib.CHARGES_OUT_DTYPE).copy()
    q = np.frombuffer(bytearray([SENTINEL]) * (8 * packed[3]), dtype=np.float64).copy()
    return q, rows


def raw(ctx, packed, workspace_bytes=None, n_points=None):
    """pw_charges through ctypes into sentinel-filled outputs (through the library's test entry when `workspace_bytes`
    is given): (rc, (charges, rows))."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec, xyz, prm, points = packed[:4]
    rec = np.ascontiguousarray(rec, dtype=_lib.CHARGES_JOB_DTYPE)
    x = np.zeros((points, 3))
    x[:len(xyz)] = xyz
    p = np.zeros((points, 2))
    p[:len(prm)] = prm
    q, rows = blank(packed)
    args = [ctx._h, rec.ctypes.data, len(rec), x.ctypes.data, p.ctypes.data, points if n_points is None else n_points,
            q.ctypes.data, rows.ctypes.data]
    if workspace_bytes is None:
        rc = L.pw_charges(*args)
    else:
        rc = L.pw_internal_charges(*args, int(workspace_bytes), None)
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


def same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def first_difference(got, want):
    for which, (a, b) in zip(("charges", "rows"), zip(got, want)):
        if a.tobytes() != b.tobytes():
            if which == "charges":
                i = int(np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))[0])
                return which, i, a[i], b[i]
            for i in range(len(a)):
                if a[i].tobytes() != b[i].tobytes():
                    return which, i, a[i], b[i]
    return None


# ---- refusals ------------------------------------------------------------------------------------------------------
def bad_batches():
    """(packed, n_points or None, what): two-job calls whose job 1 is refused for `what`."""
    good = [Case("good 0", *cluster(5, 61)), Case("good 1", *cluster(7, 62))]

    def with_job(change):
        packed = list(pack(good, share=False))
        packed[0] = packed[0].copy()
        change(packed)
        return tuple(packed)

    def setter(name, value):
        def change(packed):
            packed[0][name][1] = value
        return change

    def value_at(which, column, value):
        def change(packed):
            packed[which] = packed[which].copy()
            packed[which][5 + 3, column] = value              # atom 3 of job 1
        return change

    out = [(with_job(setter("n", 0)), None, "n < 1"),
           (with_job(setter("xyz_first", -1)), None, "atoms outside xyz"),
           (with_job(setter("xyz_first", 6)), None, "atoms outside xyz"),
           (with_job(setter("param_first", 6)), None, "parameters outside params"),
           (with_job(setter("charge_first", 6)), None, "outside charges"),
           (with_job(setter("out", -1)), None, "a negative row"),
           (with_job(setter("out", 0)), None, "shares its row of out"),
           (with_job(setter("charge_first", 4)), None, "shares entries of charges"),
           (with_job(setter("total_charge", np.inf)), None, "total_charge is not finite"),
           (with_job(setter("coulomb", np.nan)), None, "coulomb is not finite"),
           (with_job(setter("coulomb", 0.0)), None, "coulomb <= 0"),
           (with_job(setter("coulomb", -1.0)), None, "coulomb <= 0"),
           (with_job(setter("tol", 1e-15)), None, "tol outside"),
           (with_job(setter("tol", 2e-2)), None, "tol outside"),
           (with_job(setter("tol", np.nan)), None, "tol outside"),
           (with_job(setter("max_iter", 0)), None, "max_iter outside"),
           (with_job(setter("max_iter", 100001)), None, "max_iter outside"),
           (with_job(value_at(1, 2, np.nan)), None, "a coordinate is not finite"),
           (with_job(value_at(1, 0, np.inf)), None, "a coordinate is not finite"),
           (with_job(value_at(2, 0, np.nan)), None, "chi is not finite"),
           (with_job(value_at(2, 1, np.inf)), None, "J is not finite"),
           (with_job(value_at(2, 1, 0.0)), None, "J <= 0"),
           (with_job(value_at(2, 1, -3.0)), None, "J <= 0")]
    return out
