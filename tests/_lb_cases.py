"""Cases for the optimiser probe (pw_internal_lb_probe, pywindow_amd/csrc/pw_lb_probe.hpp): one Lbfgsb<N> on one
team, state in, state out.  Everything here is plain data and plain Python; the tests (test_lb_probe.py, on the
host context) run the cases.

A constructed case starts from a SETUP image, fields edited BY NAME through the library's field table.  What an
operation is not defined to read is NaN, what it is not defined to write is a sentinel.  The builder does not assume
that a case reaches its edge: `sweep_ut` / `sweep_un` restate the two triangular sweeps in plain Python (fma through exact
fractions, the 16-term block rule for rows 16 and up) and yields every dividend; a case's class -- "plain" (the
speculative form stands), "guarded" (it must repeat with guards), "singular" (return k + 1) -- is computed from
those with the predicate of pw_plain_exponent, and asserted against what the case was built for.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
import struct
from fractions import Fraction

import numpy as np

M = 10
M2 = 20
SENT = struct.unpack("<d", struct.pack("<Q", 0x7FF8DEADBEEF0001))[0]       # a NaN with a payload of its own
SENT_BITS = 0x7FF8DEADBEEF0001
OP = dict(SETUP=1, TABLES=2, FACTOR=3, FORMT=4, FORMK=5, BMV=6, CMPRLB=7, SUBSM=8, STEP=9, MINIMIZE=10)
F_DEVICE_ONLY, F_SCRATCH, F_CASE = 1, 2, 4
TASK = dict(START=0, NEW_X=1, FG=3, CONVERGENCE=4, STOP=5, WARNING=6, ERROR=7, ABNORMAL=8)
PW_E_BAD_ARG = -2


# ---- the library's entries ---------------------------------------------------------------------------------------------
class _Field(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 12), ("offset", ctypes.c_int), ("count", ctypes.c_int), ("type", ctypes.c_int),
                ("flags", ctypes.c_int)]


@functools.lru_cache(None)
def _entry():
    from pywindow_amd import _lib

    L = _lib.load()
    L.pw_internal_lb_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t]
    L.pw_internal_lb_probe.restype = ctypes.c_int
    L.pw_internal_lb_fields.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    L.pw_internal_lb_fields.restype = ctypes.c_int
    return L


@functools.lru_cache(None)
def fields(n: int):
    """name -> (byte offset, count, dtype, flags), and the size of a case"""
    size = ctypes.c_size_t(0)
    cnt = _entry().pw_internal_lb_fields(n, None, 0, ctypes.byref(size))
    buf = (_Field * cnt)()
    assert _entry().pw_internal_lb_fields(n, buf, cnt, ctypes.byref(size)) == cnt
    tab = {f.name.decode(): (f.offset, f.count, np.float64 if f.type == 0 else np.int32, f.flags) for f in buf}
    return tab, size.value


@functools.lru_cache(None)
def host_ctx():
    from pywindow_amd import _lib

    return _lib.Context(-1)


class Case:
    """The bytes of one case; fields by name as numpy views."""

    def __init__(self, n: int, raw=None):
        self.n = n
        self.tab, self.size = fields(n)
        self.raw = np.zeros(self.size, np.uint8) if raw is None else np.array(raw, np.uint8, copy=True)

    def __getitem__(self, name):
        off, cnt, dt, _ = self.tab[name]
        return self.raw[off:off + cnt * np.dtype(dt).itemsize].view(dt)

    def __setitem__(self, name, value):
        self[name][...] = value

    def copy(self):
        return Case(self.n, self.raw)

    def ops(self, *ops):
        """ops: (name, a, b, c) tuples, missing arguments 0"""
        assert len(ops) <= 8
        self["nops"] = len(ops)
        o = self["ops"]
        o[:] = 0
        for k, op in enumerate(ops):
            op = (op,) if isinstance(op, str) else op
            o[4 * k] = OP[op[0]]
            o[4 * k + 1:4 * k + len(op)] = op[1:]
        return self

    def rets(self):
        return [int(v) for v in self["ret"][:int(self["nops"][0])]]

    def mat(self, name, ld):
        """column-major view: mat[i, j] is element (i, j)"""
        return self[name].reshape(-1, ld).T


def run_rc(ctx, cases):
    """Run a batch (all of one N) in ONE call; returns (rc, the cases afterwards)."""
    n = cases[0].n
    blob = np.concatenate([c.raw for c in cases])
    rc = _entry().pw_internal_lb_probe(ctx._h, n, blob.ctypes.data, len(cases), cases[0].size)
    size = cases[0].size
    return rc, [Case(n, blob[i * size:(i + 1) * size]) for i in range(len(cases))]


def run(ctx, cases):
    rc, out = run_rc(ctx, cases)
    assert rc == 0, _entry().pw_last_error()
    return out


# ---- comparing two runs of a case ---------------------------------------------------------------------------------------
def bits(a):
    return np.asarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def same(a, b):
    """bit for bit, a NaN matching a NaN"""
    if a.dtype == np.float64:
        return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def differences(dev: Case, host: Case):
    """Names of the fields in which a device run differs from the host run: every field the table marks neither
    device-only nor scratch, the return codes, and the scratch (wa) while every operation returned 0."""
    out = []
    clean = all(r == 0 for r in host.rets())
    for name, (_, _, _, flags) in host.tab.items():
        if flags & F_DEVICE_ONLY or name in ("nops", "ops") or name.startswith("in_"):
            continue
        if flags & F_SCRATCH and not clean:
            continue
        if not same(dev[name], host[name]):
            a, b = dev[name], host[name]
            at = int(np.nonzero(~((bits(a) == bits(b)) | ((a != a) & (b != b)) if a.dtype == np.float64 else a == b))[0][0])
            out.append(f"{name}[{at}]: device {a[at]!r} ({int(bits(a)[at]):#x}) host {b[at]!r} ({int(bits(b)[at]):#x})")
    return out


# ---- base images ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _setup_raw(n, x0, l, u, nbd):
    c = Case(n)
    c["factr"], c["pgtol"], c["maxls"] = 1e7, 1e-5, 20
    c["in_x0"], c["in_l"], c["in_u"], c["in_nbd"] = x0, l, u, nbd
    c.ops("SETUP")
    return run(host_ctx(), [c])[0].raw


def setup_image(n, x0=None, l=None, u=None, nbd=None) -> Case:
    """What SETUP leaves (pair[] included), ready for editing: the scalars the routines index with are in range."""
    x0 = tuple(x0 if x0 is not None else [0.25] * n)
    l = tuple(l if l is not None else [-2.0] * n)
    u = tuple(u if u is not None else [2.0] * n)
    nbd = tuple(nbd if nbd is not None else [2] * n)
    c = Case(n, _setup_raw(n, x0, l, u, nbd))
    c["ileave"] = n + 1
    c["epsmch"] = 2.220446049250313e-16
    c["theta"] = 1.0
    c["index"] = np.arange(n)
    c["indx2"] = np.arange(n)
    c.ops()
    return c


def poison(c: Case, reads=(), keeps=()):
    """NaN into every double array the operation is not defined to read, the sentinel into those it must not write;
    `reads` are left alone."""
    for name, (_, cnt, dt, flags) in c.tab.items():
        if dt is not np.float64 or cnt == 1 or flags & F_CASE or name in reads:
            continue
        c[name] = SENT if name in keeps else np.nan
    return c


# ---- the two triangular sweeps, restated ----------------------------------------------------------------------------------
def fma(a, b, c):
    """fused a * b + c, rounded once (exact rationals)"""
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b + c
    if not math.isfinite(c):
        return c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        if (a == 0.0 or b == 0.0) and c == 0.0:
            neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
            return -0.0 if neg else 0.0
        return 0.0
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def div(a, b):
    """IEEE a / b (b != 0: the singularity test comes first)"""
    return float(np.float64(a) / np.float64(b))


def sweep_ut(n, U, x):
    """solve U^T x = b, DOT order (p_dtrsv_ut / lb_solve_ut_reg); U[i][j], i <= j.  Returns x and every dividend."""
    x = list(x)
    acc = [0.0] * n
    dividends = []
    with np.errstate(all="ignore"):
        for s in range(n):
            xs = x[s] - acc[s] if s > 0 else x[s]
            dividends.append(xs)
            xs = div(xs, U[s][s])
            x[s] = xs
            for i in range(s + 1, n):
                if i >= 16 and s < 16:
                    if s == 15:     # rows 16.. take their first 16 terms through the SIMD ddot kernel order
                        sl = [((U[l][i] * x[l] + U[4 + l][i] * x[4 + l]) + U[8 + l][i] * x[8 + l]) + U[12 + l][i] * x[12 + l]
                              for l in range(4)]
                        acc[i] = (sl[0] + sl[2]) + (sl[1] + sl[3])
                else:
                    acc[i] = fma(xs, U[s][i], acc[i])
    return x, dividends


def sweep_un(n, U, x):
    """solve U x = b, AXPY order (p_dtrsv_un / lb_solve_un_reg)"""
    x = list(x)
    dividends = []
    with np.errstate(all="ignore"):
        for i in range(n - 1, -1, -1):
            dividends.append(x[i])
            xi = div(x[i], U[i][i])
            x[i] = xi
            for k in range(i):
                x[k] = fma(-xi, U[k][i], x[k])
    return x, dividends


def plain(v) -> bool:
    """pw_plain_exponent: biased exponent in 700..1400"""
    e = (struct.unpack("<Q", struct.pack("<d", float(v)))[0] >> 52) & 0x7FF
    return 700 <= e <= 1400


def bmv_restated(col, SY, WT, v):
    """Lbfgsb::bmv, general form.  Returns (ret, p, dividends, divisors, (dividends of the U' sweep in step order,
    of the U sweep in step order))."""
    for k in range(col):
        if WT[k][k] == 0.0:
            return k + 1, None, [], [], ([], [])
    dividends, divisors = [], []
    with np.errstate(all="ignore"):
        p = [0.0] * (2 * col)
        for i in range(col):
            s = 0.0
            for k in range(i):
                num = float(np.float64(SY[i][k]) * np.float64(v[k]))
                dividends.append(num)
                s = s + div(num, SY[k][k])
            p[col + i] = v[col + i] + s if i else v[col]
        hi, d1 = sweep_ut(col, WT, p[col:])
        root = [float(np.sqrt(np.float64(SY[i][i]))) for i in range(col)]
        pa = [div(v[i], root[i]) for i in range(col)]
        dividends += [v[i] for i in range(col)] + pa
        hi, d2 = sweep_un(col, WT, hi)
        dividends += d1 + d2
        for i in range(col):
            s = 0.0
            for k in range(i + 1, col):
                num = float(np.float64(SY[k][i]) * np.float64(hi[k]))
                dividends.append(num)
                s = s + div(num, SY[i][i])
            p[i] = div(-pa[i], root[i]) + s
        p[col:] = hi
        divisors = [SY[i][i] for i in range(col)] + root + [WT[i][i] for i in range(col)]
    return 0, p, dividends, divisors, (d1, d2)


def klass(ret, dividends, divisors):
    if ret != 0:
        return "singular"
    return "plain" if all(plain(d) for d in dividends) and all(plain(d) for d in divisors) else "guarded"


SPECIALS = [("+0", 0.0), ("-0", -0.0), ("tiny", 2.0 ** -400), ("huge", 2.0 ** 400), ("inf", math.inf), ("nan", math.nan)]


def _upper(rng, n):
    U = np.triu(rng.uniform(-1.0, 1.0, (n, n)))
    U[np.diag_indices(n)] = rng.uniform(0.5, 2.0, n)
    return U


def _lower_sy(rng, n):
    L = np.tril(rng.uniform(-1.0, 1.0, (n, n)))
    L[np.diag_indices(n)] = rng.uniform(0.5, 2.0, n)
    return L


# ---- BMV -------------------------------------------------------------------------------------------------------------------
BMV_V, BMV_P = 2 * M, 0       # cmprlb's own offsets


def bmv_case(col, SY, WT, v):
    c = setup_image(3)
    poison(c, reads=("l", "u", "x", "le", "ue"), keeps=("ws", "wy", "ss", "wn", "wn1d", "z", "r", "d", "t", "xp", "g"))
    c["sy"], c["wt"], c["wa"] = np.nan, np.nan, SENT
    sy, wt = c.mat("sy", M), c.mat("wt", M)
    sy[:col, :col] = np.where(np.tri(col, dtype=bool), SY, np.nan)
    wt[:col, :col] = np.where(np.tri(col, dtype=bool).T, WT, np.nan)
    c["wa"][BMV_V:BMV_V + 2 * col] = v
    c["col"] = col
    return c.ops(("TABLES", 0), ("TABLES", 1), ("BMV", BMV_V, BMV_P))


def bmv_cases():
    """[(name, wanted class, case, restated p or None)].  After a singular return the REGISTER routine (lb_bmv_wave, a
    device team) has written nothing: all of p is the sentinel, bit for bit.  The team-memory form the host runs for
    col > 2 has formed p[col..] before dtrtrs meets the zero diagonal, so on the host only p[..col) is held to that."""
    out = []
    for col in range(1, M + 1):
        rng = np.random.default_rng(1000 + col)
        SY, WT, v = _lower_sy(rng, col), _upper(rng, col), rng.uniform(-2.0, 2.0, 2 * col)
        todo = [("plain", "plain", SY, WT, v)]
        # a dividend that is not plain at the first / the last step of each sweep: the row is cut loose from the others,
        # so its dividend in the U^T sweep is v[col + k] itself, and in the U sweep the quotient of that
        for where, k in (("first", 0), ("last", col - 1)):
            for tag, val in SPECIALS:
                S2, W2, v2 = SY.copy(), WT.copy(), v.copy()
                S2[k, :k] = 0.0
                S2[k + 1:, k] = 0.0
                W2[:k, k] = 0.0
                W2[k, k + 1:] = 0.0
                v2[col + k] = val
                todo.append((f"dividend {tag} {where}", "guarded", S2, W2, v2))
        for tag, val in (("tiny", 2.0 ** -400), ("huge", 2.0 ** 800)):
            S2 = SY.copy()
            S2[col // 2, col // 2] = val
            todo.append((f"divisor SY {tag}", "guarded", S2, WT, v))
        for tag, val in (("tiny", 2.0 ** -400), ("huge", 2.0 ** 400)):
            W2 = WT.copy()
            W2[col - 1, col - 1] = val
            todo.append((f"divisor WT {tag}", "guarded", SY, W2, v))
        for k in sorted({0, col - 1}):
            for tag, val in SPECIALS[:2]:
                W2 = WT.copy()
                W2[k, k] = val
                todo.append((f"singular {tag} at {k}", "singular", SY, W2, v))
        W2, v2 = WT.copy(), v.copy()
        W2[col // 2, col // 2] = 1e-300
        v2[col:] = 1e10 * (1.0 + np.abs(v[col:]))
        todo.append(("overflow half-way", "guarded", SY, W2, v2))
        for name, want, S_, W_, v_ in todo:
            ret, p, dividends, divisors, (d1, d2) = bmv_restated(col, S_.tolist(), W_.tolist(), v_.tolist())
            got = klass(ret, dividends, divisors)
            assert got == want, (col, name, got)
            if want == "singular":
                assert ret == int(name.split()[-1]) + 1
            if name.startswith("dividend"):
                # where it was put: that step of the U' sweep, and the mirrored step of the U sweep (which runs from
                # the last row to the first)
                k = 0 if name.endswith("first") else col - 1
                assert not plain(d1[k]) and not plain(d2[col - 1 - k]), (col, name, d1, d2)
            if name == "overflow half-way":
                assert any(not math.isfinite(q) for q in p) and all(plain(d) for d in dividends[:1]), (col, p)
            out.append((f"bmv col={col} {name}", want, bmv_case(col, S_, W_, v_), p))
    return out


# ---- SUBSM ------------------------------------------------------------------------------------------------------------------
def subsm_case(col, nfree, head, theta, order, WN, ws, wy, dd, xs, x=None, l=None, u=None, nbd=None, g=None):
    c = setup_image(3, x0=x, l=l, u=u, nbd=nbd)
    poison(c, reads=("l", "u", "x", "le", "ue"), keeps=("sy", "ss", "wt", "wn1d", "d", "t"))
    c["wn"] = np.nan
    wn = c.mat("wn", M2)
    n = 2 * col
    wn[:n, :n] = np.where(np.tri(n, dtype=bool).T, WN, np.nan)
    c["ws"], c["wy"] = np.nan, np.nan
    for j in range(col):
        pj = (head + j) % M
        c["ws"][3 * pj:3 * pj + 3] = ws[j]
        c["wy"][3 * pj:3 * pj + 3] = wy[j]
    c["r"][:nfree] = dd
    c["z"] = xs
    c["g"] = g if g is not None else [0.3, -0.2, 0.1]
    c["wa"] = np.nan
    c["col"], c["nfree"], c["head"], c["theta"] = col, nfree, head, theta
    c["index"] = order
    return c.ops(("TABLES", 2), ("TABLES", 3), "SUBSM")


def subsm_wv(col, nfree, theta, order, ws, wy, dd):
    wv = [0.0] * (2 * col)
    with np.errstate(all="ignore"):
        for i in range(col):
            t1 = t2 = np.float64(0.0)
            for j in range(nfree):
                t1 = t1 + np.float64(wy[i][order[j]]) * np.float64(dd[j])
                t2 = t2 + np.float64(ws[i][order[j]]) * np.float64(dd[j])
            wv[i], wv[col + i] = float(t1), float(np.float64(theta) * t2)
    return wv


def subsm_solves_restated(col, WN, wv):
    n = 2 * col
    for k in range(n):
        if WN[k][k] == 0.0:
            return k + 1, None, [], []
    x, d1 = sweep_ut(n, WN, wv)
    x = [-q for q in x[:col]] + x[col:]
    x, d2 = sweep_un(n, WN, x)
    return 0, x, d1 + d2, [WN[k][k] for k in range(n)]     # (dividends: n of the U' sweep, then n of the U sweep)


def subsm_cases():
    """[(name, wanted class, case, restated wv after the solves or None)]"""
    out = []
    orders = list(itertools.permutations(range(3)))
    count = 0
    for col in range(3, M + 1):
        for nfree in (1, 2, 3):
            for head in (0, 7):
                rng = np.random.default_rng(2000 + 100 * col + 10 * nfree + head)
                order = list(orders[count % 6])
                count += 1
                theta = float(rng.choice([0.5, 1.75, 3.0]))
                n = 2 * col
                WN = _upper(rng, n)
                ws, wy = rng.uniform(-1.0, 1.0, (col, 3)), rng.uniform(-1.0, 1.0, (col, 3))
                dd, xs = rng.uniform(-1.0, 1.0, nfree), rng.uniform(-1.0, 1.0, 3)
                todo = [("plain", "plain", WN, ws, wy)]
                k0 = order[0]
                # the edge classes once per col, on one (nfree, head) each; the plain class on all of them
                edges = nfree == 1 + col % 3 and head == (7 if col % 2 else 0)
                for where, row in (("first", 0), ("last", n - 1)) if edges else ():
                    for tag, val in SPECIALS:
                        if row == 0 and tag == "-0":
                            continue        # wv[0] is a sum that starts from +0: it is never -0
                        W2, s2, y2 = WN.copy(), ws.copy(), wy.copy()
                        W2[:row, row] = 0.0
                        W2[row, row + 1:] = 0.0
                        src = y2 if row == 0 else s2
                        src[row % col, :] = 0.0
                        src[row % col, k0] = val
                        todo.append((f"dividend {tag} {where}", "guarded", W2, s2, y2))
                if edges:
                    for tag, val in (("tiny", 2.0 ** -400), ("huge", 2.0 ** 400)):
                        W2 = WN.copy()
                        W2[col, col] = val
                        todo.append((f"divisor WN {tag}", "guarded", W2, ws, wy))
                    for k in (0, n - 1):
                        for tag, val in SPECIALS[:2]:
                            W2 = WN.copy()
                            W2[k, k] = val
                            todo.append((f"singular {tag} at {k}", "singular", W2, ws, wy))
                    W2 = WN.copy()
                    W2[col, col] = 1e-300
                    todo.append(("overflow half-way", "guarded", W2, ws * 1e10, wy * 1e10))
                for name, want, W_, s_, y_ in todo:
                    dd_ = np.ones(nfree) if name.startswith("dividend") else dd
                    wv = subsm_wv(col, nfree, theta, order, s_.tolist(), y_.tolist(), dd_.tolist())
                    ret, x, dividends, divisors = subsm_solves_restated(col, W_.tolist(), wv)
                    got = klass(ret, dividends, divisors)
                    assert got == want, (col, nfree, head, name, got)
                    if want == "singular":
                        assert ret == int(name.split()[-1]) + 1
                    if name.startswith("dividend"):
                        # that step of the U' sweep and the mirrored step of the U sweep (last row first)
                        k = 0 if "first" in name else n - 1
                        assert not plain(dividends[k]) and not plain(dividends[n + (n - 1 - k)]), (col, name, dividends)
                    if name == "overflow half-way":
                        assert any(math.isinf(q) or math.isnan(q) for q in x) and math.isfinite(dividends[0])
                    out.append((f"subsm col={col} nfree={nfree} head={head} {name}", want,
                                subsm_case(col, nfree, head, theta, order, W_, s_, y_, dd_, xs), x))
    return out


def subsm_negzero_cases():
    """dd[i] = -0.0 and every product -0: the -0.0 a missing term is replaced by is all that keeps the sign.  The
    products' signs follow the solved wv, which the host context supplies (two passes)."""
    out = []
    for col in (3, 6, 9, 10):
        for nfree in (1, 2, 3):
            rng = np.random.default_rng(3000 + 10 * col + nfree)
            n = 2 * col
            WN = _upper(rng, n)
            ws, wy = rng.uniform(0.5, 1.0, (col, 3)), rng.uniform(0.5, 1.0, (col, 3))
            xs = rng.uniform(-1.0, 1.0, 3)
            dd = -np.zeros(nfree)
            first = run(host_ctx(), [subsm_case(col, nfree, 7, 1.5, [2, 0, 1], WN, ws, wy, dd, xs)])[0]
            wv = first["wa"][:n]
            assert np.all(wv == 0.0)
            sign = np.where(np.signbit(wv), 1.0, -1.0)      # the factor that makes a product with wv a -0
            wy2, ws2 = wy * sign[:col, None], ws * sign[col:, None]
            c = subsm_case(col, nfree, 7, 1.5, [2, 0, 1], WN, ws2, wy2, dd, xs)
            again = run(host_ctx(), [c])[0]
            assert np.array_equal(np.signbit(again["wa"][:n]), np.signbit(wv))
            with np.errstate(all="ignore"):
                for j in range(col):
                    for k in (2, 0, 1)[:nfree]:
                        a, b = wy2[j, k] * wv[j] / 1.5, ws2[j, k] * wv[col + j]
                        assert a == 0.0 and b == 0.0 and np.signbit(a) and np.signbit(b)
            assert np.all(np.signbit(again["r"][:nfree])) and np.all(again["r"][:nfree] == 0.0)
            out.append((f"subsm col={col} nfree={nfree} every product -0", c))
    return out


def nextafter(x, up):
    return float(np.nextafter(x, math.inf if up else -math.inf))


def subsm_bound_cases():
    """x + d exactly on a bound and one ulp either side, for every kind of bound: [(name, case, iword expected, x)].
    The variable's rows of WS and WY are zero, so its d is dd / theta exactly (theta = 2)."""
    out = []
    col, nfree = 4, 3
    rng = np.random.default_rng(4000)
    WN = _upper(rng, 2 * col)
    lo, up, x0 = 0.5, 1.5, 0.75
    for nb in (0, 1, 2, 3):
        for side, bound in (("lower", lo), ("upper", up)):
            for tag in ("on", "inside", "outside"):
                target = bound
                if tag != "on":
                    target = nextafter(bound, up=(side == "lower") == (tag == "inside"))
                d = target - x0
                assert x0 + d == target         # (the step lands where it is meant to, exactly)
                ws, wy = rng.uniform(-1.0, 1.0, (col, 3)), rng.uniform(-1.0, 1.0, (col, 3))
                ws[:, 1] = 0.0
                wy[:, 1] = 0.0
                dd = np.array([2.0 * d, 1e-3, -2e-3])
                xs = np.array([0.1, x0, -0.2])
                c = subsm_case(col, nfree, 0, 2.0, [1, 0, 2], WN, ws, wy, dd, xs, x=[0.1, x0, -0.2], l=[-50.0, lo, -50.0],
                               u=[50.0, up, 50.0], nbd=[2, nb, 2], g=[0.0, 0.0, 0.0])
                nx = x0 + d
                if nb in (1, 2):
                    nx = max(lo, nx)
                if nb in (2, 3):
                    nx = min(up, nx)
                hit = (nb in (1, 2) and nx == lo) or (nb in (2, 3) and nx == up)
                out.append((f"subsm nbd={nb} {side} {tag}", c, int(hit), nx))
    return out


# ---- FACTOR / FORMT ------------------------------------------------------------------------------------------------------------
PIVOTS = [("0", 0.0), ("-0", -0.0), ("neg", -1.5), ("nan", math.nan), ("inf", math.inf), ("subnormal", 5e-324 * 1024)]


def spd(rng, n):
    R = rng.uniform(-1.0, 1.0, (n, n))
    return R.T @ R + n * np.eye(n)


def factor_case(which, n, A):
    c = setup_image(3)
    poison(c, reads=("l", "u", "x", "le", "ue"), keeps=("ws", "wy", "sy", "ss", "z", "r", "d", "t", "xp", "g", "wn1d", "wa"))
    name, ld, at = ("wt", M, 0) if which == 1 else ("wn", M2, 0 if which == 2 else n)
    c["wt" if which != 1 else "wn"] = SENT
    c[name] = SENT
    m = c.mat(name, ld)
    m[at:at + n, at:at + n] = np.where(np.tri(n, dtype=bool).T, A, SENT)
    c["col"] = n
    return c.ops(("FACTOR", which))


def factor_cases():
    """[(name, which, n, A, case)]: SPD matrices, and the first non-positive pivot at each j with each value (column j
    is cut loose from the rows above it, so its pivot is A[j][j] itself)"""
    out = []
    for which in (1, 2, 3):
        for n in range(1, M + 1):
            rng = np.random.default_rng(5000 + 100 * which + n)
            A = spd(rng, n)
            out.append((f"factor {which} n={n} spd", which, n, A, factor_case(which, n, A)))
            for j in range(n):
                for tag, val in PIVOTS:
                    B = A.copy()
                    B[:j, j] = 0.0
                    B[j, j] = val
                    out.append((f"factor {which} n={n} pivot {tag} at {j}", which, n, B, factor_case(which, n, B)))
    return out


def formt_cases():
    out = []
    for n in range(1, M + 1):
        rng = np.random.default_rng(6000 + n)
        for tag in ("spd", "pivot", "nan"):
            c = setup_image(3)
            poison(c, reads=("l", "u", "x", "le", "ue"), keeps=("ws", "wy", "wn", "z", "r", "d", "t", "xp", "g", "wn1d", "wa"))
            c["sy"], c["ss"], c["wt"] = np.nan, np.nan, SENT
            sy, ss = c.mat("sy", M), c.mat("ss", M)
            sy[:n, :n] = np.where(np.tri(n, dtype=bool), _lower_sy(rng, n), np.nan)
            S = spd(rng, n)
            if tag == "pivot":
                S[n // 2, n // 2] = -1e3
            if tag == "nan":
                sy[n - 1, 0] = np.nan
            ss[:n, :n] = np.where(np.tri(n, dtype=bool).T, S, np.nan)
            c["col"], c["theta"] = n, 1.75
            out.append((f"formt n={n} {tag}", c.ops("FORMT"), 0 if tag == "spd" else (-3 if tag == "pivot" else None)))
    return out


# ---- FORMK / CMPRLB -----------------------------------------------------------------------------------------------------------------
def formk_base(col, nfree, head, theta, seed, iupdat=None):
    rng = np.random.default_rng(seed)
    c = setup_image(3)
    poison(c, reads=("l", "u", "x", "le", "ue"), keeps=("ss", "wt", "z", "r", "d", "t", "xp", "g", "wa"))
    c["ws"], c["wy"] = rng.uniform(-1.0, 1.0, 3 * M), rng.uniform(-1.0, 1.0, 3 * M)
    c["sy"] = np.nan
    c.mat("sy", M)[np.diag_indices(M)] = rng.uniform(20.0, 40.0, M)
    c["col"], c["nfree"], c["head"], c["theta"] = col, nfree, head, theta
    c["index"] = rng.permutation(3)
    # the old parts of WN1 as earlier calls would have left them for this free set: Y'Y over the free variables,
    # S'S over the active ones, and S'Y over the free ones on and above the diagonal, the active ones below it
    c["wn"], c["wn1d"] = 0.0, 0.0
    wn = c.mat("wn", M2)
    free, act = [int(k) for k in c["index"][:nfree]], [int(k) for k in c["index"][nfree:]]
    S = np.array([c["ws"][3 * ((head + j) % M):3 * ((head + j) % M) + 3] for j in range(col)])
    Y = np.array([c["wy"][3 * ((head + j) % M):3 * ((head + j) % M) + 3] for j in range(col)])
    for i in range(col):
        for j in range(col):
            if j <= i:
                yy, ss_ = float(Y[i, free] @ Y[j, free]), float(S[i, act] @ S[j, act])
                if i == j:
                    c["wn1d"][i], c["wn1d"][M + i] = yy, ss_
                else:
                    wn[i, j], wn[M + i, M + j] = yy, ss_
            wn[M + i, j] = float(S[i, free] @ Y[j, free]) if i <= j else float(S[i, act] @ Y[j, act])
    c["updatd"], c["iupdat"] = 1, col if iupdat is None else iupdat
    c["nenter"], c["ileave"] = 0, 4
    return c.ops("FORMK")


def formk_cases():
    """[(name, case, wanted return or None)].  updatd off / a changed free set start from what an updating call on
    the host context left in WN1 (two passes)."""
    out = []
    seed = 7000
    for col in range(1, M + 1):
        for nfree in (0, 1, 2, 3):
            seed += 1
            base = formk_base(col, nfree, 7 if col % 2 else 0, 1.75, seed)
            out.append((f"formk col={col} nfree={nfree} updatd", base, 0 if nfree else None))
            if nfree in (1, 2):
                left = run(host_ctx(), [base])[0]
                assert left.rets() == [0]
                for tag, nenter, ileave in (("kept", 0, 4), ("enter", 1, 4), ("leave", 0, 3), ("both", 1, 3)):
                    c = base.copy()
                    c["wn"], c["wn1d"] = left["wn"], left["wn1d"]
                    c["updatd"], c["nenter"], c["ileave"] = 0, nenter, ileave
                    c["indx2"] = [int(c["index"][2]), 0, int(c["index"][0])]
                    out.append((f"formk col={col} nfree={nfree} old parts {tag}", c, None))
    for iupdat in (10, 11):
        # every cell of the old WN1 its own value, so a shift that reads a cell after it was written shows
        c = formk_base(10, 2, 3, 0.75, 7100, iupdat=iupdat)
        rng = np.random.default_rng(7101)
        c["wn"], c["wn1d"] = rng.uniform(-1.0, 1.0, M2 * M2), rng.uniform(1.0, 2.0, M2)
        c["nenter"], c["ileave"], c["indx2"] = 1, 3, [1, 0, 2]
        out.append((f"formk col=10 iupdat={iupdat}", c, None))
    for col in (3, 7, 10):
        c = formk_base(col, 2, 0, 1.75, 7200 + col)
        c.mat("sy", M)[col // 2, col // 2] = -1e6
        out.append((f"formk col={col} first block fails", c, -1))
        c = formk_base(col, 1, 0, -40.0, 7300 + col)
        c.mat("sy", M)[np.diag_indices(M)] = 1e3
        out.append((f"formk col={col} second block fails", c, -2))
    return out


def cmprlb_cases():
    out = []
    for col in range(3, M + 1):
        for nfree in (1, 2, 3):
            rng = np.random.default_rng(8000 + 10 * col + nfree)
            c = setup_image(3)
            poison(c, reads=("l", "u", "le", "ue"), keeps=("ss", "wn", "wn1d", "d", "t", "xp"))
            c["ws"], c["wy"] = rng.uniform(-1.0, 1.0, 3 * M), rng.uniform(-1.0, 1.0, 3 * M)
            c["sy"], c["wt"] = np.nan, np.nan
            c.mat("sy", M)[:col, :col] = np.where(np.tri(col, dtype=bool), _lower_sy(rng, col), np.nan)
            c.mat("wt", M)[:col, :col] = np.where(np.tri(col, dtype=bool).T, _upper(rng, col), np.nan)
            c["x"], c["z"], c["g"] = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
            c["r"] = SENT
            c["wa"] = np.nan
            c["wa"][2 * M:2 * M + 2 * col] = rng.uniform(-1.0, 1.0, 2 * col)
            c["col"], c["nfree"], c["head"], c["theta"], c["cnstnd"] = col, nfree, 7, 1.75, 1
            c["index"] = rng.permutation(3)
            out.append((f"cmprlb col={col} nfree={nfree}", c.ops(("TABLES", 0), ("TABLES", 1), "CMPRLB")))
    return out


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
INF = math.inf


def _sgn(v):
    return 1.0 if v > 0.0 else (-1.0 if v < 0.0 else 0.0)


def rosen(x):
    return 100 * (x[1] - x[0] ** 2) ** 2 + (1 - x[0]) ** 2 + 100 * (x[2] - x[1] ** 2) ** 2 + (1 - x[1]) ** 2


def illquad(x):
    return 0.5 * (x[0] ** 2 + 1e6 * x[1] ** 2 + 1e-6 * x[2] ** 2) + x[0] * x[2] * 1e-3


def kinks(x):
    return abs(x[0]) + 10 * abs(x[1] - 0.3) + (x[2] - 1) ** 2 + 0.1 * x[0] * x[1]


def powell(x):
    return (x[0] + 10 * x[1]) ** 2 + 5 * (x[2] - x[0]) ** 2 + (x[1] - 2 * x[2]) ** 4 + 10 * (x[0] - x[2]) ** 4


def neck1(z):
    return (z[0] ** 2 - 2) ** 2 + 0.1 * z[0] + abs(z[0] - 1.3)


# the objectives of LbProbeObjective (pw_lb_probe.hpp), statement for statement: f and the explicit gradient
def fg_analytic(oid, x):
    x = [float(v) for v in x]
    if oid == 0:
        x0, x1, x2 = x
        a, b, c, e = x1 - x0 * x0, 1.0 - x0, x2 - x1 * x1, 1.0 - x1
        return (100.0 * a * a + b * b + 100.0 * c * c + e * e,
                [-400.0 * a * x0 - 2.0 * b, 200.0 * a - 400.0 * c * x1 - 2.0 * e, 200.0 * c])
    if oid == 1:
        x0, x1, x2 = x
        return (0.5 * (x0 * x0 + 1e6 * x1 * x1 + 1e-6 * x2 * x2) + x0 * x2 * 1e-3,
                [x0 + x2 * 1e-3, 1e6 * x1, 1e-6 * x2 + x0 * 1e-3])
    if oid == 2:
        x0, x1, x2 = x
        q = x2 - 1.0
        return (abs(x0) + 10.0 * abs(x1 - 0.3) + q * q + 0.1 * x0 * x1,
                [_sgn(x0) + 0.1 * x1, 10.0 * _sgn(x1 - 0.3) + 0.1 * x0, 2.0 * q])
    if oid == 3:
        x0, x1, x2 = x
        a, b, c, d = x0 + 10.0 * x1, x2 - x0, x1 - 2.0 * x2, x0 - x2
        c2, d2 = c * c, d * d
        c3, d3 = c2 * c, d2 * d
        return (a * a + 5.0 * b * b + c2 * c2 + 10.0 * (d2 * d2),
                [2.0 * a - 10.0 * b + 40.0 * d3, 20.0 * a + 4.0 * c3, 10.0 * b - 8.0 * c3 - 40.0 * d3])
    z = x[0]
    q = z * z - 2.0
    return q * q + 0.1 * z + abs(z - 1.3), [4.0 * z * q + 0.1 + _sgn(z - 1.3)]


# the issue's table: (name, objective, objective id of MINIMIZE, x0, l, u, nbd, what the run must reach with the
# lockstep tool's forward-difference gradient: calls, max col, max iupdat, the set of nfree seen, info seen, ending)
RUNS = [
    ("rosen free", rosen, 0, (-1.2, 1.0, 1.0), (-INF,) * 3, (INF,) * 3, (0, 0, 0),
     dict(calls=121, col=10, iupdat=52)),
    ("rosen boxed", rosen, 0, (-1.2, 0.5, 1.5), (-1.5, -0.5, 0.2), (0.8, 0.9, 2.0), (2, 2, 2),
     dict(calls=22, col=9, nfree={0, 2, 3})),
    ("rosen mixed bounds", rosen, 0, (-1.2, 0.5, 1.5), (-1.5, 0.0, 0.9), (0.0, 0.7, 0.0), (1, 3, 1),
     dict(calls=29, nfree={0, 1, 2, 3})),
    ("ill-conditioned quadratic", illquad, 1, (1.0, 1.0, 1.0), (-INF,) * 3, (INF,) * 3, (0, 0, 0),
     dict(calls=70, col=10, info={-9}, ending="ABNORMAL")),
    ("kinks", kinks, 2, (1.0, 1.0, 3.0), (-2.0, -2.0, -2.0), (2.0, 2.0, 0.5), (2, 2, 2),
     dict(calls=71, info={-5}, nfree={0, 1, 2, 3})),
    ("powell", powell, 3, (3.0, -1.0, 0.5), (0.1, -2.0, -1.0), (4.0, 2.0, 1.0), (2, 2, 2),
     dict(calls=34, col=10, iupdat=15)),
    ("neck n=1", neck1, 4, (3.0,), (-0.5,), (INF,), (1,),
     dict(calls=18, col=7)),
]


def run_start(run_):
    """the case a run starts from (task START), before its first STEP"""
    _, _, _, x0, l, u, nbd, _ = run_
    n = len(x0)
    lo = [0.0 if math.isinf(v) else v for v in l]
    up = [0.0 if math.isinf(v) else v for v in u]
    c = Case(n)
    c["factr"], c["pgtol"], c["maxls"] = 1e7, 1e-5, 20
    c["in_x0"], c["in_l"], c["in_u"], c["in_nbd"] = x0, lo, up, nbd
    c.ops("SETUP")
    c = run(host_ctx(), [c])[0]
    return c.ops("STEP")


def drive_steps(ctx, starts, fgs, maxcalls=400, other=None):
    """STEP in lockstep over several runs: ONE call of the hook per call index carries every run still going.
    fgs[i](x) -> (f, g).  Returns the list of states per run after every call.  With `other` (states from another
    context, same shape) the first differing (run, call, field) raises."""
    cur = [s.copy() for s in starts]
    hist = [[] for _ in starts]
    live = list(range(len(starts)))
    for call in range(maxcalls):
        if not live:
            break
        by_n = {}
        for i in live:
            by_n.setdefault(cur[i].n, []).append(i)
        for ids in by_n.values():
            for i, c in zip(ids, run(ctx, [cur[i] for i in ids])):
                cur[i] = c
        nxt = []
        for i in live:
            c = cur[i]
            hist[i].append(c.copy())
            if other is not None:
                assert call < len(other[i]), f"run {i}: the device goes on after call {call + 1}, the host has ended"
                diff = differences(c, other[i][call])
                assert not diff, f"run {i}, call {call + 1}: " + "; ".join(diff[:4])
            task = int(c["task"][0])
            if task == TASK["FG"]:
                f, g = fgs[i](c["x"].copy())
                c["in_f"], c["in_g"] = f, g
                nxt.append(i)
            elif task == TASK["NEW_X"]:
                nxt.append(i)
        live = nxt
    assert not live, "a run did not end"
    return hist


def fd_fg(run_):
    """f and the lockstep tool's forward-difference gradient"""
    import lockstep_lbfgsb as LS

    _, fun, _, _, l, u, _, _ = run_
    lb, ub = np.array(l, float), np.array(u, float)

    def fg(x):
        f = fun(x)
        return f, LS.fd_grad(fun, x, f, lb, ub)
    return fg


# ---- formt, formk, cmprlb restated: the statements in plain Python, the factorisations and solves by live LAPACK ---------------
def _upper_after_potrf(A, n):
    """dpotrf 'U' on the upper triangle of A: (what it leaves in the upper triangle, info)"""
    from scipy.linalg import lapack

    U, info = lapack.dpotrf(np.asfortranarray(np.triu(A[:n, :n])), lower=0, clean=0)
    return U, int(info)


def formt_restated(c: Case):
    """WT = theta SS + L D^-1 L' in formt's order of operations, then dpotrf: (return code, upper triangle, dpotrf's info)"""
    col, theta = int(c["col"][0]), float(c["theta"][0])
    SY, SS = c.mat("sy", M), c.mat("ss", M)
    W = np.zeros((col, col))
    with np.errstate(all="ignore"):
        for i in range(col):
            for j in range(i, col):
                if i == 0:
                    W[0, j] = theta * SS[0, j]
                else:
                    ddum = 0.0
                    for k in range(i):
                        ddum = ddum + SY[i, k] * SY[j, k] / SY[k, k]
                    W[i, j] = ddum + theta * SS[i, j]
        U, info = _upper_after_potrf(W, col)
    return (-3 if info else 0), U, info


def formk_restated(c: Case):
    """Lbfgsb::formk statement by statement: WN1 (its strict lower triangle in `wn`, its diagonal in `wn1d`) after
    the shift, the new row and column and the change of the free set; then the upper triangle of WN and the
    factorisation by LAPACK (dpotrf, dtrtrs 'T' with col right-hand sides, b_ddot's fma chain, dpotrf).
    Returns (return code, wn as a 2m x 2m matrix, wn1d; info of the failing dpotrf or 0)."""
    from scipy.linalg import lapack

    N = 3
    col, nsub, head, theta = int(c["col"][0]), int(c["nfree"][0]), int(c["head"][0]), float(c["theta"][0])
    updatd, iupdat, nenter, ileave = int(c["updatd"][0]), int(c["iupdat"][0]), int(c["nenter"][0]), int(c["ileave"][0])
    index, indx2 = [int(k) for k in c["index"]], [int(k) for k in c["indx2"]]
    wn, d = c.mat("wn", M2).copy(), c["wn1d"].copy()
    ws, wy, SY = c["ws"].reshape(M, N), c["wy"].reshape(M, N), c.mat("sy", M)

    def get(i, j):
        return d[i] if i == j else wn[i, j]

    def put(i, j, v):
        if i == j:
            d[i] = v
        else:
            wn[i, j] = v
    with np.errstate(all="ignore"):
        if updatd:
            if iupdat > M:
                # the old part moves up and left by one: (r, jy) <- (r + 1, jy + 1), every cell from its OLD value
                old_wn, old_d = wn.copy(), d.copy()

                def old(i, j):
                    return old_d[i] if i == j else old_wn[i, j]
                for jy in range(M - 1):
                    for r in range(jy, M - 1):
                        put(r, jy, old(r + 1, jy + 1))
                        put(M + r, M + jy, old(M + r + 1, M + jy + 1))
                    for r in range(M - 1):
                        put(M + r, jy, old(M + r + 1, jy + 1))
            ipntr = (head + col - 1) % M
            for jy in range(col):
                jpntr = (head + jy) % M
                t1 = t2 = t3 = np.float64(0.0)
                for k in range(nsub):
                    t1 = t1 + wy[ipntr, index[k]] * wy[jpntr, index[k]]
                for k in range(nsub, N):
                    t2 = t2 + ws[ipntr, index[k]] * ws[jpntr, index[k]]
                    t3 = t3 + ws[ipntr, index[k]] * wy[jpntr, index[k]]
                put(col - 1, jy, t1)
                put(M + col - 1, M + jy, t2)
                put(M + col - 1, jy, t3)
            for i in range(col):
                ip = (head + i) % M
                t3 = np.float64(0.0)
                for k in range(nsub):
                    t3 = t3 + ws[ip, index[k]] * wy[ipntr, index[k]]
                put(M + i, col - 1, t3)
        upcl = col - 1 if updatd else col
        if nenter > 0 or ileave <= N:
            for iy in range(upcl):
                for jy in range(iy + 1):
                    ip, jp = (head + iy) % M, (head + jy) % M
                    t1 = t2 = t3 = t4 = np.float64(0.0)
                    for k in range(nenter):
                        t1 = t1 + wy[ip, indx2[k]] * wy[jp, indx2[k]]
                        t2 = t2 + ws[ip, indx2[k]] * ws[jp, indx2[k]]
                    for k in range(ileave - 1, N):
                        t3 = t3 + wy[ip, indx2[k]] * wy[jp, indx2[k]]
                        t4 = t4 + ws[ip, indx2[k]] * ws[jp, indx2[k]]
                    put(iy, jy, get(iy, jy) + t1 - t3)
                    put(M + iy, M + jy, get(M + iy, M + jy) - t2 + t4)
            for ii in range(upcl):
                for jy in range(upcl):
                    ip, jp = (head + ii) % M, (head + jy) % M
                    t1 = t3 = np.float64(0.0)
                    for k in range(nenter):
                        t1 = t1 + ws[ip, indx2[k]] * wy[jp, indx2[k]]
                    for k in range(ileave - 1, N):
                        t3 = t3 + ws[ip, indx2[k]] * wy[jp, indx2[k]]
                    if ii <= jy:
                        put(M + ii, jy, get(M + ii, jy) + t1 - t3)
                    else:
                        put(M + ii, jy, get(M + ii, jy) - t1 + t3)
        # the upper triangle of WN
        for iy in range(col):
            for jy in range(col):
                if jy <= iy:
                    w = get(iy, jy) / theta
                    if jy == iy:
                        w = w + SY[iy, iy]
                    wn[jy, iy] = w
                    wn[col + jy, col + iy] = get(M + iy, M + jy) * theta
                wn[jy, col + iy] = -get(M + iy, jy) if jy < iy else get(M + iy, jy)
        n2 = 2 * col
        K = np.triu(wn[:n2, :n2])
        U11, info = _upper_after_potrf(K, col)
        wn[:col, :col][np.tri(col, dtype=bool).T] = U11[np.tri(col, dtype=bool).T]
        if info:
            return -1, wn, d, info
        X = lapack.dtrtrs(np.asfortranarray(U11), np.asfortranarray(K[:col, col:]), lower=0, trans=1)[0]
        X = X.reshape(col, col)
        wn[:col, col:n2] = X
        K22 = K[col:, col:].copy()
        for i in range(col):
            for j in range(i, col):
                dot = 0.0
                for k in range(col):
                    dot = fma(float(X[k, j]), float(X[k, i]), dot)
                K22[i, j] = K22[i, j] + dot
        U22, info = _upper_after_potrf(K22, col)
        blk = wn[col:n2, col:n2]
        blk[np.tri(col, dtype=bool).T] = U22[np.tri(col, dtype=bool).T]
        # (what dpotrf leaves of the second block after a failure is compared up to the failing column only)
    return (-2 if info else 0), wn, d, info


def cmprlb_restated(c: Case):
    """r of the free variables: -theta (z - x) - g, plus W M W' applied through bmv (bmv_restated)"""
    col, nfree, head, theta = int(c["col"][0]), int(c["nfree"][0]), int(c["head"][0]), float(c["theta"][0])
    index = [int(k) for k in c["index"]]
    ws, wy = c["ws"].reshape(M, 3), c["wy"].reshape(M, 3)
    SY = c.mat("sy", M)[:col, :col].tolist()
    WT = c.mat("wt", M)[:col, :col].tolist()
    v = c["wa"][2 * M:2 * M + 2 * col].tolist()
    ret, p, *_ = bmv_restated(col, SY, WT, v)
    assert ret == 0
    r = []
    for i in range(nfree):
        k = index[i]
        r.append(np.float64(-theta) * (c["z"][k] - c["x"][k]) - c["g"][k])
    for j in range(col):
        pj = (head + j) % M
        a1, a2 = np.float64(p[j]), np.float64(theta) * np.float64(p[col + j])
        for i in range(nfree):
            k = index[i]
            r[i] = r[i] + wy[pj, k] * a1 + ws[pj, k] * a2
    return [float(q) for q in r], p


# What the same runs reach with the ANALYTIC gradients (fg_analytic; MINIMIZE runs these): calls of STEP, max col, max
# iupdat, the sizes of the free set seen, the ending.  One more start, on the kink of `kinks`, where the first line
# search fails with no correction pair: an ABNORMAL end with info -9 through both drivers.
ANALYTIC_REACH = [
    dict(calls=114, col=10, iupdat=49, nfree={3}, ending="CONVERGENCE"),
    dict(calls=22, col=9, iupdat=9, nfree={0, 2, 3}, ending="CONVERGENCE"),
    dict(calls=20, col=8, iupdat=8, nfree={1, 2, 3}, ending="CONVERGENCE"),
    dict(calls=17, col=2, iupdat=2, nfree={3}, ending="CONVERGENCE"),
    dict(calls=58, col=3, iupdat=3, nfree={0, 1, 2, 3}, ending="CONVERGENCE"),
    dict(calls=34, col=10, iupdat=15, nfree={0, 2, 3}, ending="CONVERGENCE"),
    dict(calls=18, col=7, iupdat=7, nfree={0, 1}, ending="CONVERGENCE"),
    dict(calls=22, col=0, iupdat=0, nfree={3}, ending="ABNORMAL", info=-9),
]
ANALYTIC_RUNS = RUNS + [("kinks from the kink", kinks, 2, (0.0, 0.3, 1.0), (-2.0,) * 3, (2.0,) * 3, (2, 2, 2), {})]
