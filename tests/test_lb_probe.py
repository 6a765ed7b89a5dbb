"""The optimiser probe on the host context (pw_internal_lb_probe, device = -1): the members of Lbfgsb<N> one at a
time against live LAPACK and against the plain-Python restatement of tests/_lb_cases.py, the builder's proof that
every constructed case reaches its edge, STEP against the hostsim's hs_lbN_step call by call, MINIMIZE against the
STEP run, and the hook's refusals.  The hook has no device side yet (pywindow_amd/csrc/pw_lb_probe.hip)."""
import math
import sys

import numpy as np
import pytest

from _util import ROOT  # noqa: E402

sys.path.insert(0, str(ROOT / "tests" / "tools"))
import _lb_cases as C  # noqa: E402

lapack = pytest.importorskip("scipy.linalg.lapack")


@pytest.fixture(scope="module")
def host():
    return C.host_ctx()


@pytest.fixture(scope="module")
def bmv(host):
    cases = C.bmv_cases()
    return cases, C.run(host, [c for _, _, c, _ in cases])


@pytest.fixture(scope="module")
def subsm(host):
    cases = C.subsm_cases()
    return cases, C.run(host, [c for _, _, c, _ in cases])


def test_the_field_table_names_every_member():
    for n in (1, 3):
        tab, size = C.fields(n)
        for name in ("l u x g ws wy sy ss wt wn wn1d z r d t xp wa acc dsy rsy sqy rsq rwt rwn iwn tri pair le ue ls ls_i cand "
                     "nbd index iwhere indx2 f factr pgtol maxls task msg prjctd cnstnd boxed updatd nintol itfile iback nskip "
                     "head col itail iter iupdat nseg nfgv info ifun iword nfree nact ileave nenter theta fold tol dnorm epsmch "
                     "gd stpmx sbgnrm stp gdold dtd ls_task").split():
            assert name in tab, name
        device_only = {k for k, v in tab.items() if v[3] & C.F_DEVICE_ONLY}
        assert device_only == set("dsy rsy sqy rsq rwt rwn iwn tri pair acc".split())
        assert tab["ws"][1] == 10 * n and tab["wn"][1] == 400 and tab["wa"][1] == 80 and tab["x"][1] == n
        spans = sorted((o, o + c * np.dtype(t).itemsize) for o, c, t, _ in tab.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= size     # no two fields overlap


def test_the_restated_sweeps_are_lapack_s():
    """sweep_ut / sweep_un against dtrtrs, bit for bit, orders 1..20 (16 and up cross the block rule)"""
    rng = np.random.default_rng(11)
    for n in range(1, 21):
        for _ in range(3):
            U, b = C._upper(rng, n), rng.uniform(-2.0, 2.0, n)
            for trans, sweep in ((1, C.sweep_ut), (0, C.sweep_un)):
                want, info = lapack.dtrtrs(np.asfortranarray(U), b.copy(), lower=0, trans=trans)
                got, _ = sweep(n, U.tolist(), b.tolist())
                assert info == 0 and np.array_equal(C.bits(np.array(got)), C.bits(want)), (n, trans)


def test_every_class_is_there_for_every_operation_and_col(bmv, subsm):
    """the builder asserts each case's class from the restated dividends while it builds; here: none is missing"""
    for (cases, _), cols in ((bmv, range(1, 11)), (subsm, range(3, 11))):
        for col in cols:
            mine = [(name, want) for name, want, c, _ in cases if int(c["col"][0]) == col]
            assert {w for _, w in mine} == {"plain", "guarded", "singular"}
            names = " | ".join(n for n, _ in mine)
            for what in ("+0 first", "tiny first", "huge first", "inf first", "nan first", "+0 last", "-0 last", "tiny last",
                         "huge last", "inf last", "nan last", "divisor", "singular +0 at 0", "singular -0 at 0",
                         f"singular +0 at {(col if cases is bmv[0] else 2 * col) - 1}", "overflow half-way"):
                assert what in names, (col, what)
    assert {(int(c["nfree"][0]), int(c["head"][0])) for _, _, c, _ in subsm[0]} == {(f, h) for f in (1, 2, 3) for h in (0, 7)}
    assert {tuple(c["index"]) for _, _, c, _ in subsm[0]} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert all(float(c["theta"][0]) != 1.0 for _, _, c, _ in subsm[0])


def test_bmv_on_the_host_is_the_restatement(bmv):
    cases, outs = bmv
    for (name, want, c, p), o in zip(cases, outs):
        col, ret = int(c["col"][0]), o.rets()[-1]
        if want == "singular":
            assert ret == int(name.split()[-1]) + 1, name
            assert np.all(C.bits(o["wa"][:col]) == C.SENT_BITS), name      # (bmv_cases: what the host form owes)
            if col <= 2:
                assert np.all(C.bits(o["wa"][:C.BMV_V]) == C.SENT_BITS), name      # the written-out forms write nothing
        else:
            assert ret == 0 and C.same(o["wa"][:2 * col], np.array(p)), name
            assert np.all(C.bits(o["wa"][2 * col:2 * C.M]) == C.SENT_BITS), name
        for keep in ("ws", "wy", "ss", "wn", "wn1d", "z", "r", "d", "t", "xp", "g"):
            assert np.all(C.bits(o[keep]) == C.SENT_BITS), (name, keep)
        assert C.same(o["sy"], c["sy"]) and C.same(o["wt"], c["wt"]), name


def test_bmv_plain_cases_are_lapack_s(bmv):
    """the two solves of the plain cases through dtrtrs, the sums around them in the statement's order"""
    cases, outs = bmv
    for (name, want, c, p), o in zip(cases, outs):
        if want != "plain":
            continue
        col = int(c["col"][0])
        SY, WT = c.mat("sy", C.M)[:col, :col], np.triu(np.nan_to_num(c.mat("wt", C.M)[:col, :col]))
        v = c["wa"][C.BMV_V:C.BMV_V + 2 * col]
        q = v[col:].copy()
        for i in range(1, col):
            s = 0.0
            for k in range(i):
                s = s + SY[i, k] * v[k] / SY[k, k]
            q[i] = v[col + i] + s
        q = lapack.dtrtrs(np.asfortranarray(WT), q, lower=0, trans=1)[0]
        q = lapack.dtrtrs(np.asfortranarray(WT), q, lower=0, trans=0)[0]
        assert np.array_equal(C.bits(q), C.bits(o["wa"][col:2 * col])), name


def test_subsm_solves_on_the_host_are_the_restatement(subsm):
    cases, outs = subsm
    for (name, want, c, x), o in zip(cases, outs):
        col, ret = int(c["col"][0]), o.rets()[-1]
        if want == "singular":
            assert ret == int(name.split()[-1]) + 1, name
            assert C.same(o["r"], c["r"]) and C.same(o["z"], c["z"]), name     # nothing written
        else:
            assert ret == 0 and C.same(o["wa"][:2 * col], np.array(x)), name
        if want == "plain":
            wv = np.array(C.subsm_wv(col, int(c["nfree"][0]), float(c["theta"][0]), list(c["index"]),
                                     *[[list(c[a][3 * ((int(c["head"][0]) + j) % C.M):][:3]) for j in range(col)] for a in ("ws", "wy")],
                                     list(c["r"])))
            U = np.asfortranarray(np.triu(np.nan_to_num(c.mat("wn", C.M2)[:2 * col, :2 * col])))
            q = lapack.dtrtrs(U, wv, lower=0, trans=1)[0]
            q[:col] = -q[:col]
            q = lapack.dtrtrs(U, q, lower=0, trans=0)[0]
            assert np.array_equal(C.bits(q), C.bits(o["wa"][:2 * col])), name
        for keep in ("sy", "ss", "wt", "wn1d", "d", "t"):
            assert np.all(C.bits(o[keep]) == C.SENT_BITS), (name, keep)


def test_subsm_keeps_the_sign_of_a_zero_direction(host):
    for name, c in C.subsm_negzero_cases():
        o = C.run(host, [c])[0]
        nf = int(c["nfree"][0])
        assert o.rets()[-1] == 0 and np.all(C.bits(o["r"][:nf]) == 0x8000000000000000), name


def test_subsm_on_a_bound_and_an_ulp_either_side(host):
    cases = C.subsm_bound_cases()
    seen = set()
    for (name, c, iword, nx), o in zip(cases, C.run(host, [c for _, c, _, _ in cases])):
        assert o.rets()[-1] == 0 and int(o["iword"][0]) == iword, name
        if iword == 0:
            assert o["z"][1] == nx, name
        seen.add((int(c["nbd"][1]), iword))
    assert seen == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)}


def test_factor_leaves_what_lapack_leaves(host):
    """dpotrf's info, its columns before the failing one and the pivot value it stores -- wherever LAPACK and the host
    form agree on info.  They must on every pivot that is not a NaN; a NaN pivot LAPACK reports (disnan) while the
    host form, the definition here, takes the square root and goes on.  After a +inf pivot the row is scaled by
    1 / inf = 0: OpenBLAS' dscal stores +0 for a zero factor whatever the entry, the host form multiplies and keeps
    the entry's sign -- there, and only there, a zero matches a zero of either sign."""
    cases = C.factor_cases()
    outs = C.run(host, [c for *_, c in cases])
    agreed = 0
    for (name, which, n, A, c), o in zip(cases, outs):
        ret = o.rets()[0]
        U, info = lapack.dpotrf(np.asfortranarray(np.triu(A)), lower=0, clean=0)
        nan_pivot = "pivot nan" in name
        if not nan_pivot:
            assert ret == info, (name, ret, info)
        if "pivot" in name and not nan_pivot and "inf" not in name and "subnormal" not in name:
            assert ret == int(name.split()[-1]) + 1, name
        if ret != info:
            continue
        agreed += 1
        ld, at = (C.M, 0) if which == 1 else (C.M2, 0 if which == 2 else n)
        mine = o.mat("wt" if which == 1 else "wn", ld)[at:at + n, at:at + n]
        upto = n if ret == 0 else ret - 1
        for j in range(upto):
            a, b = mine[:j + 1, j].copy(), U[:j + 1, j].copy()
            if "pivot inf" in name:
                a, b = a + 0.0, b + 0.0         # (-0 + 0 = +0)
            assert C.same(a, b), (name, j)
        if ret:
            assert C.same(mine[ret - 1:ret, ret - 1].copy(), U[ret - 1:ret, ret - 1].copy()), name
        # nothing outside the upper triangle of the block
        full = o.mat("wt" if which == 1 else "wn", ld).copy()
        full[at:at + n, at:at + n][np.tri(n, dtype=bool).T] = C.SENT
        assert np.all(C.bits(np.ascontiguousarray(full)) == C.SENT_BITS), name
    assert agreed >= len(cases) - sum("pivot nan" in name for name, *_ in cases)


UP = lambda n: np.tri(n, dtype=bool).T      # noqa: E731  (the upper triangle, diagonal included)


def test_formt_is_dpotrf_of_the_restated_matrix(host):
    """WT against dpotrf of theta SS + L D^-1 L' formed in formt's order: the return code, and bit for bit every column
    LAPACK finished (all of them after a return of 0) -- col 1 and 2 take the written-out scalar form"""
    cases = C.formt_cases()
    full = 0
    for (name, c, want), o in zip(cases, C.run(host, [c for _, c, _ in cases])):
        ret, U, info = C.formt_restated(c)
        n = int(c["col"][0])
        assert o.rets() == [ret] and (want is None or ret == want), (name, o.rets(), ret)
        mine = o.mat("wt", C.M)[:n, :n]
        for j in range(n if info == 0 else info - 1):
            assert C.same(mine[:j + 1, j].copy(), U[:j + 1, j].copy()), (name, j)
        if info == 0 and np.all(np.isfinite(U[UP(n)])):
            full += 1
            assert np.all(U[np.diag_indices(n)] > 0.0)
        keep = o.mat("wt", C.M).copy()
        keep[:n, :n][UP(n)] = C.SENT
        assert np.all(C.bits(np.ascontiguousarray(keep)) == C.SENT_BITS), name      # nothing outside the triangle
        assert np.all(C.bits(o["wn"]) == C.SENT_BITS), name
    assert full >= 10


def test_formk_is_the_restatement_and_lapack(host):
    """formk against its statements in plain Python (tests/_lb_cases.py: formk_restated) and live LAPACK for the
    factorisation: WN1 -- the strict lower triangle of wn and wn1d, bit for bit: the new row and column, the shift by
    its explicit definition (every cell from its OLD value; the host runs the in-place loop), the change of the free
    set -- the return code, and after a return of 0 the whole factor in the upper triangle."""
    cases = C.formk_cases()
    outs = C.run(host, [c for _, c, _ in cases])
    low = np.tri(C.M2, k=-1, dtype=bool)
    seen = set()
    for (name, c, want), o in zip(cases, outs):
        ret, wn, d, info = C.formk_restated(c)
        col = int(c["col"][0])
        assert o.rets() == [ret] and (want is None or ret == want), (name, o.rets(), ret)
        got = o.mat("wn", C.M2)
        assert C.same(np.ascontiguousarray(got[low]), np.ascontiguousarray(wn[low])) and C.same(o["wn1d"], d), name
        if ret == 0:
            m = np.zeros((C.M2, C.M2), bool)
            m[:2 * col, :2 * col] = UP(2 * col)
            assert C.same(np.ascontiguousarray(got[m]), np.ascontiguousarray(wn[m])), name
            assert np.all(np.isfinite(got[m])) and np.all(got[np.diag_indices(2 * col)] > 0.0), name
        # the call changed WN1 (so the comparison above is not one of inputs with themselves)
        if int(c["updatd"][0]) or int(c["nenter"][0]) or int(c["ileave"][0]) <= 3:
            assert not (C.same(o["wn"], c["wn"]) and C.same(o["wn1d"], c["wn1d"])), name
        seen.add((ret, int(c["updatd"][0]), int(c["nenter"][0]) > 0, int(c["ileave"][0]) <= 3, int(c["iupdat"][0]) > C.M))
    assert {s[0] for s in seen} == {0, -1, -2}
    assert {s[1:] for s in seen} >= {(1, False, False, False), (0, True, False, False), (0, False, True, False),
                                      (0, True, True, False), (1, True, True, True), (1, True, True, False)}
    assert {int(c["nfree"][0]) for _, c, _ in cases} == {0, 1, 2, 3} and {int(c["col"][0]) for _, c, _ in cases} == set(range(1, 11))
    # the shift moved something: the case with iupdat = 11 differs from the one with 10 in the old part
    by = {name: o for (name, _, _), o in zip(cases, outs)}
    a, b = by["formk col=10 iupdat=10"].mat("wn", C.M2), by["formk col=10 iupdat=11"].mat("wn", C.M2)
    assert not np.array_equal(a[1:9, 0], b[1:9, 0])


def test_cmprlb_is_the_restatement(host):
    """r of the free variables and the product bmv left in wa, bit for bit, against the statements in plain Python"""
    cases = C.cmprlb_cases()
    for (name, c), o in zip(cases, C.run(host, [c for _, c in cases])):
        nf, col = int(c["nfree"][0]), int(c["col"][0])
        r, p = C.cmprlb_restated(c)
        assert o.rets()[-1] == 0 and np.all(np.isfinite(r)) and any(q != 0.0 for q in r), name
        assert C.same(o["r"][:nf], np.array(r)) and C.same(o["wa"][:2 * col], np.array(p)), name
        assert np.all(C.bits(o["r"][nf:]) == C.SENT_BITS), name
        for keep in ("ss", "wn", "wn1d", "d", "t", "xp"):
            assert np.all(C.bits(o[keep]) == C.SENT_BITS), (name, keep)


# ---- whole runs --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fd_runs(host):
    starts = [C.run_start(r) for r in C.RUNS]
    return starts, C.drive_steps(host, starts, [C.fd_fg(r) for r in C.RUNS])


def test_step_is_the_hostsim_s_step_after_every_call(hostsim, fd_runs):
    import lockstep_lbfgsb as LS

    dp, ip = LS.dp, LS.ip
    for run_, hist in zip(C.RUNS, fd_runs[1]):
        _, _, _, x0, l, u, nbd, reach = run_
        n = len(x0)
        lay, tot = LS.layout(n)
        low = np.array([0.0 if math.isinf(v) else v for v in l])
        up = np.array([0.0 if math.isinf(v) else v for v in u])
        h = getattr(LS.L, f"hs_lb{n}_new")(LS.P(np.array(x0, float)), LS.P(low), LS.P(up), np.array(nbd, np.int32).ctypes.data_as(ip),
                                          1e7, 1e-5, 20)
        fg = C.fd_fg(run_)
        mx, mf, mg, mset = np.array(x0, float), 0.0, np.zeros(n), 0
        mwa, mint, mdbl = np.zeros(tot), np.zeros(16, np.int32), np.zeros(16)
        assert len(hist) == reach["calls"]
        for call, st in enumerate(hist):
            getattr(LS.L, f"hs_lb{n}_step")(h, LS.P(mx), mf, LS.P(mg), mset)
            getattr(LS.L, f"hs_lb{n}_dump")(h, LS.P(mwa), mint.ctypes.data_as(ip), LS.P(mdbl))
            where = (run_[0], call + 1)
            assert C.same(st["x"], mx), where
            ints = "task msg col head iter iupdat nfgv ifun iback info nfree nskip updatd".split()
            assert [int(st[k][0]) for k in ints] == [int(v) for v in mint[:13]], where
            dbls = "theta stp gd gdold dtd dnorm sbgnrm stpmx fold".split()
            assert C.same(np.array([st[k][0] for k in dbls]), mdbl[:9]), where
            for k, (a, b) in lay.items():
                if k != "snd":
                    assert C.same(st[k], mwa[a:b]), (where, k)
            if mint[0] == C.TASK["FG"]:
                mf, mg = fg(mx.copy())
                mset = 1
            else:
                mset = 0
        getattr(LS.L, f"hs_lb{n}_free")(h)


def test_minimize_is_the_step_run(host):
    """MINIMIZE on the analytic objectives against STEP driven with the same statements in Python; what each run
    reaches with these gradients is pinned, so a change of a functor cannot quietly lose an edge"""
    starts = [C.run_start(r) for r in C.ANALYTIC_RUNS]
    hist = C.drive_steps(host, starts, [(lambda x, o=r[2]: C.fg_analytic(o, x)) for r in C.ANALYTIC_RUNS])
    for run_, st, hh, reach in zip(C.ANALYTIC_RUNS, starts, hist, C.ANALYTIC_REACH):
        o = C.run(host, [st.copy().ops(("MINIMIZE", run_[2], 400, 400))])[0]
        last = hh[-1]
        assert len(hh) == reach["calls"] and int(last["task"][0]) == C.TASK[reach["ending"]], run_[0]
        assert max(int(s["col"][0]) for s in hh) == reach["col"] and max(int(s["iupdat"][0]) for s in hh) == reach["iupdat"], run_[0]
        assert {int(s["nfree"][0]) for s in hh} == reach["nfree"], run_[0]
        assert int(last["info"][0]) == reach.get("info", 0), run_[0]
        assert C.same(o["x"], last["x"]) and int(o["task"][0]) == int(last["task"][0]), run_[0]
        assert int(o["nit"][0]) == sum(int(s["task"][0]) == C.TASK["NEW_X"] for s in hh), run_[0]
        assert int(o["nfev"][0]) == sum(int(s["task"][0]) == C.TASK["FG"] for s in hh), run_[0]
        for k in ("msg", "col", "head", "iter", "iupdat", "nfgv", "info", "nfree", "theta", "f", "sbgnrm", "g", "ws", "wy", "sy", "ss"):
            assert C.same(o[k], last[k]), (run_[0], k)
    # the limits end a run at a new iterate, task NEW_X
    o = C.run(host, [starts[0].copy().ops(("MINIMIZE", 0, 5, 400))])[0]
    assert int(o["nit"][0]) == 5 and int(o["task"][0]) == C.TASK["NEW_X"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_hook_refuses_an_image_that_is_not_safe(host):
    good = C.bmv_cases()[30][2]
    rc, _ = C.run_rc(host, [good])
    assert rc == 0
    edits = [("col", -1), ("col", 11), ("head", -1), ("head", 10), ("itail", 10), ("itail", -1), ("nfree", -1), ("nfree", 4),
             ("nenter", 4), ("nenter", -1), ("nact", 4), ("nact", -1), ("ileave", 0), ("ileave", 5), ("maxls", 65),
             ("iupdat", -1), ("iupdat", 10), ("iupdat", 1 << 21), ("iter", -1), ("task", 2), ("task", 9), ("task", -1),
             ("ls_task", 5), ("ls_task", -1)]      # (iupdat 10 with col 4: past m the shift wants col = m)
    edits += [(k, [0, v, 0]) for k in ("index", "indx2") for v in (-1, 3)] + [("nbd", [0, 4, 0]), ("nbd", [-1, 0, 0])]
    edits += [("in_nbd", [0, 0, 4]), ("nops", 9), ("nops", -1), ("pair", 3 | 7 << 8)]
    for name, value in edits:
        c = good.copy()
        c[name] = value
        before = c.raw.copy()
        rc, out = C.run_rc(host, [good, c])
        assert rc == C.PW_E_BAD_ARG and np.array_equal(out[1].raw, before) and np.array_equal(out[0].raw, good.raw), (name, value)
    for ops in ([("TABLES", 4)], [("TABLES", -1)], [("FACTOR", 0)], [("FACTOR", 4)], [("BMV", 61, 0)], [("BMV", -1, 40)],
                [("BMV", 0, 61)], [("BMV", 0, 19)], [("BMV", 30, 20)], [("MINIMIZE", 4, 10, 10)], [("MINIMIZE", -1, 10, 10)],
                [("MINIMIZE", 0, 501, 10)], [("MINIMIZE", 0, 10, 501)], [("MINIMIZE", 0, 0, 10)]):
        rc, _ = C.run_rc(host, [good.copy().ops(*ops)])
        assert rc == C.PW_E_BAD_ARG, ops
    c = good.copy()
    c["ops"][0] = 11
    assert C.run_rc(host, [c])[0] == C.PW_E_BAD_ARG
    c["ops"][0] = 0
    assert C.run_rc(host, [c])[0] == C.PW_E_BAD_ARG
    one = C.setup_image(1)
    assert C.run_rc(host, [one.copy().ops(("MINIMIZE", 0, 10, 10))])[0] == C.PW_E_BAD_ARG
    assert C.run_rc(host, [one.copy().ops(("MINIMIZE", 4, 10, 10))])[0] == 0
    # the size of a case is part of the call
    L = C._entry()
    assert L.pw_internal_lb_probe(host._h, 3, good.raw.ctypes.data, 1, good.size - 8) == C.PW_E_BAD_ARG
    assert L.pw_internal_lb_probe(host._h, 2, good.raw.ctypes.data, 1, good.size) == C.PW_E_BAD_ARG
    # the 0 a run starts with passes while there is no correction pair
    fresh = C.setup_image(3)
    fresh["ileave"], fresh["col"] = 0, 0
    assert C.run_rc(host, [fresh.ops("STEP")])[0] == 0
