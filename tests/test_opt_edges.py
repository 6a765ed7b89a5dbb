"""The optimiser chains at the edges of their candidate lists, on the CPU: the host context (the kernel source for a
one-lane team, which evaluates every atom) against live SciPy on every constructed case of tests/_opt_cases.py, and
the conditions that make a case what its name says -- counted with numpy from the points SciPy evaluated.  A case that
stops reaching its edge fails here; tests/test_gpu_opt_edges.py then runs the same cases through the device-only
lists (NearGap4 / NearGap1) and compares with these results."""
import numpy as np
import pytest

pytest.importorskip("scipy.optimize")
import _opt_cases as C  # noqa: E402
from pywindow_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def host_ctx():
    return _lib.Context(-1, host_threads=4)


def switches(inside):
    """(times the flag goes True -> False, times it goes False -> True) along a sequence."""
    inside = np.asarray(inside, bool)
    return int((inside[:-1] & ~inside[1:]).sum()), int((~inside[:-1] & inside[1:]).sum())


# ---- the bookkeeping itself ----------------------------------------------------------------------------------------
def test_bookkeeping():
    vdw = np.array([1.7, 1.2, 1.7, 1.5, 1.2, 1.7])
    assert C.stored_order(vdw).tolist() == [0, 2, 5, 1, 4, 3]
    assert C.stored_order(np.full(5, 1.2)).tolist() == [0, 1, 2, 3, 4]
    assert [C.stored_index(vdw, a) for a in range(6)] == [0, 3, 1, 5, 4, 2]
    xyz = np.array([[3.0, 0, 0], [0, 2.6, 0], [0, 0, -3.2], [9.0, 0, 0], [0, -2.5, 0], [-3.5, 0, 0]])
    p = np.zeros(3)          # gaps 1.3, 1.4, 1.5, 7.5, 1.3, 1.8: the first of the two smallest holds
    assert C.holder(xyz, vdw, p) == 0 and C.candidates(xyz, vdw, p) == 5
    assert [C.list_position(xyz, vdw, p, a) for a in (0, 2, 5, 1, 4)] == [0, 1, 2, 3, 4]
    # a gap within 1e-9 of the slack: the case is refused, not counted either way
    xyz[5, 0] = -(1.3 + C.SLACK + 1.7) + 5e-10
    with pytest.raises(C.CaseRejected):
        C.candidates(xyz, vdw, p)
    assert [c.nbd for c in C.cc3_boxes()[-2:]] == [(0, 0, 0), (0, 1, 3)]


# ---- pore cases: the host context against SciPy --------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PORE_NAMES)
def test_host_context_matches_scipy(host_ctx, name):
    case = C.pore_case(name)
    rec = host_ctx.analyse(case.batch(), C.PORE_STAGES, case.params)
    C.check_pore_record(case, rec[0], "host")
    mixed = host_ctx.analyse(C.mixed_batch(case), C.PORE_STAGES, case.params)
    assert mixed[1].tobytes() == rec[0].tobytes(), C.diff_fields(mixed[1], rec[0])
    assert tuple(mixed["n_atoms"]) == (163, len(case.xyz), 151)


@pytest.mark.parametrize("n", (31, 32, 33))
def test_small_box_keeps_its_count(n):
    """31 and 32 keep a list throughout (32: a full one), 33 never has one."""
    case = C.pore_case(f"shell{n}/box0.1")
    assert len(case.xyz) == n + 40 and (case.counts == n).all(), (case.name, case.counts)
    assert case.ref["res"].nit >= 8 and len(case.counts) >= 200          # (a run of some length, not a start that converged)


@pytest.mark.parametrize("name", ("placed/one radius", "placed/two radii"))
def test_placed_holders(name):
    """A full list whose last, seventeenth and first entries hold the minimum at recorded points -- the last at the
    final one -- and sit in the third, second and first ballot block of 64 stored atoms."""
    case = C.pore_case(name)
    assert len(case.xyz) >= 130 and (case.counts == C.LIST4).all()
    along, final = C.placed_facts(case)
    assert final[0] == 31 and final[1] >= 128, final
    assert any(pos == 16 and 64 <= idx < 128 for pos, idx in along), sorted(set(along))
    assert any(pos == 0 and idx < 64 for pos, idx in along), sorted(set(along))
    two = len(set(case.vdw)) == 2
    assert two == ("two" in case.name)
    # two radii: the stored order is not the input order, and the atom reported is the input index
    assert two == (not np.array_equal(C.stored_order(case.vdw), np.arange(len(case.vdw))))
    if two:
        assert C.stored_index(case.vdw, case.ref["atom"]) != case.ref["atom"]
        assert len({case.vdw[a] for a in C.stored_order(case.vdw)[[5, 135]]}) == 2     # the list spans both groups


@pytest.mark.parametrize("n", (32, 33, 65))
def test_wide_box_crosses_the_capacity(n):
    """The count reaches the shell's size and falls far below it; above 32 atoms in the shell, rebuilds go from a
    list to none and back within one run."""
    case = C.pore_case(f"shell{n}/box1")
    assert case.counts.max() == n and case.counts.min() <= 12, (case.name, case.counts)
    down, up = switches(case.counts <= C.LIST4)
    assert (down >= 1 and up >= 1) if n > C.LIST4 else (down == up == 0), (case.name, case.counts)
    if n == C.LIST4:          # exactly full, and not all the time
        assert switches(case.counts == C.LIST4)[0] >= 1 and switches(case.counts == C.LIST4)[1] >= 1


def test_tilted_shell_needs_the_whole_slack():
    """One list from the start to the end, full, and points whose holder a slack of DELTA would have left out."""
    case = C.pore_case("tilted32/thin box")
    assert (case.counts == C.LIST4).all() and case.ref["res"].nit >= 3
    refs = C.references(case)
    assert (refs == case.start).all()
    assert C.beyond_delta(case) >= 8
    # (the other runs of a full list never need it: what this case adds)
    assert all(C.beyond_delta(C.pore_case(n)) == 0 for n in ("shell32/box0.1", "placed/one radius", "placed/two radii"))


def test_cc3_boxes_cover_the_endings_and_the_bound_kinds():
    cases = C.cc3_boxes()
    assert {tuple(C.TASKS[str(c.ref["res"].message)][:2]) for c in cases} == {(4, 401), (4, 402), (8, 0)}
    assert {k for c in cases for k in c.nbd} == {0, 1, 2, 3}
    by = {c.name[4:]: c for c in cases}
    # ends on two bounds, stopped by the projected gradient
    c = by["ends on two bounds"]
    x = c.ref["res"].x
    assert sum(x[k] in c.box[k] for k in range(3)) == 2 and "PROJECTED GRADIENT" in c.ref["res"].message
    # the open boxes let the centre leave the cage: ABNORMAL, far beyond the exponents of an ordinary run
    for name in ("open", "mixed kinds"):
        r = by[name].ref
        assert r["res"].message.startswith("ABNORMAL") and np.abs(r["points"]).max() > 1e15, (name, r["res"])
        assert by[name].counts.max() == len(by[name].xyz)          # (every atom is a candidate out there)
    # forward differences that do not fit: 1e-8 is more than either side of the thin axis has, at every point
    c = by["thin axis"]
    lo, hi = c.box[1]
    assert all(max(p[1] - lo, hi - p[1]) < 1e-8 for p in c.ref["points"])
    # ... and a step that would leave the box is taken backwards
    c = by["start on an upper bound"]
    assert c.start[1] == c.box[1][1] and c.start[1] + 1e-8 > c.box[1][1]
    c = by["start in a corner"]
    assert all(c.start[k] in c.box[k] for k in range(3))
    assert all(cc.counts.max() < C.LIST4 for cc in cases if cc.nbd == (2, 2, 2))     # the ordinary runs never fill a list


def test_far_frames_straddle_the_cutoff():
    """|p|^2 of every point SciPy evaluates is below 1e9 for the first shift and at or above it for the second."""
    near, far = C.cc3_far()
    assert ((near.ref["points"] ** 2).sum(axis=1) < 1.0e9).all() and (near.ref["points"] ** 2).sum(axis=1).max() > 0.999e9
    assert ((far.ref["points"] ** 2).sum(axis=1) >= 1.0e9).all() and (far.ref["points"] ** 2).sum(axis=1).min() < 1.001e9
    assert near.counts.max() <= C.LIST4 and far.counts.max() <= C.LIST4      # (only the cut-off takes the list away)


# ---- window cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.RIMS)
def test_window_reaches_its_rim(host_ctx, m):
    case = C.window_case(m)
    ref = case.ref
    assert ref["win"] is not None and len(ref["win"][0]) == 1 and len(ref["detail"]["windows"]) == 1
    assert abs(ref["win"][0][0] - 4.60) < 0.01
    rot, p = ref["detail"]["windows"][0]["rot"], case.final_point()
    mask = C.listed(rot, case.vdw, p)
    assert mask.sum() == case.m and np.array_equal(mask, case.is_rim)      # the rim, all of it, nothing else
    if case.m in C.LAST_HOLDER:
        h = C.holder(rot, case.vdw, p)
        assert C.list_position(rot, case.vdw, p, h) == C.LAST_HOLDER[case.m] == case.m - 1
    rec, dbg = case.analyse_debug(host_ctx)
    C.check_window_capture(case, rec[0], dbg[0], "host")


def test_window_search_beyond_the_cutoff(host_ctx):
    """The in-plane search of a window whose neck search was held 31700 A out: every point it evaluates has
    |p|^2 >= 1e9, where no list is kept although the atoms that could hold the minimum would fit one."""
    case = C.window_far_z()
    w = case.ref["detail"]["windows"][0]
    assert w["z"].x[0] == C.FAR_Z and C.FAR_Z ** 2 >= 1.0e9 > (C.FAR_Z - 100.0) ** 2
    assert C.candidates(w["rot"], case.vdw, np.array([0.0, 0.0, C.FAR_Z])) <= C.LIST1
    assert np.isfinite(case.ref["win"][0]).all() and np.isfinite(case.ref["win"][1]).all()
    rec, dbg = case.analyse_debug(host_ctx)
    C.check_window_capture(case, rec[0], dbg[0], "host")


def test_neck_searches_run_with_and_without_a_list():
    """The neck search (one variable, the four-point list) ends on the window's axis, off the rim's centre: it sees a
    part of the rim there -- a list for the small rims, more than 32 atoms and no list for the large ones."""
    counts = {}
    for m in C.RIMS:
        w = C.window_case(m).ref["detail"]["windows"][0]
        counts[m] = C.candidates(w["rot"], C.window_case(m).vdw, np.array([0.0, 0.0, w["z"].x[0]]))
        assert w["z"].nit >= 1
    assert max(counts[m] for m in (20, 32, 33)) <= C.LIST4 < min(counts[m] for m in (63, 64, 65)), counts
