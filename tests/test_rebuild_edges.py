"""The periodic pre-processing at its edges, on the CPU (tests/_rebuild_cases.py): the sweep reaches every branch class of
the walk, the lists and the cell checks; the oracle and the host build of the kernel source - its slab and its
"team-shared" memory filled with 0xFF - agree exactly in all three memory layouts and with the reference's own output
(tests/golden/rebuild_edges.npz, make_golden.py rebuild_edges); a frame the kernel refuses is refused for a reason that an
independent count confirms.  The two defects of DESIGN.md 3b are cases of the fixture: `thin_reproducer` and `own_copy`."""
import ctypes

import numpy as np
import pytest

import _rebuild_cases as RC
from _util import GOLDEN

LAYOUTS = (1, 3, 0)          # bit sets; bit sets and scan coordinates in team-shared memory; stamp arrays
pytestmark = pytest.mark.filterwarnings("ignore::PendingDeprecationWarning")
NAMES = [c["name"] for c in RC.cases()]


def test_the_sweep_reaches_every_class(hostsim):
    """Dropping a case, or moving a constant of pw_rebuild.hpp, shows here."""
    per_case = {c["name"]: RC.classes(c) for c in RC.cases()}
    got = set().union(*per_case.values())
    want = RC.all_classes()
    assert want - got == set(), f"classes without a case: {sorted(want - got, key=str)}"
    assert got - want - RC.OPTIONAL == set(), f"classes nobody asked for: {sorted(got - want, key=str)}"
    k = RC.constants()
    assert per_case["star17"] >= {("status", k["RB_ST_NB_OVERFLOW"]), ("candidates", k["RB_NB_CAP"] + 1)}
    assert ("candidates", k["RB_NB_CAP"]) in per_case["star16"] and ("status", 0) in per_case["star16"]
    assert ("entry", "hit as cell atom and as image atom") in per_case["own_copy"]
    assert ("cell", "thin", "sheared") in per_case["thin_reproducer"]


def test_the_graphs_are_what_the_distances_say():
    """Synthetic systems: candidate list = bonded partners, every pair CLEAR of every threshold of the bond test."""
    cap = RC.constants()["RB_NB_CAP"]
    for c in RC.cases():
        r = RC.check_graph(c)
        if c["lists"] is not None:
            # the screen's survivors are the partners too: what RB_NB_CAP counts
            assert r[2] == max(len(v) for v in r[0].values()), c["name"]
            assert (r[2] > cap) == bool(c["status"] & RC.constants()["RB_ST_NB_OVERFLOW"]), c["name"]


def test_the_layout_arithmetic_is_the_kernels(hostsim):
    """_rebuild_cases restates RebuildWs::fast_bytes / scan_bytes to tell which layout a launch takes."""
    lib = ctypes.CDLL(str(hostsim / "librebuildprobe.so"))
    lib.hs_rebuild_fast_bytes.restype = ctypes.c_long
    lib.hs_rebuild_scan_bytes.restype = ctypes.c_long
    k = RC.constants()
    assert RC.shared_bytes() >= 2 * 4 * k["RB_LWORK"] + 4 * k["RB_LFINAL"]
    for n in (1, 2, 15, 16, 17, 343, 1344, 4550, 10752, 15625):
        assert lib.hs_rebuild_scan_bytes(n) == RC.scan_bytes(n)
        for rebuild in (0, 1):
            for bits in (0, 1):
                for scan in (0, 1):
                    assert lib.hs_rebuild_fast_bytes(n, rebuild, bits, scan) == RC.fast_bytes(n, rebuild, bits, scan)
    # the layouts the existing device tests were written for (tests/test_rebuild.py)
    assert RC.device_layout(1344, True) == (True, True) and RC.device_layout(5376, True)[0] and not RC.device_layout(10752, True)[0]


def test_the_forced_layouts_are_layouts_the_device_takes(hostsim):
    """At the sizes of the sweep the hook's three values give three layouts: bit sets (one-wave walk) under 1 and 3, none
    (stamp arrays, team loop) under 0; the scan arrays in team-shared memory under 3 where they fit."""
    for group in RC.topologies():
        n, rebuild = group[0]["n"], group[0]["rebuild"]
        if n <= 10000:
            assert RC.device_layout(n, rebuild, 1) == (True, False) and RC.device_layout(n, rebuild, 0) == (False, False)
            assert RC.device_layout(n, rebuild, 3)[0]
    assert any(RC.device_layout(g[0]["n"], g[0]["rebuild"], 3) == (True, True) for g in RC.topologies())
    assert RC.device_layout(15625, False) == (True, False)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN / "rebuild_edges.npz")
    assert sorted(str(n) for n in g["names"]) == sorted(c["name"] for c in RC.cases() if c["fixture"])
    return g


@pytest.fixture(scope="module")
def host_results(hostsim):
    """Every case through the host build, once per layout."""
    return {(c["name"], layout): RC.host_raw(hostsim, c, layout) for c in RC.cases() for layout in LAYOUTS}


@pytest.fixture(scope="module")
def oracle_results():
    return {c["name"]: RC.oracle_flat(c) for c in RC.cases()}


def equal_flat(raw, flat):
    """The host build's (status, n_mol, offsets, src, image, xyz) against (offsets, src, xyz)."""
    return (np.array_equal(raw[2], flat[0]) and np.array_equal(raw[3], flat[1]) and
            raw[5].tobytes() == np.ascontiguousarray(flat[2]).tobytes())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_host_build_agree(name, host_results, oracle_results):
    """Exactly: molecule count, atom order, coordinate bits; in every layout; a refused frame carries the status the
    case was built for and nothing else."""
    c = RC.case(name)
    for layout in LAYOUTS:
        raw = host_results[name, layout]
        assert raw[0] == c["status"], f"{name} layout {layout}: status {raw[0]}"
        if c["status"] == 0:
            assert equal_flat(raw, oracle_results[name]), f"{name} layout {layout}"
        assert RC.same_raw(raw, host_results[name, LAYOUTS[0]]), f"{name}: layout {layout} differs from layout {LAYOUTS[0]}"


@pytest.mark.parametrize("name", [n for n in NAMES if RC.case(n)["fixture"]])
def test_the_reference_itself(name, golden, host_results, oracle_results):
    """The fixture is what the generator makes today; the oracle equals the reference on every case, the host build
    on every case it does not refuse (thin_reproducer: refused since the heights are tested; own_copy: reproduced
    since a walk through an atom with a copy of its own predicts nothing)."""
    c = RC.case(name)
    s = c["system"]
    assert np.array_equal(golden[f"{name}__in_coordinates"], s["coordinates"]) and list(golden[f"{name}__in_elements"]) == list(s["elements"])
    assert ("lattice" in s) == (f"{name}__in_lattice" in golden.files) and ("lattice" not in s or np.array_equal(golden[f"{name}__in_lattice"], s["lattice"]))
    ref = (golden[f"{name}__offset"], golden[f"{name}__src"], golden[f"{name}__xyz"])
    got = oracle_results[name]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes(), f"oracle/{name}"
    for layout in LAYOUTS:
        raw = host_results[name, layout]
        assert raw[0] == c["status"]
        if raw[0] == 0:
            assert equal_flat(raw, ref), f"host build/{name} layout {layout}"


def test_both_reproducers_are_in_the_fixture(golden):
    names = [str(n) for n in golden["names"]]
    assert "thin_reproducer" in names and "own_copy" in names
    # what the reference makes of them: molecules of 1, 1 and 7 atoms; O1 H3 N0 C2 and C2 O1 N0 N0 C2 H3
    assert np.diff(golden["thin_reproducer__offset"]).tolist() == [1, 1, 7]
    assert golden["own_copy__src"].tolist() == [1, 3, 0, 2, 2, 1, 0, 0, 2, 3] and golden["own_copy__offset"].tolist() == [0, 4, 10]


def test_sheared_thin_cells_are_refused(hostsim):
    """The recipe that showed the defect (40 sheared cells 1.8 - 3 A high, default_rng(1)): whatever the host build does not refuse it
    answers as the oracle does, and it refuses exactly the cells with a perpendicular height below max_dist - here all of
    them, two of which it used to answer wrongly; tests/test_rebuild_edges.py::test_fuzz_thin_cells has the mixed regime."""
    k = RC.constants()
    refused = 0
    for t, (m, xyz) in enumerate(RC.sheared_thin_trials()):
        c = RC.make_case(f"trial{t}", ["C"] * 4, xyz, m, rebuild=True)
        thin = RC.heights(m).min() < RC.max_dist(["C"])
        want = RC.oracle_flat(c)
        for layout in LAYOUTS:
            raw = RC.host_raw(hostsim, c, layout)
            assert raw[0] == (k["RB_ST_THIN_CELL"] if thin else 0), (t, layout, RC.heights(m))
            assert thin or equal_flat(raw, want), (t, layout)
        refused += thin
    assert refused > 0


def independent_reasons(c):
    """Why the kernel may refuse this system, counted without it: a perpendicular height below max_dist; more than
    RB_NB_CAP partners inside the generous screen (every range of the bond test widened by 5e-3)."""
    k = RC.constants()
    reasons = 0
    if c["rebuild"] and RC.heights(c["system"]["lattice"]).min() < RC.max_dist(c["system"]["elements"]):
        reasons |= k["RB_ST_THIN_CELL"]
    if RC.brute_lists(c)[2] > k["RB_NB_CAP"]:
        reasons |= k["RB_ST_NB_OVERFLOW"]
    return reasons


def fuzz(hostsim, seed, count, lo, hi, ties):
    rng = np.random.default_rng(seed)
    flagged = 0
    for t in range(count):
        lattice = RC.random_cell(rng, lo, hi)
        el, xyz = RC.random_chain(rng, int(rng.integers(6, 30)), lattice, ties=ties)
        c = RC.make_case(f"fuzz{seed}_{t}", el, xyz, lattice, rebuild=True)
        want = None
        for layout in LAYOUTS:
            raw = RC.host_raw(hostsim, c, layout)
            if raw[0]:
                # a flag is no excuse: it has to be justified, bit by bit
                assert raw[0] & ~independent_reasons(c) == 0, (seed, t, layout, raw[0], RC.heights(lattice))
            else:
                want = RC.oracle_flat(c) if want is None else want
                assert equal_flat(raw, want), (seed, t, layout)
        flagged += raw[0] != 0
    return flagged


@pytest.mark.parametrize("ties", [False, True], ids=["as drawn", "on ties of the eighth decimal"])
def test_fuzz_wrapped_chains(hostsim, ties):
    """250 random wrapped chains of C / N / O / H in random triclinic cells 4 - 12 A high: every unflagged system is
    the oracle's exactly, and at most 2 % are flagged."""
    flagged = fuzz(hostsim, 300 + ties, 250, 4.0, 12.0, ties)
    print("flagged", flagged, "of 250")
    assert flagged <= 5


@pytest.mark.parametrize("ties", [False, True], ids=["as drawn", "on ties of the eighth decimal"])
def test_fuzz_thin_cells(hostsim, ties):
    """Cells 1.8 - 4 A high, around max_dist: each flag justified by an independent count, every unflagged system exact."""
    flagged = fuzz(hostsim, 400 + ties, 120, 1.8, 4.0, ties)
    print("flagged", flagged, "of 120")
    assert 0 < flagged < 120


def test_status_text_states_the_constants():
    """PW_RB_NB_CAP of the header, RB_NB_CAP of the kernel and the binding's message say the same number."""
    import re

    from _util import ROOT
    from pywindow_amd import _lib

    k = RC.constants()
    header = (ROOT / "include" / "pywindow_amd.h").read_text()
    assert int(re.search(r"#define PW_RB_NB_CAP (\d+)", header).group(1)) == k["RB_NB_CAP"] == _lib.RB_NB_CAP
    assert 2 * k["RB_NB_CAP"] <= k["RB_SEG_CAP"]
    assert f"more than {k['RB_NB_CAP']} candidate" in _lib.rb_status_text(k["RB_ST_NB_OVERFLOW"])
    assert "perpendicular height" in _lib.rb_status_text(k["RB_ST_THIN_CELL"])
    assert _lib.rb_status_text(17).startswith("status bits 17: 1 = ") and "16 = " in _lib.rb_status_text(17)
