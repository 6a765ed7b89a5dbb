"""The device-only parts of the optimiser chains -- the candidate lists of NearGap4 / NearGap1 (pw_unit.hpp) under the
pore-centre and window-neck L-BFGS-B runs and the in-plane simplex, and the register solves of pw_lbfgsb.hpp they
drive -- on the constructed cases of tests/_opt_cases.py: lists of 31, 32 (full) and 33 (none) atoms, holders at list
positions 0, 16 and 31 from all three ballot blocks, runs that switch between a list and none, every kind of bound,
every ending SciPy has for them, |p|^2 either side of the 1e9 cut-off, rims of 63, 64 and 65 atoms with the holder
last.  tests/test_opt_edges.py proves on the CPU that each case reaches its edge.  Here the device is compared with
the host context (which has no lists: every atom, one lane) as bytes, whole records and whole stage captures, and with
live SciPy / the oracle exactly.

What the speculative (SPEC) solves do on these cases was counted once with a diagnostic build (DESIGN.md section 2,
"What the edge cases reach in the speculative solves"): no case makes lb_bmv_wave or lb_subsm_solves_wave repeat with
guards, none takes their singular exits, and the neck searches never call them -- these tests do not cover those
routes.  lb_potrf_wave's exit on a pivot that is not positive IS reached: by "cc3/ends on two bounds", "cc3/open" and
"cc3/mixed kinds" (three, three and two times).

Teeth, shown on a scratch build: the rebuild slack DELTA -> test_pore_centre[tilted32/thin box]; no c1 ->
test_pore_centre[placed/*] and every run with a list of more than 16; state from the first ballot block ->
test_pore_centre[shell33/*] and every test_window; total <= 65 in NearGap1 -> test_window[65], and no test outside
this file.  (Dropping the |p|^2 < 1e9 test changes no result: below some 1e5 A a list holds every atom that can hold the
minimum either way.  The cases beyond the cut-off show that the device agrees with the host and SciPy there.)"""
import numpy as np
import pytest

pytest.importorskip("scipy.optimize")
import _opt_cases as C  # noqa: E402
from pywindow_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_ctx():
    return _lib.Context(-1, host_threads=4)


def same_bytes(dev, host, what):
    assert dev.tobytes() == host.tobytes(), (what, [(u, C.diff_fields(dev[u], host[u])) for u in range(len(dev))
                                                    if dev[u].tobytes() != host[u].tobytes()])


@pytest.mark.parametrize("name", C.PORE_NAMES)
def test_pore_centre(hip_ctx, host_ctx, name):
    """One launch of the case alone, one with two CC3 frames of other sizes beside it."""
    case = C.pore_case(name)
    dev = hip_ctx.analyse(case.batch(), C.PORE_STAGES, case.params)
    same_bytes(dev, host_ctx.analyse(case.batch(), C.PORE_STAGES, case.params), name)
    C.check_pore_record(case, dev[0], "device")
    mixed = hip_ctx.analyse(C.mixed_batch(case), C.PORE_STAGES, case.params)
    same_bytes(mixed, host_ctx.analyse(C.mixed_batch(case), C.PORE_STAGES, case.params), name + " (mixed batch)")
    C.check_pore_record(case, mixed[1], "device, mixed batch")
    assert mixed[1].tobytes() == dev[0].tobytes(), C.diff_fields(mixed[1], dev[0])


@pytest.mark.parametrize("m", C.RIMS)
def test_window(hip_ctx, host_ctx, m):
    case = C.window_case(m)
    check_window(hip_ctx, host_ctx, case)


def check_window(hip_ctx, host_ctx, case):
    rec, dbg = case.analyse_debug(hip_ctx)
    hrec, hdbg = case.analyse_debug(host_ctx)
    same_bytes(rec, hrec, f"{case.name} record")
    same_bytes(dbg, hdbg, f"{case.name} capture")
    C.check_window_capture(case, rec[0], dbg[0], "device")


def test_window_search_beyond_the_cutoff(hip_ctx, host_ctx):
    """NearGap1 where |p|^2 >= 1e9 takes its list away (tests/test_opt_edges.py has the conditions)."""
    check_window(hip_ctx, host_ctx, C.window_far_z())
