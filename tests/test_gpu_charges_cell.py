"""Periodic charge equilibration on the device: pw_charges_cell on gfx950 against the host path (device = -1) and against
the restatement of the definition (tests/_charges_cell_cases.py), as BYTES -- the order of every list, every sum and every
step of the solver are part of the definition, so neither the launch geometry, where a job's vectors live (LDS up to 1536
atoms, the workspace beyond), whether a row is stored or recomputed, how the jobs are gathered into launches nor what the
workspace held before may show.  tests/test_charges_cell.py holds the host path to the definition and to numpy."""
import functools

import numpy as np
import pytest

import _charges_cell_cases as C
import _stat_edges as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def test_the_case_list(hip_ctx, host):
    """Device == host path == restatement, job by job and as one batch with holes; two consecutive device calls agree; the
    rows of out and entries of charges nobody owns keep the sentinel."""
    jobs = list(C.cases()) + [C.breakdown_case()]
    for c in jobs:
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c], packed)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    packed = C.pack(jobs, hole=2, pad=3)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, packed)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
    rows = got[1].view(np.uint8).reshape(len(got[1]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 2 * len(jobs)
    owned = np.zeros(packed[4], dtype=bool)
    for r in packed[0]:
        owned[r["charge_first"]:r["charge_first"] + r["n"]] = True
    assert (got[0].view(np.uint8).reshape(-1, 8)[~owned] == C.SENTINEL).all() and (~owned).sum() >= 2 * len(jobs)


def test_breakdown_is_a_result_on_the_device(hip_ctx, host):
    """The flag, NaN charges of the one bit pattern, the step count of the host: nothing runs past max_iter."""
    jobs = [C.breakdown_case(), [c for c in C.cases() if c.name == "coincident, two elements"][0]]
    packed = C.pack(jobs, reverse=True)
    rc, got = C.raw(hip_ctx, packed)
    assert rc == 0 and C.same(got, C.raw(host, packed)[1]) and C.same(got, C.expected(jobs, packed))
    assert (got[1]["flags"] & C.BREAKDOWN).all() and (got[0][:packed[6]].view(np.uint64) == 0x7FF8000000000000).all()


@functools.lru_cache(maxsize=None)
def capacity_jobs():
    """Around the limit of the vectors in LDS (1536 atoms): 1535 and 1536 stay, 1537 goes to the workspace; small jobs in
    between.  A cutoff of 6 Angstrom and an Ewald tolerance of 1e-3 keep the rows short (about 2.4 MB of workspace a big
    job: apart at a budget of 3 MB, together at the default), tol = 1e-4 the solver; the host path is their reference."""
    from pywindow_amd import _lib

    cap = _lib.CHARGES_CELL_LDS_ATOMS
    big = [C.gas_case(n, 300 + n, C.SKEWED if n % 2 else C.ORTHO, cutoff=6.0, tolerance=1e-3, tol=1e-4, converges=False)
           for n in (cap - 1, cap, cap + 1)]
    small = list(C.cases()[:5])
    return [small[0], big[2], small[2], big[0], small[3], big[1], small[4]]


@functools.lru_cache(maxsize=None)
def capacity_expected():
    from pywindow_amd import _lib

    packed = C.pack(capacity_jobs(), hole=1)
    rc, want = C.raw(_lib.Context(-1, host_threads=16), packed)
    assert rc == 0 and (want[1]["flags"][1::2] == 0).all()
    return packed, want


@pytest.mark.parametrize("workspace_bytes", (1, 3_000_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_charges_cell with every job a launch of its own, with 3 MB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; right after a call of other shapes
    and values: the host's bytes, and entries nobody owns untouched."""
    packed, want = capacity_expected()
    for poison in (False, True):
        assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, C.first_difference(got, want))


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, n_points, n_kvecs, what in C.bad_batches():
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=1, n_points=n_points, n_kvecs=n_kvecs)
        assert rc == -2 and C.same(got, C.blank(packed)), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_charges_cell: job 1: ") and what in message, (what, message)


def test_the_cc3_cell_and_the_charged_field_with_qeq_cell(hip_ctx):
    """One frame of the golden CC3 cell at the defaults: device == host path as bytes, converged in fewer than 100 steps; and
    charges="qeq-cell" through rigid_guest_field on the device equals device = -1."""
    import pywindow_amd as pw

    elements, xyz, lattice = C.cc3_cell()
    dev, ref = (pw.equilibrate_cell_charges(xyz, elements, lattice, device=device) for device in (0, -1))
    assert dev.charges.tobytes() == ref.charges.tobytes() and dev.raw.tobytes() == ref.raw.tobytes()
    assert bool(dev.converged) and int(dev.flags) == 0 and int(dev.iterations) < 100 and abs(dev.charges.sum()) < 1e-9
    kw = dict(guest="CO2", temperatures=[250.0], spacing=2.0, cutoff=9.0, directions=pw.sphere_directions(4), charges="qeq-cell")
    a, b = (pw.rigid_guest_field(xyz, elements, lattice, device=device, **kw) for device in (0, -1))
    assert a.raw.tobytes() == b.raw.tobytes() and a.levels.tobytes() == b.levels.tobytes()
    assert a.zbar.tobytes() == b.zbar.tobytes() and bool(a.charges_converged) and a.series("henry")[1].all()
