"""Charge equilibration on the device: pw_charges on gfx950 against the host path (device = -1) and against the
restatement of the definition (tests/_charges_cases.py), as BYTES -- the order of every sum and every step of the solver
are part of the definition, so neither the launch geometry, where a job's vectors live (LDS up to 512 atoms, a global
workspace beyond), how the jobs are gathered into launches nor what the workspace held before may show.
tests/test_charges.py holds the host path to the definition and to numpy."""
import functools

import numpy as np
import pytest

import _charges_cases as C
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
    """Device == host path == restatement, job by job and as one batch with holes, and two consecutive device calls agree."""
    jobs = list(C.cases()) + [C.breakdown_case()]
    for c in jobs:
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c], packed)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    packed = C.pack(jobs, hole=2)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, packed)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
    rows = got[1].view(np.uint8).reshape(len(got[1]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 2 * len(jobs)


def test_breakdown_is_a_result_on_the_device(hip_ctx, host):
    """Bit 1, NaN charges of the one bit pattern, the iteration counts of the host: nothing runs past max_iter."""
    jobs = [C.breakdown_case(), [c for c in C.cases() if c.name == "coincident, two elements"][0]]
    packed = C.pack(jobs)
    rc, got = C.raw(hip_ctx, packed)
    assert rc == 0 and C.same(got, C.raw(host, packed)[1]) and C.same(got, C.expected(jobs, packed))
    assert (got[1]["flags"] & C.BREAKDOWN).all() and (got[0][:packed[5]].view(np.uint64) == 0x7FF8000000000000).all()


def test_a_batch_of_64_mixed_jobs_sharing_parameters_with_outputs_in_reverse(hip_ctx, host):
    jobs = list(C.mixed_batch())
    packed = C.pack(jobs, hole=1, reverse=True, pad=3)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, packed)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])


@functools.lru_cache(maxsize=None)
def capacity_jobs():
    """Around the limit of the vectors in LDS (512 atoms): 511 and 512 stay, 513 and 600 go to the workspace (57 and
    67 kB of it: apart at a budget of 100 kB, together at the default); small jobs in between.  tol = 1e-4 keeps them
    short; the host path is their reference."""
    big = []
    for n in (511, 512, 513, 600):
        x, p = C.cluster(n, 300 + n)
        big.append(C.Case(f"capacity n={n}", 2.5 * x, p, tol=1e-4, converges=False))       # (a 30 Angstrom box: positive definite)
    small = list(C.cases()[:6])
    return [small[0], big[2], small[3], big[0], big[3], small[4], big[1], small[5]]


@functools.lru_cache(maxsize=None)
def capacity_expected():
    from pywindow_amd import _lib

    packed = C.pack(capacity_jobs(), hole=1)
    rc, want = C.raw(_lib.Context(-1, host_threads=16), packed)
    assert rc == 0 and (want[1]["flags"][1::2] == 0).all()
    return packed, want


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_charges with every job a launch of its own, with 100 kB a launch and with the default; the
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

    for packed, n_points, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, n_points=n_points)
            assert rc == -2 and C.same(got, C.blank(packed)), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_charges: job 1: ") and what in message, (what, message)


def test_molecule_and_dlpoly_on_jittered_cc3_frames(hip_ctx, tmp_path):
    """equilibrate_charges, Molecule.calculate_charges and DLPOLY.charges on 8 jittered CC3 frames, and the rigid guest's
    affinity with charges="qeq": device against host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 700 + t, sigma=0.04) for t in range(8)]
    one = [pw.equilibrate_charges(base, elements, device=device) for device in (0, -1)]
    assert one[0].charges.tobytes() == one[1].charges.tobytes() and one[0].raw.tobytes() == one[1].raw.tobytes()
    assert bool(one[0].converged) and abs(one[0].charges.sum()) < 1e-9
    got = []
    for device in (0, -1):
        mol = pw.Molecule({"elements": elements, "coordinates": frames[0]}, "cc3", 0)
        got.append(mol.calculate_charges(device=device))
        assert mol.properties["charges"] is mol.charges
    assert got[0].tobytes() == got[1].tobytes()
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    traj.analysis()
    dev, ref = traj.charges(device=0), traj.charges(device=-1)
    assert dev.charges.shape == (8, 168) and dev.charges.tobytes() == ref.charges.tobytes() and dev.raw.tobytes() == ref.raw.tobytes()
    assert dev.converged.all() and dev.series("dipole_norm")[1].all() and len(set(dev.iterations[:, 0].tolist())) > 1
    dirs = pw.sphere_directions(16)
    auto = [traj.rigid_affinity("CO2", 298.0, directions=dirs, charges="qeq", device=device) for device in (0, -1)]
    by_hand = traj.rigid_affinity("CO2", 298.0, directions=dirs, charges=dev.charges, device=0)
    assert auto[0].raw.tobytes() == auto[1].raw.tobytes() and auto[0].levels.tobytes() == auto[1].levels.tobytes()
    assert auto[0].levels.tobytes() == by_hand.levels.tobytes() and auto[0].charged and auto[0].series("henry")[1].all()
