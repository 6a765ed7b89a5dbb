"""The barrier a guest crosses at every window on the device: pw_passage on gfx950 against the host path (device = -1)
and against the definition by another algorithm (tests/_passage_cases.py: a bottleneck Dijkstra), as BYTES -- every
output is a comparison of doubles or a count, so neither the launch geometry, how the jobs are gathered into launches
nor what the workspace held before may show.  numpy only; tests/test_passage.py holds the host path to the definition."""
import numpy as np
import pytest

import _passage_cases as C
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
    """Device == host path == definition, job by job and as one batch with holes, and two consecutive device calls agree."""
    for c in C.cases():
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
    jobs = C.cases()
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got.tobytes(), dtype=np.uint8).reshape(len(got), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_passage with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; right after a call of other shapes
    and values: the same bytes, and rows nobody owns untouched."""
    jobs = C.cases()
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, hole=1)
    for poison in (False, True):
        assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, C.first_difference(got, want))
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes, grids=3)   # (without the fourth bit grid)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, "three grids", C.first_difference(got, want))


def test_lennard_jones_jobs_equal_the_jobs_given_the_map_of_pw_affinity(hip_ctx):
    """field_first == -1 against the same job handed the energies pw_affinity returns on the same context."""
    for c in C.lj_cases():
        packed = C.pack([c], fields=[C.affinity_map(hip_ctx, c)])
        assert packed[0]["field_first"][0] == 0
        rc, got = C.raw(hip_ctx, packed)
        want = C.raw(hip_ctx, C.pack([c]))[1]
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_one_64_cubed_grid(hip_ctx, host):
    """128 KiB of bit grids in LDS, 4096 rows: sixteen a thread."""
    c = C.big_cases()[0]
    packed = C.pack([c])
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected([c])
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed, workspace_bytes=0, grids=3)[1])


def test_a_batch_of_64_mixed_jobs(hip_ctx, host):
    jobs = C.mixed_batch()
    packed = C.pack(jobs, hole=1)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    rc, again = C.raw(hip_ctx, packed, workspace_bytes=30_000)
    assert rc == 0 and C.same(again, want)


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank(packed[5])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_passage: job 1: ") and what in message, (what, message)


def test_the_fills_of_a_row_stay_within_the_bound(hip_ctx, host):
    """The measurement entry's count of flood fills: at most the 64 bisection steps and the three fills round them, on
    both paths."""
    from pywindow_amd import _lib

    jobs = C.cases()
    rec, xyz, coef, planes, field, n_out = C.pack(jobs)
    for ctx in (hip_ctx, host):
        fills = np.full(n_out, -1, dtype=np.int32)
        ctx.passage(rec, xyz, coef, planes, field, fills=fills)
        assert fills.min() >= 0 and fills.max() <= 67 and fills.max() > 3
    assert _lib.PAS_NO_EXIT == C.NO_EXIT and _lib.PAS_SEED_CLOSED == C.SEED_CLOSED


def test_cc3_orderings_and_molecule_device_against_host(hip_ctx):
    """On the bundled CC3: Xe has an interior saddle and a barrier above its well at every window; the activation
    energies order Xe > Kr > He at every window; the well is calculate_guest_affinity's min_energy.  Device == host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    got = {}
    for guest in ("Xe", "Kr", "He"):
        mol = pw.Molecule({"elements": elements, "coordinates": base}, "cc3", 0)
        got[guest] = mol.calculate_guest_passage(guest, device=0)
        assert mol.properties["guest_passage"]["n_windows"] == 4 == got[guest].n_windows
        assert got[guest].raw.tobytes() == mol.calculate_guest_passage(guest, device=-1).raw.tobytes()
        assert (got[guest].raw["flags"] == 0).all()
        af = mol.calculate_guest_affinity(guest, device=0)
        assert (got[guest].well == af.min_energy).all(), guest
    xe = got["Xe"]
    assert not xe.free_exit.any() and (xe.barrier > xe.well).all()
    assert (xe.activation > got["Kr"].activation).all() and (got["Kr"].activation > got["He"].activation).all()
    mol = pw.Molecule({"elements": elements, "coordinates": base}, "cc3", 0)
    none = mol.calculate_guest_passage("Xe", close=None, device=0)
    assert none.raw.shape == (1,) and none.n_windows == 0 and none.barrier[0] == xe.barrier.min()


def test_molecule_and_dlpoly_on_jittered_cc3_frames(hip_ctx, tmp_path):
    """Molecule.calculate_guest_passage and DLPOLY.passage on 8 jittered CC3 frames: device against host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 700 + t, sigma=0.04) for t in range(8)]
    for xyz in frames:
        got = []
        for device in (0, -1):
            mol = pw.Molecule({"elements": elements, "coordinates": xyz}, "cc3", 0)
            got.append(mol.calculate_guest_passage("Xe", device=device))
        assert got[0].raw.tobytes() == got[1].raw.tobytes() and got[0].raw.shape == (4,)
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    traj.analysis()
    dev = traj.passage("Xe", device=0)
    ref = traj.passage("Xe", device=-1)
    assert dev.raw.shape == (8, 4) and dev.raw.tobytes() == ref.raw.tobytes() and dev.frames.tolist() == list(range(8))
    values, valid = dev.series("activation")
    assert valid.all() and len(set(values.tolist())) > 3 and (values == dev.activation.min(axis=1)).all()
    assert traj.passage("Kr", frames=[1, 5], device=0).raw.tobytes() == traj.passage("Kr", frames=[1, 5], device=-1).raw.tobytes()


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids -- the first with a field of its caller's, the others with 1 and 5 atoms; one, no and
    two planes -- at every budget of a launch from one word to all their words and eight more (tests/_grid_sweep.py):
    every place where the planner can close a launch group.  Nothing of the inputs starts at 0 and the rows of out go
    to the jobs from the back to the front."""
    import _affinity_cases as A
    import _grid_sweep as G

    planes = ([[1.0, 0.0, 0.0, 1.5]], None, [[0.0, 1.0, 0.0, 0.5], [0.0, 0.0, 1.0, 1.5]])
    jobs = [C.Case(f"sweep-{k}", d, (0, 0, 0), C.random_field(d, 70, blocked=0.2) if k == 0 else None,
                   *A.shell_atoms(n, d, 1.0, 70 + k), planes=planes[k]) for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), (1, 1, 1), C.random_field((2, 2, 2), 80 + k), *A.shell_atoms(2, (2, 2, 2), 1.0, 80 + k),
                   planes=[[1.0, 1.0, 0.0, 5.0]]) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert rec["plane_first"][0] > 0 and rec["plane_first"][2] > 0 and rec["field_first"][0] > 0 and (rec["field_first"][1:] == -1).all()
    assert (np.diff(rec["out_first"]) < 0).all()
    G.budget_sweep(C, hip_ctx, host, tuple(packed), [d[0] * d[1] * d[2] for d in G.DIMS])
