"""The Lennard-Jones energy map of a cavity on the device: pw_affinity on gfx950 against the host path (device = -1) and
against the definition (tests/_affinity_cases.py: reference), as BYTES -- the order of every sum is part of the
definition, so neither the launch geometry, how the jobs are gathered into launches nor what the workspace held before
may show.  numpy only; tests/test_affinity.py holds the host path to the definition."""
import numpy as np
import pytest

import _affinity_cases as C
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


def case_list(host):
    return C.cases() + [C.with_edge_on_a_voxel(host)[0]] + C.big_cases()[:1]


def test_the_case_list(hip_ctx, host):
    """Device == host path == definition, job by job and as one batch with holes, and two consecutive device calls agree."""
    for c in case_list(host):
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
    jobs = case_list(host)
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, host, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host, workspace_bytes):
    """Through pw_internal_affinity with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; with energy maps and without;
    right after a call of other shapes and values: the same bytes, and entries nobody owns untouched."""
    jobs = case_list(host)
    for energies in (True, False):
        packed = C.pack(jobs, hole=1, energies=energies)
        want = C.expected(jobs, host, hole=1, energies=energies)
        for poison in (False, True):
            assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
            S.set_poison(poison)
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
            S.set_poison(False)
            assert rc == 0 and C.same(got, want), (workspace_bytes, energies, poison, C.first_difference(got, want))


def test_a_batch_of_64_mixed_jobs(hip_ctx, host):
    jobs = C.mixed_batch()
    assert len(jobs) == 64 and len({c.dims for c in jobs}) > 10 and {len(c.betas) for c in jobs} >= {1, 8}
    packed = C.pack(jobs, hole=1)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, host, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    rc, again = C.raw(hip_ctx, packed, workspace_bytes=30_000)
    assert rc == 0 and C.same(again, want)


def test_4096_chunks_go_through_the_reduce(hip_ctx, host):
    """One 64^3 grid without a mask and 8 atoms."""
    c = C.big_cases()[1]
    assert c.dims == (64, 64, 64) and c.words is None and len(c.xyz) == 8
    packed = C.pack([c])
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected([c], host)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert int(got[0]["n_voxels"][0]) == 64 * 4096


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank_of(packed)), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_affinity: job 1: ") and what in message, (what, message)


def test_molecule_and_dlpoly_on_jittered_cc3_frames(hip_ctx, tmp_path):
    """Molecule.calculate_guest_affinity and DLPOLY.affinity on 8 jittered CC3 frames: device against host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 700 + t, sigma=0.04) for t in range(8)]
    for xyz in frames[:2]:
        got = []
        for device in (0, -1):
            mol = pw.Molecule({"elements": elements, "coordinates": xyz}, "cc3", 0)
            got.append(mol.calculate_guest_affinity("Xe", 298.0, device=device))
        assert got[0].raw.tobytes() == got[1].raw.tobytes() and got[0].levels.tobytes() == got[1].levels.tobytes()
        assert got[0].closed and got[0].min_energy < 0.0
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    traj.analysis()
    edges = np.linspace(-40.0, 10.0, 11)
    dev = traj.affinity("Xe", [298.0, 195.0], edges=edges, energies=True, device=0)
    ref = traj.affinity("Xe", [298.0, 195.0], edges=edges, energies=True, device=-1)
    assert dev.raw.shape == (8,) and dev.raw.tobytes() == ref.raw.tobytes() and dev.levels.tobytes() == ref.levels.tobytes()
    assert np.array_equal(dev.counts, ref.counts) and all(a.tobytes() == b.tobytes() for a, b in zip(dev.energies, ref.energies))
    assert dev.closed.all() and len(set(dev.n_voxels.tolist())) > 3 and dev.series("heat")[1].all()


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms, the second with a mask, at every budget of a launch from one word
    to all their words and eight more (tests/_grid_sweep.py): every place where the planner can close a launch group.
    Nothing of the inputs starts at 0 and the outputs go to the jobs from the back to the front."""
    import _grid_sweep as G

    betas, edges = ((0.4,), (0.2, 0.9), (0.3,)), ((), (-0.5, 0.5), (0.0,))
    jobs = [C.Case(f"sweep-{k}", d, *C.shell_atoms(n, d, 1.0, 70 + k), words=C.words_with(d, 7, 70) if k == 1 else None,
                   betas=betas[k], edges=edges[k]) for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), *C.shell_atoms(2, (2, 2, 2), 1.0, 80 + k), words=C.words_with((2, 2, 2), 3, 80 + k),
                   betas=(0.1, 0.2), edges=(0.0,)) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert rec["word_first"][1] > 0 and (rec["beta_first"] > 0).all() and (rec["edge_first"][1:] > 0).all()
    assert all((np.diff(rec[name]) < 0).all() for name in ("out", "level_first", "hist_first", "energy_first"))
    V = [packed[10][q] for q in at]
    words = [((c.dims[1] * c.dims[2] + 2) // 2 if c.words is not None else 0)
             + -(-v // 64) * (2 * len(c.betas) + 4 + len(c.edges)) + v + 1 for c, v in zip(jobs, V)]
    G.budget_sweep(C, hip_ctx, host, tuple(packed), words)
