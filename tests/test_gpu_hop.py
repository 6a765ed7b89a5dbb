"""The free-energy profile of a guest through a window on the device: pw_hop on gfx950 against the host path
(device = -1) and against the definition by another algorithm (tests/_hop_cases.py: a breadth-first search a slab), as
BYTES -- neither the launch geometry, how the jobs are gathered into launches nor what the workspace held before may
show.  numpy only; tests/test_hop.py holds the host path to the definition."""
import numpy as np
import pytest

import _hop_cases as C
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
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
    jobs = C.cases()
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, host, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got[2].tobytes(), dtype=np.uint8).reshape(len(got[2]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host, workspace_bytes):
    """Through pw_internal_hop with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; right after a call of other shapes
    and values: the same bytes, and entries nobody owns untouched."""
    jobs = C.cases()
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, host, hole=1)
    for poison in (False, True):
        assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, C.first_difference(got, want))


def test_lennard_jones_jobs_equal_the_jobs_given_the_map_of_pw_affinity(hip_ctx):
    """field_first == -1 against the same job handed the energies pw_affinity returns on the same context."""
    for c in C.lj_cases():
        packed = C.pack([c], fields=[C.affinity_map(hip_ctx, c)])
        assert packed[0]["field_first"][0] == 0
        rc, got = C.raw(hip_ctx, packed)
        want = C.raw(hip_ctx, C.pack([c]))[1]
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_the_sums_are_pw_affinitys_with_the_slab_as_a_mask(hip_ctx):
    """Six jobs: every slab's returned words fed to pw_affinity on the device as a one-slab mask; (Z, E) equal as bytes."""
    chosen = [c for c in C.lj_cases() if c.words][:6]
    assert len(chosen) == 6
    for c in chosen:
        rc, (slabs, sums, out, words) = C.raw(hip_ctx, C.pack([c]))
        assert rc == 0
        assert sums.tobytes() == C.affinity_of_the_words(hip_ctx, c, words).tobytes(), c.name


def test_a_batch_of_64_mixed_jobs(hip_ctx, host):
    jobs = C.mixed_batch()
    packed = C.pack(jobs, hole=1)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, host, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    rc, again = C.raw(hip_ctx, packed, workspace_bytes=30_000)
    assert rc == 0 and C.same(again, want)


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, told, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, told=told)
            assert rc == -2 and C.same(got, C.blank(packed[6])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_hop: job 1: ") and what in message, (what, message)


def test_the_measurement_entry_times_the_two_kernels(hip_ctx):
    """kernel_ms of Context.hop: the whole, the field kernels and the slab kernels; a job with a field of its own has no
    field kernel."""
    jobs = C.lj_cases()
    rec, xyz, coef, planes, field, betas, sizes = C.pack(jobs)
    ms = []
    hip_ctx.hop(rec, betas, xyz, coef, planes, field, kernel_ms=ms)
    total, field_ms, slab_ms = ms[0]
    assert total > 0.0 and field_ms > 0.0 and slab_ms > 0.0 and field_ms + slab_ms <= total * 1.01 + 0.01


def same_hopping(a, b):
    return (a.slabs.tobytes() == b.slabs.tobytes() and a.Z.tobytes() == b.Z.tobytes() and a.E.tobytes() == b.E.tobytes()
            and a.flags.tobytes() == b.flags.tobytes() and a.n_slabs.tobytes() == b.n_slabs.tobytes())


def test_cc3_orderings(hip_ctx):
    """On the bundled CC3, orderings only: every window is valid and no free exit; the dividing slab lies within 1 A
    of the window plane; rate He > Kr > Xe and free barrier Xe > Kr > He at every window; the Xe rate at cap = 25 and at
    cap = 100 agree to 1e-3 relative (a prototype gave four equal figures: three orders of margin)."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    got = {}
    for guest in ("He", "Kr", "Xe"):
        mol = pw.Molecule({"elements": elements, "coordinates": base}, "cc3", 0)
        hp = got[guest] = mol.calculate_guest_hopping(guest, device=0)
        assert mol.properties["guest_hopping"]["n_windows"] == 4 and hp.rate.shape == (4, 1)
        assert hp.valid.all() and not hp.free_exit.any(), guest
        q_t = np.array([hp.q[w, hp.l_t[w, 0]] for w in range(4)])
        print(guest, "rate", hp.rate[:, 0], "free_barrier", hp.free_barrier[:, 0], "q_t", q_t)
        assert (np.abs(q_t) <= 1.0).all(), (guest, q_t)
    assert (got["He"].rate > got["Kr"].rate).all() and (got["Kr"].rate > got["Xe"].rate).all()
    assert (got["Xe"].free_barrier > got["Kr"].free_barrier).all() and (got["Kr"].free_barrier > got["He"].free_barrier).all()
    mol = pw.Molecule({"elements": elements, "coordinates": base}, "cc3", 0)
    xe = mol.calculate_guest_hopping("Xe", device=0)
    centre, wins = mol.pore_opt_COM, mol.properties["windows"]["centre_of_mass"]
    low = pw.guest_hopping(base, elements, "Xe", centre, wins, [298.0], cap=25.0, device=0)
    high = pw.guest_hopping(base, elements, "Xe", centre, wins, [298.0], cap=100.0, device=0)
    print("cap 25", low.rate[:, 0], "cap 100", high.rate[:, 0])
    assert same_hopping(high, xe)
    assert (np.abs(low.rate - high.rate) <= 1e-3 * high.rate).all()


def test_molecule_and_dlpoly_on_jittered_cc3_frames(hip_ctx, tmp_path):
    """Molecule.calculate_guest_hopping and DLPOLY.hopping on 8 jittered CC3 frames: device against host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 700 + t, sigma=0.04) for t in range(8)]
    for xyz in frames:
        got = []
        for device in (0, -1):
            mol = pw.Molecule({"elements": elements, "coordinates": xyz}, "cc3", 0)
            got.append(mol.calculate_guest_hopping("Xe", device=device))
        assert same_hopping(got[0], got[1]) and got[0].slabs.shape[:2] == (1, 4) and got[0].single
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    traj.analysis()
    dev = traj.hopping("Xe", [298.0, 350.0], device=0)
    ref = traj.hopping("Xe", [298.0, 350.0], device=-1)
    assert dev.Z.shape[:2] == (8, 4) and dev.Z.shape[3] == 2 and same_hopping(dev, ref) and dev.frames.tolist() == list(range(8))
    values, valid = dev.series("rate")
    best = np.where(dev.valid[:, :, 0], dev.rate[:, :, 0], -np.inf).max(axis=1)
    assert valid.any() and (values[valid] == best[valid]).all() and (dev.series("escape_rate")[0][valid] >= values[valid]).all()
    print("rates", dev.rate[:, :, 0], "mean", dev.mean_rate())
    assert same_hopping(traj.hopping("Kr", 298.0, frames=[1, 5], device=0), traj.hopping("Kr", 298.0, frames=[1, 5], device=-1))


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids -- the first with a field of its caller's, the others with 1 and 5 atoms; one, no and
    two planes; one, two and one betas; the second without words -- at every budget of a launch from one word to all
    their words and eight more (tests/_grid_sweep.py): every place where the planner can close a launch group.  Nothing
    of the inputs starts at 0 and the outputs go to the jobs from the back to the front."""
    import _affinity_cases as A
    import _grid_sweep as G

    planes = ([[1.0, 0.0, 0.0, 1.5]], None, [[0.0, 1.0, 0.0, 0.5], [0.0, 0.0, 1.0, 1.5]])
    betas = ((0.4,), (0.2, 0.9), (0.3,))
    jobs = [C.Case(f"sweep-{k}", d, (0, 0), C.random_field(d, 70) if k == 0 else None, *A.shell_atoms(n, d, 1.0, 70 + k),
                   planes=planes[k], betas=betas[k], words=k != 1) for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), (1, 1), C.random_field((2, 2, 2), 80 + k), *A.shell_atoms(2, (2, 2, 2), 1.0, 80 + k),
                   planes=[[1.0, 1.0, 0.0, 5.0]], betas=(0.1, 0.2)) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert rec["plane_first"][0] > 0 and rec["plane_first"][2] > 0 and (rec["beta_first"] > 0).all()
    assert rec["field_first"][0] > 0 and (rec["field_first"][1:] == -1).all() and rec["word_first"][1] == -1
    assert all((np.diff(rec[name]) < 0).all() for name in ("slab_first", "sum_first", "out")) and rec["word_first"][0] > rec["word_first"][2] > 0
    G.budget_sweep(C, hip_ctx, host, tuple(packed), [d[0] * d[1] * d[2] for d in G.DIMS])
