"""Rigid non-linear guests on the device: pw_rigid_body_affinity on gfx950 against the host path (device = -1) and against
the definition (tests/_rigid_body_cases.py: reference), as BYTES -- the order of every sum is part of the definition, so
neither the launch geometry, which kernel instance serves a job, the block of poses that is in LDS, how the jobs are
gathered into launches nor what the workspace held before may show.  numpy only; tests/test_rigid_body.py holds the host
path to the definition."""
import numpy as np
import pytest

import _affinity_cases as A
import _rigid_body_cases as C
import _rigid_cases as R
import _stat_edges as S

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def hooks_off_afterwards():
    yield
    S.set_launch_cap(0)
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
    rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host, workspace_bytes):
    """Through pw_internal_rigid_body_affinity with every job a launch of its own, with 100 kB a launch and with the
    default; the workspace and the compact result filled with 0xFF before the first kernel or not; with maps and without;
    right after a call of other shapes and values: the same bytes, and entries nobody owns untouched."""
    jobs = C.cases()
    for maps in (True, False):
        packed = C.pack(jobs, hole=1, maps=maps)
        want = C.expected(jobs, host, hole=1, maps=maps)
        for poison in (False, True):
            assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
            S.set_poison(poison)
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
            S.set_poison(False)
            assert rc == 0 and C.same(got, want), (workspace_bytes, maps, poison, C.first_difference(got, want))


def test_a_batch_of_64_mixed_jobs(hip_ctx, host):
    """Every kernel instance, charged and not, in one call; and again at 30 kB a launch."""
    jobs = C.mixed_batch()
    assert len(jobs) == 64 and len({c.dims for c in jobs}) > 10 and {len(c.betas) for c in jobs} >= {1, 8}
    assert {C.body_class(c.S, c.charged) for c in jobs} == set(range(10)) and {c.M for c in jobs} == {6, C.pose_block() + 3}
    packed = C.pack(jobs, hole=1)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, host, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    rc, again = C.raw(hip_ctx, packed, workspace_bytes=30_000)
    assert rc == 0 and C.same(again, want)


def test_256_chunks_go_through_the_reduce(hip_ctx, host):
    """One 64 x 64 x 4 grid without a mask, 8 poses, 3 sites and 8 atoms."""
    c = C.grid_case()[0]
    packed = C.pack([c])
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected([c], host)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert int(got[0]["n_voxels"][0]) == 64 * 256


def test_linear_guests_as_tables_are_the_devices_pw_rigid_affinity(hip_ctx):
    """Every job of tests/_rigid_cases.py's case list and mixed batch with p = t * d, one batch each: the bytes of the
    DEVICE's pw_rigid_affinity, out, levels and maps."""
    for jobs in (R.cases(), R.mixed_batch()):
        rc, got = C.raw(hip_ctx, C.pack([C.from_linear(c) for c in jobs], hole=1))
        rc_l, want = R.raw(hip_ctx, R.pack(jobs, hole=1))
        assert rc == 0 and rc_l == 0 and C.same(got, want), C.first_difference(got, want)


def test_one_site_at_the_centre_in_one_pose_is_pw_affinity_on_the_device(hip_ctx):
    jobs = A.cases()
    rc, (out, levels, _) = C.raw(hip_ctx, C.pack([C.from_affinity(c) for c in jobs]))
    rc_a, (out_a, levels_a, _, _) = A.raw(hip_ctx, A.pack(jobs, energies=False))
    assert rc == 0 and rc_a == 0 and levels.tobytes() == levels_a.tobytes()
    for name in ("n_voxels", "u_min", "min_voxel", "flags"):
        assert out[name].tobytes() == out_a[name].tobytes(), name
    assert np.array_equal(out["n_blocked_poses"], out_a["n_blocked"]) and np.array_equal(out["n_dead"], out_a["n_blocked"])


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank_of(packed)), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_rigid_body_affinity: job 1: ") and what in message, (what, message)


def cap_jobs():
    """Seven jobs of seven instance classes, charged and not: more poses than a block with more atoms than a tile
    first (an instance of two poses a pass) and again in the fifth job (one pose a pass), each followed by a job that
    stages its atoms once and has fewer poses than a block; a masked job; last chunks of 1 and of 64 voxels."""
    PB, tile = C.pose_block(), C.TILE
    shapes = [((5, 13, 1), tile + 2, 3, PB + 3, 0), ((8, 8, 1), 4, 4, 9, 1), ((7, 5, 2), 7, 5, 5, 1), ((4, 4, 4), 3, 1, 5, 0),
              ((43, 3, 1), tile + 1, 7, PB + 1, 0), ((3, 2, 2), 5, 8, 9, 1), ((6, 5, 2), 6, 3, 2 * PB, 1)]
    out = []
    for k, (dims, n, S_, M, charged) in enumerate(shapes):
        words = C.words_with(dims, 40, 950 + k) if k == 2 else None
        out.append(C.Case(f"cap-{k}", dims, *C.guest_atoms(n, S_, dims, 0.7, 960 + k), C.table(S_, M, 0.4, 970 + k), words=words, h=0.7,
                          cutoff2=(0.0, 16.0)[k % 2], betas=((0.4,), (0.0, 0.8), (0.1, 0.5, 0.9))[k % 3], charged=charged,
                          map_level=(k % 3) - 1 if k % 3 else -1))
    return out


def test_every_workgroup_takes_more_than_one_item(hip_ctx, host):
    """One batch in one call with 1, 2, 3 and 5 workgroups a launch (pw_internal_launch_cap), poisoned and not, so that a
    workgroup restages poses and atoms after a finished item of another job: the host path's bytes, the sentinel where
    nobody writes, and every instance of the batch reported as cut."""
    jobs = cap_jobs()
    PB = C.pose_block()
    assert any(c.M > PB and len(c.xyz) > C.TILE for c in jobs)
    classes = {C.body_class(c.S, c.charged) for c in jobs}
    assert len(classes) == 7 and sum(-(-int(C.region(c).sum()) // 64) for c in jobs) >= 2 * max(CAPS)
    packed = C.pack(jobs, hole=1)
    rc, want = C.raw(host, packed)
    assert rc == 0 and C.same(want, C.expected(jobs, host, hole=1))
    for cap in CAPS:
        for poison in (False, True):
            S.set_poison(poison)
            S.set_launch_cap(cap)
            try:
                rc, got = C.raw(hip_ctx, packed)
            finally:
                cut = S.set_launch_cap(0)
                S.set_poison(False)
            assert rc == 0 and C.same(got, want), (cap, poison, C.first_difference(got, want))
            assert cut >= len(classes), (cap, poison, cut)
            rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
            assert int((rows == C.SENTINEL).all(axis=1).sum()) == len(jobs), (cap, poison)


def test_molecule_and_dlpoly_on_jittered_cc3_frames(hip_ctx, tmp_path):
    """Molecule.calculate_rigid_guest_affinity and DLPOLY.rigid_affinity on 8 jittered CC3 frames, SF6 uncharged and H2O
    with framework charges, in rotation_set(4, 2): device against host."""
    import pywindow_amd as pw
    from pywindow_amd import synth

    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 700 + t, sigma=0.04) for t in range(8)]
    rng = np.random.default_rng(3)
    q = rng.uniform(-0.4, 0.4, len(elements))
    q -= q.mean()
    rot = pw.rotation_set(4, 2)
    for guest, charges in (("SF6", None), ("H2O", q)):
        got = []
        for device in (0, -1):
            mol = pw.Molecule({"elements": elements, "coordinates": frames[0]}, "cc3", 0)
            got.append(mol.calculate_rigid_guest_affinity(guest, 298.0, rotations=rot, charges=charges, device=device))
        assert got[0].raw.tobytes() == got[1].raw.tobytes() and got[0].levels.tobytes() == got[1].levels.tobytes()
        assert got[0].closed and got[0].min_energy < 0.0 and got[0].charged == (charges is not None)
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    traj.analysis()
    for guest, charges in (("SF6", None), ("H2O", q)):
        dev = traj.rigid_affinity(guest, [298.0, 195.0], rotations=rot, charges=charges, device=0)
        ref = traj.rigid_affinity(guest, [298.0, 195.0], rotations=rot, charges=charges, device=-1)
        assert dev.raw.shape == (8,) and dev.raw.tobytes() == ref.raw.tobytes() and dev.levels.tobytes() == ref.levels.tobytes()
        assert dev.closed.all() and len(set(dev.n_voxels.tolist())) > 3 and dev.series("heat")[1].all()


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms -- two, three and five sites, the second with a mask and charged,
    the first two with maps -- at every budget of a launch from one word to all their words and eight more
    (tests/_grid_sweep.py): every place where the planner can close a launch group.  Nothing of the inputs starts at 0
    and the outputs go to the jobs from the back to the front."""
    import _grid_sweep as G

    sites, n_poses, betas, level = (2, 3, 5), (1, 3, 2), ((0.4,), (0.2, 0.9), (0.3,)), (0, 1, -1)
    jobs = [C.Case(f"sweep-{k}", d, *C.guest_atoms(n, sites[k], d, 1.0, 70 + k), C.table(sites[k], n_poses[k], 0.3, 70 + k),
                   words=A.words_with(d, 7, 70) if k == 1 else None, betas=betas[k], charged=int(k == 1), map_level=level[k])
            for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), *C.guest_atoms(2, 2, (2, 2, 2), 1.0, 80 + k), C.table(2, 2, 0.3, 80 + k),
                   words=A.words_with((2, 2, 2), 3, 80 + k), betas=(0.1, 0.2), map_level=0) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert rec["word_first"][1] > 0 and all((rec[name] > 0).all() for name in ("beta_first", "pose_first"))
    assert all((np.diff(rec[name]) < 0).all() for name in ("out", "level_first")) and rec["map_first"][0] > rec["map_first"][1] > 0
    V = [packed[9][q] for q in at]
    words = [((c.dims[1] * c.dims[2] + 2) // 2 if c.words is not None else 0) + -(-v // 64) * (2 * len(c.betas) + 6)
             + (2 * v if c.map_level >= 0 else 0) + 1 for c, v in zip(jobs, V)]
    G.budget_sweep(C, hip_ctx, host, tuple(packed), words)
