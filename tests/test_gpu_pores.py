"""The probe-swept cavity for a ladder of probes on the device: pw_pore_sizes on gfx950 against the host path
(device = -1) and against the definition (tests/_pores_cases.py: reference), EXACTLY -- every output is an integer, the
fill is a least fixed point and the sweep has no floating point, so neither the launch geometry, the order of the
levels, how the jobs are gathered into launches nor what the workspace held before may show.  numpy only;
tests/test_pores.py holds the host path to the definition."""
import numpy as np
import pytest

import _cavity_cases as C
import _pores_cases as P
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
    for c in P.cases():
        packed = P.Packed([c])
        rc, got = P.raw(hip_ctx, packed)
        want = packed.expected()
        assert rc == 0 and P.same(got, want), (c.name, P.first_difference(got, want))
        assert P.same(got, P.raw(host, packed)[1]), c.name
    packed = P.Packed(P.cases(), hole=3)
    rc, got = P.raw(hip_ctx, packed)
    want = packed.expected()
    assert rc == 0 and P.same(got, want), P.first_difference(got, want)
    assert P.same(got, P.raw(host, packed)[1]) and P.same(got, P.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got[1].tobytes(), dtype=np.uint8).reshape(len(got[1]), -1)
    assert (rows == P.SENTINEL).all(axis=1).sum() == 3 * len(P.cases())


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_pore_sizes with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact results filled with 0xFF before the first kernel or not; with masks for all jobs, for
    some and for none; right after a call of other shapes and values: the same integers, and entries nobody owns
    untouched."""
    jobs = P.mixed_batch()
    some = [k % 3 != 1 for k in range(len(jobs))]
    for masks in (True, some, False):
        packed = P.Packed(jobs, hole=1, masks=masks)
        want = packed.expected()
        for poison in (False, True):
            assert P.raw(hip_ctx, P.Packed(P.other_shapes()))[0] == 0
            S.set_poison(poison)
            rc, got = P.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
            S.set_poison(False)
            assert rc == 0 and P.same(got, want), (workspace_bytes, poison, P.first_difference(got, want))


def test_a_batch_of_64_jobs_of_mixed_grids_and_ladders(hip_ctx, host):
    jobs = P.mixed_batch()
    assert len(jobs) == 64
    packed = P.Packed(jobs, hole=1)
    rc, got = P.raw(hip_ctx, packed)
    want = packed.expected()
    assert rc == 0 and P.same(got, want), P.first_difference(got, want)
    assert P.same(got, P.raw(host, packed)[1])
    levels, out, _ = got
    for k, c in enumerate(jobs):
        first = int(packed.rec["level_first"][k])
        assert out["n_domain"][int(packed.rec["out"][k])] == levels["n_largest"][first:first + c.L].sum(), c.name


def test_every_levels_reach_is_pw_cavity_at_that_probe_on_the_same_context(hip_ctx):
    for name in ("atoms-0", "atoms-1", "atoms-5", "atoms-200", "tie", "ladder-64"):
        c = next(c for c in P.cases() if c.name == name)
        rc, (levels, out, mask) = P.raw(hip_ctx, P.Packed([c]))
        cav, words = hip_ctx.cavity(*C.pack([c.level(q) for q in range(c.L)])[:4])
        assert rc == 0 and np.array_equal(levels["n_reach"], cav["n_voxels"]) and np.array_equal(levels["n_face"], cav["n_face"])
        assert np.array_equal(levels["flags"], cav["flags"]) and np.array_equal(mask[:len(mask) // c.L], words[:len(words) // c.L])


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in P.bad_batches():
        for budget in (None, 1):
            rc, got = P.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and P.same(got, packed.blank()), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_pore_sizes: job 1: ") and what in message, (what, message)
    packed = P.bad_batches()[2][0]
    with pytest.raises(ValueError, match="job 1: the probes are not strictly ascending"):
        hip_ctx.pore_sizes(packed.rec, packed.xyz, packed.radii, packed.probes, packed.planes)


def test_the_public_layer_on_jittered_cc3_frames(hip_ctx):
    """pw.pore_size_distribution_batch on 20 jittered CC3 frames with 12 levels, each frame seeded at its optimised
    pore centre and closed at planes through its own windows (one analysis on the device finds them): device against
    host, and every level's reach against pw.cavity_grid_batch."""
    import pywindow_amd as pw
    from pywindow_amd import engine, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 500 + t, sigma=0.05) for t in range(20)])
    recs = engine.analyse([(elements, f) for f in frames], device=0)
    assert (recs["n_windows"] == 4).all()
    planes = [window_planes(r["pore_opt_c"], engine.windows_of(r)[1]) for r in recs]
    radii = VDW[element_ids(elements)]
    kw = dict(probes=0.25 * np.arange(12), spacing=0.5, half_widths=recs["maxd"] / 2.0, planes=planes, masks=True)
    dev = pw.pore_size_distribution_batch(frames, radii, recs["pore_opt_c"], device=0, **kw)
    ref = pw.pore_size_distribution_batch(frames, radii, recs["pore_opt_c"], device=-1, **kw)
    assert dev.levels.tobytes() == ref.levels.tobytes() and dev.raw.tobytes() == ref.raw.tobytes()
    assert all(np.array_equal(a, b) for x, y in zip(dev.masks, ref.masks) for a, b in zip(x, y))
    assert dev.closed.all() and (np.diff(dev.cumulative, axis=1) <= 0).all() and len(set(dev.levels["n_swept"][:, 6].tolist())) > 5
    assert np.array_equal(dev.cumulative[:, 0], dev.domain_volume) and (dev.raw["n_none"] == 0).all()
    cav = pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], 1.5, 0.5, recs["maxd"] / 2.0, planes, device=0)
    assert np.array_equal(dev.reach_volume[:, 6], cav.volume) and np.array_equal(dev.series("reach_volume", 6)[1], cav.closed)


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms and ladders of 2, 1 and 3 probes -- the first with ready-made open
    words, the second without a mask -- at every budget of a launch from one word to all their words and eight more
    (tests/_grid_sweep.py): every place where the planner can close a launch group.  Nothing of the inputs starts at 0
    and the outputs go to the jobs from the back to the front."""
    import _grid_sweep as G

    rng = np.random.default_rng(70)
    ladder = ([0.0, 0.3], [0.2], [0.0, 0.3, 0.6])
    planes = (None, [[1.0, 0.0, 0.0, 2.5]], [[0.0, 1.0, 0.0, 1.5], [0.0, 0.0, 1.0, 9.0]])
    jobs = []
    for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS)):
        xyz, radii = C.random_atoms(n, d, 70 + k, 1.0, radius=(0.2, 0.6))
        given = rng.integers(0, 1 << d[0], (len(ladder[k]), d[1] * d[2]), dtype=np.uint64) if k == 0 else None
        jobs.append(P.Case(f"sweep-{k}", d, (0, 0, 0), ladder[k], 1.0, xyz=xyz, radii=radii, planes=planes[k], words=given))
    pads = []
    for k in range(3):
        xyz, radii = C.random_atoms(2, (2, 2, 2), 80 + k, 1.0)
        pads.append(P.Case(f"pad-{k}", (2, 2, 2), (1, 1, 1), [0.0, 0.1], 1.0, xyz=xyz, radii=radii, planes=[[1.0, 1.0, 0.0, 5.0]],
                           words=np.full((2, 4), 3, dtype=np.uint64)))
    order, at = G.interleaved(pads, jobs)
    packed = P.Packed(order, hole=1, masks=[c.name != "sweep-1" for c in order])
    rec = packed.rec = np.ascontiguousarray(packed.rec[at])
    packed.open_first = np.ascontiguousarray(packed.open_first[at])
    packed.jobs, packed.with_mask = jobs, [True, False, True]
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["radius_first"][1:] > 0).all()
    assert (rec["plane_first"][1:] > 0).all() and (rec["probe_first"] > 0).all()
    assert packed.open_first[0] > 0 and (packed.open_first[1:] == -1).all() and rec["mask_first"][1] == -1
    assert all((np.diff(rec[name]) < 0).all() for name in ("out", "level_first")) and rec["mask_first"][0] > rec["mask_first"][2] > 0
    words = [c.L * c.dims[1] * c.dims[2] * (int(c.words is not None) + int(k != 1)) + 1 for k, c in enumerate(jobs)]
    G.budget_sweep(P, hip_ctx, host, packed, words)
