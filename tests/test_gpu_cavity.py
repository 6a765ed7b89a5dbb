"""The cavity of a cage on the device: pw_cavity on gfx950 against the host path (device = -1) and against the definition
(tests/_cavity_cases.py: reference), EXACTLY -- every output is an integer and the fill is a least fixed point, so
neither the launch geometry, the order in which rows are swept, how the jobs are gathered into launches nor what the
workspace held before may show.  numpy only; tests/test_cavity.py holds the host path to the definition."""
import numpy as np
import pytest

import _cavity_cases as C
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
    rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_cavity with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; with masks and without; right
    after a call of other shapes and values: the same integers, and entries nobody owns untouched."""
    jobs = C.cases() + C.big_cases()[:2]
    for mask in (True, False):
        packed = C.pack(jobs, hole=1, mask=mask)
        want = C.expected(jobs, hole=1, mask=mask)
        for poison in (False, True):
            assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
            S.set_poison(poison)
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
            S.set_poison(False)
            assert rc == 0 and C.same(got, want), (workspace_bytes, mask, poison, C.first_difference(got, want))


def test_atoms_beyond_any_staging_many_planes_and_the_largest_grid(hip_ctx, host):
    """5000 atoms on a 16^3 grid (the kernel stages nothing: an atom is a scalar load), 200 planes, 64^3 voxels."""
    for c in C.big_cases():
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
    assert len(C.big_cases()[0].xyz) == 5000 and len(C.big_cases()[1].planes) == 200 and C.big_cases()[2].dims == (64, 64, 64)
    full = C.reference_cached(C.big_cases()[3])[0]
    assert full["n_voxels"] == 64 ** 3 and full["n_face"] == 64 ** 3 - 62 ** 3


def test_a_batch_of_64_jobs_of_mixed_grid_sizes(hip_ctx, host):
    jobs = C.mixed_batch()
    assert len(jobs) == 64 and (64, 64, 64) in [c.dims for c in jobs] and len({c.dims for c in jobs}) > 10
    packed = C.pack(jobs, hole=1)
    rc, got = C.raw(hip_ctx, packed)
    want = C.expected(jobs, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    rc, again = C.raw(hip_ctx, packed, workspace_bytes=300_000)
    assert rc == 0 and C.same(again, want)


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank(packed[4], packed[5])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_cavity: job 1: ") and what in message, (what, message)
    packed = C.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        hip_ctx.cavity(packed[0], packed[1], packed[2], packed[3])


def test_the_public_layer_on_jittered_cc3_frames(hip_ctx):
    """pw.cavity_grid_batch on 20 jittered CC3 frames, each seeded at its optimised pore centre and closed at planes
    through its own windows (one analysis on the device finds them): device against host."""
    import pywindow_amd as pw
    from pywindow_amd import engine, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 500 + t, sigma=0.05) for t in range(20)])
    recs = engine.analyse([(elements, f) for f in frames], device=0)
    assert (recs["n_windows"] == 4).all()
    planes = [window_planes(r["pore_opt_c"], engine.windows_of(r)[1]) for r in recs]
    kw = dict(probe=0.0, spacing=0.5, half_widths=recs["maxd"] / 2.0, planes=planes, mask=True)
    dev = pw.cavity_grid_batch(frames, VDW[element_ids(elements)], recs["pore_opt_c"], device=0, **kw)
    ref = pw.cavity_grid_batch(frames, VDW[element_ids(elements)], recs["pore_opt_c"], device=-1, **kw)
    assert dev.raw.tobytes() == ref.raw.tobytes() and {tuple(s) for s in dev.shape} <= {(46, 46, 46), (48, 48, 48)}
    assert all(np.array_equal(a, b) for a, b in zip(dev.mask, ref.mask))
    assert np.array_equal(dev.volume, ref.volume) and np.array_equal(dev.gyration, ref.gyration)
    assert dev.closed.all() and (dev.volume > recs["pore_vol_opt"]).all() and len(set(dev.n_voxels.tolist())) > 5
    assert np.array_equal(dev.series("volume")[1], dev.n_face == 0)


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms -- the first with ready-made open words, the second without a
    mask -- at every budget of a launch from one word to all their words and eight more (tests/_grid_sweep.py): every
    place where the planner can close a launch group.  Nothing of the inputs starts at 0 and the outputs go to the jobs
    from the back to the front."""
    import _grid_sweep as G

    rng = np.random.default_rng(70)
    planes = (None, [[1.0, 0.0, 0.0, 2.5]], [[0.0, 1.0, 0.0, 1.5], [0.0, 0.0, 1.0, 9.0]])
    jobs = [C.Case(f"sweep-{k}", d, (0, 0, 0), *C.random_atoms(n, d, 70 + k, 1.0, radius=(0.2, 0.6)), probe=0.1 * k, h=1.0,
                   planes=planes[k], words=rng.integers(0, 1 << d[0], d[1] * d[2], dtype=np.uint64) if k == 0 else None)
            for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), (1, 1, 1), *C.random_atoms(2, (2, 2, 2), 80 + k, 1.0), h=1.0, planes=[[1.0, 1.0, 0.0, 5.0]],
                   words=np.full(4, 3, dtype=np.uint64)) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    open_first = packed[7] = np.ascontiguousarray(packed[7][at])
    rec["mask_first"][1] = -1
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["radius_first"][1:] > 0).all()
    assert (rec["plane_first"][1:] > 0).all() and open_first[0] > 0 and (open_first[1:] == -1).all()
    assert (np.diff(rec["out"]) < 0).all() and rec["mask_first"][0] > rec["mask_first"][2] > 0
    words = [c.dims[1] * c.dims[2] * (int(c.words is not None) + int(k != 1)) + 1 for k, c in enumerate(jobs)]
    G.budget_sweep(C, hip_ctx, host, tuple(packed), words)
