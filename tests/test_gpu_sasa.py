"""The accessible surface of a cage on the device: pw_sasa on gfx950 against the host path (device = -1) and against the
definition (tests/_sasa_cases.py: reference, no culling), EXACTLY -- every output is an integer, so neither the launch
geometry, the list of near atoms or its overflow path, where the grid's words are read from, how many workgroups a job
takes nor what the device memory held before may show.  numpy only; tests/test_sasa.py holds the host path to the
definition."""
import numpy as np
import pytest

import _sasa_cases as C
import _stat_edges as S

pytestmark = pytest.mark.gpu

# the kernel's alternative paths, one at a time and together: a list of 1 and of 3 entries and none at all (overflow),
# every grid read from global memory and grids of up to 64 x 64 rows staged in LDS, 5 and 64 atoms a workgroup
HOOKS = (dict(list_capacity=1), dict(list_capacity=3), dict(list_capacity=-1), dict(lds_words=-1), dict(lds_words=4096),
         dict(lds_words=40), dict(block_atoms=5), dict(block_atoms=64),
         dict(list_capacity=3, lds_words=-1, block_atoms=5), dict(list_capacity=-1, lds_words=4096, block_atoms=1))


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def test_the_case_list(hip_ctx, host):
    """Device == host path == definition, job by job and as batches with holes, and two consecutive device calls agree."""
    for c in C.cases():
        packed = C.pack([c])
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
    for jobs in C.by_directions(C.cases()):
        packed = C.pack(jobs, hole=3)
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected(jobs, hole=3)
        assert rc == 0 and C.same(got, want), (jobs[0].name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
        rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
        assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


def test_5000_atoms_have_no_capacity(hip_ctx, host):
    """More near atoms than a wave's list holds for some atoms and fewer for others, ten workgroups for the job."""
    c = C.big_case()
    reach = c.radii
    d = np.sqrt(((c.xyz[:200, None, :] - c.xyz[None, :, :]) ** 2).sum(axis=2))
    near = (d < reach[:200, None] + reach[None, :]).sum(axis=1) - 1
    assert near.max() > 128 > near.min() and len(c.xyz) == 5000 and len(c.directions) == 64
    packed = C.pack([c])
    want = C.expected([c])
    rc, got = C.raw(hip_ctx, packed)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert C.same(got, C.raw(host, packed)[1])
    for hook in (dict(list_capacity=-1), dict(block_atoms=5000), dict(list_capacity=40, block_atoms=77)):
        rc, got = C.raw(hip_ctx, packed, hook=hook)
        assert rc == 0 and C.same(got, want), (hook, C.first_difference(got, want))


@pytest.mark.parametrize("hook", HOOKS, ids=lambda h: "-".join(f"{k}={v}" for k, v in h.items()))
def test_no_path_shows_in_the_result(hip_ctx, hook):
    """Through pw_internal_sasa with every alternative path forced, one at a time and together; the device result
    filled with 0xFF before the kernel or not; right after a call of other shapes and values: the same integers, and
    entries nobody owns untouched."""
    for jobs in C.by_directions(C.cases()):
        packed = C.pack(jobs, hole=1)
        want = C.expected(jobs, hole=1)
        for poison in (False, True):
            assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
            S.set_poison(poison)
            rc, got = C.raw(hip_ctx, packed, hook=hook)
            S.set_poison(False)
            assert rc == 0 and C.same(got, want), (hook, poison, jobs[0].name, C.first_difference(got, want))


def test_the_default_paths_with_poison_and_the_timed_entry(hip_ctx):
    for jobs in C.by_directions(C.cases()):
        packed = C.pack(jobs, hole=1)
        S.set_poison(True)
        rc, got, ms = C.raw(hip_ctx, packed, timed=True)
        S.set_poison(False)
        assert rc == 0 and C.same(got, C.expected(jobs, hole=1)) and ms > 0.0


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, null, what in C.bad_batches():
        for hook in (None, dict(list_capacity=1, lds_words=-1, block_atoms=2)):
            rc, got = C.raw(hip_ctx, packed, hook=hook, sizes=sizes, null=null)
            assert rc == -2 and C.same(got, C.blank(packed[6], packed[5])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_sasa: job 1: ") and what in message, (what, message)
    packed = next(b for b in C.bad_batches() if b[3] == "a coordinate is not finite")[0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        hip_ctx.sasa(packed[0], packed[1], packed[2], packed[3], packed[4])


def test_the_public_layer_on_jittered_cc3_frames(hip_ctx):
    """pw.surface_area_batch on 20 jittered CC3 frames with their cavities from pw.cavity_grid_batch(mask=True), each
    seeded at its optimised pore centre and closed at planes through its own windows: device against host."""
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
    cav = pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], probe=0.0, spacing=0.5, half_widths=recs["maxd"] / 2.0,
                               planes=planes, mask=True, device=0)
    dev = pw.surface_area_batch(frames, radii, cavity=cav, device=0)
    ref = pw.surface_area_batch(frames, radii, cavity=cav, device=-1)
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.exposed.tobytes() == ref.exposed.tobytes()
    assert dev.inside.tobytes() == ref.inside.tobytes() and dev.exposed.shape == (20, len(base))
    assert np.array_equal(dev.area, ref.area) and np.array_equal(dev.internal_area, ref.internal_area)
    assert dev.closed.all() and (0 < dev.internal_area).all() and (dev.internal_area < dev.area).all()
    assert len(set(dev.internal_area.tolist())) > 5 and (dev.raw["flags"] == 1).all()
    assert np.array_equal(dev.series("internal_area")[1], cav.closed)


def test_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """A call whose jobs have unused atoms, radii and words before the first of them and between them -- every first is
    positive and every uploaded span starts past 0 (tests/_grid_sweep.py) -- and own their outputs from the back to the
    front: the host context's integers, on the default path and with the alternative paths forced, under poison."""
    import _grid_sweep as G

    jobs = next(g for g in C.by_directions(C.cases()) if sum(bool(c.dims) for c in g) > 1 and sum(not c.dims for c in g) > 1)
    u = jobs[0].directions
    pads = [C.Case(f"pad-{k}", *C.random_atoms(2, 3.0, 80 + k), u, dims=(3, 2, 2), h=0.5, words=np.full(4, 5, dtype=np.uint64))
            for k in range(len(jobs))]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    atoms, grid = rec["n"] > 0, rec["word_first"] >= 0
    assert atoms.sum() > 2 and grid.sum() > 1 and (~grid).sum() > 1
    assert (rec["atom_first"][atoms] > 0).all() and (rec["radius_first"][atoms] > 0).all() and (rec["word_first"][grid] > 0).all()
    assert (np.diff(rec["out"]) < 0).all() and (np.diff(rec["count_first"][atoms]) < 0).all()
    rc, want = C.raw(host, tuple(packed))
    assert rc == 0
    S.set_poison(True)
    for hook in (None, dict(list_capacity=-1, lds_words=-1, block_atoms=2), dict(lds_words=4096)):
        rc, got = C.raw(hip_ctx, tuple(packed), hook=hook)
        assert rc == 0 and C.same(got, want), (hook, C.first_difference(got, want))
