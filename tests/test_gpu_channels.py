"""The pore network of a periodic cell on the device: pw_channels on gfx950 against the host path (device = -1) and
against the definition (tests/_channels_cases.py: reference), EXACTLY -- every output is an integer and every fill is a
least fixed point, so neither the launch geometry, the order in which rows are swept, which fills were run and which
inferred, how the jobs are gathered into launches nor what the workspace held before may show.  numpy only;
tests/test_channels.py holds the host path to the definition."""
import numpy as np
import pytest

import _channels_cases as C
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
    for c in C.cases() + C.big_cases():
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
    """Through pw_internal_channels with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact results filled with 0xFF before the first kernel or not; right after a call of other
    shapes and values: the same integers, and entries nobody owns untouched.  (The cases ask for masks and labels, for
    one of them and for neither.)"""
    jobs = C.cases()
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, hole=1)
    for poison in (False, True):
        assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, C.first_difference(got, want))


def test_a_batch_of_mixed_grids_with_the_largest(hip_ctx, host):
    jobs = C.mixed_batch()
    assert (64, 64, 64) in [c.dims for c in jobs] and len({c.dims for c in jobs}) > 8
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
            assert rc == -2 and C.same(got, C.blank(*packed[3:7])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_channels: job 1: ") and what in message, (what, message)
    packed = C.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        hip_ctx.channels(packed[0], packed[1], packed[2])


def test_the_public_layer_on_the_cc3_cell(hip_ctx):
    """pw.channel_network on the CC3 cell of tests/golden/rebuild.npz on a ladder of probes, with masks and labels:
    device against host."""
    import pywindow_amd as pw

    elements, xyz, lattice = C.crystal("cc3_cell")
    kw = dict(probe=[1.2, 1.6, 1.82], spacing=0.5, c_max=128, mask=True, labels=True)
    dev = pw.channel_network(xyz, elements, lattice, device=0, **kw)
    ref = pw.channel_network(xyz, elements, lattice, device=-1, **kw)
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.components.tobytes() == ref.components.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(dev.accessible_words, ref.accessible_words))
    assert all(np.array_equal(a, b) for a, b in zip(dev.labels, ref.labels))
    assert dev.dimensionality.tolist() == [3, 0, 0] and dev.n_open.tolist() == [5928, 2032, 884]
    assert dev.n_components.tolist() == [41, 76, 104] and dev.limiting_probe == 1.2


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms -- the first with ready-made open words, the second without a
    mask, the third without labels -- at every budget of a launch from one word to all their words and eight more
    (tests/_grid_sweep.py): every place where the planner can close a launch group.  Nothing of the inputs starts at 0
    and the outputs go to the jobs from the back to the front."""
    import _grid_sweep as G

    rng = np.random.default_rng(70)
    step = (1.0, 0.25, 1.0, 0.0, -0.25, 1.0)
    jobs = [C.Case(f"sweep-{k}", d, *C.random_atoms(n, d, 70 + k, step, radius=(0.2, 0.6)), probe=0.1 * k, step=step, c_max=3 - k,
                   mask=k != 1, labels=k != 2,
                   words=rng.integers(0, 1 << d[0], d[1] * d[2], dtype=np.uint64) if k == 0 else None)
            for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), *C.random_atoms(2, (2, 2, 2), 80 + k, step), step=step, c_max=2,
                   words=np.full(4, 3, dtype=np.uint64)) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    open_first = packed[8] = np.ascontiguousarray(packed[8][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["radius_first"][1:] > 0).all()
    assert open_first[0] > 0 and (open_first[1:] == -1).all() and rec["mask_first"][1] == -1 and rec["label_first"][2] == -1
    assert (np.diff(rec["out"]) < 0).all() and (np.diff(rec["comp_first"]) < 0).all() and rec["mask_first"][0] > rec["mask_first"][2] > 0
    words = [c.dims[1] * c.dims[2] * (int(c.words is not None) + int(c.mask)) +
             (c.dims[0] * c.dims[1] * c.dims[2] + 7) // 8 * int(c.labels) + 1 for c in jobs]
    G.budget_sweep(C, hip_ctx, host, tuple(packed), words)
