"""Guest percolation on the device: pw_percolation on gfx950 against the host path (device = -1) and against the
definition (tests/_percolation_cases.py: reference), EXACTLY -- the field is the defined sum, every level a comparison
of doubles and every count an integer, so neither the launch geometry, the order in which rows are swept, which
evaluations and fills were run and which inferred, how the jobs are gathered into launches nor what the workspace held
before may show.  numpy only; tests/test_percolation.py holds the host path to the definition."""
import numpy as np
import pytest

import _percolation_cases as P
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
    """Device == host path == definition, job by job -- fields and atoms, the 64^3 among them -- and as one batch with
    holes, forwards and with the outputs handed out from the back; two consecutive device calls agree."""
    for c in P.cases() + P.atom_cases() + P.big_cases():
        packed = P.pack([c])
        rc, got = P.raw(hip_ctx, packed)
        want = P.expected([c])
        assert rc == 0 and P.same(got, want), (c.name, P.first_difference(got, want))
        assert P.same(got, P.raw(host, packed)[1]), c.name
    jobs = P.cases() + P.atom_cases()
    for reverse in (False, True):
        packed = P.pack(jobs, hole=3, reverse=reverse)
        rc, got = P.raw(hip_ctx, packed)
        want = P.expected(jobs, hole=3, reverse=reverse)
        assert rc == 0 and P.same(got, want), P.first_difference(got, want)
        assert P.same(got, P.raw(host, packed)[1]) and P.same(got, P.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got[1].tobytes(), dtype=np.uint8).reshape(len(got[1]), -1)
    assert (rows == P.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_percolation with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact results filled with 0xFF before the first kernel or not; right after a call of other
    shapes and values: the same bytes, and entries nobody owns untouched."""
    jobs = P.cases() + P.atom_cases()
    packed = P.pack(jobs, hole=1)
    want = P.expected(jobs, hole=1)
    for poison in (False, True):
        assert P.raw(hip_ctx, P.pack(P.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = P.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and P.same(got, want), (workspace_bytes, poison, P.first_difference(got, want))


def test_a_batch_of_mixed_grids_with_the_largest(hip_ctx, host):
    jobs = P.mixed_batch()
    assert (64, 64, 64) in [c.dims for c in jobs] and len({c.dims for c in jobs}) > 8
    packed = P.pack(jobs, hole=1)
    diagnostics = []
    rc, got = P.raw(hip_ctx, packed, diagnostics=diagnostics)
    want = P.expected(jobs, hole=1)
    assert rc == 0 and P.same(got, want), P.first_difference(got, want)
    assert P.same(got, P.raw(host, packed)[1])
    n_eval, n_fill = diagnostics[0]
    assert (n_eval >= 0).all() and (n_eval <= 6 * 64 + 7).all() and (n_fill >= 0).all()
    rc, again = P.raw(hip_ctx, packed, workspace_bytes=300_000)
    assert rc == 0 and P.same(again, want)


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in P.bad_batches():
        for budget in (None, 1):
            rc, got = P.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and P.same(got, P.blank(*packed[4:7])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_percolation: job 1: ") and what in message, (what, message)
    packed = P.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        hip_ctx.percolation(packed[0], packed[1], packed[2], packed[3])


def test_the_field_of_an_orthorhombic_cell_is_pw_affinitys(hip_ctx):
    """bx = cx = cy = 0 and ax = by = cz = h: the map of the new field kernel equals byte for byte the energies of the
    merged cubic-grid field kernel for the same atoms (pw_affinity with its energy map), both on the device."""
    import pywindow_amd as pw

    for c in [c for c in P.atom_cases() if c.name.startswith("orthorhombic") and len(c.xyz)]:
        _, got = P.raw(hip_ctx, P.pack([c]))
        cubic = pw.guest_affinity(c.xyz, c.coef, None, 300.0, grid=(c.origin, float(c.step[0]), c.dims), energies=True,
                                  core2=c.core2, cutoff2=c.cutoff2, device=0)
        assert np.asarray(cubic.energies).tobytes() == got[2].tobytes(), c.name


def test_against_pw_channels(hip_ctx):
    for name in ("ties-(3, 4, 5)", "normal-(6, 5, 4)", "ties-blocked-(2, 2, 7)", "nx=64", "rows=7x37", "double-helix-tiled-twice"):
        (c,) = [c for c in P.cases() if c.name == name]
        P.check_against_channels(hip_ctx, c.field)


def test_the_public_layer_on_the_cc3_cell(hip_ctx):
    """pw.guest_percolation with Xe on the CC3 cell of tests/golden/rebuild.npz at spacing 1.0 and cutoff 8.0, with the
    map: device against host, bytes."""
    import pywindow_amd as pw

    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="Xe", spacing=1.0, cutoff=8.0, maps=True)
    dev = pw.guest_percolation(xyz, elements, lattice, device=0, **kw)
    ref = pw.guest_percolation(xyz, elements, lattice, device=-1, **kw)
    assert dev.levels.tobytes() == ref.levels.tobytes() and dev.raw.tobytes() == ref.raw.tobytes()
    assert dev.maps.tobytes() == ref.maps.tobytes() and dev.maps.shape == (25, 25, 25)
    assert np.isfinite(dev.barrier).all() and (np.diff(dev.barrier) >= 0).all() and dev.dimensionality_at(dev.barrier[2]) == 3


def test_every_budget_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids -- a field of the caller's, 1 atom without a map and 5 atoms with one -- at every budget
    of a launch from one word to all their words and eight more (tests/_grid_sweep.py): every place where the planner can
    close a launch group.  Nothing of the inputs starts at 0 and the outputs go to the jobs from the back to the front."""
    import _grid_sweep as G

    rng = np.random.default_rng(70)
    step = (1.0, 0.25, 1.0, 0.0, -0.25, 1.0)

    def atoms(n, d, seed):
        xyz, _ = P.CC.random_atoms(n, d, seed, step)
        return dict(dims=d, xyz=xyz, coef=rng.uniform(0.5, 2.0, (n, 2)), core2=0.04, cutoff2=9.0, step=step)

    jobs = [P.Case("sweep-0", rng.integers(-2, 3, G.DIMS[0][::-1]).astype(np.float64), map=True),
            P.Case("sweep-1", **atoms(G.ATOMS[1], G.DIMS[1], 71)),
            P.Case("sweep-2", map=True, **atoms(G.ATOMS[2], G.DIMS[2], 72))]
    pads = [P.Case("pad-0", **atoms(2, (2, 2, 2), 80)), P.Case("pad-1", **atoms(2, (2, 2, 2), 81)),
            P.Case("pad-2", rng.normal(size=(2, 2, 2)), map=True)]
    order, at = G.interleaved(pads, jobs)
    packed = list(P.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert rec["field_first"][0] > 0 and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert (np.diff(rec["out"]) < 0).all() and (np.diff(rec["level_first"]) < 0).all() and rec["map_first"][0] > rec["map_first"][2] > 0
    assert rec["map_first"][1] == -1
    G.budget_sweep(P, hip_ctx, host, tuple(packed), [c.voxels for c in jobs])
