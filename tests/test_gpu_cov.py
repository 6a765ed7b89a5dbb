"""pw_covariance and pw_project on the device: gfx950 against the host path (device = -1) on the RAW BYTES -- the
result is defined to the bit (pywindow_amd/csrc/pw_cov.hpp), so neither the tiles, the lane squares, the fold across
the lanes, the launch geometry nor how a job's tiles and chunks are cut into launches to bound the workspace may show --
and against the long-double truth within the bar of tests/test_cov.py.  numpy only."""
import numpy as np
import pytest

import _cov_cases as C
import _stat_edges as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(scope="module")
def wanted(host):
    """The host path's (mean, scatter | None) of every case, job by job."""
    return {name: C.one(host, name) for name, *_ in C.cases()}


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def equal(got, want) -> bool:
    return C.same(got[0], want[0]) and ((got[1] is None and want[1] is None) or C.same(got[1], want[1]))


def test_the_case_list_job_by_job(hip_ctx, wanted):
    for name, X, tr, scatter in C.cases():
        got = C.one(hip_ctx, name)
        assert equal(got, wanted[name]), name
        r = C.reference(name)
        if scatter:
            C.held(got[1], r["scatter"], r["scatter_t"], r["scatter_abs"], name)
        C.held(got[0], r["mean"], r["mean_t"], np.abs(C.moved(X, tr)).max(axis=0), name)


def test_the_case_list_as_one_batch(hip_ctx, wanted):
    items = [(X, tr, scatter) for _, X, tr, scatter in C.cases()]
    got, mean, scatter, spans = C.run(hip_ctx, items, hole=5)
    for (name, *_), g in zip(C.cases(), got):
        assert equal(g, wanted[name]), name
    assert C.untouched(mean)[~C.owned(len(mean), [sp[0] for sp in spans])].all()
    assert C.untouched(scatter)[~C.owned(len(scatter), [sp[1] for sp in spans])].all()


@pytest.mark.parametrize("count", C.BATCHES)
def test_batches_of_small_jobs_with_holes(hip_ctx, host, count):
    items = C.small_items(count)
    want = C.run(host, items, hole=3)
    got = C.run(hip_ctx, items, hole=3)
    assert C.same(got[1], want[1]) and C.same(got[2], want[2])


def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, wanted):
    """Through pw_internal_covariance at workspaces of 1 B (every tile and chunk a launch of its own), 100 kB and the
    default, with the workspace and the device results filled with 0xFF before the first kernel, right after a call of
    another shape: the same bytes."""
    names = ("T=513 D=257", "T=513 D=258 moved", "T=257 D=129 moved", "T=2 D=3", "the mean only, moved T=257 D=129")
    for budget in (1, 100_000, 0):
        for poison in (False, True):
            C.one(hip_ctx, "T=255 D=129")
            S.set_poison(poison)
            got = {name: C.one(hip_ctx, name, workspace_bytes=budget) for name in names}
            S.set_poison(False)
            for name in names:
                assert equal(got[name], wanted[name]), (name, budget, poison)


@pytest.mark.parametrize("k", [1, 2, 65])
def test_projections(hip_ctx, host, wanted, k):
    parts = []
    for name in ("T=257 D=129", "T=257 D=129 moved", "T=2 D=3 moved", "T=513 D=257", "T=513 D=258 moved"):
        _, X, tr, _ = C.case(name)
        parts.append((X, tr, wanted[name][0], C.vectors(name, k)))
    want = [C.project(host, *p) for p in parts]
    for poison in (False, True):
        S.set_poison(poison)
        got = [C.project(hip_ctx, *p) for p in parts]
        batch, proj, spans = C.project_batch(hip_ctx, parts, hole=4)
        S.set_poison(False)
        for w, g, b in zip(want, got, batch):
            assert C.same(g, w) and C.same(b, w)
        assert C.untouched(proj)[~C.owned(len(proj), spans)].all()
    name = "T=513 D=257"
    ref, truth, scale = C.projection_reference(name, parts[3][3], parts[3][2])
    C.held(got[3], ref, truth, scale, f"{name} k={k}")


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    x = np.arange(24.0)
    x[20] = np.inf
    rec = np.array([(0, 4, 3, -1, 0, 0), (12, 4, 3, -1, 3, 9)], dtype=np.int64).view(_lib.COV_JOB_DTYPE).reshape(-1)
    mean, scatter = C.sentinel(6), C.sentinel(18)
    with pytest.raises(ValueError, match="job 1: a value of the matrix is not finite"):
        hip_ctx.covariance(rec, x, None, mean=mean, scatter=scatter)
    assert C.untouched(mean).all() and C.untouched(scatter).all()


def test_principal_modes_of_65_frames_of_65_atoms(hip_ctx):
    """The mean structure, the scatter matrix and the projections of the device equal the host path's bytes.  The
    eigenvectors are handed over, not recomputed, so LAPACK has no part in the comparison."""
    import pywindow_amd as pw

    rng = np.random.default_rng(65)
    base = 5.0 * rng.standard_normal((65, 3))
    coords = np.array([(base + 0.1 * rng.standard_normal(base.shape)) @ C.random_rotation(rng).T + rng.uniform(-2, 2, 3)
                       for _ in range(65)])
    mass = rng.choice([1.008, 12.011, 14.007, 15.999], 65)
    for w, reference in ((None, "mean"), (mass, "mean"), (mass, 7)):
        ref = pw.principal_modes(coords, w, reference, n_modes=10, device=-1)
        dev = pw.principal_modes(coords, w, reference, vectors=ref.vectors, device=0)
        assert dev.rounds == ref.rounds and C.same(dev.transforms.view(np.uint8), ref.transforms.view(np.uint8))
        assert C.same(dev.mean_structure, ref.mean_structure) and C.same(dev.scatter, ref.scatter)
        assert C.same(dev.projection, ref.projection) and dev.projection.shape == (65, 10)
        assert C.same(dev.rmsf, ref.rmsf) and C.same(dev.cross_correlation, ref.cross_correlation)
