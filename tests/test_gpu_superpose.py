"""Least-squares superposition on the device: pw_superpose on gfx950 against the host path (device = -1) on the RAW
BYTES of the result rows -- the result is defined to the bit (pywindow_amd/csrc/pw_superpose.hpp), so neither the fold
across the lanes, the lane-a-job solve, the launch geometry nor how the jobs are cut into launches to bound the
workspace may show.  numpy only; tests/test_superpose.py holds the host path to the references."""
import numpy as np
import pytest

import _stat_edges as S
import _superpose_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def test_the_case_list_job_by_job(hip_ctx, host):
    for name, x, y, w in C.cases():
        packed = C.pack([(x, y, w)])
        got = hip_ctx.superpose(*packed)
        assert np.array_equal(got.view(np.uint8), host.superpose(*packed).view(np.uint8)), name


@pytest.mark.parametrize("count", C.BATCHES)
def test_batches_with_holes(hip_ctx, host, count):
    """1, 63, 64, 65 and 257 jobs in one call, a row nobody owns in front of every job's row: the host path's bytes,
    the same bytes from a second call, and the rows in between untouched."""
    rec, xyz, wts = C.pack(C.batch(count), hole=1)
    rc, want = C.raw(host, rec, xyz, wts)
    rc_dev, got = C.raw(hip_ctx, rec, xyz, wts)
    assert rc == 0 and rc_dev == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert C.untouched(got)[0::2].all() and not C.untouched(got)[1::2].any()
    assert C.same_bytes(C.raw(hip_ctx, rec, xyz, wts)[1], got)                     # two consecutive device calls


def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host):
    """Through pw_internal_superpose at workspaces of 1 B (every job a launch of its own), 100 kB and the default, with
    the workspace and the compact result filled with 0xFF before the first kernel, right after a call of other shapes
    and values: the same bytes, and rows nobody owns untouched."""
    rec, xyz, wts = C.pack(C.batch(65), hole=2)
    want = C.raw(host, rec, xyz, wts)[1]
    other = C.pack(C.batch(7)[::-1])
    for budget in (1, 100_000, 0):
        for poison in (False, True):
            hip_ctx.superpose(*other)
            S.set_poison(poison)
            rc, got = C.raw(hip_ctx, rec, xyz, wts, workspace_bytes=budget)
            S.set_poison(False)
            assert rc == 0 and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (budget, poison)
            assert C.untouched(got).sum() == 2 * 65


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    x = np.arange(30.0).reshape(10, 3) ** 1.5
    x[7, 1] = np.inf
    rec = np.array([(0, 2, -1, 2, 0), (0, 5, -1, 5, 1)], dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    rc, rows = C.raw(hip_ctx, rec, x, None)
    assert rc == -2 and C.untouched(rows).all() and b"job 1: a coordinate is not finite" in _lib.load().pw_last_error()


def test_rmsd_matrix_of_65_frames(hip_ctx):
    import pywindow_amd as pw

    rng = np.random.default_rng(65)
    base = 5.0 * rng.standard_normal((168, 3))
    coords = np.array([C.moved(base, C.random_rotation(rng), rng.uniform(-2, 2, 3), 0.1, rng) for _ in range(65)])
    mass = rng.choice([1.008, 12.011, 14.007, 15.999], 168)
    for w in (None, mass):
        dev, ref = pw.rmsd_matrix(coords, w, device=0), pw.rmsd_matrix(coords, w, device=-1)
        assert dev.shape == (65, 65) and np.array_equal(dev.view(np.uint64), ref.view(np.uint64))
        assert np.array_equal(dev, dev.T) and not dev.diagonal().any() and dev[0, 1] > 0.05
