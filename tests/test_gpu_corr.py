"""Time correlation on the device: pw_corr_sums on gfx950 against the host path (device = -1), BIT FOR BIT -- the
sums are defined by the source (fixed chunks, explicit FMAs in time order, chunks added in order, csrc/pw_corr.hpp),
not by the launch nor by how the lags are cut into slabs to bound the workspace.  numpy only; tests/test_corr.py
holds the host path to a long-double sum, to numpy and to the definition."""
import time

import numpy as np
import pytest

import _corr_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_accuracy_cases_device_equals_host(hip_ctx, host):
    jobs = [(a, None if b is a else b, lags) for _, a, b, lags in C.accuracy_cases()]
    for job in jobs:                                           # one at a time ...
        packed = C.pack([job])
        got = hip_ctx.corr_sums(*packed)
        assert same_bits(got, host.corr_sums(*packed)) and np.abs(got).max() > 0.0
    packed = C.pack(jobs)                                      # ... and as one batch
    got = hip_ctx.corr_sums(*packed)
    assert same_bits(got, host.corr_sums(*packed))
    assert same_bits(got, hip_ctx.corr_sums(*packed))          # two consecutive device calls


def test_mixed_batch_of_64_jobs(hip_ctx, host):
    packed = C.pack(C.mixed_batch())
    got = hip_ctx.corr_sums(*packed)
    assert same_bits(got, host.corr_sums(*packed))
    assert same_bits(got, hip_ctx.corr_sums(*packed))
    for budget in (1, 100_000, 1 << 30):
        assert same_bits(got, C.internal_sums(hip_ctx, *packed, workspace_bytes=budget)), budget
    for job in C.mixed_batch():
        alone = C.pack([job])
        assert same_bits(hip_ctx.corr_sums(*alone), host.corr_sums(*alone))


def test_one_long_job_and_the_workspace_bound(hip_ctx, host):
    """1 000 000 entries x 32 768 lags: 3.2e10 terms.  The job's [chunks][lags] partial sums would be 1954 x 32 768 x 8 B
    = 512 MB, above the default budget of the workspace, so the default call already goes through in slabs of lags;
    with the budget forced to 1 MiB and to 1 GiB (one launch pair) the bits are the same."""
    n, lags = 1_000_000, 32_768
    assert -(-n // C.source_constant("CORR_CHUNK")) * lags * 8 > 64 << 20
    packed = C.pack([(C.centred(C.ar1(n, 0.999, 9)), None, lags)])
    t0 = time.perf_counter()
    want = host.corr_sums(*packed)
    host_s = time.perf_counter() - t0
    hip_ctx.corr_sums(*C.pack([(np.arange(8.0), None, 4)]))    # (first use of the kernels)
    t0 = time.perf_counter()
    got = hip_ctx.corr_sums(*packed)
    dev_s = time.perf_counter() - t0
    print(f"1 000 000 x 32 768 lags: host path (16 threads) {host_s:.2f} s, device call {dev_s * 1e3:.1f} ms")
    assert same_bits(got, want) and got[0] > 0.0
    assert same_bits(got, C.internal_sums(hip_ctx, *packed, workspace_bytes=1 << 20))
    assert same_bits(got, C.internal_sums(hip_ctx, *packed, workspace_bytes=1 << 30))


def test_512_jobs_of_10000_x_5000(hip_ctx, host):
    rng = np.random.default_rng(512)
    jobs = [(C.centred(C.ar1(10_000, 0.9 + 0.0001 * k, k)), None if k % 2 else rng.standard_normal(10_000), 5000) for k in range(512)]
    packed = C.pack(jobs)
    t0 = time.perf_counter()
    want = host.corr_sums(*packed)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = hip_ctx.corr_sums(*packed)
    dev_s = time.perf_counter() - t0
    print(f"512 x 10 000 x 5000 lags: host path (16 threads) {host_s:.2f} s, device call {dev_s * 1e3:.1f} ms")
    assert got.shape == (512 * 5000,) and same_bits(got, want)


def test_bad_arguments_never_launch(hip_ctx):
    for bad, what in (((np.array([1.0, np.nan, 2.0]), None, 2), "NaN"), ((np.arange(3.0), None, 4), "n_lags > n"),
                      ((np.arange(3.0), None, 0), "n_lags < 1")):
        with pytest.raises(ValueError, match="job 1: .*" + what):
            hip_ctx.corr_sums(*C.pack([(np.arange(5.0), None, 3), bad]))


def test_the_public_route_per_molecule(hip_ctx):
    from pywindow_amd import records
    from test_kde import golden_store

    g = golden_store().records
    recs = np.concatenate([g, g[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    store = records.RecordStore(recs[by], pos[by], np.tile([0, 1], 20))
    for quantity, other in (("pore_diameter_opt", "windows_min"), ("maximum_diameter", None), ("windows_mean", "windows_max")):
        dev = store.correlation(quantity, other, per_molecule=True, device=0)
        ref = store.correlation(quantity, other, per_molecule=True, device=-1)
        assert sorted(dev) == sorted(ref) == [0, 1]
        for m in (0, 1):
            for f in ("lag", "sums", "pairs", "covariance", "correlation"):
                assert same_bits(getattr(dev[m], f), getattr(ref[m], f)), (quantity, m, f)
            assert (dev[m].mean_a, dev[m].mean_b, dev[m].n, dev[m].time, dev[m].n_effective) == \
                   (ref[m].mean_a, ref[m].mean_b, ref[m].n, ref[m].time, ref[m].n_effective)
        assert np.abs(dev[0].sums).max() > 0.0
