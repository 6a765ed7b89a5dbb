"""Spectra on the device: pw_dft_sums on gfx950 against the host path (device = -1), BIT FOR BIT -- the sums are
defined by the source (exact integer phases, fixed chunks, explicit FMAs in time order, chunks rotated and added in
order, csrc/pw_dft.hpp), not by the launch nor by how the frequencies are cut into slabs to bound the workspace.
numpy only; tests/test_dft.py holds the host path to the definition, mpmath, a long-double sum, the FFT and SciPy."""
import numpy as np
import pytest

import _dft_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_accuracy_cases_device_equals_host(hip_ctx, host):
    jobs = [c[1:] for c in C.accuracy_cases()]
    for job in jobs:                                           # one at a time ...
        packed = C.pack([job])
        got = hip_ctx.dft_sums(*packed)
        assert same_bits(got, host.dft_sums(*packed)) and np.abs(got).max() > 0.0
    packed = C.pack(jobs)                                      # ... and as one batch
    got = hip_ctx.dft_sums(*packed)
    assert same_bits(got, host.dft_sums(*packed))
    assert same_bits(got, hip_ctx.dft_sums(*packed))           # two consecutive device calls


def test_the_edge_grid(hip_ctx, host):
    """n around the chunk x n_freq around the tile of 128 (and the 64 lanes of a wavefront)."""
    rng = np.random.default_rng(5)
    jobs = []
    for n in (1, 2, 511, 512, 513, 1025, 1537):
        a = rng.standard_normal(n)
        for nf in (1, 63, 64, 65, 129, 257):
            jobs.append((a, 4 * max(n, 65) + 1, 1, 1, nf))
    packed = C.pack(jobs)
    got = hip_ctx.dft_sums(*packed)
    assert same_bits(got, host.dft_sums(*packed)) and len(got) == 7 * (1 + 63 + 64 + 65 + 129 + 257)
    for job in jobs:
        alone = C.pack([job])
        assert same_bits(hip_ctx.dft_sums(*alone), host.dft_sums(*alone)), (len(job[0]), job[4])


def test_steps_of_two_and_the_largest_period(hip_ctx, host):
    rng = np.random.default_rng(6)
    a = rng.standard_normal(5000)
    big = 1 << 31
    jobs = [(a, 20_001, 2, 2, 5000), (a, 20_000, 1, 2, 300), (a, big, big - 700, 1, 700), (a, big, big - 1399, 2, 700),
            (a, big - 1, big - 2 - 3 * 200, 3, 201)]
    jobs += C.edge_jobs()
    packed = C.pack(jobs)
    got = hip_ctx.dft_sums(*packed)
    assert same_bits(got, host.dft_sums(*packed)) and np.abs(got).max() > 0.0


def test_mixed_batch_of_64_jobs(hip_ctx, host):
    packed = C.pack(C.mixed_batch())
    got = hip_ctx.dft_sums(*packed)
    assert same_bits(got, host.dft_sums(*packed))
    assert same_bits(got, hip_ctx.dft_sums(*packed))
    for budget in (1, 100_000, 1 << 30):
        assert same_bits(got, C.internal_sums(hip_ctx, *packed, workspace_bytes=budget)[:len(got)]), budget
    for job in C.mixed_batch():
        if len(job[0]) and job[4]:
            alone = C.pack([job])
            assert same_bits(hip_ctx.dft_sums(*alone), host.dft_sums(*alone))


def test_one_long_job_and_the_workspace_bound(hip_ctx, host):
    """200 000 entries x 4096 frequencies: 8.2e8 terms.  Twiddles and partial sums are 4096 x (8192 + 16 x 391) B = 59 MB;
    with the budget forced to 1 B (one tile a launch), 100 kB and 1 MiB the frequencies go through in slabs, and the
    bits are the same."""
    n, nf = 200_000, 4096
    packed = C.pack([(C.centred(C.ar1(n, 0.999, 9)), 4 * n, 1, 1, nf)])
    want = host.dft_sums(*packed)
    got = hip_ctx.dft_sums(*packed)
    assert same_bits(got, want) and np.abs(got).min() > 0.0
    for budget in (1, 100_000, 1 << 20):
        assert same_bits(got, C.internal_sums(hip_ctx, *packed, workspace_bytes=budget)), budget


def test_the_twiddle_hook_device_equals_host(hip_ctx, host):
    for j, period, k in C.twiddle_cases():
        dev, ref = C.twiddles(hip_ctx, j, period, k), C.twiddles(host, j, period, k)
        assert same_bits(dev[0], ref[0]) and same_bits(dev[1], ref[1]), (j, period)


def test_bad_arguments_never_launch(hip_ctx):
    x = np.arange(3.0)
    for bad, what in (((np.array([1.0, np.nan, 2.0]), 12, 1, 1, 2), "NaN"), ((x, 1, 0, 1, 1), "period"),
                      ((x, 12, 0, 0, 2), "j_step"), ((x, 12, 10, 1, 3), "n_freq - 1")):
        with pytest.raises(ValueError, match="job 1: .*" + what):
            hip_ctx.dft_sums(*C.pack([(np.arange(5.0), 20, 1, 1, 3), bad]))


def test_the_public_route_per_molecule(hip_ctx):
    from pywindow_amd import records
    from test_kde import golden_store

    g = golden_store().records
    recs = np.concatenate([g, g[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    store = records.RecordStore(recs[by], pos[by], np.tile([0, 1], 20))
    for quantity in ("pore_diameter_opt", "maximum_diameter", "windows_mean"):
        dev = store.spectrum(quantity, per_molecule=True, device=0)
        ref = store.spectrum(quantity, per_molecule=True, device=-1)
        assert sorted(dev) == sorted(ref) == [0, 1]
        for m in (0, 1):
            for f in ("frequency", "j", "power", "amplitude", "sums"):
                assert same_bits(getattr(dev[m], f), getattr(ref[m], f)), (quantity, m, f)
            assert (dev[m].period, dev[m].n_valid, dev[m].mean, dev[m].peak_frequency, dev[m].peak_power) == \
                   (ref[m].period, ref[m].n_valid, ref[m].mean, ref[m].peak_frequency, ref[m].peak_power)
        assert np.abs(dev[0].sums).max() > 0.0
