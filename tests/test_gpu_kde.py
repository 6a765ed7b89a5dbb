"""Trajectory distributions on the device: pw_kde_sums and pw_exp on gfx950 against the host path
(device = -1), BIT FOR BIT -- the sums are defined by the source (fixed chunks, fixed order of additions,
csrc/pw_kde.hpp), not by the launch.  numpy only; tests/test_kde.py holds the host path to SciPy and to a
long-double sum."""
import time

import numpy as np
import pytest

import _kde_cases as K
from _util import GOLDEN, check_records, load_group

pytestmark = pytest.mark.gpu

#: seconds the host path (16 threads) may take for the 4e6 x 1000 job: it measured 0.54 s on the MI355X machine's
#: host, which is 8.6 s of one core; 30 s says "something is wrong", not "a busy machine"
HOST_BIG_LIMIT_S = 30.0


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_pw_exp_device_equals_host_bit_for_bit(hip_ctx, host):
    x = K.exp_arguments()
    assert len(x) >= 1_000_000
    assert same_bits(K.internal_exp(hip_ctx, x), K.internal_exp(host, x))


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
def test_scipy_cases_device_equals_host(hip_ctx, host, bw):
    from pywindow_amd import distributions

    jobs = []
    for _, x, g in K.scipy_cases():
        h, _ = distributions.bandwidth(x, bw)
        jobs.append((x, g, 1.0 / h))
    for job in jobs:                                           # one at a time ...
        packed = K.pack([job])
        assert same_bits(hip_ctx.kde_sums(*packed), host.kde_sums(*packed))
    packed = K.pack(jobs)                                      # ... and as one batch
    both = hip_ctx.kde_sums(*packed)
    assert same_bits(both, host.kde_sums(*packed))
    # the public route
    for _, x, g in K.scipy_cases()[:3]:
        a = distributions.gaussian_kde_1d(x, g, bw, device=0)
        b = distributions.gaussian_kde_1d(x, g, bw, device=-1)
        assert same_bits(a.density, b.density) and a.bandwidth == b.bandwidth


def test_batch_of_64_small_jobs(hip_ctx, host):
    packed = K.pack(K.mixed_batch())
    got = hip_ctx.kde_sums(*packed)
    assert same_bits(got, host.kde_sums(*packed))
    assert same_bits(got, hip_ctx.kde_sums(*packed))           # two consecutive device calls
    rec = packed[0]
    for j in rec[rec["n_samples"] == 0]:
        assert (got[int(j["point_first"]):int(j["point_first"] + j["n_points"])] == 0.0).all()


def test_four_million_samples(hip_ctx, host):
    rng = np.random.default_rng(4)
    x = np.where(rng.random(4_000_000) < 0.3, rng.normal(3.4, 0.2, 4_000_000), rng.normal(3.9, 0.15, 4_000_000))
    g = K.example_grid(x, 1000)
    packed = K.pack([(x, g, 1.0 / (x.std(ddof=1) * len(x) ** -0.2))])
    t0 = time.perf_counter()
    want = host.kde_sums(*packed)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = hip_ctx.kde_sums(*packed)
    dev_s = time.perf_counter() - t0
    print(f"4e6 x 1000: host path (16 threads) {host_s:.2f} s, device call {dev_s * 1e3:.1f} ms")
    assert same_bits(got, want)
    assert same_bits(got, hip_ctx.kde_sums(*packed))
    assert host_s <= HOST_BIG_LIMIT_S


def test_bad_arguments_never_launch(hip_ctx):
    x, g = np.array([1.0, 2.0, 3.0]), np.linspace(0.0, 4.0, 9)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            hip_ctx.kde_sums(*K.pack([(x, g, r)]))
    with pytest.raises(ValueError, match="NaN"):
        hip_ctx.kde_sums(*K.pack([(np.array([1.0, np.nan]), g, 1.0)]))


def test_call_while_an_analysis_is_in_flight(hip_ctx, host):
    """A resident analysis of 1000 units is launched (asynchronous) and the KDE call goes onto the same context
    before anything waits for it: same sums as on a quiet context, and the analysis' records are still the
    goldens'."""
    from pywindow_amd import _lib, synth
    from pywindow_amd import element_data as E

    elements, frames = synth.synthetic_units(1000)
    ids = E.element_ids(elements)
    res = hip_ctx.upload(_lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids]))
    x = K.synthetic("bimodal", 400000)
    packed = K.pack([(x, K.example_grid(x, 1000), 1.0 / 0.03)] + K.mixed_batch()[:8])
    quiet = hip_ctx.kde_sums(*packed)
    res.launch()
    busy = hip_ctx.kde_sums(*packed)
    recs = res.download()
    res.free()
    assert same_bits(busy, quiet) and same_bits(busy, host.kde_sums(*packed))
    check_records(recs[:64], load_group("synth64"), where="analysis around a KDE call")


def test_trajectory_distribution_end_to_end(hip_ctx, tmp_path):
    from pywindow_amd.trajectory import DLPOLY

    g = np.load(GOLDEN / "history20.npz")
    path = tmp_path / "HISTORY_singlemol_short"
    path.write_bytes(g["file_bytes"].tobytes())
    traj = DLPOLY(path)
    traj.analysis(swap_atoms={"he": "H"}, forcefield="opls")
    for quantity in ("windows", "pore_diameter_opt", "maximum_diameter"):
        dev = traj.distribution(quantity)
        ref = traj.analysis_store.distribution(quantity, device=-1)
        assert dev.n == ref.n and dev.bandwidth == ref.bandwidth and same_bits(dev.x, ref.x)
        assert same_bits(dev.density, ref.density)
    assert same_bits(traj.analysis_store.samples("windows"), K.golden_cc3()["windows"])
