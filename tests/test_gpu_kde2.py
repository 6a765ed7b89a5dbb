"""Joint distributions on the device: pw_kde2_sums on gfx950 against the host path (device = -1), BIT FOR BIT
-- the sums are defined by the source (fixed chunks, fixed order of additions, csrc/pw_kde.hpp), not by the
launch nor by how the mesh is cut into slabs to bound the workspace.  numpy only; tests/test_kde2.py holds the
host path to SciPy and to a long-double sum."""
import time

import numpy as np
import pytest

import _kde2_cases as K2
import _kde_cases as K
from _util import GOLDEN, check_records, load_group

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def mesh_job(n, rho, seed, nx, ny, bw="scott"):
    from pywindow_amd import distributions

    x, y = K2.correlated(n, rho, seed)
    w, _ = K2.whitening(distributions.bandwidth_2d(np.vstack([x, y]), bw)[0])
    return np.stack([x, y], axis=1), K2.mesh_points(K2.axis(x, nx, 1.0), K2.axis(y, ny, 1.0)), w


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
def test_scipy_cases_device_equals_host(hip_ctx, host, bw):
    from pywindow_amd import distributions

    jobs = []
    for _, x, y, ax, ay in K2.scipy_cases():
        w, _ = K2.whitening(distributions.bandwidth_2d(np.vstack([x, y]), bw)[0])
        jobs.append((np.stack([x, y], axis=1), K2.mesh_points(ax, ay), w))
    for job in jobs:                                           # one at a time ...
        packed = K2.pack([job])
        got = hip_ctx.kde2_sums(*packed)
        assert same_bits(got, host.kde2_sums(*packed)) and got.max() > 0.0
    packed = K2.pack(jobs)                                     # ... and as one batch
    assert same_bits(hip_ctx.kde2_sums(*packed), host.kde2_sums(*packed))
    # the public route
    for _, x, y, ax, ay in K2.scipy_cases()[:3]:
        a = distributions.gaussian_kde_2d(x, y, (ax, ay), bw, device=0)
        b = distributions.gaussian_kde_2d(x, y, (ax, ay), bw, device=-1)
        assert same_bits(a.density, b.density) and same_bits(a.covariance, b.covariance)


def test_mixed_batch_of_64_small_jobs(hip_ctx, host):
    packed = K2.pack(K2.mixed_batch())
    got = hip_ctx.kde2_sums(*packed)
    assert same_bits(got, host.kde2_sums(*packed))
    assert same_bits(got, hip_ctx.kde2_sums(*packed))          # two consecutive device calls
    rec = packed[0]
    for j in rec[rec["n_samples"] == 0]:
        assert (got[int(j["point_first"]):int(j["point_first"] + j["n_points"])] == 0.0).all()


def test_64_per_molecule_maps_in_one_call(hip_ctx, host):
    packed = K2.pack([mesh_job(1000, 0.1 * (k % 9), 100 + k, 64, 64) for k in range(64)])
    got = hip_ctx.kde2_sums(*packed)
    assert got.shape == (64 * 4096,) and same_bits(got, host.kde2_sums(*packed))


def test_100000_samples_on_256_x_256_and_the_workspace_bound(hip_ctx, host):
    """6.6e9 terms.  The job's [chunks][m] partial sums would be 196 x 65 536 x 8 B = 103 MB, above the default budget
    of the workspace, so the default call already goes through in slabs; with the budget forced to 1 MiB (103 launch
    pairs) the bits are the same."""
    assert -(-100_000 // K.source_constant("KDE_CHUNK")) * 65536 * 8 > 64 << 20
    packed = K2.pack([mesh_job(100_000, 0.8, 3, 256, 256)])
    t0 = time.perf_counter()
    want = host.kde2_sums(*packed)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = hip_ctx.kde2_sums(*packed)
    dev_s = time.perf_counter() - t0
    print(f"100 000 x 256 x 256: host path (16 threads) {host_s:.2f} s, device call {dev_s * 1e3:.1f} ms")
    assert same_bits(got, want) and got.max() > 1.0
    assert same_bits(got, K2.internal_sums(hip_ctx, *packed, workspace_bytes=1 << 20))
    assert same_bits(got, K2.internal_sums(hip_ctx, *packed, workspace_bytes=1 << 30))     # one launch pair


def test_the_result_does_not_depend_on_the_workspace_budget(hip_ctx, host):
    """A mixed batch with an example-sized map (4000 x 128 x 128) in the middle: the default, a budget of one byte
    (every slab one tile of points, one launch pair each), 100 kB and 3 MB all give the host path's bits."""
    jobs = K2.mixed_batch()
    jobs.insert(30, mesh_job(4000, 0.7, 8, 128, 128))
    packed = K2.pack(jobs)
    want = host.kde2_sums(*packed)
    assert same_bits(hip_ctx.kde2_sums(*packed), want)
    for budget in (1, 100_000, 3_000_000):
        assert same_bits(K2.internal_sums(hip_ctx, *packed, workspace_bytes=budget), want), budget


def test_400000_samples_on_256_x_256(hip_ctx, host):
    """2.6e10 terms (about 50 ms of kernels at the 1-D rates); 1-D-style partials would be 410 MB.  The host path
    takes seconds for all of it, so it recomputes every 16th point as a job of its own -- a point's sum is its own."""
    xy, pts, w = mesh_job(400_000, 0.8, 4, 256, 256)
    t0 = time.perf_counter()
    got = hip_ctx.kde2_sums(*K2.pack([(xy, pts, w)]))
    print(f"400 000 x 256 x 256: device call {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert same_bits(got[::16], host.kde2_sums(*K2.pack([(xy, pts[::16], w)])))
    assert got.max() > 1.0 and (got >= 0.0).all()


def test_bad_arguments_never_launch(hip_ctx):
    xy, pts = np.array([[1.0, 2.0], [2.0, 1.0], [3.0, 5.0]]), K2.mesh_points(np.linspace(0.0, 4.0, 9), np.linspace(0.0, 5.0, 4))
    for w in ((0.0, 0.0, 1.0), (1.0, 0.0, -1.0), (float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0)):
        with pytest.raises(ValueError, match="job 0: factors"):
            hip_ctx.kde2_sums(*K2.pack([(xy, pts, w)]))
    with pytest.raises(ValueError, match="NaN"):
        hip_ctx.kde2_sums(*K2.pack([(np.array([[1.0, np.nan]]), pts, (1.0, 0.0, 1.0))]))
    with pytest.raises(ValueError, match="NaN"):
        hip_ctx.kde2_sums(*K2.pack([(xy, np.array([[np.inf, 0.0]]), (1.0, 0.0, 1.0))]))


def test_call_while_an_analysis_is_in_flight(hip_ctx, host):
    """A resident analysis of 1000 units is launched (asynchronous) and the KDE call goes onto the same context
    before anything waits for it: same sums as on a quiet context, and the analysis' records are still the
    goldens'."""
    from pywindow_amd import _lib, synth
    from pywindow_amd import element_data as E

    elements, frames = synth.synthetic_units(1000)
    ids = E.element_ids(elements)
    res = hip_ctx.upload(_lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids]))
    packed = K2.pack([mesh_job(40_000, 0.5, 12, 128, 128)] + K2.mixed_batch()[:8])
    quiet = hip_ctx.kde2_sums(*packed)
    res.launch()
    busy = hip_ctx.kde2_sums(*packed)
    recs = res.download()
    res.free()
    assert same_bits(busy, quiet) and same_bits(busy, host.kde2_sums(*packed))
    check_records(recs[:64], load_group("synth64"), where="analysis around a 2-D KDE call")


def test_trajectory_joint_distribution_end_to_end(hip_ctx, tmp_path):
    from pywindow_amd.trajectory import DLPOLY

    g = np.load(GOLDEN / "history20.npz")
    path = tmp_path / "HISTORY_singlemol_short"
    path.write_bytes(g["file_bytes"].tobytes())
    traj = DLPOLY(path)
    traj.analysis(swap_atoms={"he": "H"}, forcefield="opls")
    dev = traj.joint_distribution("pore_diameter_opt", "windows")
    ref = traj.analysis_store.joint_distribution("pore_diameter_opt", "windows", device=-1)
    assert dev.density.shape == (128, 128) and dev.n == ref.n == len(K.golden_cc3()["windows"])
    assert same_bits(dev.x, ref.x) and same_bits(dev.y, ref.y) and same_bits(dev.covariance, ref.covariance)
    assert same_bits(dev.density, ref.density) and dev.density.max() > 0.0
