"""Weighted KDE sums under many weight vectors on the device: pw_kde_wsums on gfx950 against the host path
(device = -1), BIT FOR BIT -- the sums are defined by the source (fixed chunks, fused multiply-adds in sample order,
csrc/pw_kde.hpp), not by the launch, the tiles or the slabs.  numpy only; tests/test_kdew.py holds the host path to
the definition, to SciPy and to a long-double sum."""
import time

import numpy as np
import pytest

import _kde_cases as K
import _kdew_cases as W
from _util import GOLDEN, check_records, load_group

pytestmark = pytest.mark.gpu

#: seconds the host path (16 threads) may take for 4000 x 1000 x 200 (8e8 weighted terms, 4e6 exponentials): about
#: 0.2 s of eight threads where this was written; 30 s says "something is wrong", not "a busy machine"
HOST_EXAMPLE_LIMIT_S = 30.0


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_edges_as_one_batch_and_one_job_at_a_time(hip_ctx, host):
    """n around the chunk, m around the point tile, R around the replica tile; weights with exact zeros, integers and
    1e-150 .. 1e150."""
    jobs = W.edge_jobs()
    packed = W.pack(jobs)
    want = host.kde_wsums(*packed)
    got = hip_ctx.kde_wsums(*packed)
    assert same_bits(got, want)
    for k, (mine, theirs) in enumerate(zip(W.unpack(packed[0], got), W.unpack(packed[0], want))):
        x, g, w, _ = jobs[k]
        assert mine.shape == (len(w), len(g)) and same_bits(mine, theirs), k
        if len(x) == 0:
            assert (mine == 0.0).all()
        one = W.pack([jobs[k]])
        assert same_bits(W.unpack(one[0], hip_ctx.kde_wsums(*one))[0], theirs), k


def test_weights_of_one_and_a_replica_alone(hip_ctx, host):
    """(a) weights of one give pw_kde_sums' bits, (b) a replica alone has the bits it has among 70."""
    rng = np.random.default_rng(70)
    x = K.synthetic("bimodal", 4000)[:1300]
    g = K.example_grid(x, 300)
    r = 1.0 / 0.11
    ones = W.pack([(x, g, np.ones((33, len(x))), r)])
    got = W.unpack(ones[0], hip_ctx.kde_wsums(*ones))[0]
    plain = hip_ctx.kde_sums(*K.pack([(x, g, r)]))
    assert same_bits(plain, host.kde_sums(*K.pack([(x, g, r)])))
    for b in (0, 31, 32):
        assert same_bits(got[b], plain), b
    w = W.edge_weights(rng, len(x), 70)
    many = W.pack([(x, g, w, r)])
    together = W.unpack(many[0], hip_ctx.kde_wsums(*many))[0]
    assert same_bits(together, W.unpack(many[0], host.kde_wsums(*many))[0])
    alone = W.pack([(x, g, w[b:b + 1], r) for b in range(70)])
    for b, s in enumerate(W.unpack(alone[0], hip_ctx.kde_wsums(*alone))):
        assert same_bits(s[0], together[b]), b


def test_slabs_do_not_take_part(hip_ctx, host):
    rng = np.random.default_rng(3)
    x = K.synthetic("normal", 4000)[:3000]
    jobs = [(x, K.example_grid(x, 300), W.edge_weights(rng, len(x), 70), 1.0 / 0.09)] + W.edge_jobs()[:6]
    packed = W.pack(jobs)
    want = host.kde_wsums(*packed)
    for budget in (1, 100_000, 1 << 20, 1 << 30):
        assert same_bits(W.internal_wsums(hip_ctx, *packed, workspace_bytes=budget), want), budget
    # two consecutive calls
    assert same_bits(hip_ctx.kde_wsums(*packed), want) and same_bits(hip_ctx.kde_wsums(*packed), want)


def test_bad_arguments_write_nothing(hip_ctx):
    import ctypes

    from pywindow_amd import _lib

    x, g = np.array([1.0, 2.0, 3.0]), np.linspace(0.0, 4.0, 9)
    good = (x, g, np.ones((2, 3)), 1.0)
    bad_weight = np.ones((2, 3))
    bad_weight[1, 1] = -1.0
    nan_weight = np.ones((2, 3))
    nan_weight[0, 2] = np.nan
    for job, what in (((x, g, bad_weight, 1.0), "a weight"), ((x, g, nan_weight, 1.0), "a weight"),
                      ((x, g, np.ones((0, 3)), 1.0), "no replica"), ((x, g, np.ones((2, 3)), 0.0), "bandwidth"),
                      ((x, g, np.ones((2, 3)), float("nan")), "bandwidth")):
        rec, xs, gs, ws = W.pack([good, job])
        with pytest.raises(ValueError, match=f"job 1: {what}"):
            hip_ctx.kde_wsums(rec, xs, gs, ws)
        sums = np.full(4 * len(g), 7.0)
        L = _lib.load()
        rc = L.pw_kde_wsums(hip_ctx._h, rec.ctypes.data, len(rec), xs.ctypes.data, gs.ctypes.data, ws.ctypes.data, sums.ctypes.data)
        assert rc == -2 and (sums == 7.0).all()


def test_the_example_shape(hip_ctx, host):
    """4000 window diameters, 1000 points, 200 bootstrap replicas."""
    from pywindow_amd import distributions

    x = K.synthetic("bimodal", 4000)
    g = K.example_grid(x, 1000)
    w = distributions.block_bootstrap_counts(1000, 30, 200, seed=1)[:, np.arange(4000) // 4].astype(np.float64)
    packed = W.pack([(x, g, w, 1.0 / distributions.bandwidth(x)[0])])
    hip_ctx.kde_wsums(*packed)
    t0 = time.perf_counter()
    got = hip_ctx.kde_wsums(*packed)
    t1 = time.perf_counter()
    want = host.kde_wsums(*packed)
    t2 = time.perf_counter()
    print(f"4000 x 1000 x 200: device call {1e3 * (t1 - t0):.2f} ms, host path (16 threads) {1e3 * (t2 - t1):.1f} ms")
    assert same_bits(got, want)
    assert t2 - t1 <= HOST_EXAMPLE_LIMIT_S


def test_trajectory_band_end_to_end(hip_ctx, tmp_path):
    from pywindow_amd.trajectory import DLPOLY

    g = np.load(GOLDEN / "history20.npz")
    path = tmp_path / "HISTORY_singlemol_short"
    path.write_bytes(g["file_bytes"].tobytes())
    traj = DLPOLY(path)
    traj.analysis(swap_atoms={"he": "H"}, forcefield="opls")
    dev = traj.distribution_band("windows")
    ref = traj.analysis_store.distribution_band("windows", device=-1)
    for field in ("x", "density", "lower", "upper"):
        assert same_bits(getattr(dev, field), getattr(ref, field)), field
    for field in ("n", "bandwidth", "factor", "replicas", "block", "level"):
        assert getattr(dev, field) == getattr(ref, field), field
    assert same_bits(dev.density, traj.distribution("windows").density)


def test_call_while_an_analysis_is_in_flight(hip_ctx, host):
    """A resident analysis of 1000 units is launched (asynchronous) and the weighted sums go onto the same context
    before anything waits for it: same sums as on a quiet context, and the analysis' records are still the goldens'."""
    from pywindow_amd import _lib, synth
    from pywindow_amd import element_data as E

    elements, frames = synth.synthetic_units(1000)
    ids = E.element_ids(elements)
    res = hip_ctx.upload(_lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids]))
    rng = np.random.default_rng(9)
    x = K.synthetic("bimodal", 400000)[:20000]
    packed = W.pack([(x, K.example_grid(x, 1000), W.edge_weights(rng, len(x), 40), 1.0 / 0.03)] + W.edge_jobs()[:8])
    quiet = hip_ctx.kde_wsums(*packed)
    res.launch()
    busy = hip_ctx.kde_wsums(*packed)
    recs = res.download()
    res.free()
    assert same_bits(busy, quiet) and same_bits(busy, host.kde_wsums(*packed))
    check_records(recs[:64], load_group("synth64"), where="analysis around a weighted KDE call")
