"""Weighted KDE sums under many weight vectors on the host path (device = -1): pw_kde_wsums against a plain-Python
restatement of its definition (bit for bit), against pw_kde_sums with weights of one, one replica against many,
a long-double sum, scipy.stats.gaussian_kde(weights=); the block bootstrap; RecordStore.distribution_band.
tests/test_gpu_kdew.py holds the device to the host path bit for bit.

Measured here (host path):
    worst |S - truth| / derived bound over the accuracy cases: 0.02 (bar 1)
    E_ours <= 1.4e-15, E_scipy <= 1.2e-13 relative to the peak over the SciPy cases
    AR(1) phi = 0.95, 4000 frames: mean width of the 95 % band over the central half of the grid with
    block = 2 x correlation time (33 frames) / with block = 1: 2.35 (the test asks for half of that)
"""
import math

import numpy as np
import pytest

import _kde_cases as K
import _kdew_cases as W
from _util import GOLDEN
from pywindow_amd import _lib, distributions, records

LD = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the definition ----------------------------------------------------------------------------------------

def test_exact_fma_of_the_restatement():
    assert np.finfo(LD).nmant >= 63
    # one rounding, not two: 1 + 2^-53 + 2^-106 rounds up only when the product is not rounded first
    a = 1.0 + 2.0 ** -52
    assert W.fma(a, a, -1.0) == 2.0 ** -51 + 2.0 ** -104 and a * a - 1.0 == 2.0 ** -51
    assert W.fma(1.0, 0.25, 0.5) == 0.75 and W.fma(0.0, 3.0, 0.0) == 0.0


@pytest.mark.parametrize("replicas", (1, 3))
@pytest.mark.parametrize("n", (1, 2, 511, 512, 513, 1025))
def test_definition_bit_for_bit(host, n, replicas):
    rng = np.random.default_rng(1000 * replicas + n)
    x = rng.normal(5.0, 0.5, n)
    g = np.array([3.1, 4.75, 5.0, 5.3, 9.0])
    w = W.edge_weights(rng, n, replicas + 1)[1:]               # (a magnitude-spanning row first)
    r = 1.0 / 0.21
    rec, xs, gs, ws = W.pack([(x, g, w, r)])
    got = W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))[0]
    assert same_bits(got, W.restated(host, x, g, w, r))


def test_no_samples_gives_zeros_and_no_points_nothing(host):
    g = np.linspace(0.0, 1.0, 7)
    jobs = [(np.zeros(0), g, np.zeros((3, 0)), 1.0), (np.array([0.5]), np.zeros(0), np.ones((2, 1)), 1.0),
            (np.array([0.5]), g, np.array([[2.0]]), 1.0)]
    rec, xs, gs, ws = W.pack(jobs)
    out = W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))
    assert out[0].shape == (3, 7) and (out[0] == 0.0).all() and out[1].shape == (2, 0)
    assert same_bits(out[2][0], 2.0 * host.kde_sums(*K.pack([(np.array([0.5]), g, 1.0)])))
    assert len(host.kde_wsums(rec[:0], xs, gs, ws)) == 0


@pytest.mark.parametrize("case", K.scipy_cases(), ids=lambda c: c[0])
def test_weights_of_one_are_the_unweighted_sums(host, case):
    """(a): fma(1, e, p) is p + e."""
    name, x, g = case
    g = g[:: max(1, len(g) // 40)] if len(x) > 4000 else g     # (the same bits point by point; 400 000 x 64 is enough)
    r = 1.0 / distributions.bandwidth(x)[0]
    plain = host.kde_sums(*K.pack([(x, g, r)]))
    rec, xs, gs, ws = W.pack([(x, g, np.ones((2, len(x))), r)])
    got = W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))[0]
    assert same_bits(got[0], plain) and same_bits(got[1], plain)


def test_a_replica_alone_has_the_bits_it_has_among_37(host):
    """(b), and neither the place in a batch, the thread count nor a repeated call takes part."""
    rng = np.random.default_rng(37)
    x = rng.normal(5.0, 0.7, 1300)
    g = K.example_grid(x, 150)
    w = W.edge_weights(rng, len(x), 37)
    r = 1.0 / 0.13
    rec, xs, gs, ws = W.pack([(x, g, w, r)])
    together = W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))[0]
    assert same_bits(together, W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))[0])
    rec1, xs1, gs1, ws1 = W.pack([(x, g, w[b:b + 1], r) for b in range(37)])
    alone = W.unpack(rec1, host.kde_wsums(rec1, xs1, gs1, ws1))
    for b in range(37):
        assert same_bits(alone[b][0], together[b]), b
    others = W.edge_jobs()[5:9]
    packed = W.pack(others + [(x, g, w, r)])
    assert same_bits(W.unpack(packed[0], host.kde_wsums(*packed))[-1], together)
    for threads in (1, 5):
        assert same_bits(W.unpack(rec, _lib.Context(-1, host_threads=threads).kde_wsums(rec, xs, gs, ws))[0], together)


# ---- accuracy ----------------------------------------------------------------------------------------------

def accuracy_cases():
    rng = np.random.default_rng(8)
    out = []
    for kind, n, m in (("normal", 10, 200), ("bimodal", 4000, 200), ("normal", 400000, 16)):
        x = K.synthetic(kind, n)
        w = np.stack([rng.random(n) + 0.01, rng.integers(0, 5, n).astype(np.float64), 10.0 ** rng.uniform(-3.0, 3.0, n)])
        out.append((f"{kind}-{n}", x, K.example_grid(x, m), w))
    return out


@pytest.mark.parametrize("case", accuracy_cases(), ids=lambda c: c[0])
def test_against_long_double_within_the_derived_bound(host, case):
    """One rounding per FMA of a chunk (512), one per chunk addition, 2 for second order, on sum_i w_i term_i (all
    terms are positive); and the term's own error as DESIGN 7b bounds it: (4 A + 4) 2^-53 relative, A the largest
    0.5 z^2 at the point."""
    name, x, g, w = case
    r = 1.0 / distributions.bandwidth(x)[0]
    rec, xs, gs, ws = W.pack([(x, g, w, r)])
    got = W.unpack(rec, host.kde_wsums(rec, xs, gs, ws))[0]
    truth = W.long_double_wsums(x, g, w, LD(r))
    chunk = K.source_constant("KDE_CHUNK")
    chunks = -(-len(x) // chunk)
    A = 0.5 * (np.maximum(np.abs(g - x.min()), np.abs(g - x.max())) * r) ** 2
    bound = ((chunk + chunks + 2) + (4.0 * A + 4.0))[None, :] * EPS * truth
    keep = truth > 1e-6 * truth.max(axis=1, keepdims=True)
    ratio = float((np.abs(got.astype(LD) - truth)[keep] / bound[keep]).max())
    print(f"weighted KDE {name}: n={len(x)} m={len(g)} R={len(w)} worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def scipy_weight_cases():
    out = []
    for n, m in ((10, 1000), (4000, 1000), (400000, 64)):
        x = K.synthetic("bimodal", n)
        rng = np.random.default_rng(n)
        out.append((f"positive-{n}", x, K.example_grid(x, m), rng.random(n) + 1e-3))
        out.append((f"multiplicity-{n}", x, K.example_grid(x, m), rng.integers(0, 4, n).astype(np.float64)))
    return out


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
@pytest.mark.parametrize("case", scipy_weight_cases(), ids=lambda c: c[0])
def test_against_scipy_with_weights(case, bw):
    from scipy import stats

    name, x, g, w = case
    kde = stats.gaussian_kde(x, bw_method=bw, weights=w)
    theirs = kde(g)
    mine = distributions.gaussian_kde_1d(x, g, bw, device=-1, weights=w)
    h, factor = distributions.bandwidth(x, bw, w)
    assert h == math.sqrt(kde.covariance[0, 0]) and factor == kde.factor
    assert mine.bandwidth == h and mine.factor == factor and mine.n == len(x)
    hl = LD(h)
    truth = W.long_double_wsums(x, g, w[None, :], LD(1.0) / hl)[0] / (w.astype(LD).sum() * hl * np.sqrt(LD(2.0) * LD(np.pi)))
    peak = truth.max()
    e_scipy = float(np.abs(theirs.astype(LD) - truth).max() / peak)
    e_ours = float(np.abs(mine.density.astype(LD) - truth).max() / peak)
    print(f"weighted KDE {name} bw={bw}: n={len(x)} m={len(g)} E_scipy={e_scipy:.3e} E_ours={e_ours:.3e}")
    assert e_ours <= max(4.0 * e_scipy, 64.0 * EPS)


def test_bandwidth_without_weights_is_unchanged_and_bad_weights_raise():
    x = K.synthetic("normal", 4000)
    for bw in K.BW_METHODS:
        from scipy import stats

        assert distributions.bandwidth(x, bw)[0] == math.sqrt(stats.gaussian_kde(x, bw_method=bw).covariance[0, 0])
        assert distributions.bandwidth(x, bw) == distributions.bandwidth(x, bw, None)
    for bad in (np.ones(3999), -np.ones(4000), np.full(4000, np.nan), np.full(4000, np.inf), np.zeros(4000), np.ones((2, 2000))):
        with pytest.raises(ValueError, match="weight"):
            distributions.bandwidth(x, "scott", bad)
    g = K.example_grid(x, 50)
    with pytest.raises(ValueError, match="weight"):
        distributions.gaussian_kde_1d(x, g, device=-1, weights=np.ones(5))
    with pytest.raises(ValueError, match="per set"):
        distributions.gaussian_kde_batch([x, x], [g, g], device=-1, weights=[None])


def test_batch_mixes_weighted_and_unweighted_sets():
    x, y = K.synthetic("normal", 600), K.synthetic("bimodal", 700)
    g = np.linspace(2.0, 9.0, 90)
    w = np.random.default_rng(3).random(700)
    a, b, c = distributions.gaussian_kde_batch([x, y, y], [g, g, g], device=-1, weights=[None, w, None])
    assert same_bits(a.density, distributions.gaussian_kde_1d(x, g, device=-1).density)
    assert same_bits(c.density, distributions.gaussian_kde_1d(y, g, device=-1).density)
    assert same_bits(b.density, distributions.gaussian_kde_1d(y, g, device=-1, weights=w).density)
    assert b.bandwidth != c.bandwidth


def test_replicas_against_numpy_and_their_errors():
    rng = np.random.default_rng(4)
    x = K.synthetic("bimodal", 900)
    g = K.example_grid(x, 120)
    w = rng.integers(0, 3, (11, 900)).astype(np.float64)
    d = distributions.gaussian_kde_replicas(x, g, w, 0.2, device=-1)
    z = (g[:, None] - x[None, :]) / 0.2
    want = (w[:, None, :] * np.exp(-0.5 * z * z)[None, :, :]).sum(axis=2) / (w.sum(axis=1)[:, None] * 0.2 * math.sqrt(2.0 * math.pi))
    assert d.shape == (11, 120) and np.abs(d - want).max() <= 1e-12 * want.max()
    assert np.abs(np.trapezoid(d, g, axis=1) - 1.0).max() <= 1e-6
    w[5] = 0.0
    with pytest.raises(ValueError, match="sums to zero"):
        distributions.gaussian_kde_replicas(x, g, w, 0.2, device=-1)
    with pytest.raises(ValueError, match="weights"):
        distributions.gaussian_kde_replicas(x, g, np.ones((3, 899)), 0.2, device=-1)
    with pytest.raises(ValueError, match="weights"):
        distributions.gaussian_kde_replicas(x, g, -np.ones((3, 900)), 0.2, device=-1)
    with pytest.raises(ValueError, match="bandwidth"):
        distributions.gaussian_kde_replicas(x, g, np.ones((3, 900)), 0.0, device=-1)


def test_error_paths_of_the_c_boundary(host):
    x, g = np.array([1.0, 2.0, 3.0]), np.linspace(0.0, 4.0, 9)
    good = (x, g, np.ones((2, 3)), 1.0)

    def call(job):
        return host.kde_wsums(*W.pack([good, job]))

    for bad in (-1.0, np.nan, np.inf):
        w = np.ones((2, 3))
        w[1, 2] = bad
        with pytest.raises(ValueError, match="job 1: a weight"):
            call((x, g, w, 1.0))
    for r in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="job 1: bandwidth"):
            call((x, g, np.ones((2, 3)), r))
    with pytest.raises(ValueError, match="job 1: no replica"):
        call((x, g, np.ones((0, 3)), 1.0))
    with pytest.raises(ValueError, match="job 1: a sample is NaN"):
        call((np.array([1.0, np.nan, 2.0]), g, np.ones((2, 3)), 1.0))
    with pytest.raises(ValueError, match="job 1: a point is NaN"):
        call((x, np.array([0.0, -np.inf]), np.ones((2, 3)), 1.0))
    rec, xs, gs, ws = W.pack([good])
    for what, args in (("samples", (rec, xs[:2], gs, ws)), ("points", (rec, xs, gs[:8], ws)), ("weights", (rec, xs, gs, ws[:5]))):
        with pytest.raises(IndexError, match=what):
            host.kde_wsums(*args)


# ---- the block bootstrap -------------------------------------------------------------------------------------

def test_block_bootstrap_counts():
    B = distributions.block_bootstrap_counts
    for n, block in ((1000, 7), (1000, 1), (10, 3), (10, 10), (7, 50), (1, 1)):
        c = B(n, block, 40, seed=3)
        assert c.shape == (40, n) and c.dtype == np.int64 and (c >= 0).all()
        assert (c.sum(axis=1) == n).all()
        assert np.array_equal(c, B(n, block, 40, seed=3))
    assert not np.array_equal(B(1000, 7, 40, seed=3), B(1000, 7, 40, seed=4))
    assert (B(50, 50, 20) == 1).all()                           # one block as long as the series: a rotation
    # the definition, draw by draw
    n, block, replicas = 23, 5, 6
    starts = np.random.default_rng(9).integers(0, n, (replicas, 5))
    want = np.zeros((replicas, n), dtype=np.int64)
    for b in range(replicas):
        for q in range(5):
            for u in range(block if q < 4 else n - 4 * block):
                want[b, (starts[b, q] + u) % n] += 1
    assert np.array_equal(B(n, block, replicas, seed=9), want)
    # block = 1: the ordinary bootstrap, every time drawn once on average
    c = B(200, 1, 4000, seed=1)
    assert np.abs(c.mean(axis=0) - 1.0).max() <= 5.0 / math.sqrt(4000)
    assert abs(c.var(axis=0).mean() - (1.0 - 1.0 / 200)) <= 0.05      # multinomial counts
    # blocks keep neighbours together: a time and the next are drawn together far more often than not
    c = B(200, 20, 2000, seed=1)
    assert np.corrcoef(c[:, 50], c[:, 51])[0, 1] > 0.8
    for bad in ((0, 1, 1), (5, 0, 1), (5, 1, 0)):
        with pytest.raises(ValueError):
            B(*bad)


# ---- bands of a store ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def history_store(tmp_path_factory):
    from pywindow_amd.trajectory import DLPOLY

    g = np.load(GOLDEN / "history20.npz")
    path = tmp_path_factory.mktemp("kdew") / "HISTORY_singlemol_short"
    path.write_bytes(g["file_bytes"].tobytes())
    traj = DLPOLY(path)
    traj.analysis(swap_atoms={"he": "H"}, forcefield="opls", device=-1)
    return traj


def numpy_replicas(values, x, weights, h):
    z = (x[:, None] - values[None, :]) / h
    return (weights[:, None, :] * np.exp(-0.5 * z * z)[None, :, :]).sum(axis=2) / (weights.sum(axis=1)[:, None] * h * math.sqrt(2.0 * math.pi))


@pytest.mark.parametrize("quantity", ("windows", "pore_diameter_opt", "maximum_diameter"))
@pytest.mark.parametrize("block", (None, 3))
def test_band_of_the_history_file(history_store, quantity, block):
    store = history_store.analysis_store
    band = store.distribution_band(quantity, points=300, replicas=60, block=block, seed=5, device=-1)
    plain = store.distribution(quantity, points=300, device=-1)
    assert isinstance(band, distributions.DistributionBand)
    assert same_bits(band.x, plain.x) and same_bits(band.density, plain.density)
    assert (band.n, band.bandwidth, band.factor, band.level) == (plain.n, plain.bandwidth, plain.factor, 0.95)
    assert (band.lower <= band.upper).all() and (band.lower >= 0.0).all() and (band.upper > band.lower).any()
    along = "windows_mean" if quantity == "windows" else quantity
    want_block = 3 if block else max(1, math.ceil(2.0 * store.correlation(along, device=-1).time))
    assert band.block == want_block and 1 <= band.replicas <= 60
    # the replicas, restated with numpy: every sample weighs as often as its frame was drawn
    values, unit = store._samples_by_unit(quantity)
    counts = distributions.block_bootstrap_counts(20, want_block, 60, seed=5)
    w = counts[:, np.asarray(store.unit_frame)[unit]].astype(np.float64)
    w = w[w.sum(axis=1) > 0]
    assert band.replicas == len(w)
    d = numpy_replicas(values, band.x, w, band.bandwidth)
    assert np.abs(band.lower - np.quantile(d, 0.025, axis=0)).max() <= 1e-12 * d.max()
    assert np.abs(band.upper - np.quantile(d, 0.975, axis=0)).max() <= 1e-12 * d.max()
    # the forwarder, the level and the seed
    again = history_store.distribution_band(quantity, points=300, replicas=60, block=block, seed=5, device=-1)
    assert same_bits(again.lower, band.lower) and same_bits(again.upper, band.upper)
    narrow = store.distribution_band(quantity, points=300, replicas=60, block=block, level=0.5, seed=5, device=-1)
    assert (narrow.lower >= band.lower).all() and (narrow.upper <= band.upper).all() and narrow.level == 0.5
    other = store.distribution_band(quantity, points=300, replicas=60, block=block, seed=6, device=-1)
    assert not same_bits(other.upper, band.upper)


def modular_store():
    """20 frames x 2 molecules (molecule 1: the golden frames backwards, its pore shifted), frame numbers 0, 5, 10 ..."""
    import test_kde

    g = test_kde.golden_store().records
    recs = np.concatenate([g, g[::-1]])
    recs["pore_d"][20:] += 0.5
    order = np.argsort(np.concatenate([np.arange(20), np.arange(20)]), kind="stable")
    return records.RecordStore(recs[order], 5 * np.repeat(np.arange(20), 2), np.tile([0, 1], 20))


@pytest.mark.parametrize("block", (None, 2))
def test_band_per_molecule_and_gaps(block):
    store = modular_store()
    bands = store.distribution_band("windows", points=100, replicas=30, block=block, per_molecule=True, device=-1)
    curves = store.distribution("windows", points=100, per_molecule=True, device=-1)
    assert sorted(bands) == [0, 1]
    values, unit = store._samples_by_unit("windows")
    for m in (0, 1):
        assert same_bits(bands[m].density, curves[m].density) and same_bits(bands[m].x, curves[m].x)
        assert (bands[m].lower <= bands[m].upper).all()
        pick = np.asarray(store.unit_molecule)[unit] == m
        counts = distributions.block_bootstrap_counts(20, bands[m].block, 30, seed=0)
        w = counts[:, np.asarray(store.unit_frame)[unit[pick]] // 5].astype(np.float64)
        d = numpy_replicas(values[pick], bands[m].x, w, bands[m].bandwidth)
        assert np.abs(bands[m].upper - np.quantile(d, 0.975, axis=0)).max() <= 1e-12 * d.max()
    # a store with gap frames and units without a value: synthetic_store of test_kde has three frames, of which
    # molecule 0 has windows in the first only
    import test_kde

    gappy = test_kde.synthetic_store()
    band = gappy.distribution_band("windows", points=50, replicas=40, block=1, per_molecule=True, device=-1)[1]
    frames, _, valid = gappy.series("windows_mean", 1)
    assert valid.tolist() == [True, False, True]
    counts = distributions.block_bootstrap_counts(3, 1, 40, seed=0)    # (replicas that drew only the gap frame are left out)
    assert band.replicas == int(((counts[:, 0] + counts[:, 2]) > 0).sum()) and (band.lower <= band.upper).all()


def test_band_errors_match_the_siblings():
    import test_kde

    store = test_kde.golden_store()
    with pytest.raises(KeyError, match="diameter_of_pore"):
        store.distribution_band("diameter_of_pore", device=-1)
    with pytest.raises(ValueError, match="per_molecule"):
        store.distribution_band("windows", per_molecule=True, device=-1)
    basic = records.RecordStore(store.records, store.unit_frame, stages=_lib.STAGE_BASIC)
    with pytest.raises(KeyError, match="windows"):
        basic.distribution_band("windows", device=-1)
    for bad in ({"replicas": 0}, {"level": 0.0}, {"level": 1.0}, {"block": 0}, {"bw_method": "scot"}):
        with pytest.raises(ValueError):
            store.distribution_band("pore_diameter", device=-1, **bad)
    with pytest.raises(Exception):
        store.distribution_band("pore_diameter", replicas=5, device=-1).block = 2        # frozen


def test_band_responds_to_correlation():
    """AR(1), phi = 0.95: neighbouring frames are not independent, and a band from single frames (block = 1) is too
    narrow.  Measured on the host path: the band from blocks of twice the correlation time is 2.35 times as wide
    over the central half of the grid; quantiles of 200 replicas are noisy at the 10 % level, so the test asks for
    half of that -- a band that ignored `block` would give 1."""
    store = W.ar1_store(4000, 0.95, 12)
    blocks = store.distribution_band("pore_diameter", points=200, device=-1)
    single = store.distribution_band("pore_diameter", points=200, block=1, device=-1)
    time = store.correlation("pore_diameter", device=-1).time
    assert blocks.block == max(1, math.ceil(2.0 * time)) and 20 <= blocks.block <= 60 and single.block == 1
    assert blocks.replicas == single.replicas == 200
    mid = slice(50, 150)
    ratio = float((blocks.upper - blocks.lower)[mid].mean() / (single.upper - single.lower)[mid].mean())
    print(f"AR(1) phi=0.95, 4000 frames: block {blocks.block}, band width ratio to block = 1: {ratio:.3f}")
    assert ratio >= 0.5 * 2.35
    assert (blocks.lower[mid] <= blocks.density[mid]).mean() > 0.9 and (blocks.density[mid] <= blocks.upper[mid]).mean() > 0.9
