"""Trajectory distributions on the host path (device = -1): pw_exp against a long-double exp, the Gaussian KDE
sums against scipy.stats.gaussian_kde (the route the reference's examples take, examples/example_7.py:55-80)
and against a long-double direct sum, the definition of the bandwidth, the extraction of samples from records,
and the error paths.  tests/test_gpu_kde.py holds the device to the host path bit for bit.

Measured here (host path; E = largest deviation from the long-double curve, relative to the peak):
    pw_exp: 0.5059 ulp at most over 2.8e6 arguments (bar 1 ulp)
    E_ours <= 1.7e-15 and E_scipy <= 1.1e-13 over every case (table in DESIGN.md, "Trajectory distributions")
"""
import math

import numpy as np
import pytest

import _kde_cases as K
from pywindow_amd import _lib, distributions, engine, records

LD = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).nmant >= 63


def test_pw_exp_within_one_ulp(host):
    assert np.finfo(LD).nmant >= 63
    x = K.exp_arguments()
    assert len(x) >= 1_000_000
    y = K.internal_exp(host, x)
    exact = np.exp(x.astype(LD))
    rounded = exact.astype(np.float64)
    normal = rounded >= np.finfo(np.float64).tiny
    err = np.abs(y[normal].astype(LD) - exact[normal]) / np.spacing(rounded[normal]).astype(LD)
    worst = float(err.max())
    print(f"pw_exp: {len(x)} arguments, largest error {worst:.4f} ulp at x = {x[normal][int(err.argmax())]!r}")
    assert worst <= 1.0
    # the stated choice below the smallest normal: zero, never a subnormal; and never above what is exact
    assert ((y[~normal] == 0.0) | (y[~normal] == np.finfo(np.float64).tiny)).all()
    assert (y[rounded < 0.5 * np.finfo(np.float64).tiny] == 0.0).all()
    assert y[x == 0.0].tolist() == [1.0] * int((x == 0.0).sum())


def long_double_curve(x, g, r):
    """sum_i exp(-0.5 ((g - x_i) r)^2) in long double, r a long double"""
    xl = x.astype(LD)
    out = np.zeros(len(g), dtype=LD)
    for j, gj in enumerate(g.astype(LD)):
        z = (gj - xl) * r
        out[j] = np.exp(LD(-0.5) * z * z).sum()
    return out


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
@pytest.mark.parametrize("case", K.scipy_cases(), ids=lambda c: c[0])
def test_against_scipy_and_long_double(case, bw):
    from scipy import stats

    name, x, g = case
    kde = stats.gaussian_kde(x, bw_method=bw)
    theirs = kde(g)
    mine = distributions.gaussian_kde_1d(x, g, bw, device=-1)
    assert mine.bandwidth == math.sqrt(kde.covariance[0, 0]) and mine.factor == kde.factor and mine.n == len(x)
    h = LD(mine.bandwidth)
    norm = LD(len(x)) * h * np.sqrt(LD(2.0) * LD(np.pi))
    truth = long_double_curve(x, g, LD(1.0) / h) / norm
    peak = truth.max()
    e_scipy = float(np.abs(theirs.astype(LD) - truth).max() / peak)
    e_ours = float(np.abs(mine.density.astype(LD) - truth).max() / peak)
    print(f"KDE {name} bw={bw}: n={len(x)} m={len(g)} E_scipy={e_scipy:.3e} E_ours={e_ours:.3e}")
    assert e_ours <= max(4.0 * e_scipy, 64.0 * EPS)

    # derived bound, relative, where the density matters: against the long-double sum with the kernel's own
    # double 1 / h.  L additions in the longest chain, A the largest 0.5 z^2 at the point (a rounding error in
    # the argument is multiplied by the argument), 4 for pw_exp and the last operations.
    r = 1.0 / mine.bandwidth
    same_r = long_double_curve(x, g, LD(r))
    sums = engine.context(-1).kde_sums(K.pack([(x, g, r)])[0], x, g)
    chunk = K.source_constant("KDE_CHUNK")
    L = chunk + -(-len(x) // chunk)
    A = 0.5 * (np.maximum(np.abs(g - x.min()), np.abs(g - x.max())) * r) ** 2
    keep = same_r > 1e-6 * same_r.max()
    rel = np.abs(sums.astype(LD) - same_r)[keep] / same_r[keep]
    bound = ((L + 4.0 * A + 4.0) * EPS)[keep]
    print(f"KDE {name} bw={bw}: largest relative error / bound = {float((rel / bound).max()):.3f}")
    assert (rel <= bound).all()
    if name == "far-tails":
        gap = np.abs(g[:, None] - x[None, :]).min(axis=1) * r
        assert (gap > 39.0).sum() > 100
        assert (mine.density[gap > 39.0] == 0.0).all() and (theirs[gap > 39.0] == 0.0).all()


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
def test_density_integrates_to_one(bw):
    x = K.synthetic("bimodal", 4000)
    g = np.linspace(x.min() - 6.0, x.max() + 6.0, 4001)
    d = distributions.gaussian_kde_1d(x, g, bw, device=-1)
    assert abs(np.trapezoid(d.density, d.x) - 1.0) <= 1e-6
    assert isinstance(d, distributions.Distribution)
    with pytest.raises(Exception):
        d.n = 3                                        # frozen


def test_same_bits_on_repeated_calls_and_anywhere_in_a_batch(host):
    x = K.synthetic("normal", 4000)[:1300]
    g = K.example_grid(x, 300)
    job = (x, g, 1.0 / 0.11)
    alone = host.kde_sums(*K.pack([job]))
    assert np.array_equal(alone, host.kde_sums(*K.pack([job])))
    others = K.mixed_batch()[3:9]
    first = host.kde_sums(*K.pack([job] + others))[: len(g)]
    last = host.kde_sums(*K.pack(others + [job]))[-len(g):]
    assert alone.tobytes() == first.tobytes() == last.tobytes()
    # nor does the number of host threads take part
    assert alone.tobytes() == _lib.Context(-1, host_threads=1).kde_sums(*K.pack([job])).tobytes()
    assert alone.tobytes() == _lib.Context(-1, host_threads=5).kde_sums(*K.pack([job])).tobytes()


def test_mixed_batch_against_numpy(host):
    jobs = K.mixed_batch()
    rec, xs, gs = K.pack(jobs)
    sums = host.kde_sums(rec, xs, gs)
    for j, (x, g, r) in zip(rec, jobs):
        got = sums[int(j["point_first"]):int(j["point_first"]) + len(g)]
        z = (g[:, None] - x[None, :]) * r
        want = np.exp(-0.5 * z * z).sum(axis=1)
        assert got.shape == want.shape
        if len(x) == 0:
            assert (got == 0.0).all()
        else:
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, want.max())


# ---- samples from records --------------------------------------------------------------------------------

def golden_store():
    g = np.load(K.GOLDEN / "md20.npz")
    n = len(g["n_windows"])
    recs = np.zeros(n, dtype=_lib.UNIT_OUT_DTYPE)
    for k in ("n_atoms", "maxd", "maxd_i", "maxd_j", "avg_d", "pore_d", "pore_atom", "pore_vol", "pore_opt_d", "pore_opt_atom",
              "pore_vol_opt", "n_windows", "com", "pore_opt_c", "win_d", "win_c"):
        recs[k] = g[k]
    return records.RecordStore(recs, np.arange(n))


def synthetic_store():
    """Six units of three frames, two molecules a frame: one with more windows than a record holds, one whose
    windows are None, one non-porous (no optimised pore, windows None), one with no windows at all."""
    rng = np.random.default_rng(5)
    recs = np.zeros(6, dtype=_lib.UNIT_OUT_DTYPE)
    recs["n_atoms"] = 10
    for k in ("maxd", "avg_d", "pore_d", "pore_vol", "pore_opt_d", "pore_vol_opt"):
        recs[k] = rng.random(6) + 1.0
    recs["win_d"] = rng.random((6, _lib.W_MAX)) + 2.0
    recs["n_windows"] = [4, _lib.W_MAX + 2, -1, -1, 0, 3]
    recs["status"] = [0, _lib.ST_WINDOW_OVERFLOW, 0, _lib.ST_NEGATIVE_PORE, 0, 0]
    extra = np.zeros(2, dtype=_lib.EXTRA_WINDOW_DTYPE)
    extra["unit"] = 1
    extra["index"] = [_lib.W_MAX, _lib.W_MAX + 1]
    extra["d"] = [7.5, 6.5]
    return records.RecordStore(recs, [0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1], extra)


def as_the_examples_collect(store, quantity):
    """The loops of examples/example_7.py:53-66 over the nested dicts, with the rule for units without a value."""
    props = engine.records_to_properties(store.records, store.stages, extra=store.extra)
    out = []
    for rec, p in zip(store.records, props):
        st = int(rec["status"])
        if quantity == "windows":
            if p["windows"]["diameters"] is not None:
                out.extend(p["windows"]["diameters"])
        elif quantity in ("pore_diameter_opt", "pore_volume_opt"):
            if not st & _lib.ST_NEGATIVE_PORE:
                out.append(p[quantity]["diameter"] if quantity == "pore_diameter_opt" else p[quantity])
        elif quantity in ("maximum_diameter", "pore_diameter"):
            out.append(p[quantity]["diameter"])
        else:
            out.append(p[quantity])
    return np.array(out, dtype=np.float64)


QUANTITIES = ("windows", "pore_diameter", "pore_diameter_opt", "maximum_diameter", "average_diameter", "pore_volume",
              "pore_volume_opt")


@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("make", (golden_store, synthetic_store), ids=("golden", "synthetic"))
def test_samples_are_what_the_examples_collect(make, quantity, caplog):
    store = make()
    got = store.samples(quantity)
    want = as_the_examples_collect(store, quantity)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    if make is synthetic_store and quantity == "windows":
        assert len(got) == 4 + _lib.W_MAX + 2 + 0 + 3 and got[4 + _lib.W_MAX:4 + _lib.W_MAX + 2].tolist() == [7.5, 6.5]
    if make is golden_store and quantity == "windows":
        assert got.tobytes() == K.golden_cc3()["windows"].tobytes()


def test_distribution_of_a_store_and_per_molecule(tmp_path):
    store = golden_store()
    d = store.distribution("windows", device=-1)
    x = store.samples("windows")
    direct = distributions.gaussian_kde_1d(x, np.linspace(x.min() - 1.0, x.max() + 1.0, 1000), device=-1)
    assert d.x.tobytes() == direct.x.tobytes() and d.density.tobytes() == direct.density.tobytes() and d.n == len(x)
    d2 = store.distribution("maximum_diameter", points=np.linspace(20.0, 30.0, 50), bw_method="silverman", device=-1)
    assert len(d2.density) == 50 and d2.x[0] == 20.0
    with pytest.raises(ValueError):
        store.distribution("windows", per_molecule=True, device=-1)      # one unit per frame: not modular

    # a modular store: 20 frames x 2 molecules
    g = golden_store().records
    recs = np.concatenate([g, g[::-1]])
    recs["pore_d"][20:] += 0.5
    order = np.argsort(np.concatenate([np.arange(20), np.arange(20)]), kind="stable")
    modular = records.RecordStore(recs[order], np.repeat(np.arange(20), 2), np.tile([0, 1], 20))
    curves = modular.distribution("pore_diameter", points=200, per_molecule=True, device=-1)
    assert sorted(curves) == [0, 1]
    for m in (0, 1):
        xm = modular.records["pore_d"][modular.unit_molecule == m]
        one = distributions.gaussian_kde_1d(xm, np.linspace(xm.min() - 1.0, xm.max() + 1.0, 200), device=-1)
        assert curves[m].density.tobytes() == one.density.tobytes() and curves[m].bandwidth == one.bandwidth
    wins = modular.distribution("windows", points=100, per_molecule=True, device=-1)
    assert wins[0].n + wins[1].n == len(modular.samples("windows"))

    # through a file
    back = records.RecordStore.load(synthetic_store().save(tmp_path / "s"))
    for q in QUANTITIES:
        assert back.samples(q).tobytes() == synthetic_store().samples(q).tobytes()
    assert back.distribution("windows", points=64, device=-1).density.tobytes() == \
        synthetic_store().distribution("windows", points=64, device=-1).density.tobytes()


def test_trajectory_distribution_after_lazy_analysis_and_reload(tmp_path):
    from pywindow_amd import synth
    from pywindow_amd.trajectory import DLPOLY

    path = synth.write_synthetic_history(tmp_path / "HISTORY", 6)
    traj = DLPOLY(path)
    traj.analysis(device=-1, lazy=True)
    d = traj.distribution("maximum_diameter", points=100, device=-1)
    assert d.n == 6 and d.density.tobytes() == traj.analysis_store.distribution("maximum_diameter", points=100, device=-1).density.tobytes()
    traj.save_records(tmp_path / "r")
    again = DLPOLY(path)
    again.load_records(tmp_path / "r")
    assert again.distribution("maximum_diameter", points=100, device=-1).density.tobytes() == d.density.tobytes()


# ---- errors ------------------------------------------------------------------------------------------------

def test_error_paths(host):
    g = np.linspace(0.0, 1.0, 10)
    with pytest.raises(ValueError, match="at least two"):
        distributions.gaussian_kde_1d([1.0], g, device=-1)
    with pytest.raises(ValueError, match="at least two"):
        distributions.gaussian_kde_1d([], g, device=-1)
    with pytest.raises(ValueError, match="variance is zero"):
        distributions.gaussian_kde_1d([2.0, 2.0, 2.0], g, device=-1)
    for bad in (0.0, -1.0, float("nan"), "scot"):
        with pytest.raises(ValueError, match="bw_method"):
            distributions.gaussian_kde_1d([1.0, 2.0], g, bad, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        distributions.gaussian_kde_1d([1.0, float("nan")], g, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        distributions.gaussian_kde_1d([1.0, 2.0], [0.0, float("inf")], device=-1)
    # the C boundary itself: PW_E_BAD_ARG with a message, nothing written
    x = np.array([1.0, 2.0, 3.0])
    for r in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="job 1: bandwidth"):
            host.kde_sums(*K.pack([(x, g, 1.0), (x, g, r)]))
    with pytest.raises(ValueError, match="job 0: a sample is NaN"):
        host.kde_sums(*K.pack([(np.array([1.0, np.nan]), g, 1.0)]))
    with pytest.raises(ValueError, match="job 0: a point is NaN"):
        host.kde_sums(*K.pack([(x, np.array([0.0, -np.inf]), 1.0)]))
    with pytest.raises(IndexError):
        rec, xs, gs = K.pack([(x, g, 1.0)])
        host.kde_sums(rec, xs[:2], gs)
    store = synthetic_store()
    with pytest.raises(KeyError, match="diameter_of_pore"):
        store.samples("diameter_of_pore")
    basic = records.RecordStore(store.records, store.unit_frame, store.unit_molecule, store.extra, stages=_lib.STAGE_BASIC)
    for q in ("windows", "pore_diameter_opt", "pore_volume_opt", "average_diameter"):
        with pytest.raises(KeyError, match=q):
            basic.samples(q)
    assert len(basic.samples("pore_diameter")) == 6
    with pytest.raises(KeyError, match="windows"):
        basic.distribution("windows", device=-1)
