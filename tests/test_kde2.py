"""Joint distributions on the host path (device = -1): the two-dimensional Gaussian KDE sums (pw_kde2_sums)
against scipy.stats.gaussian_kde with a 2 x n dataset and against a long-double direct sum, the kernel's
covariance against SciPy's bit for bit, the marginal identity, the pairing of samples from records, and the
error paths.  tests/test_gpu_kde2.py holds the device to the host path bit for bit.

Measured here (host path; E = largest deviation from the long-double map, relative to its peak):
    E_ours <= 7.6e-15 (rho = 0.999; 6e-16 elsewhere) and E_scipy up to 1.8e-8 over every case (table in DESIGN.md, "Joint distributions")
"""
import math

import numpy as np
import pytest

import _kde2_cases as K2
import _kde_cases as K
from pywindow_amd import _lib, distributions, engine, records
from test_kde import golden_store, synthetic_store

LD = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


# ---- covariance, SciPy, long double ------------------------------------------------------------------------

@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
@pytest.mark.parametrize("case", K2.scipy_cases(), ids=lambda c: c[0])
def test_covariance_is_scipys_bit_for_bit(case, bw):
    from scipy import stats

    _, x, y, _, _ = case
    d = np.vstack([x, y])
    kde = stats.gaussian_kde(d, bw_method=bw)
    covariance, factor = distributions.bandwidth_2d(d, bw)
    assert covariance.shape == (2, 2) and covariance.tobytes() == kde.covariance.tobytes()
    assert factor == kde.factor
    if bw == "silverman":                          # in two dimensions Silverman's factor IS Scott's
        assert factor == distributions.bandwidth_2d(d, "scott")[1]


def long_double_map(x, y, ax, ay, covariance):
    """The density on the mesh, (ny, nx), summed in long double with the inverse of the (double) covariance formed
    in long double."""
    assert np.finfo(LD).nmant >= 63
    c00, c01, c11 = LD(covariance[0, 0]), LD(covariance[0, 1]), LD(covariance[1, 1])
    det = c00 * c11 - c01 * c01
    i00, i01, i11 = c11 / det, -c01 / det, c00 / det
    pts = K2.mesh_points(ax, ay).astype(LD)
    xl, yl = x.astype(LD), y.astype(LD)
    out = np.zeros(len(pts), dtype=LD)
    step = max(1, 2_000_000 // len(x))
    for j0 in range(0, len(pts), step):
        dx = pts[j0:j0 + step, 0, None] - xl[None, :]
        dy = pts[j0:j0 + step, 1, None] - yl[None, :]
        energy = LD(0.5) * (dx * dx * i00 + LD(2.0) * dx * dy * i01 + dy * dy * i11)
        out[j0:j0 + step] = np.exp(-energy).sum(axis=1)
    norm = LD(len(x)) * LD(2.0) * LD(np.pi) * np.sqrt(det)
    return (out / norm).reshape(len(ay), len(ax))


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
@pytest.mark.parametrize("case", K2.scipy_cases(), ids=lambda c: c[0])
def test_against_scipy_and_long_double(case, bw):
    from scipy import stats

    name, x, y, ax, ay = case
    kde = stats.gaussian_kde(np.vstack([x, y]), bw_method=bw)
    theirs = kde(K2.mesh_points(ax, ay).T).reshape(len(ay), len(ax))
    mine = distributions.gaussian_kde_2d(x, y, (ax, ay), bw, device=-1)
    assert mine.density.shape == (len(ay), len(ax)) and mine.n == len(x)
    assert mine.x.tobytes() == ax.tobytes() and mine.y.tobytes() == ay.tobytes()
    assert mine.covariance.tobytes() == kde.covariance.tobytes() and mine.factor == kde.factor
    truth = long_double_map(x, y, ax, ay, kde.covariance)
    peak = truth.max()
    e_scipy = float(np.abs(theirs.astype(LD) - truth).max() / peak)
    e_ours = float(np.abs(mine.density.astype(LD) - truth).max() / peak)
    print(f"KDE2 {name} bw={bw}: n={len(x)} mesh={len(ax)}x{len(ay)} E_scipy={e_scipy:.3e} E_ours={e_ours:.3e}")
    assert e_ours <= max(4.0 * e_scipy, 64.0 * EPS)
    if name == "far-tails":
        w, _ = K2.whitening(kde.covariance)
        pts = K2.mesh_points(ax, ay)
        gap = np.full(len(pts), np.inf)
        for i0 in range(0, len(x), 500):
            dx = pts[:, None, 0] - x[None, i0:i0 + 500]
            dy = pts[:, None, 1] - y[None, i0:i0 + 500]
            gap = np.minimum(gap, np.sqrt((dx * w[0]) ** 2 + (dx * w[1] + dy * w[2]) ** 2).min(axis=1))
        far = (gap > 39.0).reshape(len(ay), len(ax))           # 0.5 * 39^2 > 745: nothing is left of any term
        assert far.sum() > 100
        assert (mine.density[far] == 0.0).all() and (theirs[far] == 0.0).all()


@pytest.mark.parametrize("bw", K.BW_METHODS, ids=str)
def test_marginal_identity_and_unit_mass(bw):
    """Exact mathematics: the joint density integrated over y is the 1-D Gaussian KDE of x with h = sqrt(c00), and the
    whole mesh integrates to 1.  Mesh 6 kernel widths beyond the samples (what is cut off: 2e-9 of a kernel), 4001
    points across y, x at a tenth of a kernel width (the trapezoid rule on a sum of Gaussians at such a step is exact
    to far below 1e-6)."""
    x, y = K2.correlated(400, 0.8, 5)
    covariance, factor = distributions.bandwidth_2d(np.vstack([x, y]), bw)
    hx, hy = math.sqrt(covariance[0, 0]), math.sqrt(covariance[1, 1])
    ax = np.linspace(x.min() - 6.0 * hx, x.max() + 6.0 * hx, 257)
    ay = np.linspace(y.min() - 6.0 * hy, y.max() + 6.0 * hy, 4001)
    assert ax[1] - ax[0] < 0.15 * hx
    d = distributions.gaussian_kde_2d(x, y, (ax, ay), bw, device=-1)
    marginal = np.trapezoid(d.density, d.y, axis=0)
    one = distributions.gaussian_kde_1d(x, ax, factor, device=-1)       # h = sqrt(var * factor^2) = sqrt(c00)
    assert abs(one.bandwidth - hx) <= 4.0 * EPS * hx
    err = float(np.abs(marginal - one.density).max())
    mass = float(np.trapezoid(marginal, d.x))
    print(f"KDE2 marginal bw={bw}: largest deviation from the 1-D curve {err:.3e} (peak {one.density.max():.3f}), mass - 1 = {mass - 1.0:.3e}")
    assert err <= 1e-6 * min(1.0, one.density.max())
    assert abs(mass - 1.0) <= 1e-6
    assert isinstance(d, distributions.Distribution2D)
    with pytest.raises(Exception):
        d.n = 3                                        # frozen


# ---- the same bits ------------------------------------------------------------------------------------------

def test_same_bits_on_repeated_calls_and_anywhere_in_a_batch(host):
    x, y = K2.correlated(1300, 0.6, 9)
    xy = np.stack([x, y], axis=1)
    pts = K2.mesh_points(K2.axis(x, 20, 1.0), K2.axis(y, 15, 1.0))
    job = (xy, pts, (1.0 / 0.11, -2.5, 1.0 / 0.3))
    alone = host.kde2_sums(*K2.pack([job]))
    assert alone.shape == (300,) and alone.max() > 1.0
    assert np.array_equal(alone, host.kde2_sums(*K2.pack([job])))
    others = K2.mixed_batch()[3:9]
    first = host.kde2_sums(*K2.pack([job] + others))[: len(pts)]
    last = host.kde2_sums(*K2.pack(others + [job]))[-len(pts):]
    assert alone.tobytes() == first.tobytes() == last.tobytes()
    for threads in (1, 5, 8):                      # nor does the number of host threads take part
        assert alone.tobytes() == _lib.Context(-1, host_threads=threads).kde2_sums(*K2.pack([job])).tobytes()


def test_mixed_batch_against_numpy(host):
    jobs = K2.mixed_batch()
    rec, xs, gs = K2.pack(jobs)
    sums = host.kde2_sums(rec, xs, gs)
    seen_peak = 0.0
    for j, (xy, pts, w) in zip(rec, jobs):
        got = sums[int(j["point_first"]):int(j["point_first"]) + len(pts)]
        want = K2.numpy_sums(xy, pts, w)
        assert got.shape == want.shape
        if len(xy) == 0:
            assert (got == 0.0).all()
        else:
            seen_peak = max(seen_peak, float(want.max()))
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, want.max())
    assert seen_peak > 1.0                         # (the jobs are not all in their tails)


# ---- pairs from records -------------------------------------------------------------------------------------

def pairs_as_the_examples_would_collect(store, qx, qy):
    """Loops over the nested dicts the way the examples collect one quantity (examples/example_7.py:53-66), for two:
    per unit, every value of qx with every value of qy (one of the two is a single value)."""
    props = engine.records_to_properties(store.records, store.stages, extra=store.extra)

    def values(rec, p, q):
        st = int(rec["status"])
        if q == "windows":
            return list(p["windows"]["diameters"]) if p["windows"]["diameters"] is not None else []
        if q in ("pore_diameter_opt", "pore_volume_opt"):
            if st & _lib.ST_NEGATIVE_PORE:
                return []
            return [p[q]["diameter"] if q == "pore_diameter_opt" else p[q]]
        if q in ("maximum_diameter", "pore_diameter"):
            return [p[q]["diameter"]]
        return [p[q]]

    vx, vy = [], []
    for rec, p in zip(store.records, props):
        for a in values(rec, p, qx):
            for b in values(rec, p, qy):
                vx.append(a)
                vy.append(b)
    return np.array(vx, dtype=np.float64), np.array(vy, dtype=np.float64)


PAIRS = (("pore_diameter_opt", "windows"), ("windows", "pore_diameter_opt"), ("pore_diameter_opt", "maximum_diameter"),
         ("maximum_diameter", "pore_diameter"), ("windows", "maximum_diameter"), ("pore_volume_opt", "average_diameter"))


@pytest.mark.parametrize("qx,qy", PAIRS)
@pytest.mark.parametrize("make", (golden_store, synthetic_store), ids=("golden", "synthetic"))
def test_sample_pairs_are_what_the_examples_would_collect(make, qx, qy):
    store = make()
    vx, vy = store.sample_pairs(qx, qy)
    wx, wy = pairs_as_the_examples_would_collect(store, qx, qy)
    assert vx.dtype == vy.dtype == np.float64
    assert vx.tobytes() == wx.tobytes() and vy.tobytes() == wy.tobytes()
    if make is synthetic_store and (qx, qy) == ("windows", "maximum_diameter"):
        # the unit with more windows than a record holds: all of them, in samples("windows")' order
        assert vx.tobytes() == store.samples("windows").tobytes()
        assert (vy[4:4 + _lib.W_MAX + 2] == store.records["maxd"][1]).all() and vx[4 + _lib.W_MAX:4 + _lib.W_MAX + 2].tolist() == [7.5, 6.5]
    if make is synthetic_store and (qx, qy) == ("pore_diameter_opt", "maximum_diameter"):
        assert len(vx) == 5                        # the non-porous unit has no optimised pore


def modular_store():
    """20 frames x 2 molecules from the golden records."""
    g = golden_store().records
    recs = np.concatenate([g, g[::-1]])
    recs["pore_opt_d"][20:] += 0.5
    order = np.argsort(np.concatenate([np.arange(20), np.arange(20)]), kind="stable")
    return records.RecordStore(recs[order], np.repeat(np.arange(20), 2), np.tile([0, 1], 20))


def same_map(a, b):
    return (a.density.tobytes() == b.density.tobytes() and a.x.tobytes() == b.x.tobytes() and a.y.tobytes() == b.y.tobytes()
            and a.n == b.n and a.covariance.tobytes() == b.covariance.tobytes() and a.factor == b.factor)


def test_joint_distribution_of_a_store_and_per_molecule(tmp_path):
    store = golden_store()
    d = store.joint_distribution("pore_diameter_opt", "windows", points=(24, 16), device=-1)
    vx, vy = store.sample_pairs("pore_diameter_opt", "windows")
    assert len(vx) == len(store.samples("windows")) == d.n and d.density.shape == (16, 24)
    direct = distributions.gaussian_kde_2d(vx, vy, (np.linspace(vx.min() - 1.0, vx.max() + 1.0, 24),
                                                    np.linspace(vy.min() - 1.0, vy.max() + 1.0, 16)), device=-1)
    assert same_map(d, direct)
    assert store.joint_distribution("pore_diameter_opt", "maximum_diameter", points=8, device=-1).density.shape == (8, 8)
    axes = (np.linspace(10.0, 14.0, 5), np.linspace(20.0, 30.0, 7))
    d2 = store.joint_distribution("pore_diameter_opt", "maximum_diameter", points=axes, bw_method="silverman", device=-1)
    assert d2.density.shape == (7, 5) and d2.x[0] == 10.0 and d2.y[-1] == 30.0
    with pytest.raises(ValueError, match="modular"):
        store.joint_distribution("pore_diameter_opt", "windows", per_molecule=True, device=-1)

    modular = modular_store()
    maps = modular.joint_distribution("pore_diameter_opt", "windows", points=(20, 12), per_molecule=True, device=-1)
    assert sorted(maps) == [0, 1]
    for m in (0, 1):
        only = records.RecordStore(modular.records[modular.unit_molecule == m], np.arange(20))
        assert same_map(maps[m], only.joint_distribution("pore_diameter_opt", "windows", points=(20, 12), device=-1))
    assert maps[0].n + maps[1].n == len(modular.samples("windows"))
    assert maps[0].density.tobytes() != maps[1].density.tobytes()

    # through a file
    back = records.RecordStore.load(synthetic_store().save(tmp_path / "s"))
    for qx, qy in PAIRS:
        for a, b in zip(back.sample_pairs(qx, qy), synthetic_store().sample_pairs(qx, qy)):
            assert a.tobytes() == b.tobytes()
    assert same_map(back.joint_distribution("windows", "maximum_diameter", points=16, device=-1),
                    synthetic_store().joint_distribution("windows", "maximum_diameter", points=16, device=-1))


def test_trajectory_joint_distribution_after_lazy_analysis_and_reload(tmp_path):
    from pywindow_amd import synth
    from pywindow_amd.trajectory import DLPOLY

    path = synth.write_synthetic_history(tmp_path / "HISTORY", 6)
    traj = DLPOLY(path)
    traj.analysis(device=-1, lazy=True)
    d = traj.joint_distribution("maximum_diameter", "pore_diameter", points=(12, 10), device=-1)
    assert d.n == 6 and d.density.shape == (10, 12) and d.density.max() > 0.0
    assert same_map(d, traj.analysis_store.joint_distribution("maximum_diameter", "pore_diameter", points=(12, 10), device=-1))
    traj.save_records(tmp_path / "r")
    again = DLPOLY(path)
    again.load_records(tmp_path / "r")
    assert same_map(again.joint_distribution("maximum_diameter", "pore_diameter", points=(12, 10), device=-1), d)


# ---- errors ------------------------------------------------------------------------------------------------

def test_error_paths(host):
    axes = (np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 3))
    with pytest.raises(ValueError, match="at least three"):
        distributions.gaussian_kde_2d([1.0, 2.0], [1.0, 3.0], axes, device=-1)
    with pytest.raises(ValueError, match="at least three"):
        distributions.gaussian_kde_2d([], [], axes, device=-1)
    with pytest.raises(ValueError, match="pairs"):
        distributions.gaussian_kde_2d([1.0, 2.0, 3.0], [1.0, 2.0], axes, device=-1)
    with pytest.raises(ValueError, match="first quantity is constant"):
        distributions.gaussian_kde_2d([2.0, 2.0, 2.0], [1.0, 2.0, 4.0], axes, device=-1)
    with pytest.raises(ValueError, match="second quantity is constant"):
        distributions.gaussian_kde_2d([1.0, 2.0, 4.0], [2.0, 2.0, 2.0], axes, device=-1)
    with pytest.raises(ValueError, match="linearly dependent"):
        distributions.gaussian_kde_2d([1.0, 2.0, 4.0], [1.0, 2.0, 4.0], axes, device=-1)
    with pytest.raises(ValueError, match="linearly dependent"):
        golden_store().joint_distribution("pore_diameter", "pore_diameter", device=-1)
    for bad in (0.0, -1.0, float("nan"), "scot"):
        with pytest.raises(ValueError, match="bw_method"):
            distributions.gaussian_kde_2d([1.0, 2.0, 4.0], [1.0, 3.0, 2.0], axes, bad, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        distributions.gaussian_kde_2d([1.0, float("nan"), 4.0], [1.0, 3.0, 2.0], axes, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        distributions.gaussian_kde_2d([1.0, 2.0, 4.0], [1.0, 3.0, 2.0], (axes[0], [0.0, float("inf")]), device=-1)
    with pytest.raises(ValueError, match="axes"):
        distributions.grid_2d([1.0, 2.0], [1.0, 2.0], (4, 5, 6))
    # the C boundary itself: PW_E_BAD_ARG with a message that names the job, nothing written
    xy = np.array([[1.0, 2.0], [2.0, 1.0], [3.0, 5.0]])
    pts = K2.mesh_points(*axes)
    good = (1.0, 0.5, 2.0)
    for w in ((0.0, 0.0, 1.0), (-2.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.0, -1.0), (float("nan"), 0.0, 1.0),
              (1.0, float("inf"), 1.0), (1.0, 0.0, float("inf")), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="job 1: factors"):
            host.kde2_sums(*K2.pack([(xy, pts, good), (xy, pts, w)]))
    with pytest.raises(ValueError, match="job 0: a sample is NaN"):
        host.kde2_sums(*K2.pack([(np.array([[1.0, 2.0], [1.0, np.nan]]), pts, good)]))
    with pytest.raises(ValueError, match="job 1: a point is NaN"):
        host.kde2_sums(*K2.pack([(xy, pts, good), (xy, np.array([[0.0, 1.0], [-np.inf, 0.0]]), good)]))
    # ... nothing written: the raw entry with a sentinel in the result
    rec, xs, gs = K2.pack([(xy, pts, good), (xy, pts, (1.0, 0.0, 0.0))])
    sums = np.full(len(gs), -7.0)
    rc = _lib.load().pw_kde2_sums(host._h, rec.ctypes.data, len(rec), xs.ctypes.data, gs.ctypes.data, sums.ctypes.data)
    assert rc == -2 and (sums == -7.0).all()
    with pytest.raises(IndexError):
        host.kde2_sums(rec, xs[:2], gs)
    assert host.kde2_sums(rec[:0], xs, gs).tolist() == [0.0] * len(gs)         # no job: nothing to do
    store = synthetic_store()
    with pytest.raises(ValueError, match="windows"):
        store.sample_pairs("windows", "windows")
    with pytest.raises(KeyError, match="diameter_of_pore"):
        store.sample_pairs("diameter_of_pore", "windows")
    basic = records.RecordStore(store.records, store.unit_frame, store.unit_molecule, store.extra, stages=_lib.STAGE_BASIC)
    with pytest.raises(KeyError, match="windows"):
        basic.joint_distribution("pore_diameter", "windows", device=-1)
    assert len(basic.sample_pairs("pore_diameter", "maximum_diameter")[0]) == 6
