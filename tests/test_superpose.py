"""Least-squares superposition on the host path (device = -1): pw_superpose against three references that owe nothing
to the library (tests/_superpose_cases.py).  The bars are margins over reference (i), the float64 SVD Kabsch, measured
against the long-double truth on the same case: ours may be 8 times as far from the truth, no more -- the 8 covers a
Jacobi and another order of summation against LAPACK.  Worst ratios measured: DESIGN.md 7h."""
import numpy as np
import pytest

import _superpose_cases as C

LD = C.LD
U = 2.0 ** -53


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=4)


@pytest.fixture(scope="module")
def rows(host):
    """One row per case of the list, job by job."""
    return {name: host.superpose(*C.pack([(x, y, w)]))[0] for name, x, y, w in C.cases()}


def orthogonality_bound():
    """|R^T R - I| for R formed from q / |q|: in exact arithmetic R^T R = |q|^4 I, and |q|^2 = 1 + e with |e| <= 4 U
    (a square root and a division, half an ulp each, on every component, twice in the square), so the exact R of the
    rounded q is off by 2 e <= 8 U.  Every entry of R is at most four products and three sums of terms that add up to
    at most |q|^2, an error of 4 U at the most; a column of three such entries against another adds 2 * 3 * 4 U = 24 U,
    and numpy's own product of three terms 3 U: 35 U.  Second-order terms are below U; 64 U is asserted."""
    return 64 * U


def test_the_case_list_is_mostly_well_conditioned():
    gaps = [r["horn"][2] for r in C.references().values()]
    assert sum(g < C.WELL_CONDITIONED for g in gaps) * 4 <= len(gaps)
    assert {len(x) for _, x, _, _ in C.cases()} == set(C.SIZES)


def test_the_references_agree_with_each_other():
    """The truth is held by the other two: (i) and (ii) are within float64 rounding of (iii) where the problem is
    well conditioned, so a mistake in the truth's own code would show here."""
    for name, r in C.references().items():
        Rt, rt = r["truth"]
        assert abs(float(LD(r["kabsch"][1]) - rt)) <= 1e-13 * max(float(rt), 1.0) and abs(float(LD(r["horn"][1]) - rt)) <= 1e-13 * max(float(rt), 1.0), name
        if r["horn"][2] >= C.WELL_CONDITIONED:
            assert float(np.abs(r["kabsch"][0] - Rt).max()) < 1e-12 and float(np.abs(r["horn"][0] - Rt).max()) < 1e-12, name


def test_rmsd_against_the_truth(rows):
    worst = 0.0
    for name, r in C.references().items():
        Rt, rt = r["truth"]
        ours, ref = abs(float(LD(rows[name]["rmsd"]) - rt)), abs(float(LD(r["kabsch"][1]) - rt))
        bar = max(8.0 * ref, 4.0 * float(np.spacing(np.float64(rt))))
        worst = max(worst, ours / bar) if bar > 0 else worst
        print(f"{name}: rmsd {float(rt):.6e}  ours {ours:.3e}  reference (i) {ref:.3e}  bar {bar:.3e}")
        assert ours <= bar, name
    print("worst ours / bar:", worst)


def test_rotation_against_the_truth(rows):
    checked = 0
    for name, r in C.references().items():
        if r["horn"][2] < C.WELL_CONDITIONED:
            continue
        Rt = r["truth"][0]
        ours = float(np.abs(rows[name]["rotation"].astype(LD) - Rt).max())
        ref = float(np.abs(r["kabsch"][0].astype(LD) - Rt).max())
        print(f"{name}: gap {r['horn'][2]:.2e}  ours {ours:.3e}  reference (i) {ref:.3e}")
        assert ours <= max(8.0 * ref, 2.0 ** -50), name
        checked += 1
    assert checked * 4 >= 3 * len(C.cases())


def test_every_rotation_is_proper(rows):
    for name, row in rows.items():
        R = row["rotation"]
        assert np.linalg.det(R) > 0.0, name
        assert np.abs(R.T @ R - np.eye(3)).max() <= orthogonality_bound(), name
        assert row["lambda"][0] >= row["lambda"][1] and 0 <= row["sweeps"] <= 30 and row["reserved"] == 0, name


def test_centres_and_apply(rows):
    from pywindow_amd import Superposition

    for name, x, y, w in C.cases():
        ww = np.ones(len(x)) if w is None else w
        for field, pts in (("centre_mobile", x), ("centre_target", y)):
            want = (ww[:, None] * pts).sum(axis=0) / ww.sum()
            assert np.abs(rows[name][field] - want).max() <= 64 * U * np.abs(pts).max(), name
        s = Superposition.from_row(rows[name])
        d = s.apply(x) - y
        assert abs(np.sqrt((ww * (d * d).sum(axis=1)).sum() / ww.sum()) - s.rmsd) <= 1e-12 * max(1.0, np.abs(y).max()), name


def test_identical_structures(rows):
    """Mobile and target the same rows: M is symmetric to the bit (the product dx_a * dy_b is rounded before the
    weight), Horn's first row is zero, the quaternion is (1, 0, 0, 0): the identity and an RMSD of exactly 0 -- within
    any residual rounding bound and any bar."""
    for name in ("identical n=168", "identical, weighted n=129"):
        assert np.array_equal(rows[name]["rotation"], np.eye(3)) and rows[name]["rmsd"] == 0.0, name


def test_moving_both_structures_together(host):
    """A common translation or rotation of both structures leaves the RMSD where it was, within the bar of
    test_rmsd_against_the_truth for the moved case -- against the long-double truth of the moved case itself, which is
    the truth of the original to its own rounding."""
    R = C.rotation_matrix([0.3, -1.0, 0.5], 1.1)
    for name in ("random n=168", "masses n=168", "random n=65", "noise of 1e-8 n=168"):
        _, x, y, w = next(c for c in C.cases() if c[0] == name)
        for xm, ym in ((x + [3.0, -2.0, 7.0], y + [3.0, -2.0, 7.0]), (x @ R.T, y @ R.T)):
            ours = host.superpose(*C.pack([(xm, ym, w)]))[0]["rmsd"]
            rt = C._truth(xm, ym, w)[1]
            ref = abs(float(LD(C.kabsch(xm, ym, w)[1]) - rt))
            assert abs(float(LD(ours) - rt)) <= max(8.0 * ref, 4.0 * float(np.spacing(np.float64(rt)))), name
            assert abs(ours - C.references()[name]["kabsch"][1]) <= 1e-13 * max(1.0, np.abs(xm).max()), name


def test_degenerate_sets(rows):
    """n = 1, n = 2, collinear, one weight: a proper rotation, a small gap that says so, and the right RMSD (the
    RMSD and properness asserted for every case above; here the gap and the exact values)."""
    one = rows["random n=1"]
    assert np.array_equal(one["rotation"], np.eye(3)) and one["rmsd"] == 0.0 and one["sweeps"] == 0
    assert np.array_equal(one["lambda"], [0.0, 0.0])
    for name in ("random n=2", "collinear n=63"):
        lam = rows[name]["lambda"]
        assert lam[0] > 0.0 and (lam[0] - lam[1]) <= 1e-12 * lam[0], name
    single = rows["one weight not zero n=4"]
    assert np.array_equal(single["rotation"], np.eye(3)) and single["rmsd"] <= 4 * U * 10.0


def test_weights_of_one_are_no_weights(host, rows):
    """pw_superpose.hpp: fma(1, x, acc) is acc + x, so weights that are all exactly 1.0 give the bits of a job without
    weights.  Other equal weights round on their own and agree to rounding only: asserted as such, not to the bit."""
    _, x, y, w = next(c for c in C.cases() if c[0] == "weights all 1.0 n=168")
    assert C.same_bytes(host.superpose(*C.pack([(x, y, None)])), host.superpose(*C.pack([(x, y, w)])))
    _, x, y, w = next(c for c in C.cases() if c[0] == "weights all 12.011 n=168")
    a, b = host.superpose(*C.pack([(x, y, None)]))[0], host.superpose(*C.pack([(x, y, w)]))[0]
    assert abs(a["rmsd"] - b["rmsd"]) <= 1e-14 and np.abs(a["rotation"] - b["rotation"]).max() <= 1e-14


@pytest.mark.parametrize("count", C.BATCHES)
def test_one_batch_equals_job_by_job(host, rows, count):
    names = [c[0] for c in C.cases()]
    rec, xyz, wts = C.pack(C.batch(count), hole=1)
    rc, got = C.raw(host, rec, xyz, wts)
    assert rc == 0 and len(got) == 2 * count
    assert C.untouched(got)[0::2].all() and not C.untouched(got)[1::2].any()
    for k in range(count):
        assert got[2 * k + 1].tobytes() == rows[names[k % len(names)]].tobytes(), k


def test_host_threads_do_not_show():
    from pywindow_amd import _lib

    packed = C.pack(C.batch(65))
    assert C.same_bytes(_lib.Context(-1, host_threads=1).superpose(*packed), _lib.Context(-1, host_threads=16).superpose(*packed))


def test_jobs_may_share_rows(host):
    """Mobile and target the same rows, and two jobs over the same rows."""
    _, x, y, w = C.cases()[10]
    n = len(x)
    xyz = np.concatenate([x, y])
    from pywindow_amd import _lib

    rec = np.array([(0, 0, -1, n, 0), (0, n, -1, n, 1), (0, n, -1, n, 2), (n, 0, -1, n, 3)],
                   dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    got = host.superpose(rec, xyz)
    assert got[0]["rmsd"] == 0.0 and got[1].tobytes() == got[2].tobytes()
    assert abs(got[3]["rmsd"] - got[1]["rmsd"]) <= 1e-14 and np.abs(got[3]["rotation"] - got[1]["rotation"].T).max() <= 1e-14


def test_every_error_returns_minus_two_and_writes_nothing(host):
    x = np.arange(30.0).reshape(10, 3) ** 1.5
    w = np.ones(10)
    good = (0, 2, 0, 2, 0)                      # rows 0 .. 3, weights 0 and 1

    def call(job, xyz=x, weights=w, n_points=None):
        from pywindow_amd import _lib

        rec = np.array([good, job], dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
        rc, rows = C.raw(host, rec, xyz, weights, n_points=n_points)
        assert rc == -2 and C.untouched(rows).all()
        return _lib.load().pw_last_error().decode()

    assert "job 1: n < 1" in call((0, 5, 0, 0, 1))
    assert "job 1: points outside" in call((0, 6, 0, 5, 1))
    assert "job 1: points outside" in call((-1, 5, 0, 5, 1))
    assert "job 1: weights outside" in call((0, 5, 6, 5, 1))
    assert "job 1: weights outside" in call((0, 5, -2, 5, 1))
    assert "job 1: a negative row" in call((0, 5, 0, 5, -1))
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[7, 1] = bad
        assert "job 1: a coordinate is not finite" in call((0, 5, -1, 5, 1), xyz=xb)
        xb[7, 1], xb[3, 2] = 1.0, bad
        assert "job 0: a coordinate is not finite" in call((4, 6, -1, 2, 1), xyz=xb)      # (job 0 reads row 3, job 1 does not)
    for bad in (-1.0, np.nan, np.inf):
        wb = w.copy()
        wb[6] = bad
        assert "job 1: a weight is negative or not finite" in call((0, 5, 5, 5, 1), weights=wb)
    wb = w.copy()
    wb[5:] = 0.0
    assert "job 1: the weights sum to 0" in call((0, 5, 5, 5, 1), weights=wb)
    assert "null array" in call((0, 5, 5, 5, 1), weights=None)
    with pytest.raises(ValueError, match="n < 1"):
        from pywindow_amd import _lib

        host.superpose(np.array([(0, 5, -1, 0, 0)], dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1), x)


def test_a_bad_row_no_job_reads_is_not_an_error(host):
    from pywindow_amd import _lib

    x = np.arange(30.0).reshape(10, 3)
    x[4, 0] = np.nan
    rec = np.array([(0, 5, -1, 4, 0)], dtype=np.int64).view(_lib.SUPERPOSE_JOB_DTYPE).reshape(-1)
    assert host.superpose(rec, x)[0]["rmsd"] >= 0.0


def test_the_public_functions():
    import pywindow_amd as pw

    _, x, y, w = next(c for c in C.cases() if c[0] == "masses n=168")
    s = pw.superpose(x, y, w, device=-1)
    both = pw.superpose_batch([(x, y, w), (y, x, None)], device=-1)
    assert isinstance(s, pw.Superposition) and s.rmsd == both[0].rmsd and np.array_equal(s.rotation, both[0].rotation)
    assert s.eigenvalues.shape == (2,) and s.rotation.shape == (3, 3) and isinstance(s.sweeps, int)
    assert abs(s.rmsd - C.references()["masses n=168"]["kabsch"][1]) < 1e-13
    for bad in ((x[:5], y[:6], None), (x, y, w[:5]), (x[:, :2], y[:, :2], None)):
        with pytest.raises(ValueError):
            pw.superpose(*bad, device=-1)
    with pytest.raises(ValueError, match="sum to 0"):
        pw.superpose(x, y, np.zeros(len(x)), device=-1)


def test_rmsd_matrix_is_symmetric_and_equals_per_pair():
    import pywindow_amd as pw
    from pywindow_amd import superposition as SP

    rng = np.random.default_rng(5)
    base = 4.0 * rng.standard_normal((37, 3))
    coords = np.array([C.moved(base, C.random_rotation(rng), rng.uniform(-2, 2, 3), 0.1, rng) for _ in range(9)])
    w = rng.uniform(1.0, 16.0, 37)
    for weights in (None, w):
        m = pw.rmsd_matrix(coords, weights, device=-1)
        assert m.shape == (9, 9) and np.array_equal(m, m.T) and np.array_equal(np.diag(m), np.zeros(9))
        for i in range(9):
            for j in range(i + 1, 9):
                assert m[i, j] == pw.superpose(coords[i], coords[j], weights, device=-1).rmsd
    slab = SP.MATRIX_SLAB
    try:
        SP.MATRIX_SLAB = 7                      # several calls: the cut does not show
        assert np.array_equal(pw.rmsd_matrix(coords, w, device=-1), m)
    finally:
        SP.MATRIX_SLAB = slab
    onto = SP.superpose_onto(coords, 3, w, device=-1)
    assert np.array_equal(onto["rmsd"][:4], m[:4, 3]) and np.allclose(onto["rmsd"], m[3], rtol=0.0, atol=1e-13)
    assert pw.rmsd_matrix(coords[:1], device=-1).shape == (1, 1)
