"""pw_covariance and pw_project on the host path (device = -1) against references that owe nothing to the library
(tests/_cov_cases.py).

ACCURACY.  The bar is the project's own (tests/test_superpose.py), for the same reason -- another order of summation
against BLAS: on every case the distance of ours from the long-double truth (iii), the largest error of an entry, is
at most 8 times that of reference (i), float64 numpy.  An entry below the floor passes whatever reference (i) did: the
floor is 4 ulp of ``sum_t |z_a z_b|`` of the truth for an entry of S, of ``sum_a |z_a V_a|`` for a projection and of
``max_t |y_ta|`` for an entry of the mean.  Worst ratios measured: DESIGN.md 7j.

EXACT PROPERTIES are asserted on the bytes."""
import numpy as np
import pytest

import _cov_cases as C

LD = C.LD


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=4)


@pytest.fixture(scope="module")
def results(host):
    """(mean, scatter | None) per case of the list, job by job."""
    return {name: C.one(host, name) for name, *_ in C.cases()}


def test_the_case_list_covers_every_edge():
    shapes = {(X.shape, tr is not None) for _, X, tr, _ in C.cases()}
    for D in C.D_PLAIN:
        assert ((C.CHUNK + 1, D), False) in shapes
    for D in C.D_MOVED:
        assert ((C.CHUNK + 1, D), True) in shapes
    for T in C.T_EDGES:
        assert {((T, 3), False), ((T, 3), True), ((T, C.TILE + 1), False), ((T, C.TILE + 1), True)} <= shapes
    assert len({name for name, *_ in C.cases()}) == len(C.cases())


def test_the_references_agree_with_each_other():
    """The truth is held by reference (i), so a mistake in the truth's own code would show here.  A float64 mean is
    off by d <= T u max|y| at the most, which moves an entry of S by T d^2 (the first order cancels: the z sum to 0);
    the sums themselves add a few u of the sum of absolute values."""
    u = 2.0 ** -53
    for name, X, tr, _ in C.cases():
        r = C.reference(name)
        T, top = len(X), float(np.abs(C.moved(X, tr)).max())
        bound = 1e-12 * float(r["scatter_abs"].max()) + T * (T * u * top) ** 2
        assert float(np.abs(r["scatter"] - r["scatter_t"]).max()) <= bound, name


def test_scatter_against_the_truth(results):
    worst = 0.0
    for name, X, tr, wanted in C.cases():
        if wanted:
            r = C.reference(name)
            worst = max(worst, C.held(results[name][1], r["scatter"], r["scatter_t"], r["scatter_abs"], name))
    print("worst ours / bar:", worst)


def test_mean_against_the_truth(results):
    worst = 0.0
    for name, X, tr, _ in C.cases():
        r = C.reference(name)
        scale = np.abs(C.moved(X, tr)).max(axis=0)
        worst = max(worst, C.held(results[name][0], r["mean"], r["mean_t"], scale, name))
    print("worst ours / bar:", worst)


@pytest.mark.parametrize("k", [1, 2, 65])
def test_projection_against_the_truth(host, results, k):
    worst = 0.0
    for name in ("T=257 D=129", "T=257 D=129 moved", "T=2 D=3 moved", "T=513 D=257", "a mean large against the spread T=300 D=7"):
        _, X, tr, _ = C.case(name)
        V, mean = C.vectors(name, k), results[name][0]
        ours = C.project(host, X, tr, mean, V)
        ref, truth, scale = C.projection_reference(name, V, mean)
        worst = max(worst, C.held(ours, ref, truth, scale, f"{name} k={k}"))
    print("worst ours / bar:", worst)


# ---- exact properties -------------------------------------------------------------------------------------------------
def test_scatter_is_symmetric_to_the_bit(results):
    for name, (mean, S) in results.items():
        assert S is None or np.array_equal(S, S.T), name
        assert not np.isnan(mean).any() and (S is None or not np.isnan(S).any()), name


def test_one_row_gives_plus_zero_everywhere(results):
    for name in ("T=1 D=3", "T=1 D=3 moved", "T=1 D=129", "T=1 D=129 moved"):
        S = results[name][1]
        assert np.array_equal(S, np.zeros_like(S)) and not np.signbit(S).any(), name


def test_a_constant_column_has_a_zero_row_and_column(results):
    mean, S = results["a constant column T=300 D=6"]
    assert mean[2] == 2.5 and not S[2].any() and not S[:, 2].any() and S[0, 0] > 0.0


def test_the_mean_only_is_the_mean_of_the_full_call(host):
    for name in ("the mean only T=300 D=9", "the mean only, moved T=257 D=129"):
        _, X, tr, _ = C.case(name)
        (alone, none), = C.run(host, [(X, tr, False)])[0]
        (full, S), = C.run(host, [(X, tr, True)])[0]
        assert none is None and S is not None and C.same(alone, full), name


@pytest.mark.parametrize("k", [1, C.TILE - 1, C.TILE, C.TILE + 2])
def test_leading_columns_alone(host, k):
    """An entry of S and of the mean is a function of its own two columns: the leading k columns alone give
    S[:k, :k] and mean[:k], on both sides of a tile edge."""
    X = np.random.default_rng(3).standard_normal((C.CHUNK + 5, C.TILE + 70))
    (mean, S), = C.run(host, [(X, None, True)])[0]
    (m, s), = C.run(host, [(np.ascontiguousarray(X[:, :k]), None, True)])[0]
    assert C.same(m, mean[:k]) and C.same(s, np.ascontiguousarray(S[:k, :k]))


def test_leading_points_alone_with_transforms(host):
    rng = np.random.default_rng(4)
    T, k = C.CHUNK + 5, C.TILE + 1
    X, tr = rng.standard_normal((T, C.TILE + 70)), C.transforms(rng, T)
    (mean, S), = C.run(host, [(X, tr, True)])[0]
    (m, s), = C.run(host, [(np.ascontiguousarray(X[:, :k]), tr, True)])[0]
    assert C.same(m, mean[:k]) and C.same(s, np.ascontiguousarray(S[:k, :k]))


def test_a_column_permutation_permutes_the_result(host):
    """fma(z_a, z_b, acc) commutes to the bit, so a permutation of the columns -- across the tile edge and across the
    diagonal -- gives the permuted S; with transforms the same holds for a permutation of the points."""
    rng = np.random.default_rng(5)
    T, D = C.CHUNK + 5, C.TILE + 70
    X = rng.standard_normal((T, D))
    p = rng.permutation(D)
    (mean, S), = C.run(host, [(X, None, True)])[0]
    (m, s), = C.run(host, [(np.ascontiguousarray(X[:, p]), None, True)])[0]
    assert C.same(m, mean[p]) and C.same(s, np.ascontiguousarray(S[np.ix_(p, p)]))
    tr = C.transforms(rng, T)
    q = (3 * rng.permutation(D // 3)[:, None] + np.arange(3)).reshape(-1)
    (mean, S), = C.run(host, [(X, tr, True)])[0]
    (m, s), = C.run(host, [(np.ascontiguousarray(X[:, q]), tr, True)])[0]
    assert C.same(m, mean[q]) and C.same(s, np.ascontiguousarray(S[np.ix_(q, q)]))


@pytest.mark.parametrize("count", C.BATCHES)
def test_one_batch_equals_job_by_job(host, count):
    items = C.small_items(count)
    alone = [C.run(host, [it])[0][0] for it in items[:7]]
    got, mean, scatter, spans = C.run(host, items, hole=3)
    for k, (m, s) in enumerate(got):
        am, as_ = alone[k % 7]
        assert C.same(m, am) and ((s is None and as_ is None) or C.same(s, as_)), k
    assert C.untouched(mean)[~C.owned(len(mean), [sp[0] for sp in spans])].all()
    assert C.untouched(scatter)[~C.owned(len(scatter), [sp[1] for sp in spans])].all()
    assert not C.untouched(mean)[C.owned(len(mean), [sp[0] for sp in spans])].any()


def test_host_threads_do_not_show():
    from pywindow_amd import _lib

    one, many = _lib.Context(-1, host_threads=1), _lib.Context(-1, host_threads=16)
    for name in ("T=513 D=257", "T=513 D=258 moved"):
        a, b = C.one(one, name), C.one(many, name)
        assert C.same(a[0], b[0]) and C.same(a[1], b[1]), name
        _, X, tr, _ = C.case(name)
        V = C.vectors(name, 5)
        assert C.same(C.project(one, X, tr, a[0], V), C.project(many, X, tr, a[0], V)), name


@pytest.mark.parametrize("workspace", [1, 100_000, 0])
def test_the_workspace_does_not_show(host, results, workspace):
    for name in ("T=513 D=257", "T=513 D=258 moved", "T=257 D=3", "the mean only T=300 D=9"):
        m, s = C.one(host, name, workspace_bytes=workspace)
        assert C.same(m, results[name][0]) and (s is None or C.same(s, results[name][1])), name


def test_projection_batch_equals_job_by_job(host, results):
    names = ["T=2 D=3 moved", "T=257 D=129", "T=255 D=3"]
    parts = [(C.case(n)[1], C.case(n)[2], results[n][0], C.vectors(n, k)) for n, k in zip(names, (2, 3, 1))]
    alone = [C.project(host, *p) for p in parts]
    got, proj, spans = C.project_batch(host, parts, hole=2)
    for a, g in zip(alone, got):
        assert C.same(a, g)
    assert C.untouched(proj)[~C.owned(len(proj), spans)].all()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def refused(ctx, jobs, data, tr, n_mean=64, n_scatter=256):
    """The library's message for a call it must refuse; both outputs still hold the sentinel."""
    from pywindow_amd import _lib

    mean, scatter = C.sentinel(n_mean), C.sentinel(n_scatter)
    rec = np.array(jobs, dtype=np.int64).view(_lib.COV_JOB_DTYPE).reshape(-1)
    with pytest.raises(ValueError) as err:
        ctx.covariance(rec, data, tr, mean=mean, scatter=scatter)
    assert C.untouched(mean).all() and C.untouched(scatter).all()
    return str(err.value)


def test_every_refusal_names_the_job_and_writes_nothing(host):
    rng = np.random.default_rng(9)
    x = rng.standard_normal(60)
    tr = C.transforms(rng, 5)
    good = (0, 4, 3, 0, 0, 0)                   # T = 4, D = 3, transforms 0 .. 3, mean 0 .. 2, S 0 .. 8

    def call(job, data=x, rows=tr, **kw):
        return refused(host, [good, job], data, rows, **kw)

    assert "job 1: T < 1" in call((0, 0, 3, -1, 10, 20))
    assert "job 1: D < 1" in call((0, 4, 0, -1, 10, 20))
    assert "job 1: D > PW_COV_MAX_D" in call((0, 1, 3073, -1, 10, 20), data=np.zeros(4000))
    assert "job 1: D is not a multiple of 3" in call((0, 4, 4, 0, 10, 20))
    assert "job 1: a matrix outside data" in call((50, 4, 3, -1, 10, 20))
    assert "job 1: a matrix outside data" in call((-1, 4, 3, -1, 10, 20))
    assert "job 1: a matrix outside data" in call((0, 1 << 62, 3, -1, 10, 20))
    assert "job 1: rows outside the transforms" in call((0, 4, 3, 2, 10, 20))
    assert "job 1: a negative row of the transforms" in call((0, 4, 3, -2, 10, 20))
    assert "job 1: a mean outside" in call((12, 4, 3, -1, 62, 20))
    assert "job 1: a mean outside" in call((12, 4, 3, -1, -1, 20))
    assert "job 1: a scatter matrix outside" in call((12, 4, 3, -1, 10, 250))
    assert "job 1: a scatter matrix outside" in call((12, 4, 3, -1, 10, -2))
    assert "job 1: shares entries of the mean" in call((12, 4, 3, -1, 2, 20))
    assert "job 1: shares entries of the scatter" in call((12, 4, 3, -1, 10, 8))
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[20] = bad
        assert "job 1: a value of the matrix is not finite" in call((12, 4, 3, -1, 10, 20), data=xb)
        tb = tr.copy()
        tb["centre_target"][4, 1] = bad
        assert "job 1: a transform is not finite" in call((12, 4, 3, 1, 10, 20), rows=tb)
        tb = tr.copy()
        tb["rotation"][0, 2, 2] = bad
        assert "job 0: a transform is not finite" in call((12, 4, 3, 1, 10, 20), rows=tb)
    # a value no job reads, and the fields of a transform the entries do not read, may hold anything
    xb = x.copy()
    xb[59] = np.nan
    assert C.run(host, [(xb[:12].reshape(4, 3), tr[:4], True)])[0][0][1].shape == (3, 3)


def test_every_refusal_of_a_projection(host):
    from pywindow_amd import _lib

    rng = np.random.default_rng(10)
    x, m, v = rng.standard_normal(60), rng.standard_normal(8), rng.standard_normal(24)
    tr = C.transforms(rng, 5)
    good = (0, 4, 3, 0, 0, 0, 2, 0)             # T = 4, D = 3, k = 2: vectors 0 .. 5, projections 0 .. 7

    def call(job, data=x, mean=m, vec=v, rows=tr, n_proj=40):
        proj = C.sentinel(n_proj)
        rec = np.array([good, job], dtype=np.int64).view(_lib.PROJECT_JOB_DTYPE).reshape(-1)
        with pytest.raises(ValueError) as err:
            host.project(rec, data, mean, vec, rows, proj=proj)
        assert C.untouched(proj).all()
        return str(err.value)

    assert "job 1: k < 1" in call((12, 4, 3, -1, 3, 6, 0, 8))
    assert "job 1: T < 1" in call((12, 0, 3, -1, 3, 6, 2, 8))
    assert "job 1: D < 1" in call((12, 4, -3, -1, 3, 6, 2, 8))
    assert "job 1: D is not a multiple of 3" in call((12, 4, 4, 0, 3, 6, 2, 8))
    assert "job 1: a matrix outside data" in call((52, 4, 3, -1, 3, 6, 2, 8))
    assert "job 1: a mean outside" in call((12, 4, 3, -1, 6, 6, 2, 8))
    assert "job 1: vectors outside" in call((12, 4, 3, -1, 3, 20, 2, 8))
    assert "job 1: projections outside" in call((12, 4, 3, -1, 3, 6, 2, 33))
    assert "job 1: shares entries of the projections" in call((12, 4, 3, -1, 3, 6, 2, 7))
    vb = v.copy()
    vb[7] = np.inf
    assert "job 1: a value of the vectors is not finite" in call((12, 4, 3, -1, 3, 6, 2, 8), vec=vb)
    mb = m.copy()
    mb[1] = np.nan
    assert "job 0: a value of the mean is not finite" in call((12, 4, 3, -1, 3, 6, 2, 8), mean=mb)
    xb = x.copy()
    xb[13] = np.nan
    assert "job 1: a value of the matrix is not finite" in call((12, 4, 3, -1, 3, 6, 2, 8), data=xb)


def test_the_public_functions():
    import pywindow_amd as pw

    _, X, tr, _ = C.case("T=257 D=129 moved")
    host = pw._lib.Context(-1)
    mean, S = pw.covariance(X, tr, device=-1)
    (m, s), = C.run(host, [(X, tr, True)])[0]
    assert S.shape == (129, 129) and C.same(mean, m) and C.same(S, s)
    assert pw.covariance(X, tr, device=-1, scatter=False)[1] is None
    V = C.vectors("T=257 D=129 moved", 3)
    P = pw.project(X, mean, V, tr, device=-1)
    assert P.shape == (257, 3) and C.same(P, C.project(host, X, tr, mean, V))
    assert pw.project(X, mean, V[0], tr, device=-1).shape == (257, 1)
    for bad in (lambda: pw.covariance(X[0], device=-1), lambda: pw.covariance(X, tr[:5], device=-1),
                lambda: pw.project(X, mean[:5], V, device=-1), lambda: pw.project(X, mean, V[:, :7], device=-1),
                lambda: pw.covariance(np.full((3, 3), np.nan), device=-1)):
        with pytest.raises(ValueError):
            bad()
