"""What the Python wrappers of the nine statistical entries (``Context.kde_sums`` ... ``Context.cluster_gromos``) check
before they call the library, through the helpers they share (``_lib._span_inside``, ``_writes_from_start``,
``_stat_call``): an input span that ends one entry past its array and a result that starts at -1, each with the
exception type and the message the wrappers have raised since they were written one by one.  Host path, arrays of a
dozen entries."""
import numpy as np
import pytest

from pywindow_amd import _lib

N = 12
X = np.linspace(-1.0, 1.0, N)


def job(dtype, **fields):
    rec = np.zeros(1, dtype=dtype)
    for name, value in fields.items():
        rec[name] = value
    return rec


def kde(ctx, **f):
    return ctx.kde_sums(job(_lib.KDE_JOB_DTYPE, **{"n_samples": N, "n_points": N, "inv_bandwidth": 1.0, **f}), X, X)


def kde2(ctx, **f):
    xy = np.stack([X, X], axis=1)
    return ctx.kde2_sums(job(_lib.KDE2_JOB_DTYPE, **{"n_samples": N, "n_points": N, "w00": 1.0, "w11": 1.0, **f}), xy, xy)


def kdew(ctx, **f):
    return ctx.kde_wsums(job(_lib.KDEW_JOB_DTYPE, **{"n_samples": N, "n_points": N, "n_replicas": 1, "inv_bandwidth": 1.0, **f}),
                         X, X, np.ones(N))


def corr(ctx, **f):
    return ctx.corr_sums(job(_lib.CORR_JOB_DTYPE, **{"n": N, "n_lags": 2, **f}), X)


def dft(ctx, **f):
    return ctx.dft_sums(job(_lib.DFT_JOB_DTYPE, **{"n": N, "period": N, "j_step": 1, "n_freq": 2, **f}), X)


def gate(ctx, **f):
    return ctx.gate_counts(job(_lib.GATE_JOB_DTYPE, **{"n": N, "n_thr": N, **f}), X, X)


def trans(ctx, **f):
    return ctx.trans_counts(job(_lib.TRANS_JOB_DTYPE, **{"n": N, "n_edges": 1, "lag_first": 1, "lag_step": 1, "n_lags": 2, **f}),
                            X, X, 2)


def superpose(ctx, **f):
    xyz = np.arange(3.0 * N).reshape(N, 3) ** 2
    return ctx.superpose(job(_lib.SUPERPOSE_JOB_DTYPE, **{"weight_first": -1, "n": N - 1, "target_first": 1, **f}), xyz)


def cluster(ctx, **f):
    return ctx.cluster_gromos(job(_lib.CLUSTER_JOB_DTYPE, **{"n": 3, "cutoff": 0.5, **f}), np.abs(X[:9]))


OUTSIDE = "a job reaches outside `%s`"
BEFORE = "a job writes before the start of the %s"
CASES = [
    (kde, {"n_samples": N + 1}, IndexError, OUTSIDE % "samples"),
    (kde, {"point_first": 1}, IndexError, OUTSIDE % "points"),
    (kde2, {"n_samples": N + 1}, IndexError, OUTSIDE % "samples"),
    (kde2, {"point_first": 1}, IndexError, OUTSIDE % "points"),
    (kdew, {"n_samples": N + 1}, IndexError, OUTSIDE % "samples"),
    (kdew, {"weight_first": 1}, IndexError, OUTSIDE % "weights"),
    (kdew, {"out_first": -1}, IndexError, BEFORE % "sums"),
    (corr, {"b_first": 1}, IndexError, OUTSIDE % "series"),
    (corr, {"out_first": -1}, IndexError, BEFORE % "sums"),
    (dft, {"n": N + 1}, IndexError, OUTSIDE % "series"),
    (dft, {"out_first": -1}, IndexError, BEFORE % "sums"),
    (gate, {"d_first": 1}, IndexError, OUTSIDE % "thresholds"),
    (gate, {"out_first": -1}, IndexError, BEFORE % "counts"),
    (trans, {"n": N + 1}, IndexError, OUTSIDE % "series"),
    (trans, {"out_first": -1}, IndexError, BEFORE % "counts"),
    # (the span of a superposition is checked by the library: PW_E_BAD_ARG, the library's message)
    (superpose, {"n": N}, ValueError, "pw_superpose: job 0: points outside xyz"),
    (superpose, {"out": -1}, ValueError, BEFORE % "result"),
    (cluster, {"d_first": 1}, IndexError, OUTSIDE % "dist"),
    (cluster, {"out_first": -1}, IndexError, BEFORE % "results"),
]


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=1)


@pytest.mark.parametrize("call", [kde, kde2, kdew, corr, dft, gate, trans, superpose, cluster], ids=lambda c: c.__name__)
def test_the_jobs_of_the_cases_are_accepted_as_they_stand(host, call):
    """(so that a case below is refused for its one changed field)"""
    call(host)


@pytest.mark.parametrize("call, fields, error, message", CASES, ids=[f"{c[0].__name__}-{'-'.join(c[1])}" for c in CASES])
def test_a_span_past_its_array_and_a_result_before_its_start(host, call, fields, error, message):
    with pytest.raises(error) as caught:
        call(host, **fields)
    assert type(caught.value) is error and str(caught.value) == message
