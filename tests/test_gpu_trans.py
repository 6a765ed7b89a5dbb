"""Lagged state-transition counts on the device: pw_trans_counts on gfx950 against the host path (device = -1) and
against the definition (tests/_trans_cases.py: reference), EXACTLY -- every output is an integer and sums of integers do
not depend on the order of the work, so neither the launch, the atomics at the end of a work item nor how the jobs are
cut into launches to bound the masks may show.  numpy only; tests/test_trans.py holds the host path to the definition."""
import numpy as np
import pytest

import _stat_edges as S
import _trans_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def same(got, want):
    return got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("n_states", sorted(C.groups()))
def test_the_case_list(hip_ctx, host, n_states):
    """The case list of tests/test_trans.py: device == host path == definition, job by job and as one batch."""
    cases = C.groups()[n_states]
    for name, a, edges, grid in cases:
        packed = C.pack([(a, edges, grid)])
        got = hip_ctx.trans_counts(*packed, n_states)
        assert same(got, C.reference_rows([(a, edges, grid)], n_states)), name
        assert same(got, host.trans_counts(*packed, n_states)), name
    jobs = [c[1:] for c in cases]
    packed = C.pack(jobs)
    got = hip_ctx.trans_counts(*packed, n_states)
    assert same(got, C.reference_rows(jobs, n_states)) and same(got, host.trans_counts(*packed, n_states)) and got.sum() > 0
    assert same(got, hip_ctx.trans_counts(*packed, n_states))                    # two consecutive device calls


@pytest.mark.parametrize("n_states", (2, 3, 16))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host, n_states):
    """Through pw_internal_trans_counts at workspaces of 1 B (every job a launch of its own), 100 kB and the default,
    with the masks and the compact result filled with 0xFF before the first kernel, right after a call of other shapes
    and values: the same integers, and rows nobody owns untouched."""
    jobs = [c[1:] for c in C.groups()[n_states]]
    rec, series, edges = C.pack(jobs, hole=1)
    want = C.raw_counts(host, rec, series, edges, n_states)[1]
    owned = want[:, 0, 0] != C.SENTINEL
    assert (~owned).sum() >= len(jobs) - 1 and same(want[owned], C.reference_rows(jobs, n_states))
    other, other_states = C.call_cases()
    for budget in (1, 100_000, 0):
        for poison in (False, True):
            hip_ctx.trans_counts(*C.pack(other), other_states)
            S.set_poison(poison)
            rc, counts = C.raw_counts(hip_ctx, rec, series, edges, n_states, workspace_bytes=budget)
            S.set_poison(False)
            assert rc == 0 and same(counts, want), (budget, poison)


def test_call_cases_and_rows_nobody_owns(hip_ctx, host):
    jobs, n_states = C.call_cases()
    rec, series, edges = C.pack(jobs, hole=2)
    rc, counts = C.raw_counts(hip_ctx, rec, series, edges, n_states)
    want = C.raw_counts(host, rec, series, edges, n_states)[1]
    assert rc == 0 and same(counts, want) and (counts == C.SENTINEL).all(axis=(1, 2)).sum() == 6
    assert same(counts[(counts != C.SENTINEL).any(axis=(1, 2))], C.reference_rows(jobs, n_states))


def test_bad_arguments_never_launch(hip_ctx):
    good = (np.arange(5.0), np.array([1.0, 2.0]), (0, 1, 3))
    x, e = np.arange(4.0), np.array([1.0])
    for job, n_states, what in (((np.array([1.0, np.inf, 2.0]), e, (0, 1, 2)), 3, "job 1: .*infinity"),
                                ((x, np.array([1.0, np.nan]), (0, 1, 2)), 3, "job 1: .*NaN or an infinity"),
                                ((x, np.array([2.0, 1.0]), (0, 1, 2)), 3, "job 1: .*increase strictly"),
                                ((x, np.array([1.0, 2.0, 3.0]), (0, 1, 2)), 3, "job 1: .*n_edges >= n_states"),
                                ((x, e, (0, 0, 2)), 3, "job 1: .*lag_step < 1"),
                                ((x, e, (0, 1, 2)), 17, r"job \d+: .*n_states outside")):
        rec, series, edges = C.pack([good, job])
        with pytest.raises(ValueError, match=what):
            hip_ctx.trans_counts(rec, series, edges, n_states)
        rc, counts = C.raw_counts(hip_ctx, rec, series, edges, n_states, np.full((5, 16, 16), C.SENTINEL, dtype=np.int64))
        assert rc == -2 and (counts == C.SENTINEL).all()


def test_the_public_route_per_molecule(hip_ctx):
    """One per_molecule batch of 8 series x 3000 frames x 600 lags over a synthetic modular store."""
    from pywindow_amd import _lib, records

    rng = np.random.default_rng(8)
    T, M = 3000, 8
    recs = np.zeros(T * M, dtype=_lib.UNIT_OUT_DTYPE)
    walk = np.cumsum(rng.standard_normal((T, M)) * 0.05, axis=0) + 3.3
    n_win = 4
    recs["n_windows"] = n_win
    recs["win_d"][:, :n_win] = walk.reshape(-1, 1) + 0.2 * rng.standard_normal((T * M, n_win))
    frame = np.repeat(np.arange(T), M)
    keep = rng.random(T * M) > 0.03                                              # absent frames: gaps
    keep[:M] = keep[-M:] = True
    store = records.RecordStore(recs[keep], frame[keep], np.tile(np.arange(M), T)[keep], stages=_lib.STAGE_WINDOWS)
    dev = store.kinetics("windows_open", max_lag=599, per_molecule=True, guest=3.3, device=0)
    ref = store.kinetics("windows_open", max_lag=599, per_molecule=True, guest=3.3, device=-1)
    assert sorted(dev) == sorted(ref) == list(range(M))
    for m in range(M):
        assert dev[m].counts.shape == (600, 5, 5) and same(dev[m].counts, ref[m].counts)
        assert dev[m].timescales.tobytes() == ref[m].timescales.tobytes() and dev[m].counts[1].sum() > 2000
    _, a, ok = store.series("windows_open", 3, guest=3.3)
    assert same(dev[3].counts[:40], C.reference(np.where(ok, a, np.nan), dev[3].edges, np.arange(40), 5))
    assert dev[0].counts.tobytes() != dev[1].counts.tobytes()
