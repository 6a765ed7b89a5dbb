"""Lagged state-transition counts on the host path (device = -1): pw_trans_counts against the definition
(tests/_trans_cases.py: reference, plain numpy) EXACTLY -- every output is an integer --, the refusals, the Kinetics
identities, a Markov chain with known rates, and the public routes over a store.  numpy only; tests/test_gpu_trans.py
holds the device to the host path and to the definition."""
import numpy as np
import pytest

import _trans_cases as C
from pywindow_amd import DLPOLY, _lib, gating, kinetics, records, synth


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=4)


def same(got, want):
    return got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("n_states", sorted(C.groups()))
def test_the_case_list_against_the_definition(host, n_states):
    """n around a word, a pack wave and a chunk, lags 0 .. 33 and n - 1 .. n + 5, lag steps inside and beyond the LDS
    window, n_lags around the tile, every padded state count, exact values, gaps at word and chunk boundaries."""
    cases = C.groups()[n_states]
    for name, a, edges, grid in cases:
        got = host.trans_counts(*C.pack([(a, edges, grid)]), n_states)
        assert same(got, C.reference_rows([(a, edges, grid)], n_states)), name
    jobs = [c[1:] for c in cases]                                                # ... and as one batch
    got = host.trans_counts(*C.pack(jobs), n_states)
    assert same(got, C.reference_rows(jobs, n_states)) and got.sum() > 0


def test_values_at_an_edge_are_in_the_upper_state(host):
    zeros = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0])
    for edge in (0.0, -0.0):
        got = host.trans_counts(*C.pack([(zeros, np.array([edge]), (0, 1, 1))]), 2)
        assert got[0].tolist() == [[1, 0], [0, 7]]
    tiny = np.array([5e-324, 0.0, -5e-324, 5e-324])
    got = host.trans_counts(*C.pack([(tiny, np.array([5e-324]), (0, 1, 2))]), 2)
    assert got[0].tolist() == [[2, 0], [0, 2]] and got[1].tolist() == [[1, 1], [1, 0]]


def test_batch_layout_rows_nobody_owns_threads_and_workspace(host):
    jobs, S = C.call_cases()
    rec, series, edges = C.pack(jobs, hole=2)
    live = (rec["n"] > 0) & (rec["n_lags"] > 0)
    assert live.sum() == 3 and not live[2] and not live[3]
    owned = np.zeros(int((rec["out_first"] + rec["n_lags"])[live].max()), dtype=bool)
    for r in rec[live]:
        owned[r["out_first"]:r["out_first"] + r["n_lags"]] = True
    rc, counts = C.raw_counts(host, rec, series, edges, S)
    assert rc == 0 and (~owned).sum() == 6 and (counts[~owned] == C.SENTINEL).all()
    assert same(counts[owned], C.reference_rows(jobs, S))
    # the two jobs that share a series differ by their edges only; states the edges cannot reach are zeros
    first = counts[owned][:300]
    assert first[0].trace() == (~np.isnan(jobs[0][0])).sum() and (counts[owned][300:400, 2:, :] == 0).all()
    # lags at and beyond n: rows of zeros, written
    assert (counts[owned][400 + 10:] == 0).all() and counts[owned][400 + 9].sum() <= 1
    got = host.trans_counts(rec, series, edges, S)
    for threads in (1, 3, 16):
        assert same(_lib.Context(-1, host_threads=threads).trans_counts(rec, series, edges, S), got)
    for budget in (1, 100_000, 0):
        assert same(C.raw_counts(host, rec, series, edges, S, np.zeros_like(got), workspace_bytes=budget)[1], got)


def test_refused_input_writes_nothing(host):
    good = (np.arange(5.0), np.array([1.0, 2.0]), (0, 1, 3))
    x = np.arange(4.0)
    e = np.array([1.0])
    bad = [((np.array([1.0, np.inf, 2.0]), e, (0, 1, 2)), 3, "job 1: .*infinity"),
           ((np.array([1.0, -np.inf]), e, (0, 1, 2)), 3, "job 1: .*infinity"),
           ((x, np.array([1.0, np.nan]), (0, 1, 2)), 3, "job 1: .*NaN or an infinity"),
           ((x, np.array([1.0, np.inf]), (0, 1, 2)), 3, "job 1: .*NaN or an infinity"),
           ((x, np.array([1.0, 1.0]), (0, 1, 2)), 3, "job 1: .*increase strictly"),
           ((x, np.array([2.0, 1.0]), (0, 1, 2)), 3, "job 1: .*increase strictly"),
           ((x, np.array([1.0, 2.0, 3.0]), (0, 1, 2)), 3, "job 1: .*n_edges >= n_states"),
           ((x, e, (0, 0, 2)), 3, "job 1: .*lag_step < 1"),
           ((x, e, (-1, 1, 2)), 3, "job 1: .*negative"),
           ((x, e, (0, 1, -2)), 3, "job 1: .*negative"),
           ((x, e, (0, 1, 2)), 0, r"job \d+: .*n_states outside"),
           ((x, e, (0, 1, 2)), 17, r"job \d+: .*n_states outside")]
    for job, S, what in bad:
        rec, series, edges = C.pack([good, job])
        if rec["n_lags"][1] < 0:
            rec["out_first"][1] = 3
        with pytest.raises(ValueError, match=what):
            host.trans_counts(rec, series, edges, S)
        counts = np.full((8, 16, 16), C.SENTINEL, dtype=np.int64)
        rc, counts = C.raw_counts(host, rec, series, edges, S, counts)
        assert rc == -2 and (counts == C.SENTINEL).all(), what
    rec, series, edges = C.pack([good])
    rec["n"][0] = -1
    assert C.raw_counts(host, rec, series, edges, 3, np.zeros((3, 3, 3), np.int64))[0] == -2
    # the Python layer
    a = np.arange(6.0)
    for edges, what in (([1.0, np.nan], "NaN or infinite"), ([1.0, np.inf], "NaN or infinite"), ([1.0, 1.0], "strictly"),
                        ([2.0, 1.0], "strictly"), (np.arange(16.0), "at most 15")):
        with pytest.raises(ValueError, match=what):
            kinetics.transition_counts(a, edges, 3, device=-1)
    with pytest.raises(ValueError, match="one flag per entry"):
        kinetics.transition_counts(a, [1.0], 3, valid=[True], device=-1)
    with pytest.raises(ValueError, match="no valid entry"):
        kinetics.transition_counts(a, [1.0], 3, valid=np.zeros(6, bool), device=-1)
    with pytest.raises(ValueError, match="valid entry is NaN or infinite"):
        kinetics.transition_counts([1.0, np.nan], [1.0], 1, device=-1)
    for lags in (-1, (0, 0, 3), (0, 1, 0), (-1, 1, 2), True, "x"):
        with pytest.raises(ValueError, match="lags"):
            kinetics.transition_counts(a, [1.0], lags, device=-1)
    with pytest.raises(ValueError, match="one stride"):
        kinetics.transition_counts_batch([(a, [1.0], None)], 2, stride=[1, 2], device=-1)
    assert kinetics.transition_counts_batch([], 3, device=-1) == []


def test_kinetics_identities_and_the_lag_grid():
    a = C.noise(5000, 31, gaps=0.05)
    ok = ~np.isnan(a)
    edges = [-0.5, 0.2, 0.9]
    k = kinetics.transition_counts(np.where(ok, a, 0.0), edges, 40, valid=ok, stride=3, device=-1)
    assert k.counts.shape == (41, 4, 4) and k.counts.dtype == np.int64 and k.lag.tolist() == (3 * np.arange(41)).tolist()
    assert np.array_equal(k.counts, C.reference(a, edges, np.arange(41), 4))
    assert np.array_equal(k.counts.sum(axis=(1, 2)), k.n_pairs)
    pop = np.bincount(np.searchsorted(edges, a[ok], side="right"), minlength=4)
    assert np.array_equal(k.counts[0], np.diag(pop)) and k.n_pairs[0] == ok.sum()
    assert np.allclose(k.population.sum(axis=1), 1.0) and np.allclose(k.population[0], pop / ok.sum())
    assert np.allclose(k.transition.sum(axis=2), 1.0) and np.array_equal(k.transition[0], np.eye(4))
    assert k.timescales.shape == (41, 3) and np.isnan(k.timescales[0]).all() and np.isfinite(k.timescales[1]).any()
    some = kinetics.transition_counts(np.where(ok, a, 0.0), edges, (2, 5, 7), valid=ok, device=-1)
    assert some.lag.tolist() == [2, 7, 12, 17, 22, 27, 32] and np.array_equal(some.counts, k.counts[2:33:5])
    # a state nobody starts from: its row of the transition matrix is nan, and so are the timescales
    none = kinetics.transition_counts([0.0, 0.0, 0.0, 0.0], [1.0], 2, device=-1)
    assert np.isnan(none.transition[:, 1]).all() and np.isnan(none.timescales).all() and none.population[1].tolist() == [1.0, 0.0]
    # one state: no edges, no timescales
    one = kinetics.transition_counts(a[ok], [], 3, device=-1)
    assert one.counts.shape == (4, 1, 1) and one.timescales.shape == (4, 0) and one.counts[:, 0, 0].tolist() == [ok.sum() - i for i in range(4)]
    # a batch gives what the single calls give, each item with its own number of states
    both = kinetics.transition_counts_batch([(np.where(ok, a, 0.0), edges, ok), (a[ok], [], None)], [40, 3], [3, 1], device=-1)
    assert np.array_equal(both[0].counts, k.counts) and np.array_equal(both[1].counts, one.counts)
    assert both[0].timescales.tobytes() == k.timescales.tobytes()


def test_two_states_give_the_openings_and_closings_of_gating():
    a = C.noise(4000, 33, gaps=0.08)
    ok = ~np.isnan(a)
    for d in (-0.3, 0.0, 0.7):
        g = gating.gate_statistics(np.where(ok, a, 0.0), [d], valid=ok, device=-1)
        k = kinetics.transition_counts(np.where(ok, a, 0.0), [d], 1, valid=ok, device=-1)
        names = list(_lib.GATE_FIELDS)
        assert k.counts[1][0][1] == g.counts[0, names.index("openings")] > 0
        assert k.counts[1][1][0] == g.counts[0, names.index("closings")] > 0
        assert k.counts[0][1][1] == g.counts[0, names.index("n_open")]


def test_a_markov_chain_with_known_rates():
    """A two-state chain, p01 = 0.05, p10 = 0.08, 200 000 steps.  The bound: transition[k][i][j] is a binomial share of
    N_i = the pairs that start in i, standard deviation sqrt(p (1 - p) / N_i) with p the exact T^k[i][j]; six of them.
    Pairs of one trajectory are not independent, so the spread is somewhat more than binomial: the numpy reference was
    checked here against the same bound before the seed was fixed (seed 1: 1.1 standard deviations at the worst over
    k <= 20; seed 2: 4.7), and is asserted to stay inside too."""
    p01, p10, n = 0.05, 0.08, 200_000
    s = C.markov_chain(n, p01, p10, seed=1)
    T = np.array([[1.0 - p01, p01], [p10, 1.0 - p10]])
    k = kinetics.transition_counts(s, [0.5], 20, device=-1)
    ref = C.reference(s, [0.5], np.arange(21), 2)
    assert np.array_equal(k.counts, ref)
    exact = -1.0 / np.log(1.0 - p01 - p10)
    for lag in range(1, 21):
        Tk = np.linalg.matrix_power(T, lag)
        N = k.counts[lag].sum(axis=1)
        bound = 6.0 * np.sqrt(Tk * (1.0 - Tk) / N[:, None])
        assert (np.abs(k.transition[lag] - Tk) <= bound).all(), lag
        assert (np.abs(ref[lag] / ref[lag].sum(axis=1)[:, None] - Tk) <= bound).all(), lag
        # the second eigenvalue of a 2 x 2 stochastic matrix is 1 - T01 - T10: within bound01 + bound10 of its exact value
        lam, slack = (1.0 - p01 - p10) ** lag, bound[0, 1] + bound[1, 0]
        assert 0.0 < lam - slack and lam + slack < 1.0
        lo, hi = -lag / np.log(lam - slack), -lag / np.log(lam + slack)
        assert lo <= k.timescales[lag, 0] <= hi and lo < exact < hi, (lag, lo, k.timescales[lag, 0], hi)


def test_ck_error_of_exact_powers_is_zero_to_rounding():
    T = np.array([[0.5, 0.25, 0.25], [0.125, 0.75, 0.125], [0.25, 0.25, 0.5]])
    scale = 2 ** 30
    lags = np.arange(0, 9)
    counts = np.array([np.round(np.linalg.matrix_power(T, int(m)) * scale).astype(np.int64) for m in lags])
    assert all((c.sum(axis=1) == scale).all() for c in counts)                  # (dyadic entries: the powers are exact)
    k = kinetics.Kinetics.from_counts([0.0, 1.0], 2 * lags, counts)
    multiples, error = k.ck_error(2)
    assert multiples.tolist() == [2, 4, 6, 8, 10, 12, 14, 16] and error.max() < 1e-15
    multiples, error = k.ck_error(4)
    assert multiples.tolist() == [4, 8, 12, 16] and error.max() < 1e-15
    off = kinetics.Kinetics.from_counts([0.0, 1.0], 2 * lags, counts[::-1].copy())
    assert off.ck_error(2)[1].max() > 0.1
    for base in (3, 0, 32, 10):
        with pytest.raises(ValueError):
            k.ck_error(base)


def test_record_store_kinetics_and_windows_open(tmp_path):
    path = synth.write_synthetic_history(tmp_path / "HISTORY", 20)
    traj = DLPOLY(path)
    order = [7, 2, 3] + [f for f in range(19, -1, -1) if f not in (7, 2, 3)]
    traj.analysis(frames=order, device=-1)
    store = traj.analysis_store
    recs = store.records
    assert (recs["n_windows"] <= _lib.W_MAX).all() and len(store.extra) == 0
    d_all = np.concatenate([r["win_d"][:r["n_windows"]] for r in recs])
    guest = float(np.median(d_all))
    frames, a, ok = store.series("windows_open", guest=guest)
    direct = np.array([(r["win_d"][:max(int(r["n_windows"]), 0)] >= guest).sum() for r in recs], dtype=np.float64)
    assert ok.all() and np.array_equal(a[np.asarray(store.unit_frame) - frames[0]], direct) and 0 < a.max() and a.min() < a.max()
    got = traj.kinetics("windows_open", guest=guest, device=-1)
    top = int(a.max())
    assert got.edges.tolist() == (0.5 + np.arange(top)).tolist() and got.lag.tolist() == list(range(11))
    assert np.array_equal(got.counts, C.reference(a, got.edges, np.arange(11), top + 1))
    assert np.array_equal(got.counts[0], np.diag(np.bincount(a.astype(int), minlength=top + 1)))
    # another quantity needs its edges; max_lag and lag_step are in samples
    _, p, pok = store.series("pore_diameter_opt")
    e = [float(np.median(p[pok]))]
    some = store.kinetics("pore_diameter_opt", edges=e, max_lag=9, lag_step=3, device=-1)
    assert some.lag.tolist() == [0, 3, 6, 9] and np.array_equal(some.counts, C.reference(np.where(pok, p, np.nan), e, [0, 3, 6, 9], 2))
    with pytest.raises(ValueError, match="edges"):
        store.kinetics("pore_diameter_opt", device=-1)
    with pytest.raises(ValueError, match="guest="):
        store.kinetics("windows_open", device=-1)
    with pytest.raises(ValueError, match="guest= belongs"):
        store.series("windows_max", guest=3.0)
    with pytest.raises(ValueError, match="modular"):
        store.kinetics("windows_max", edges=e, per_molecule=True, device=-1)
    # a modular store: two molecules a frame, frames 0, 2, 4, ...; all molecules in one call
    both = np.concatenate([store.records, store.records[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    modular = records.RecordStore(both[by], 2 * pos[by], np.tile([0, 1], 20))
    each = modular.kinetics("windows_open", guest=guest, per_molecule=True, device=-1)
    assert sorted(each) == [0, 1]
    for m in (0, 1):
        only = records.RecordStore(modular.records[m::2], modular.unit_frame[m::2])
        want = only.kinetics("windows_open", guest=guest, device=-1)
        assert np.array_equal(each[m].counts, want.counts) and each[m].lag.tolist() == (2 * np.arange(11)).tolist()
        assert np.array_equal(modular.kinetics("windows_open", guest=guest, molecule=m, device=-1).counts, want.counts)
    # every earlier call of series() is what it was
    assert store.series("n_windows")[1].tolist() == store.series("n_windows", None)[1].tolist()
