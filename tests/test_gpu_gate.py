"""Gating statistics on the device: pw_gate_counts on gfx950 against the host path (device = -1) and against the
definition (tests/_gate_cases.py: reference), EXACTLY -- every output is an integer, sums and maxima of integers do not
depend on the order of the work, so neither the launch, the atomics of the chunk kernel nor how the thresholds are cut
into slabs to bound the workspace may show.  numpy only; tests/test_gate.py holds the host path to the definition."""
import numpy as np
import pytest

import _gate_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def same(got, want):
    return all(g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("n_bins", C.EDGE_BINS)
def test_the_edge_grid(hip_ctx, host, n_bins):
    """n around the chunk x n_thr around the 64 lanes of a wavefront and the tile of 256, about 10 % gaps."""
    jobs = C.edge_grid()
    packed = C.pack(jobs)
    got = hip_ctx.gate_counts(*packed, n_bins)
    assert same(got, host.gate_counts(*packed, n_bins)) and got[0][:, :2].sum() > 0
    assert same(got, hip_ctx.gate_counts(*packed, n_bins))                       # two consecutive device calls
    for job in jobs:                                                             # one job at a time
        alone = C.pack([job])
        assert same(hip_ctx.gate_counts(*alone, n_bins), host.gate_counts(*alone, n_bins)), (len(job[0]), len(job[1]))


def test_small_cases_against_the_definition(hip_ctx, host):
    """Runs against the edges of a chunk, degenerate series, exact thresholds, the overflow bin."""
    cases = C.small_cases()
    for name, a, thr, n_bins in cases:
        packed = C.pack([(a, thr)])
        got = hip_ctx.gate_counts(*packed, n_bins)
        assert same(got, C.reference_rows([(a, thr)], n_bins)), name
        assert same(got, host.gate_counts(*packed, n_bins)), name
    for n_bins in (0, 4, 7):                                                     # ... and as one batch
        jobs = [(a, thr) for _, a, thr, _ in cases]
        got = hip_ctx.gate_counts(*C.pack(jobs), n_bins)
        assert same(got, C.reference_rows(jobs, n_bins)) and same(got, hip_ctx.gate_counts(*C.pack(jobs), n_bins))


def test_thresholds_are_compared_exactly(hip_ctx):
    (_, a, thr), (_, zeros, zthr) = C.exactness_cases()
    counts, _ = hip_ctx.gate_counts(*C.pack([(a, thr)]), 0)
    for v in np.unique(a):
        at, above = np.flatnonzero(thr == v), np.flatnonzero(thr == np.nextafter(v, np.inf))
        assert (counts[at, 0] == (a >= v).sum()).all() and (counts[above, 0] == (a > v).sum()).all()
    for d in np.unique(thr):
        rows = counts[thr == d]
        assert (rows == rows[0]).all()
    counts, _ = hip_ctx.gate_counts(*C.pack([(zeros, zthr)]), 0)
    assert np.array_equal(counts[0], counts[1]) and counts[0, 0] == 7 and counts[2, 0] == 1 and counts[3, 0] == 7


def test_batch_layout_and_rows_nobody_owns(hip_ctx, host):
    jobs = C.mixed_batch()
    rec, series, thr = C.pack(jobs, hole=2)
    live = (rec["n"] > 0) & (rec["n_thr"] > 0)
    owned = np.zeros(int((rec["out_first"] + rec["n_thr"])[live].max()), dtype=bool)
    for r in rec[live]:
        owned[r["out_first"]:r["out_first"] + r["n_thr"]] = True
    for n_bins in (0, 5):
        rc, counts, hist = C.raw_counts(hip_ctx, rec, series, thr, n_bins)
        want = C.raw_counts(host, rec, series, thr, n_bins)
        assert rc == 0 and same((counts, hist), want[1:])
        assert (~owned).sum() >= 96 and (counts[~owned] == C.SENTINEL).all() and (hist[~owned] == C.SENTINEL).all()
        assert same((counts[owned], hist[owned]), C.reference_rows([j for j in jobs if len(j[0]) and len(j[1])], n_bins))
    got = hip_ctx.gate_counts(rec, series, thr, 5)
    assert same(got, hip_ctx.gate_counts(rec, series, thr, 5))
    for budget in (1, 100_000, 0):
        zeros = (np.zeros_like(got[0]), np.zeros_like(got[1]))
        assert same(C.raw_counts(hip_ctx, rec, series, thr, 5, *zeros, workspace_bytes=budget)[1:], got), budget
    for job in jobs:                                                             # one job at a time
        if len(job[0]) and len(job[1]):
            alone = C.pack([job])
            assert same(hip_ctx.gate_counts(*alone, 5), host.gate_counts(*alone, 5))


def test_one_long_job_and_the_workspace_bound(hip_ctx, host):
    """200 000 entries x 2048 thresholds: 4.1e8 steps, 391 chunks.  The summaries are 391 x 2048 x 4 B = 3.2 MB; with the
    budget forced to 1 B and 100 kB the thresholds go through one tile of 256 a launch, and the counts are the same."""
    a, thr = C.long_job()
    packed = C.pack([(a, thr)])
    want = host.gate_counts(*packed, 64)
    got = hip_ctx.gate_counts(*packed, 64)
    assert same(got, want) and got[0][:, 8].max() > 100 and got[1].sum() == got[0][:, 8:10].sum()
    for budget in (1, 100_000, 0):
        rc, counts, hist = C.raw_counts(hip_ctx, *packed, 64, workspace_bytes=budget)
        assert rc == 0 and same((counts, hist), want), budget


def test_identities_on_random_input(hip_ctx):
    rng = np.random.default_rng(12)
    a = C.smooth_noise(20_000, 12, gaps=0.02)
    thr = np.sort(rng.uniform(np.nanmin(a), np.nanmax(a), 300))
    counts, hist = hip_ctx.gate_counts(*C.pack([(a, thr)]), 1024)
    assert (counts[:, 0] + counts[:, 1] == (~np.isnan(a)).sum()).all()
    assert np.array_equal(hist.sum(axis=2), counts[:, 8:10])
    assert counts[:, 4:6].max() < 1024
    assert np.array_equal((hist * np.arange(1, 1025)).sum(axis=2), counts[:, 10:12])
    assert (counts[:, 8] <= np.minimum(counts[:, 6], counts[:, 7] + 1)).all()
    assert (counts[:, 9] <= np.minimum(counts[:, 7], counts[:, 6] + 1)).all()
    assert (np.diff(counts[:, 0]) <= 0).all() and counts[0, 0] > counts[-1, 0]
    assert (counts[:, 2:4] >= counts[:, 6:8]).all() and (counts[:, 6:8] >= counts[:, 8:10]).all()


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    good = (np.arange(5.0), np.array([1.0, 2.0]))
    x = np.arange(3.0)
    for bad, n_bins, what in (((np.array([1.0, np.inf, 2.0]), np.array([1.0])), 3, "job 1: .*infinity"),
                              ((x, np.array([1.0, np.nan])), 3, "job 1: .*threshold is a NaN"),
                              ((x, np.array([1.0])), -1, r"job \d+: .*n_bins is negative")):
        rec, series, thr = C.pack([good, bad])
        with pytest.raises(ValueError, match=what):
            hip_ctx.gate_counts(rec, series, thr, n_bins)
        rc, counts, hist = C.raw_counts(hip_ctx, rec, series, thr, n_bins)
        assert rc == -2 and (counts == C.SENTINEL).all() and (hist == C.SENTINEL).all()
    rec, series, thr = C.pack([good, (x, np.array([1.0]))])
    rc, counts, _ = C.raw_counts(hip_ctx, rec, series, thr, 3, hist=None)        # hist missing with n_bins > 0
    assert rc == -2 and (counts == C.SENTINEL).all() and b"job 0: hist is null" in _lib.load().pw_last_error()


def same_gating(a, b):
    import dataclasses

    for f in (x.name for x in dataclasses.fields(a)):
        x, y = getattr(a, f), getattr(b, f)
        if f == "n_valid":
            if x != y:
                return False
        elif x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def test_the_public_route_per_molecule(hip_ctx):
    from pywindow_amd import records
    from test_kde import golden_store

    g = golden_store().records
    recs = np.concatenate([g, g[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    store = records.RecordStore(recs[by], pos[by], np.tile([0, 1], 20))
    dev = store.gating("windows_max", per_molecule=True, device=0)
    ref = store.gating("windows_max", per_molecule=True, device=-1)
    assert sorted(dev) == sorted(ref) == [0, 1]
    for m in (0, 1):
        assert same_gating(dev[m], ref[m]) and dev[m].counts.shape == (200, 12) and dev[m].open_lengths.shape == (200, 64)
    assert dev[0].counts[:, 6].max() > 0 and dev[0].counts.tobytes() != dev[1].counts.tobytes()
    for m in (0, 1):
        _, p, ok = store.series("pore_diameter_opt", m)
        thr = [float(np.median(p[ok])), float(p[ok].max()), float(p[ok].min()), 0.0]
        got = store.gating("pore_diameter_opt", thresholds=thr, molecule=m, n_bins=8, device=0)
        want = [C.reference(np.where(ok, p, np.nan), d, 8) for d in thr]
        assert np.array_equal(got.counts, np.array([w[0] for w in want])) and got.counts[0, 6] > 0
        assert np.array_equal(got.open_lengths, np.array([w[1][0] for w in want]))
        assert np.array_equal(got.closed_lengths, np.array([w[1][1] for w in want]))
    with pytest.raises(ValueError, match="molecule="):
        store.gating("windows_max", device=0)
    single = records.RecordStore(g, np.arange(20))
    with pytest.raises(ValueError, match="per_molecule needs a modular"):
        single.gating("windows_max", per_molecule=True, device=0)
