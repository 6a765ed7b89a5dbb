"""Gating statistics on the host path (device = -1): pw_gate_counts against the definition (tests/_gate_cases.py:
reference), exactly -- every output is an integer, so every comparison is np.array_equal on int64 and nothing is
left to a tolerance -- and the public functions on top of it.  The host path runs the chunk walk, the summaries and
the merge of csrc/pw_gate.hpp, the functions the gfx950 kernels run; tests/test_gpu_gate.py holds the device to it."""
import numpy as np
import pytest

import _gate_cases as C
from pywindow_amd import DLPOLY, _lib, gating, records, synth


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=4)


def same(got, want):
    return all(g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def test_the_constants_the_cases_are_built_on():
    assert (C.CHUNK, C.TILE, C.source_constant("GATE_FIELDS")) == (512, 256, C.FIELDS) and len(_lib.GATE_FIELDS) == C.FIELDS
    assert _lib.GATE_JOB_DTYPE.itemsize == 40


@pytest.mark.parametrize("n_bins", C.EDGE_BINS)
def test_the_edge_grid(host, n_bins):
    """n around the chunk x n_thr around the 64 lanes of a wavefront and the tile, about 10 % gaps."""
    jobs = C.edge_grid()
    assert len(jobs) == 64 and np.isnan(jobs[-1][0]).sum() > 100
    got = host.gate_counts(*C.pack(jobs), n_bins)
    assert same(got, C.reference_rows(jobs, n_bins)) and got[0][:, :2].sum() > 0
    for job in jobs[::9]:                                      # ... and alone
        assert same(host.gate_counts(*C.pack([job]), n_bins), C.reference_rows([job], n_bins))


@pytest.mark.parametrize("case", C.small_cases(), ids=lambda c: c[0] + f"-B{c[3]}")
def test_small_cases(host, case):
    name, a, thr, n_bins = case
    got = host.gate_counts(*C.pack([(a, thr)]), n_bins)
    assert same(got, C.reference_rows([(a, thr)], n_bins)), name


def test_what_the_patterns_are_there_for(host):
    """The cases do what their names say: spelled out by hand, not by the reference."""
    Cn, f = C.CHUNK, _lib.GATE_FIELDS.index
    by_name = {n: (a, t) for n, a, t in C.chunk_edge_cases() + C.degenerate_cases()}

    def row(name, q=0, n_bins=7):
        counts, hist = host.gate_counts(*C.pack([by_name[name]]), n_bins)
        return counts[q], hist[q]

    c, h = row("run-of-2C+3-from-C-2")                         # one complete open run across three boundaries
    assert c.tolist() == [2 * Cn + 3, Cn + 3, 1, 2, 2 * Cn + 3, Cn - 2, 1, 1, 1, 0, 2 * Cn + 3, 0] and h[0, 6] == 1 and h.sum() == 1
    c, h = row("run-of-2C+3-from-C-2-to-the-end")              # the same run against the end: censored
    assert c[f("open_runs")] == 1 and c[f("openings")] == 1 and c[f("complete_open_runs")] == 0 and h.sum() == 0
    c, h = row("censored-gap-left")                            # gap | open x C | closed x 2 | open: the long run is censored
    assert c[f("longest_open")] == Cn and c[f("complete_open_runs")] == 0 and c[f("complete_closed_runs")] == 1 and h[0].sum() == 0
    c, h = row("gap-at-C-1-and-C")                             # a gap cuts the open run in two censored ones
    assert c[f("open_runs")] == 2 and c[f("openings")] == 1 and c[f("closings")] == 1 and c[8:].sum() == 0
    c, h = row("all-gap")
    assert not c.any() and not h.any()
    c, h = row("alternating")                                  # 2C + 1 runs of one entry; the two at the ends are censored
    assert c.tolist() == [Cn + 1, Cn, Cn + 1, Cn, 1, 1, Cn, Cn, Cn - 1, Cn, Cn - 1, Cn] and h[:, 0].tolist() == [Cn - 1, Cn]
    c, h = row("one-valid-entry-between-gaps")
    assert c.tolist() == [1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and not h.any()
    c, h = row("run-exactly-[C-1,C]-swapped")                  # the same for closed runs
    assert c[f("complete_closed_runs")] == 1 and c[f("complete_closed_frames")] == 2 and c[f("closings")] == 1 and h[1, 1] == 1
    c, h = row("all-open", q=0)
    assert c[f("n_open")] == c[f("longest_open")] == 2 * Cn + 1 and c[f("open_runs")] == 1 and c[6:].sum() == 0


def test_thresholds_are_compared_exactly(host):
    (_, a, thr), (_, zeros, zthr) = C.exactness_cases()
    counts, _ = host.gate_counts(*C.pack([(a, thr)]), 0)
    for v in np.unique(a):
        at, above = np.flatnonzero(thr == v), np.flatnonzero(thr == np.nextafter(v, np.inf))
        assert len(at) and len(above)
        assert (counts[at, 0] == (a >= v).sum()).all() and (counts[above, 0] == (a > v).sum()).all()   # equal: open
    for d in np.unique(thr):                                   # equal thresholds, equal rows, wherever they stand
        rows = counts[thr == d]
        assert (rows == rows[0]).all()
    counts, _ = host.gate_counts(*C.pack([(zeros, zthr)]), 0)
    assert np.array_equal(counts[0], counts[1]) and counts[0, 0] == 7     # -0.0 against 0.0: open both ways
    assert counts[2, 0] == 1 and counts[3, 0] == 7


def test_histogram_overflow(host):
    a, thr, B = C.overflow_case()
    counts, hist = host.gate_counts(*C.pack([(a, thr)]), B)
    assert hist[0].tolist() == [[0, 0, 1, 2], [0, 0, 1, 2]] and counts[0, 8:].tolist() == [3, 3, 12, 12]
    assert same((counts, hist), C.reference_rows([(a, thr)], B))


def test_batch_layout_and_rows_nobody_owns(host):
    jobs = C.mixed_batch()
    rec, series, thr = C.pack(jobs, hole=2)
    assert len(series) < sum(len(a) for a, _ in jobs) and ((rec["n"] == 0) | (rec["n_thr"] == 0)).sum() >= 8
    for n_bins in (0, 5):
        rc, counts, hist = C.raw_counts(host, rec, series, thr, n_bins)
        want = C.reference_rows([j for j in jobs if len(j[0]) and len(j[1])], n_bins)
        owned = np.zeros(len(counts), dtype=bool)
        for r in rec[(rec["n"] > 0) & (rec["n_thr"] > 0)]:
            owned[r["out_first"]:r["out_first"] + r["n_thr"]] = True
        assert rc == 0 and same((counts[owned], hist[owned]), want)
        assert (~owned).sum() >= 2 * 48 and (counts[~owned] == C.SENTINEL).all() and (hist[~owned] == C.SENTINEL).all()
    # the threads of the host path and the budget of the workspace change nothing
    got = host.gate_counts(rec, series, thr, 5)
    for threads in (1, 3, 16):
        assert same(_lib.Context(-1, host_threads=threads).gate_counts(rec, series, thr, 5), got)
    for budget in (1, 100_000, 0):
        zeros = (np.zeros_like(got[0]), np.zeros_like(got[1]))
        assert same(C.raw_counts(host, rec, series, thr, 5, *zeros, workspace_bytes=budget)[1:], got)


def test_identities_on_random_input(host):
    rng = np.random.default_rng(12)
    a = C.smooth_noise(20_000, 12, gaps=0.02)
    thr = np.sort(rng.uniform(np.nanmin(a), np.nanmax(a), 300))
    counts, hist = host.gate_counts(*C.pack([(a, thr)]), 1024)
    n_valid = int((~np.isnan(a)).sum())
    assert (counts[:, 0] + counts[:, 1] == n_valid).all()
    assert np.array_equal(hist.sum(axis=2), counts[:, 8:10])
    assert counts[:, 4:6].max() < 1024                         # B beyond the longest run: the histogram holds every length
    assert np.array_equal((hist * np.arange(1, 1025)).sum(axis=2), counts[:, 10:12])
    assert (counts[:, 8] <= np.minimum(counts[:, 6], counts[:, 7] + 1)).all()
    assert (counts[:, 9] <= np.minimum(counts[:, 7], counts[:, 6] + 1)).all()
    assert (np.diff(counts[:, 0]) <= 0).all() and counts[0, 0] > counts[-1, 0]     # open_fraction falls with the threshold
    assert (counts[:, 2:4] >= counts[:, 6:8]).all() and (counts[:, 6:8] >= counts[:, 8:10]).all()


def test_bad_arguments_write_nothing(host):
    good = (np.arange(5.0), np.array([1.0, 2.0]))
    x = np.arange(3.0)
    for bad, n_bins, what in (((np.array([1.0, np.inf, 2.0]), np.array([1.0])), 3, "job 1: .*infinity"),
                              ((np.array([1.0, -np.inf, 2.0]), np.array([1.0])), 0, "job 1: .*infinity"),
                              ((x, np.array([1.0, np.nan])), 3, "job 1: .*threshold is a NaN"),
                              ((x, np.array([np.inf])), 3, "job 1: .*threshold is a NaN or an infinity"),
                              ((x, np.array([1.0])), -1, r"job \d+: .*n_bins is negative")):
        rec, series, thr = C.pack([good, bad])
        with pytest.raises(ValueError, match=what):
            host.gate_counts(rec, series, thr, n_bins)
        rc, counts, hist = C.raw_counts(host, rec, series, thr, n_bins)
        assert rc == -2 and (counts == C.SENTINEL).all() and (hist == C.SENTINEL).all()
        assert b"job " in _lib.load().pw_last_error()
    rec, series, thr = C.pack([good, (x, np.array([1.0]))])
    rc, counts, _ = C.raw_counts(host, rec, series, thr, 3, hist=None)           # hist missing with n_bins > 0
    assert rc == -2 and (counts == C.SENTINEL).all() and b"job 0: hist is null" in _lib.load().pw_last_error()
    rc, counts, _ = C.raw_counts(host, rec, series, thr, 0, hist=None)           # ... and fine without bins
    assert rc == 0 and counts[:, :2].sum(axis=1).tolist() == [5, 5, 3]
    for field, value, what in (("n", -1, "negative"), ("n", (1 << 31) + 1, "too long"), ("out_first", -1, "negative"),
                               ("d_first", -1, "negative"), ("n_thr", -2, "negative")):
        broken = rec.copy()
        broken[field][1] = value
        rc, counts, hist = C.raw_counts(host, broken, series, thr, 2, counts=np.full((4, 12), C.SENTINEL),
                                        hist=np.full((4, 2, 2), C.SENTINEL))
        assert rc == -2 and (counts == C.SENTINEL).all() and (hist == C.SENTINEL).all()
        assert b"job 1: " in _lib.load().pw_last_error() and what.encode() in _lib.load().pw_last_error()
    with pytest.raises(IndexError):
        host.gate_counts(rec, series[:4], thr)
    with pytest.raises(IndexError):
        host.gate_counts(rec, series, thr[:2])
    counts, hist = host.gate_counts(rec[:0], series, thr, 4)                     # no job: nothing to do
    assert counts.shape == (0, 12) and hist.shape == (0, 2, 4)
    rec, series, thr = C.pack([(np.zeros(0), np.array([1.0])), (x, np.zeros(0)), (np.array([np.nan, 1.0]), np.array([0.5]))])
    counts, hist = host.gate_counts(rec, series, thr, 2)                         # n == 0, n_thr == 0 write nothing; NaN is a gap
    assert counts.tolist() == [[1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0]] and not hist.any()


# ---- the public functions ------------------------------------------------------------------------------------

def same_gating(a, b):
    for f in (x.name for x in gating.dataclasses.fields(gating.Gating)):
        x, y = getattr(a, f), getattr(b, f)
        if f == "n_valid":
            if x != y:
                return False
        elif x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def test_gate_statistics_against_the_definition():
    a = C.smooth_noise(3000, 41, gaps=0.0)
    valid = np.random.default_rng(41).random(3000) > 0.05
    thr = np.array([0.3, -0.2, 0.3, 1.1])
    g = gating.gate_statistics(a, thr, valid, n_bins=16, stride=5, device=-1)
    want = [C.reference(np.where(valid, a, np.nan), d, 16) for d in thr]
    c = np.array([w[0] for w in want])
    assert g.counts.dtype == np.int64 and np.array_equal(g.counts, c) and g.n_valid == valid.sum()
    assert np.array_equal(g.threshold, thr) and np.array_equal(g.open_fraction, c[:, 0] / valid.sum())
    assert np.array_equal(g.openings, c[:, 6]) and np.array_equal(g.closings, c[:, 7])
    assert np.array_equal(g.open_runs, c[:, 2]) and np.array_equal(g.closed_runs, c[:, 3])
    assert np.array_equal(g.longest_open, 5 * c[:, 4]) and np.array_equal(g.longest_closed, 5 * c[:, 5])
    assert np.array_equal(g.mean_open, 5 * c[:, 10] / c[:, 8]) and np.array_equal(g.mean_closed, 5 * c[:, 11] / c[:, 9])
    assert np.array_equal(g.open_lengths, np.array([w[1][0] for w in want]))
    assert np.array_equal(g.closed_lengths, np.array([w[1][1] for w in want]))
    assert g.length.tolist() == list(range(5, 85, 5)) and g.open_lengths.shape == (4, 16)
    with pytest.raises(Exception):
        g.n_valid = 3                              # frozen
    # one call for many equals one call each; what a gap holds is ignored
    items = [(a, thr, valid), (a[:700], thr[:1], None), (np.where(valid, a, 1e300), thr, valid)]
    batch = gating.gate_statistics_batch(items, 16, [5, 1, 5], device=-1)
    assert same_gating(batch[0], g) and same_gating(batch[2], g)
    assert same_gating(batch[1], gating.gate_statistics(a[:700], thr[:1], n_bins=16, device=-1))
    assert gating.gate_statistics_batch([], device=-1) == []
    # no complete run: the mean is nan; no bins: empty histograms
    g = gating.gate_statistics([1.0, 1.0, 3.0, 3.0], [2.0, 0.0], device=-1)
    assert np.isnan(g.mean_open).all() and np.isnan(g.mean_closed).all() and g.open_lengths.shape == (2, 0) and len(g.length) == 0
    assert g.open_fraction.tolist() == [0.5, 1.0] and g.openings.tolist() == [1, 0]


def test_error_paths_of_the_python_surface():
    x = np.arange(10.0)
    with pytest.raises(ValueError, match="NaN or infinite"):
        gating.gate_statistics(np.array([1.0, np.nan, 3.0]), [1.0], device=-1)
    with pytest.raises(ValueError, match="NaN or infinite"):
        gating.gate_statistics(np.array([1.0, np.inf, 3.0]), [1.0], device=-1)
    with pytest.raises(ValueError, match="one flag"):
        gating.gate_statistics(x, [1.0], np.ones(9, dtype=bool), device=-1)
    with pytest.raises(ValueError, match="no valid entry"):
        gating.gate_statistics(x, [1.0], np.zeros(10, dtype=bool), device=-1)
    with pytest.raises(ValueError, match="at least one"):
        gating.gate_statistics(x, [], device=-1)
    with pytest.raises(ValueError, match="threshold is NaN or infinite"):
        gating.gate_statistics(x, [1.0, np.inf], device=-1)
    with pytest.raises(ValueError, match="n_bins"):
        gating.gate_statistics(x, [1.0], n_bins=-1, device=-1)
    with pytest.raises(ValueError, match="one stride"):
        gating.gate_statistics_batch([(x, [1.0], None)], stride=[1, 2], device=-1)


def test_trajectory_gating_and_per_molecule(tmp_path):
    path = synth.write_synthetic_history(tmp_path / "HISTORY", 20)
    traj = DLPOLY(path)
    order = [7, 2, 3] + [f for f in range(19, -1, -1) if f not in (7, 2, 3)]
    traj.analysis(frames=order, device=-1)
    store = traj.analysis_store
    frames, a, ok = store.series("windows_max")
    got = traj.gating(device=-1)                               # windows_max, 200 thresholds from min to max, 64 bins
    grid = np.linspace(a[ok].min(), a[ok].max(), 200)
    assert same_gating(got, gating.gate_statistics(a, grid, ok, 64, int(frames[1] - frames[0]), device=-1))
    assert got.open_fraction[0] == 1.0 and 0.0 < got.open_fraction[-1] < 1.0 and got.open_lengths.shape == (200, 64)
    _, p, pok = store.series("pore_diameter_opt")
    thr = [float(np.median(p[pok])), float(p[pok].min()), 1e3]
    some = traj.gating("pore_diameter_opt", thresholds=thr, n_bins=8, device=-1)
    with np.errstate(invalid="ignore"):
        want = [C.reference(np.where(pok, p, np.nan), d, 8) for d in thr]
    assert np.array_equal(some.counts, np.array([w[0] for w in want])) and some.counts[0, 2] > 0
    assert np.array_equal(some.open_lengths, np.array([w[1][0] for w in want]))
    assert np.array_equal(some.closed_lengths, np.array([w[1][1] for w in want]))
    with pytest.raises(ValueError, match="modular"):
        store.gating("windows_max", per_molecule=True, device=-1)
    with pytest.raises(ValueError, match="molecule= needs"):
        store.gating("windows_max", molecule=0, device=-1)
    with pytest.raises(ValueError, match="at least one"):
        store.gating("windows_max", thresholds=0, device=-1)
    with pytest.raises(ValueError, match="not a bool"):
        store.gating("windows_max", thresholds=True, device=-1)
    # a modular store: two molecules a frame, frames 0, 2, 4, ...
    recs = np.concatenate([store.records, store.records[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    modular = records.RecordStore(recs[by], 2 * pos[by], np.tile([0, 1], 20))
    each = modular.gating("pore_diameter", thresholds=12, per_molecule=True, n_bins=4, device=-1)
    assert sorted(each) == [0, 1]
    for m in (0, 1):
        only = records.RecordStore(modular.records[m::2], modular.unit_frame[m::2])
        assert same_gating(each[m], only.gating("pore_diameter", thresholds=12, n_bins=4, device=-1))
        assert same_gating(each[m], modular.gating("pore_diameter", thresholds=12, molecule=m, n_bins=4, device=-1))
        assert each[m].length.tolist() == [2, 4, 6, 8]             # the stride of the frame axis is passed on
    assert each[0].counts.tobytes() != each[1].counts.tobytes()
    with pytest.raises(ValueError, match="molecule="):
        modular.gating("windows_max", device=-1)
