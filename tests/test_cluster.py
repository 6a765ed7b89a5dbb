"""Conformational clustering of frames (pw_cluster_gromos) on the host path, Context(-1): every case of
tests/_cluster_cases.py is np.array_equal with the definition written directly in numpy (C.reference), one job at a
time and as one batch; the invariants of a clustering; the refusals; and the Python layers above the entry
(pywindow_amd.clustering, DLPOLY.conformations).  tests/test_gpu_cluster.py holds the device to the same."""
import numpy as np
import pytest

import _cluster_cases as C
import pywindow_amd as pw
from pywindow_amd import _lib, synth


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=16)


def test_the_reference_on_cases_known_by_hand():
    labels, centres, sizes = C.reference(C.ring(70), 1.0)
    assert centres[0] == 0 and sizes[0] == 3 and set(np.flatnonzero(labels == 0)) == {69, 0, 1}
    d, group = C.cliques((40, 40))
    labels, centres, sizes = C.reference(d, 1.0)
    assert list(centres) == [0, 40] and list(sizes) == [40, 40] and np.array_equal(labels, group)
    labels, centres, sizes = C.reference(C.late_tie(), 1.0)
    assert list(centres[:3]) == [20, 0, 5] and list(sizes[:3]) == [26, 5, 5] and (sizes[3:] == 1).all()
    nb = C.late_tie() <= 1.0
    assert nb[5].sum() == 7 and nb[0].sum() == 6                     # before the first removal Q counted more than P


def test_planted_conformers():
    d, cutoff, group = C.planted()
    inside = group[:, None] == group[None, :]
    off = ~np.eye(len(d), dtype=bool)
    assert d[inside & off].max() < cutoff < d[~inside].min()
    got = pw.cluster_frames(d, cutoff, device=-1)
    assert got.n_clusters == 3 and list(got.sizes) == [50, 30, 20]
    for k in range(3):
        assert len(set(group[got.members(k)])) == 1 and len(got.members(k)) == got.sizes[k]
    assert np.array_equal(got.labels, np.argsort(np.argsort(-np.bincount(group)))[group])


def invariants(d, cutoff, labels, centres, sizes, found):
    n = len(d)
    assert labels.shape == (n,) and (0 <= labels).all() and (labels < found).all()
    assert np.array_equal(np.bincount(labels, minlength=found), sizes[:found])
    assert (np.diff(sizes[:found]) <= 0).all() and sizes[:found].sum() == n
    assert (centres[found:] == -1).all() and (sizes[found:] == 0).all()
    for k in range(found):
        c = int(centres[k])
        assert labels[c] == k
        for j in np.flatnonzero(labels == k):
            assert j == c or d[min(c, j), max(c, j)] <= cutoff


def test_every_case_one_job_at_a_time(host):
    for name, d, cutoff in C.cases():
        rc, got = C.raw(host, *C.pack([(d, cutoff)]))
        assert rc == 0 and C.same(got, C.expected([(d, cutoff)])), name
        invariants(d, cutoff, *got[:3], int(got[3][0]))


def test_every_case_as_one_batch_with_holes(host):
    jobs = [c[1:] for c in C.cases()]
    rc, got = C.raw(host, *C.pack(jobs, hole=3))
    want = C.expected(jobs, hole=3)
    assert rc == 0 and C.same(got, want)
    assert (got[0] == C.SENTINEL).sum() == 3 * len(jobs) and (got[3] >= 1).all()


def test_jobs_that_share_a_matrix_and_a_job_without_frames(host):
    jobs = C.call_cases()
    rec, dist = C.pack(jobs, hole=2)
    assert len(set(rec["d_first"][rec["n"] > 0].tolist())) == 2 and (rec["n"] == 0).sum() == 1
    rc, got = C.raw(host, rec, dist)
    assert rc == 0 and C.same(got, C.expected(jobs, hole=2))
    assert got[3][4] == 0 and len(set(got[3].tolist())) >= 5
    labels, centres, sizes, found = host.cluster_gromos(*C.pack(jobs))   # the bound method: -1 / -1 / 0 where nobody writes
    want = C.expected(jobs)
    assert C.same((labels, centres, sizes, found), want)


@pytest.mark.parametrize("threads", (1, 3, 16))
def test_host_threads_agree(threads):
    ctx = _lib.Context(-1, host_threads=threads)
    jobs = [c[1:] for c in C.cases() if len(c[1]) >= 257] + C.call_cases()
    rc, got = C.raw(ctx, *C.pack(jobs, hole=1))
    assert rc == 0 and C.same(got, C.expected(jobs, hole=1))


def test_refusals_leave_the_outputs_untouched(host):
    good = (C.cloud_matrix(5, 1), 1.0)
    nan_upper = C.cloud_matrix(6, 2)
    nan_upper[1, 4] = np.nan
    nan_lower = C.cloud_matrix(6, 2)
    nan_lower[4, 1] = nan_lower[2, 2] = np.nan
    rc, got = C.raw(host, *C.pack([good, (nan_lower, 1.0)]))
    assert rc == 0 and C.same(got, C.expected([good, (nan_lower, 1.0)]))      # legal: never read

    def refused(rec, dist, what, n_dist=None):
        rc, got = C.raw(host, rec, dist, n_dist=n_dist)
        assert rc == -2 and all((a == C.SENTINEL).all() for a in got), what
        message = _lib.load().pw_last_error().decode()
        assert "job 1" in message and what in message, message

    refused(*C.pack([good, (nan_upper, 1.0)]), "NaN in the strict upper triangle")
    refused(*C.pack([good, (good[0], np.nan)]), "cutoff is a NaN")
    for field in ("d_first", "n", "out_first"):
        rec, dist = C.pack([good, good])
        rec[field][1] = -1
        refused(rec, dist, "negative field")
    rec, dist = C.pack([good, good])
    rec["n"][1] = _lib.CLUSTER_MAX_N + 1
    refused(rec, dist, "n above PW_CLUSTER_MAX_N")
    rec, dist = C.pack([good, (C.cloud_matrix(7, 3), 1.0)])
    refused(rec, dist, "reaches outside dist", n_dist=len(dist) - 1)
    rec["d_first"][1] += 1
    refused(rec, dist, "reaches outside dist")


def test_python_layer_errors():
    d = C.cloud_matrix(6, 2)
    with pytest.raises(ValueError, match="square"):
        pw.cluster_frames(d[:, :5], 1.0, device=-1)
    with pytest.raises(ValueError, match="square"):
        pw.cluster_frames(d.reshape(-1), 1.0, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        pw.cluster_frames(d, np.nan, device=-1)
    bad = d.copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match="job 0: a NaN in the strict upper triangle"):
        pw.cluster_frames(bad, 1.0, device=-1)
    with pytest.raises(ValueError, match="frames"):
        pw.cluster_frames(d, 1.0, device=-1, frames=[1, 2])
    ctx = _lib.Context(-1)
    rec, dist = C.pack([(d, 1.0)])
    with pytest.raises(IndexError, match="outside `dist`"):
        ctx.cluster_gromos(rec, dist[:-1])
    with pytest.raises(IndexError, match="labels"):
        ctx.cluster_gromos(rec, dist, labels=np.zeros(5, dtype=np.int32))
    got = pw.cluster_frames(d, 1.0, device=-1)
    with pytest.raises(IndexError):
        got.members(got.n_clusters)
    with pytest.raises(ValueError, match="max_states"):
        got.state_series(17)
    assert pw.cluster_frames_scan(d, [], device=-1) == []
    empty = pw.cluster_frames(np.zeros((0, 0)), 1.0, device=-1)
    assert empty.n_clusters == 0 and empty.labels.shape == (0,)


def test_scan_equals_single_calls_and_the_definition():
    d = C.cloud_matrix(257, 21)
    cuts = [float(np.quantile(C.upper_values(d), q)) for q in (0.02, 0.2, 0.5)]
    scan = pw.cluster_frames_scan(d, cuts, device=-1)
    for cut, got in zip(cuts, scan):
        lab, cen, siz = C.reference(d, cut)
        one = pw.cluster_frames(d, cut, device=-1)
        for g in (got, one):
            assert g.cutoff == cut and g.frames is None and g.n_clusters == len(cen)
            assert C.same((g.labels, g.centres, g.sizes), (lab, cen, siz))
    assert scan[0].n_clusters > scan[1].n_clusters > scan[2].n_clusters


def test_state_series_feeds_transition_counts():
    d = C.cloud_matrix(400, 41, blobs=6)
    got = pw.cluster_frames(d, float(np.quantile(C.upper_values(d), 0.04)), device=-1)
    assert got.n_clusters > 6
    for max_states in (16, 4, 1):
        series, edges = got.state_series(max_states)
        S = min(got.n_clusters, max_states)
        merged = np.minimum(got.labels, S - 1)
        assert series.dtype == np.float64 and np.array_equal(series, merged) and np.array_equal(edges, 0.5 + np.arange(S - 1))
        kin = pw.transition_counts(series, edges, 5, device=-1)
        assert kin.counts.shape == (6, S, S)
        for lag in range(6):
            want = np.zeros((S, S), dtype=np.int64)
            np.add.at(want, (merged[:len(merged) - lag], merged[lag:]), 1)
            assert np.array_equal(kin.counts[lag], want)


def _history(tmp_path, cell=None):
    elements, base = synth.load_cc3_base()
    rng = np.random.default_rng(6)
    squeezed = base * np.array([1.0, 1.0, 1.06])                     # a second conformation: the cage stretched by 6 %
    frames = [(squeezed if t % 3 == 2 else base) + rng.normal(0.0, 0.005, base.shape) for t in range(9)]
    return pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=cell))


def test_conformations_of_a_trajectory(tmp_path):
    traj = _history(tmp_path)
    m = traj.rmsd_matrix(device=-1)
    noise, apart = m[0, 1], m[0, 2]
    assert noise < 0.05 < 0.2 < apart
    got = traj.conformations(0.1, device=-1)
    want = pw.cluster_frames(m, 0.1, device=-1)
    assert C.same((got.labels, got.centres, got.sizes), (want.labels, want.centres, want.sizes))
    assert got.n_clusters == 2 and list(got.sizes) == [6, 3] and np.array_equal(got.frames, np.arange(9))
    assert np.array_equal(got.labels, (np.arange(9) % 3 == 2).astype(np.int32))
    some = traj.conformations([0.1, 10.0], frames=[1, 2, 5, 8], device=-1)
    assert [c.n_clusters for c in some] == [2, 1] and np.array_equal(some[0].frames, [1, 2, 5, 8])
    assert np.array_equal(some[0].labels, [1, 0, 0, 0]) and list(some[0].frames[some[0].members(0)]) == [2, 5, 8]


def test_a_periodic_trajectory_is_refused(tmp_path):
    traj = _history(tmp_path, cell=np.eye(3) * 40.0)
    with pytest.raises(ValueError, match="periodic or modular"):
        traj.conformations(0.1, device=-1)
