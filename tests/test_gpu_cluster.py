"""Conformational clustering of frames on the device: pw_cluster_gromos on gfx950 against the host path (device = -1)
and against the definition (tests/_cluster_cases.py: reference), EXACTLY -- every output is an integer and the centre of
a round is an integer maximum, so neither the launch geometry, the slabs the matrix is uploaded in, how the jobs are
gathered into launches nor the rounds queued between two looks at the done flags may show.  numpy only;
tests/test_cluster.py holds the host path to the definition."""
import numpy as np
import pytest

import _cluster_cases as C
import _stat_edges as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def test_the_case_list(hip_ctx, host):
    """Device == host path == definition, job by job and as one batch, and two consecutive device calls agree."""
    for name, d, cutoff in C.cases():
        packed = C.pack([(d, cutoff)])
        rc, got = C.raw(hip_ctx, *packed)
        assert rc == 0 and C.same(got, C.expected([(d, cutoff)])), name
        assert C.same(got, C.raw(host, *packed)[1]), name
    jobs = [c[1:] for c in C.cases()]
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(hip_ctx, *packed)
    assert rc == 0 and C.same(got, C.expected(jobs, hole=3)) and C.same(got, C.raw(host, *packed)[1])
    assert (got[0] == C.SENTINEL).sum() == 3 * len(jobs)
    assert C.same(got, C.raw(hip_ctx, *packed)[1])


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_rounds_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_cluster_gromos with a slab of one row and every job a launch of its own, with 100 kB and with
    the default; 1, 7 and the default number of rounds between two looks at the done flags; the bit matrices, the
    active words, the key slots and the compact result filled with 0xFF before the first kernel or not; right after a
    call of other shapes and values: the same integers, and entries nobody owns untouched."""
    small = [c[1:] for c in C.cases() if len(c[1]) <= 257]
    large = [c[1:] for c in C.cases() if len(c[1]) > 257]
    for jobs, rounds_list in ((small + C.call_cases(), (1, 7, 0)), (large, (7, 0))):
        rec, dist = C.pack(jobs, hole=1)
        want = C.expected(jobs, hole=1)
        for rounds in rounds_list:
            for poison in (False, True):
                assert C.raw(hip_ctx, *C.pack(C.other_shapes()))[0] == 0
                S.set_poison(poison)
                rc, got = C.raw(hip_ctx, rec, dist, workspace_bytes=workspace_bytes, rounds_per_check=rounds)
                S.set_poison(False)
                assert rc == 0 and C.same(got, want), (workspace_bytes, rounds, poison)


def test_all_singletons_with_a_look_after_every_round(hip_ctx):
    """n = 1025 rounds of one frame each, the done flags copied back after every one of them."""
    jobs = [c[1:] for c in C.cases() if c[0] == "n=1025-all-singletons"]
    rc, got = C.raw(hip_ctx, *C.pack(jobs), workspace_bytes=0, rounds_per_check=1)
    assert rc == 0 and C.same(got, C.expected(jobs)) and got[3][0] == 1025


def test_call_cases_and_entries_nobody_owns(hip_ctx, host):
    jobs = C.call_cases()
    rec, dist = C.pack(jobs, hole=2)
    rc, got = C.raw(hip_ctx, rec, dist)
    assert rc == 0 and C.same(got, C.expected(jobs, hole=2)) and C.same(got, C.raw(host, rec, dist)[1])
    assert all((a == C.SENTINEL).sum() == 2 * 6 for a in got[:3]) and got[3][4] == 0


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    good = (C.cloud_matrix(5, 1), 1.0)
    nan_upper = C.cloud_matrix(6, 2)
    nan_upper[1, 4] = np.nan
    batches = [(C.pack([good, (nan_upper, 1.0)]), None, "NaN in the strict upper triangle"),
               (C.pack([good, (good[0], np.nan)]), None, "cutoff is a NaN")]
    for field in ("d_first", "n", "out_first"):
        rec, dist = C.pack([good, good])
        rec[field][1] = -1
        batches.append(((rec, dist), None, "negative field"))
    rec, dist = C.pack([good, good])
    rec["n"][1] = _lib.CLUSTER_MAX_N + 1
    batches.append(((rec, dist), None, "n above PW_CLUSTER_MAX_N"))
    rec, dist = C.pack([good, (C.cloud_matrix(7, 3), 1.0)])
    batches.append(((rec, dist), len(dist) - 1, "reaches outside dist"))
    for (rec, dist), n_dist, what in batches:
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, rec, dist, workspace_bytes=budget, n_dist=n_dist)
            assert rc == -2 and all((a == C.SENTINEL).all() for a in got), what
            message = _lib.load().pw_last_error().decode()
            assert "job 1" in message and what in message, message
    with pytest.raises(ValueError, match="job 1: a NaN in the strict upper triangle"):
        hip_ctx.cluster_gromos(*C.pack([good, (nan_upper, 1.0)]))


def test_the_public_scan(hip_ctx):
    """cluster_frames_scan at n = 1025 with 8 cutoffs, one call and one upload of the matrix: device against host."""
    import pywindow_amd as pw

    d = C.cloud_matrix(1025, 51, blobs=7)
    v = C.upper_values(d)
    cuts = [float(np.quantile(v, q)) for q in (0.002, 0.01, 0.03, 0.08, 0.2, 0.4, 0.7, 1.0)]
    dev = pw.cluster_frames_scan(d, cuts, device=0)
    ref = pw.cluster_frames_scan(d, cuts, device=-1)
    assert len(dev) == len(ref) == 8
    for a, b in zip(dev, ref):
        assert a.cutoff == b.cutoff and C.same((a.labels, a.centres, a.sizes), (b.labels, b.centres, b.sizes))
        assert a.sizes.sum() == 1025 and (np.diff(a.sizes) <= 0).all()
    counts = [c.n_clusters for c in dev]
    assert counts == sorted(counts, reverse=True) and counts[0] > 50 and counts[-1] == 1
    lab, cen, siz = C.reference(d, cuts[3])
    assert C.same((dev[3].labels, dev[3].centres, dev[3].sizes), (lab, cen, siz))
