"""The edge sweeps of the statistical entries (tests/_stat_edges.py), without a GPU: (1) every sweep reaches every
path of its kernels -- the set of classes computed from the batch EQUALS the full set computed from the constants of
the sources, so a sweep that silently shrinks fails here and not on the device; (2) the host path, which
tests/test_gpu_stat_edges.py holds the device to bit for bit, is itself held to references that owe nothing to
pw_*.hpp wherever one exists exactly: integer-valued series in int64 (pw_corr_sums, and j = 0 of pw_dft_sums) and the
definition in Python (pw_gate_counts).  No comparison here carries a tolerance."""
import numpy as np
import pytest

import _gate_cases as GA
import _stat_edges as S

ids = lambda e: e.name


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.mark.parametrize("entry", S.ENTRIES[:-1], ids=ids)
def test_the_sweep_reaches_every_class(entry):
    shapes = entry.shapes()
    reached, full = entry.classes(shapes), entry.all_classes()
    assert reached == full, (sorted(full - reached, key=str)[:10], sorted(reached - full, key=str)[:10])
    assert len(full) >= 60 and len(shapes) == len(set(shapes)) == len(entry.jobs())
    # ... and a shorter sweep does not: the comparison is a condition, not a tally
    assert entry.classes(shapes[:len(shapes) // 2]) != full
    assert entry.classes([s for s in shapes if s[0] % 8 != 3]) != full


def test_the_classes_follow_the_constants_of_the_sources():
    """What the issue of the missing residues was: every count of a lane is congruent to n modulo CORR_LANE_LAGS."""
    C, R, W = S.corr_constants()
    assert (C, R, W) == (S.constant("CORR_CHUNK", "pw_corr.hpp"), S.constant("CORR_LANE_LAGS", "pw_corr.hpp"), 64)
    earlier = [0, 1, 2, 7, 8, 9, 17, 20, 63, 511, 512, 513, 700, 1000, 1024, 1025, 1500, 1541, 2000, 10_000]
    missing = S.corr_all_classes() - S.corr_classes([(n, n) for n in earlier if n])
    assert {("n mod R", 3), ("n mod R", 6)} <= missing
    k = S.dft_constants()
    missing = S.dft_all_classes() - S.dft_classes([((c - 1) * k["C"] + 1, 3) for c in (1, 2, 3, 4, 8, 9, 10, 32, 34, 196)])
    assert ("chunks mod WC", 5) in missing and {("reduce: chunks", c) for c in (15, 16, 17, 31, 33)} <= missing
    # the largest job of any sweep: about 20 000 entries x a few hundred outputs
    assert max(n for n, _ in S.dft_shapes()) <= 21_000 and max(n * m for n, m in S.gate_shapes()) <= 300_000


def test_corr_host_path_against_int64_sums(host):
    entry = next(e for e in S.ENTRIES if e.name == "corr")
    jobs = entry.jobs("integer")
    want = S.corr_exact(jobs)
    assert np.abs(want).max() < 2 ** 53 and np.abs(want).max() > 2 ** 20
    (got,) = entry.run(host, entry.pack(jobs))
    assert got.shape == want.shape and (got == want.astype(np.float64)).all()
    assert (got.astype(np.int64) == want).all()


def test_dft_host_path_at_frequency_zero(host):
    entry = next(e for e in S.ENTRIES if e.name == "dft")
    jobs = entry.jobs("integer")
    where, sums = S.dft_exact_j0(jobs)
    re, im = entry.run(host, entry.pack(jobs))
    assert len(where) == len(jobs) and (re[where] == sums).all() and (im[where] == 0.0).all()
    assert np.abs(sums).max() > 1000.0 and np.abs(im).max() > 0.0


@pytest.mark.parametrize("n_bins", S.GATE_BINS)
def test_gate_host_path_against_the_definition(host, n_bins):
    """Every 13th job of the sweep (the definition in Python is slow); the twelve counts do not depend on n_bins, so
    the definition is computed once, with the bins of the larger case."""
    entry = next(e for e in S.ENTRIES if e.name == f"gate-{n_bins}-bins")
    jobs = entry.jobs()[::S.GATE_SUBSET]
    assert {len(t) for _, t in jobs} == set(S.gate_thresholds()) and len(jobs) == 80
    counts, hist = entry.run(host, entry.pack(jobs))
    want_counts, want_hist = GA.reference_rows(jobs, max(S.GATE_BINS))
    assert np.array_equal(counts, want_counts) and counts[:, 8:10].sum() > 1000
    assert np.array_equal(hist, want_hist if n_bins else want_hist[:, :, :0])


@pytest.mark.parametrize("entry", S.ENTRIES, ids=ids)
def test_the_poison_switch_leaves_the_host_path_alone(host, entry):
    """pw_internal_poison_scratch is exported, and for a device = -1 context it does nothing; the flag is cleared on
    the way out."""
    packed = entry.pack(entry.mixed())
    want = entry.run(host, packed, fill=S.SENTINEL)
    with S.poisoned():
        got = entry.run(host, packed, fill=S.SENTINEL)
    assert S.same(got, want)
    assert all(not np.isnan(g[m]).any() and (g[~m] == S.SENTINEL).all() for g, m in zip(got, entry.owned(packed)))
