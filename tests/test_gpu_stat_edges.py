"""The statistical entries on the device at every edge of their register tiles (tests/_stat_edges.py; the coverage of
the sweeps is asserted in tests/test_stat_edges.py): pw_kde_sums, pw_kde2_sums, pw_kde_wsums, pw_corr_sums, pw_dft_sums
and pw_gate_counts on gfx950 against the host path (device = -1), BIT FOR BIT, and against the exact references where
one exists -- (1) as they are, (2) with the partial-sum workspace and the compact device result filled with 0xFF
before the first kernel (pw_internal_poison_scratch), at three workspace budgets: a partial that a reduce kernel reads
and no partial kernel wrote is then a NaN (a gate summary: garbage) and not the right value a previous call left in
the same block of the pool, (3) right after a call with other sizes and other values.  No comparison carries a
tolerance, and every argument is valid."""
import numpy as np
import pytest

import _gate_cases as GA
import _kde_cases as K
import _stat_edges as S

pytestmark = pytest.mark.gpu

ids = lambda e: e.name


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(scope="module")
def expected(host):
    """(packed batch, the host path's result) of an entry's sweep, computed once and shared."""
    cache = {}

    def get(entry, **how):
        key = (entry.name, tuple(sorted(how.items())))
        if key not in cache:
            packed = entry.pack(entry.jobs(**how))
            cache[key] = (packed, entry.run(host, packed))
        return cache[key]

    return get


@pytest.fixture(scope="module", autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def gate_definition_holds(entry, result):
    """Every 13th job of the gate sweep against the definition in Python (the bins of the larger case serve both)."""
    jobs = entry.jobs()
    rec = entry.pack(jobs)[0]
    rows = np.concatenate([np.arange(r["out_first"], r["out_first"] + r["n_thr"]) for r in rec[::S.GATE_SUBSET]])
    counts, hist = GA.reference_rows(jobs[::S.GATE_SUBSET], max(S.GATE_BINS))
    return np.array_equal(result[0][rows], counts) and np.array_equal(result[1][rows], hist if entry.n_bins else hist[:, :, :0])


def exact_anchors_hold(entry, result, jobs):
    if entry.name == "corr":
        want = S.corr_exact(jobs)
        return result[0].shape == want.shape and bool((result[0] == want.astype(np.float64)).all())
    where, sums = S.dft_exact_j0(jobs)
    return bool((result[0][where] == sums).all() and (result[1][where] == 0.0).all())


def sweep_as_expected(entry, hip_ctx, expected):
    """Test 1's statement: the sweep on the device is the host path's, and the exact anchors'."""
    packed, want = expected(entry)
    got = entry.run(hip_ctx, packed)
    assert S.same(got, want) and all(g.size == 0 or np.abs(g).max() > 0 for g in got)
    if entry.name in ("corr", "dft"):
        packed, want = expected(entry, kind="integer")
        got = entry.run(hip_ctx, packed)
        assert S.same(got, want) and exact_anchors_hold(entry, got, entry.jobs(kind="integer"))
    if entry.name.startswith("gate"):
        assert gate_definition_holds(entry, got)


@pytest.mark.parametrize("entry", S.ENTRIES, ids=ids)
def test_the_sweep_device_equals_host_and_the_exact_anchors(hip_ctx, expected, entry):
    sweep_as_expected(entry, hip_ctx, expected)


def test_weights_of_one_give_the_bits_of_the_plain_sums(hip_ctx):
    """pw_kde_wsums over its whole sweep with every weight 1.0: each replica's row is pw_kde_sums' of the same job."""
    kdew = next(e for e in S.ENTRIES if e.name == "kdew")
    jobs = kdew.jobs(ones=True)
    packed = kdew.pack(jobs)
    (sums,) = kdew.run(hip_ctx, packed)
    plain = hip_ctx.kde_sums(*K.pack([(x, g, r) for x, g, _, r in jobs]))
    at = 0
    for (x, g, w, _), rec in zip(jobs, packed[0]):
        rows = sums[rec["out_first"]:rec["out_first"] + len(w) * len(g)].reshape(len(w), len(g))
        assert (rows.view(np.uint64) == plain[at:at + len(g)].view(np.uint64)[None, :]).all(), (len(x), len(g), len(w))
        at += len(g)
    assert at == len(plain) and plain.max() > 0.0


@pytest.mark.parametrize("entry", S.ENTRIES, ids=ids)
def test_the_sweep_with_poisoned_scratch(hip_ctx, host, entry):
    """The sweep and the existing mixed batch, with entries of the result that nobody owns, at three budgets of the
    workspace: the poisoned calls return what the clean call and the host path return, no NaN (no garbage) reaches an
    owned output, and what nobody owns keeps the caller's sentinel."""
    for jobs in (entry.jobs(), entry.mixed()):
        packed = S.pack_with_holes(entry, jobs)
        owned = entry.owned(packed)
        assert all((~m).sum() >= 8 for m in owned)
        clean = entry.run(hip_ctx, packed, fill=S.SENTINEL)
        want = entry.run(host, packed, fill=S.SENTINEL)
        assert S.same(clean, want)
        with S.poisoned():
            for budget in entry.budgets:
                got = entry.run(hip_ctx, packed, budget, fill=S.SENTINEL)
                assert all(not np.isnan(g[m]).any() for g, m in zip(got, owned)), budget
                assert S.same(got, clean) and S.same(got, want), budget
                assert all((g[~m] == S.SENTINEL).all() for g, m in zip(got, owned)), budget


@pytest.mark.parametrize("entry", S.ENTRIES, ids=ids)
def test_different_work_first(hip_ctx, expected, entry):
    """What two consecutive identical calls cannot see: the call before the sweep has the sweep's shapes in the
    opposite order, less one, and other values -- the blocks of the pool are as large and hold other numbers."""
    other = entry.pack(entry.jobs(seed=1, reverse=True))
    assert all(abs(a.size - b.size) <= 0.02 * b.size + 600 and not S.same((a,), (b,)) for a, b in zip(other[1:], expected(entry)[0][1:]))
    entry.run(hip_ctx, other)
    sweep_as_expected(entry, hip_ctx, expected)


def test_the_flag_is_cleared_after_a_failure(hip_ctx):
    with pytest.raises(ZeroDivisionError):
        with S.poisoned():
            1 // 0
    # (nothing reads the flag but the entries: a poisoned call and a clean one differ in nothing that can be seen, which
    # is what the tests above assert; here only that leaving the block by an exception runs the hook again)
    entry = S.ENTRIES[0]
    packed = entry.pack(entry.mixed())
    assert S.same(entry.run(hip_ctx, packed), (hip_ctx.kde_sums(*packed),))
