"""The grid, crystal and statistical kernels whose workgroups stride over the work items of a launch, on gfx950 with
the launch-cap hook set (pw_internal_launch_cap; pw_stat_host.hpp: launch_blocks): one batch in one call with 1, 2, 3 and
5 workgroups a launch, so that every workgroup takes a second item and more -- at cap 1 one workgroup walks the whole
batch in order -- with the workspace filled with 0xFF before the first kernel and not.  The device must return the BYTES
of the host path (device = -1) on the same packed arrays, entries nobody owns must keep the caller's sentinel, and the
hook's counter must show that every capped kernel of the entry was given fewer workgroups than it had items.  The
reference is the host path, never the device without the hook.  What each batch puts next to what is asserted without a
GPU in tests/test_launch_cap.py; the batches are in tests/_launch_cap_cases.py.

GPU time on one MI355X: the file in 4.6 s; per test (all caps, poisoned and not, the host reference included) in each
docstring.  No test asserts a time."""
import numpy as np
import pytest

import _affinity_cases as A
import _launch_cap_cases as L
import _stat_edges as S

pytestmark = pytest.mark.gpu

ids = lambda e: e.name


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def hooks_off_afterwards():
    yield
    S.set_launch_cap(0)
    S.set_poison(False)


def capped(cap, poison, call):
    """call() with the cap and the poison set, both put back: (its result, how many launches were cut)."""
    S.set_poison(poison)
    S.set_launch_cap(cap)
    try:
        got = call()
    finally:
        cut = S.set_launch_cap(0)
        S.set_poison(False)
    return got, cut


def sentinel_rows(rows, sentinel):
    flat = np.frombuffer(rows.tobytes(), dtype=np.uint8).reshape(len(rows), -1)
    return int((flat == sentinel).all(axis=1).sum())


@pytest.mark.parametrize("entry", L.GRID_ENTRIES, ids=ids)
def test_every_workgroup_takes_more_than_one_item(hip_ctx, host, entry):
    """One batch in one call at caps 1, 2, 3 and 5, poisoned and not, against the host path's bytes.
    GPU time: 0.01 s each for pw_affinity, pw_passage, pw_hop, pw_percolation, pw_basins and pw_rigid_affinity, 0.02 s for
    pw_rigid_cell and pw_rigid_cell_ewald, 0.07 s for pw_charges, 0.95 s for pw_charges_cell (its 1537-atom job)."""
    packed = entry.packed()
    rc, want = entry.run(host, packed)
    assert rc == 0
    for cap in entry.caps:
        for poison in (False, True):
            (rc, got), cut = capped(cap, poison, lambda: entry.run(hip_ctx, packed))
            assert rc == 0 and entry.same(got, want), (cap, poison, entry.first_difference(got, want))
            assert cut >= len(entry.kernels), (cap, poison, cut, entry.kernels)
            assert sentinel_rows(entry.out_rows(got), entry.C.SENTINEL) == entry.hole * len(entry.jobs()), (cap, poison)


@pytest.mark.parametrize("entry", L.STAT_ENTRIES, ids=ids)
def test_the_edge_sweeps_of_the_statistical_entries(hip_ctx, host, entry):
    """The sweep of tests/test_gpu_stat_edges.py, with entries of the result nobody owns, at caps 1 and 3 against the
    host path (and, for pw_corr_sums, the exact lagged sums of the integer-valued series).
    GPU time: kde 0.11 s, kde2 0.3 s, kdew 1.8 s, corr 0.5 s."""
    batches = [(S.pack_with_holes(entry, entry.jobs()), None)]
    if entry.name == "corr":
        batches.append((entry.pack(entry.jobs(kind="integer")), S.corr_exact(entry.jobs(kind="integer"))))
    for packed, exact in batches:
        owned = entry.owned(packed)
        want = entry.run(host, packed, fill=S.SENTINEL)
        for cap in L.STAT_CAPS:
            for poison in (False, True):
                got, cut = capped(cap, poison, lambda: entry.run(hip_ctx, packed, fill=S.SENTINEL))
                assert S.same(got, want), (cap, poison)
                assert cut >= len(L.STAT_KERNELS[entry.name]), (cap, poison, cut)
                assert all((g[~m] == S.SENTINEL).all() for g, m in zip(got, owned)), (cap, poison)
                assert exact is None or bool((got[0] == exact.astype(np.float64)).all()), (cap, poison)


def test_one_launch_past_the_real_cap(hip_ctx, host):
    """pw_affinity with the hook off: 65536 items of sixteen unmasked 64^3 jobs and a 17th job of another kind (masked,
    five atoms, two betas, two edges) that workgroup 0 takes as its second item.  The device returns the host path's
    bytes, and the same bytes when the 17 jobs are sent as two calls of 16 and 1.
    GPU time: 0.03 s."""
    jobs = L.past_the_cap_jobs()
    packed = A.pack(jobs, hole=1, energies=False)
    rc, want = A.raw(host, packed)
    assert rc == 0
    assert S.set_launch_cap(0) == 0
    rc, got = A.raw(hip_ctx, packed)
    assert rc == 0 and A.same(got, want), A.first_difference(got, want)
    assert S.set_launch_cap(0) == 1                                  # (one launch had more items than the cap of its site)
    # as two calls of 16 and 1: each job's outputs, laid out as in the call of 17
    pieces = []
    for part in (jobs[:16], jobs[16:]):
        sub = A.pack(part, hole=1, energies=False)
        rc, piece = A.raw(hip_ctx, sub)
        assert rc == 0
        pieces.append((sub[0], piece))
    assert S.set_launch_cap(0) == 0                                  # (neither of them did)
    rec = packed[0]
    k = 0
    for sub_rec, (out, levels, hist, _) in pieces:
        for r in sub_rec:
            J = rec[k]
            assert out[r["out"]].tobytes() == got[0][J["out"]].tobytes(), k
            nb, ne = int(J["n_betas"]), int(J["n_edges"])
            assert levels[r["level_first"]:r["level_first"] + nb].tobytes() == got[1][J["level_first"]:J["level_first"] + nb].tobytes(), k
            assert hist[r["hist_first"]:r["hist_first"] + ne].tobytes() == got[2][J["hist_first"]:J["hist_first"] + ne].tobytes(), k
            k += 1
    assert k == 17
