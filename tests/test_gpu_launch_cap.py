"""The grid, crystal and statistical kernels whose workgroups stride over the work items of a launch, on gfx950 with
the launch-cap hook set (pw_internal_launch_cap; pw_stat_host.hpp: launch_blocks): one batch in one call with 1, 2, 3 and
5 workgroups a launch, so that every workgroup takes a second item and more -- at cap 1 one workgroup walks the whole
batch in order -- with the workspace filled with 0xFF before the first kernel and not.  The device must return the BYTES
of the host path (device = -1) on the same packed arrays, entries nobody owns must keep the caller's sentinel, and the
hook's counter must show that every capped kernel of the entry was given fewer workgroups than it had items.  The
reference is the host path, never the device without the hook.  What each batch puts next to what is asserted without a
GPU in tests/test_launch_cap.py; the batches are in tests/_launch_cap_cases.py.

The trajectory entries (pw_dft_sums, pw_gate_counts, pw_trans_counts, pw_superpose, pw_cluster_gromos, pw_covariance,
pw_project, pw_shape_batch) stride by workgroup, by wave or by thread behind caps of their own (2^20, 65536, 2048, 4096):
the same statements hold for them, with the independent exact references where one exists (the definitions in Python
of _trans_cases, _gate_cases and _cluster_cases, the integer sums of _stat_edges), and two tests leave the hook off and
send one launch past a cap that a trajectory reaches: 8200 frames through pw_cluster_count_kernel (2048 x 4) and
4 x 65536 + 5 rows through pw_cov_project_kernel.

GPU time on one MI355X: the file in 9.5 s (4.6 s before the trajectory entries), and 6.2 s more where
the session has not yet built tests/hostsim; per test (all caps, poisoned and
not, the host reference included) in each docstring.  No test asserts a time."""
import numpy as np
import pytest

import _affinity_cases as A
import _cluster_cases as CL
import _cov_cases as CV
import _dft_cases as DF
import _gate_cases as GA
import _launch_cap_cases as L
import _shape_cases as SH
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
    host path and the exact references: for pw_corr_sums the lagged sums of the integer-valued series, for pw_dft_sums
    the integer sums at j = 0, for pw_gate_counts the definition in Python on every 13th job.
    GPU time: kde 0.11 s, kde2 0.3 s, kdew 1.8 s, corr 0.5 s, dft 1.1 s, gate 2.3 s with 0 bins (the definition in Python is
    computed there) and 0.5 s with 5."""
    holed = S.pack_with_holes(entry, entry.jobs())
    batches = [(holed, None)]
    if entry.name == "corr":
        want_sums = S.corr_exact(entry.jobs(kind="integer")).astype(np.float64)
        batches.append((entry.pack(entry.jobs(kind="integer")), lambda got: bool((got[0] == want_sums).all())))
    if entry.name == "dft":
        where, sums = S.dft_exact_j0(entry.jobs(kind="integer"))
        batches.append((entry.pack(entry.jobs(kind="integer")), lambda got: bool((got[0][where] == sums).all() and (got[1][where] == 0.0).all())))
    if entry.name.startswith("gate"):
        subset = holed[0][::S.GATE_SUBSET]
        rows = np.concatenate([np.arange(r["out_first"], r["out_first"] + r["n_thr"]) for r in subset])
        counts, hist = GA.reference_rows(entry.jobs()[::S.GATE_SUBSET], max(S.GATE_BINS))
        hist = hist if entry.n_bins else hist[:, :, :0]
        batches[0] = (holed, lambda got: np.array_equal(got[0][rows], counts) and np.array_equal(got[1][rows], hist))
    for packed, exact in batches:
        owned = entry.owned(packed)
        want = entry.run(host, packed, fill=S.SENTINEL)
        for cap in L.STAT_CAPS:
            for poison in (False, True):
                got, cut = capped(cap, poison, lambda: entry.run(hip_ctx, packed, fill=S.SENTINEL))
                assert S.same(got, want), (cap, poison)
                assert cut >= len(L.STAT_KERNELS[entry.name]), (cap, poison, cut)
                assert all((g[~m] == S.SENTINEL).all() for g, m in zip(got, owned)), (cap, poison)
                assert exact is None or exact(got), (cap, poison)


def test_the_twiddle_hook_takes_a_second_argument_a_thread(hip_ctx, host):
    """pw_dft_phase_kernel (thread-strided, 256 a workgroup) on 2637 arguments at caps 1, 2, 3 and 5 against the host path.
    GPU time: under 0.01 s."""
    j, period, k = L.twiddle_batch()
    assert len(k) > 2 * 256 * max(L.CAPS) and len(k) % 256
    want = DF.twiddles(host, j, period, k)
    for cap in L.CAPS:
        got, cut = capped(cap, False, lambda: DF.twiddles(hip_ctx, j, period, k))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), cap
        assert cut == 1, (cap, cut)


@pytest.mark.parametrize("entry", L.TRAJ_ENTRIES, ids=ids)
def test_every_workgroup_of_a_trajectory_kernel_turns_again(hip_ctx, host, entry):
    """One batch in one call at every cap of the entry, poisoned and not, at every workspace budget of the entry, against
    the host path's bytes and the entry's exact reference; the rows nobody owns keep the sentinel.
    GPU time: pw_trans_counts 0.04, 0.04, 0.05 and 0.06 s (2, 4, 5 and 16 states), pw_superpose 0.06 s, pw_cluster_gromos 0.10 s,
    pw_covariance 0.09 s, pw_project under 0.01 s."""
    packed = entry.packed()
    want = entry.run(host, packed)
    assert entry.untouched(want) and entry.exact(want) in (None, True)
    for budget in entry.budgets:
        for cap in entry.caps:
            for poison in (False, True):
                got, cut = capped(cap, poison, lambda: entry.run(hip_ctx, packed, budget))
                assert entry.same(got, want), (budget, cap, poison)
                assert cut >= (len(entry.kernels) if budget == entry.budgets[0] else entry.cut_small), (budget, cap, poison, cut)
                assert entry.untouched(got), (budget, cap, poison)
                assert entry.exact(got) in (None, True), (budget, cap, poison)


def test_the_shape_kernel_takes_a_second_unit(hip_ctx, hostsim):
    """pw_shape_batch has no host path: twelve edge units, one of several buffers followed by a one-atom unit and back,
    at caps 1, 2, 3 and 5 against the host build of pw_shape.hpp (tests/hostsim), as tests/test_gpu_shape.py compares.
    GPU time: 0.02 s (and the session's build of tests/hostsim where no test before it asked for it)."""
    import ctypes

    from pywindow_amd import _lib

    def same_values(a, b):                                           # (any NaN matches any NaN: tests/test_gpu_shape.py)
        a, b = (np.ascontiguousarray(v).reshape(-1).view(np.float64) for v in (a, b))
        keep = ~np.isnan(a)
        return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint64)[keep], b.view(np.uint64)[keep])

    off, xyz, mass = L.SHAPE.packed()
    want = SH.host_shape(ctypes.CDLL(str(hostsim / "libshapeprobe.so")), off, xyz, mass)
    for cap in L.SHAPE.caps:
        got, cut = capped(cap, False, lambda: hip_ctx.shape(_lib.Batch(off, xyz, np.ones(len(mass)), mass)))
        assert same_values(got.view(np.float64), want.view(np.float64)), cap
        assert cut == 1, (cap, cut)


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


def test_8200_frames_pass_the_cap_of_the_count_kernel(hip_ctx, host):
    """pw_cluster_gromos with the hook off on 8200 frames: (n + 3) / 4 = 2050 workgroups' worth of pw_cluster_count_kernel
    behind its cap of 2048, so the waves of workgroups 0 and 1 take a second row.  Four tight groups on a line and frame
    8195 between two of them with the most neighbours: the first centre is found on a second turn; four rounds.  The device returns the host path's labels, centres, sizes and count, and the counter reports the count
    launches of one look at the done flags (CLUSTER_ROUNDS) as cut and no other.  The host path is held to the definition
    in Python on this matrix by tests/test_launch_cap.py.
    GPU time: 0.13 s (the 540 MB matrix is built once and freed)."""
    rec, dist = L.past_the_cap_cluster()
    rc, want = CL.raw(host, rec, dist)
    assert rc == 0 and int(want[3][0]) == 3 and int(want[1][0]) == L.PAST_THE_CAP_CENTRE >= 2048 * 4
    assert S.set_launch_cap(0) == 0
    rc, got = CL.raw(hip_ctx, rec, dist)
    cut = S.set_launch_cap(0)
    del dist
    assert rc == 0 and CL.same(got, want)
    assert cut == S.constant("CLUSTER_ROUNDS", "pw_cluster.hpp"), cut


def test_a_projection_passes_the_cap_of_the_project_kernel(hip_ctx, host):
    """pw_project with the hook off on T = 4 x 65536 + 5 rows, D = 3, k = 2: 65538 workgroups' worth behind the cap of
    65536, so the waves of workgroups 0 and 1 take a second row.  The host path's bytes; one launch is reported cut.
    GPU time: 0.02 to 0.3 s."""
    parts = L.past_the_cap_projection()
    want = CV.project_batch(host, parts, hole=1)[1]
    assert S.set_launch_cap(0) == 0
    got = CV.project_batch(hip_ctx, parts, hole=1)[1]
    assert S.set_launch_cap(0) == 1
    assert CV.same(got, want) and CV.untouched(got[[0, -1]]).all()
