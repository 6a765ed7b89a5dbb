"""The batches of the launch-cap tests (tests/_launch_cap_cases.py, run on the device by tests/test_gpu_launch_cap.py)
without a GPU: what each batch puts next to what is ASSERTED from its packed records -- with the tile sizes read from
the sources -- every capped kernel has at least 2 x 5 work items, so that at the largest cap every workgroup takes a
second one, and the host path (device = -1) returns the same bytes whatever the hook is set to and never counts a
launch.  The same for the trajectory entries, whose kernels count in workgroups' worth of waves or threads; the source
check: every strided launch of their seven files takes its grid from launch_blocks with the cap it had; and the host
path on the 8200-frame matrix of the hook-off clustering against the definition in Python."""
import re

import numpy as np
import pytest

import _affinity_cases as A
import _launch_cap_cases as L
import _stat_edges as S
from _util import ROOT

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


@pytest.mark.parametrize("entry", L.GRID_ENTRIES, ids=ids)
def test_what_the_batch_puts_next_to_what(entry):
    packed = entry.packed()
    missing = [what for what, holds in entry.properties(packed).items() if not holds]
    assert not missing, missing
    items = entry.items(packed)
    assert set(items) == set(entry.kernels) and len(entry.kernels) >= 1
    assert all(v >= L.MIN_ITEMS for v in items.values()), items
    assert max(entry.caps) * 2 <= L.MIN_ITEMS and entry.caps == (1, 2, 3, 5)


@pytest.mark.parametrize("entry", L.GRID_ENTRIES, ids=ids)
def test_the_host_path_never_reads_the_hook(host, entry):
    packed = entry.packed()
    assert S.set_launch_cap(0) == 0
    rc, want = entry.run(host, packed)
    assert rc == 0
    for cap in (1, 3):
        assert S.set_launch_cap(cap) == 0
        rc, got = entry.run(host, packed)
        assert rc == 0 and entry.same(got, want), (cap, entry.first_difference(got, want))
    assert S.set_launch_cap(0) == 0


@pytest.mark.parametrize("entry", L.STAT_ENTRIES, ids=ids)
def test_the_statistical_sweeps_have_the_items_and_the_host_path_returns_0(host, entry):
    """The sweeps are those of tests/test_stat_edges.py, hundreds of jobs each: no new shapes."""
    assert entry.name in L.STAT_KERNELS and len(L.STAT_KERNELS[entry.name]) == (3 if entry.name == "dft" else 2)
    jobs = entry.jobs()
    assert len(jobs) >= L.MIN_ITEMS                                  # (a job has at least one item of each of the two kernels)
    packed = S.pack_with_holes(entry, entry.mixed())
    assert S.set_launch_cap(1) == 0
    want = entry.run(host, packed, fill=S.SENTINEL)
    assert S.set_launch_cap(0) == 0
    assert S.same(entry.run(host, packed, fill=S.SENTINEL), want)
    if entry.name == "dft" or entry.name.startswith("gate"):
        # the thread-strided kernels count in workgroups of 256: from the packed records of the sweep the GPU test runs
        launches, items = L.stat_items(entry, S.pack_with_holes(entry, jobs))
        assert launches == 1 and tuple(items) == L.STAT_KERNELS[entry.name]
        assert all(v >= L.MIN_ITEMS for v in items.values()), items
    assert 1 in L.STAT_CAPS and 2 * max(L.STAT_CAPS) <= L.MIN_ITEMS


def test_the_twiddle_batch_has_the_arguments_and_the_host_path_counts_nothing(host):
    import _dft_cases as DF

    j, period, k = L.twiddle_batch()
    assert len(k) > 2 * 256 * max(L.CAPS) and len(k) % 256 != 0
    assert re.search(r"pw_dft_phase_kernel, dim3\(\(unsigned\)launch_blocks\(\(n \+ 255\) / 256, ", (ROOT / "pywindow_amd" / "csrc" / "pw_dft.hip").read_text())
    want = DF.twiddles(host, j, period, k)
    assert S.set_launch_cap(1) == 0
    got = DF.twiddles(host, j, period, k)
    assert S.set_launch_cap(0) == 0
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("entry", L.TRAJ_ENTRIES + (L.SHAPE,), ids=ids)
def test_what_the_trajectory_batches_put_next_to_what(entry):
    packed = entry.packed()
    missing = [what for what, holds in entry.properties(packed).items() if not holds]
    assert not missing, missing
    items = entry.items(packed)
    assert tuple(items) == tuple(entry.kernels) and len(entry.kernels) >= 1
    assert entry.caps in (L.CAPS, L.STAT_CAPS) and 1 in entry.caps
    assert all(v >= 2 * max(entry.caps) for v in items.values()), items


@pytest.mark.parametrize("entry", L.TRAJ_ENTRIES, ids=ids)
def test_the_host_path_of_a_trajectory_entry_never_reads_the_hook(host, entry):
    packed = entry.packed()
    assert S.set_launch_cap(0) == 0
    want = entry.run(host, packed)
    assert entry.untouched(want) and entry.exact(want) in (None, True)
    for cap in (1, 3):
        assert S.set_launch_cap(cap) == 0
        for budget in entry.budgets:
            assert entry.same(entry.run(host, packed, budget), want), (cap, budget)
    assert S.set_launch_cap(0) == 0


#: what each touched file hands to launch_blocks as its cap, launch site by launch site in the order of the text
SITES = {"pw_dft.hip": ["1l << 20"] * 4, "pw_gate.hip": ["1l << 20"] * 2, "pw_trans.hip": ["1l << 20"] * 2,
         "pw_superpose.hip": ["1l << 16"] * 3, "pw_cluster.hip": ["1l << 16", "1l << 16", "2048"], "pw_cov.hip": ["1l << 16"] * 5,
         "pw_shape.hip": ["4096"]}


@pytest.mark.parametrize("source", sorted(SITES))
def test_every_strided_launch_of_the_trajectory_files_goes_through_launch_blocks(source):
    text = (ROOT / "pywindow_amd" / "csrc" / source).read_text()
    assert re.findall(r"launch_blocks\(.*?, (1l << \d+|\d+)\)", text) == SITES[source]
    assert not re.search(r"\b\w+_grid\(", text) and not re.search(r"\? U : 4096", text)
    assert '#include "pw_stat_host.hpp"' in text
    # every launch but those of one workgroup a job and the circumcircle's takes its grid from launch_blocks
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)[^;]*?dim3\((.*?)\), dim3\(", text, flags=re.S)
    free = {"pw_cluster_init_kernel", "pw_cluster_pick_kernel", "pw_circumcircle_kernel"}
    assert launches and all(("launch_blocks(" in grid) != (name in free) for name, grid in launches), launches


def test_8200_frames_on_the_host_path_are_the_definition(host):
    """The matrix of tests/test_gpu_launch_cap.py's hook-off clustering, once: the host path against the definition in
    Python, and the packed record gives the count kernel more workgroups' worth than its cap."""
    import _cluster_cases as CL

    rec, d = L.past_the_cap_cluster()
    n = int(rec["n"][0])
    cap = int(re.search(r"pw_cluster_count_kernel, dim3\(\(unsigned\)launch_blocks\(\(G\.n_max \+ 3\) / 4, (\d+)\)",
                        (ROOT / "pywindow_amd" / "csrc" / "pw_cluster.hip").read_text()).group(1))
    assert cap == 2048 and (n + 3) // 4 > cap and len(rec) == 1 and d.shape == (n, n)
    # neither the pack nor the mirror launch reaches its cap of 65536: only the count launches are cut
    stride = ((n + 63) // 64 + 1) & ~1
    rows = L.budget_constant("CLUSTER_SLAB_BYTES", "pw_cluster.hpp") // (8 * n)
    assert (rows * stride + 3) // 4 <= 65536 and (((n + 63) // 64) ** 2 + 3) // 4 <= 65536
    rc, got = CL.raw(host, rec, d)
    assert rc == 0
    labels, centres, sizes = CL.reference(d, float(rec["cutoff"][0]))
    del d
    k = len(centres)
    assert k == 3 and int(centres[0]) == L.PAST_THE_CAP_CENTRE >= cap * 4 and int(got[3][0]) == k <= S.constant("CLUSTER_ROUNDS", "pw_cluster.hpp") - 1
    assert np.array_equal(got[0], labels) and np.array_equal(got[1][:k], centres) and np.array_equal(got[2][:k], sizes)
    assert (got[1][k:] == -1).all() and (got[2][k:] == 0).all()


def test_the_projection_past_the_real_cap_has_two_workgroups_more():
    (X, tr, mean, V), = L.past_the_cap_projection()
    waves = S.constant("COV_PROJ_WAVES", "pw_cov.hip")
    cap = re.search(r"launch_blocks\(\(T \+ COV_PROJ_WAVES - 1\) / COV_PROJ_WAVES, 1l << (\d+)\)", (ROOT / "pywindow_amd" / "csrc" / "pw_cov.hip").read_text())
    assert X.shape == (4 * 65536 + 5, 3) and tr is None and V.shape == (2, 3)
    assert (len(X) + waves - 1) // waves == (1 << int(cap.group(1))) + 2


def test_the_batch_past_the_real_cap_has_one_item_more():
    jobs = L.past_the_cap_jobs()
    packed = A.pack(jobs, hole=1, energies=False)
    rec, V = packed[0], packed[10]
    assert len(jobs) == 17 and all(c.dims == (64, 64, 64) and c.words is None and len(c.xyz) == 1 and len(c.betas) == 1 and len(c.edges) == 0
                                   for c in jobs[:16])
    last = jobs[16]
    assert last.dims == (3, 2, 2) and last.words is not None and len(last.xyz) == 5 and len(last.betas) == 2 and len(last.edges) == 2
    assert sum(L.chunks_of(v) for v in V[:16]) == L.REAL_CAP and sum(L.chunks_of(v) for v in V) == L.REAL_CAP + 1
    # the cap of the launch site, and one launch for the 17 jobs: their workspace is within the default budget
    text = (ROOT / "pywindow_amd" / "csrc" / "pw_affinity.hip").read_text()
    assert re.search(r"launch_blocks\(G\.items, (\d+)\)", text).group(1) == str(L.REAL_CAP)
    budget = re.search(r"AFF_WORKSPACE_BYTES = (\d+)l? << (\d+)", (ROOT / "pywindow_amd" / "csrc" / "pw_affinity.hpp").read_text())
    words = sum(((c.dims[1] * c.dims[2] + 2) // 2 if c.words is not None else 0) + L.chunks_of(v) * (2 * len(c.betas) + 4 + len(c.edges)) + 1
                for c, v in zip(jobs, V))
    assert 8 * words <= int(budget.group(1)) << int(budget.group(2))
    assert (rec["energy_first"] == -1).all()


def test_the_hook_is_exported_and_off_at_start():
    assert S.set_launch_cap(0) == 0 and S.set_launch_cap(7) == 0 and S.set_launch_cap(0) == 0
