"""The batches of the launch-cap tests (tests/_launch_cap_cases.py, run on the device by tests/test_gpu_launch_cap.py)
without a GPU: what each batch puts next to what is ASSERTED from its packed records -- with the tile sizes read from
the sources -- every capped kernel has at least 2 x 5 work items, so that at the largest cap every workgroup takes a
second one, and the host path (device = -1) returns the same bytes whatever the hook is set to and never counts a
launch."""
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
    assert entry.name in L.STAT_KERNELS and len(L.STAT_KERNELS[entry.name]) == 2
    jobs = entry.jobs()
    assert len(jobs) >= L.MIN_ITEMS                                  # (a job has at least one item of each of the two kernels)
    packed = S.pack_with_holes(entry, entry.mixed())
    assert S.set_launch_cap(1) == 0
    want = entry.run(host, packed, fill=S.SENTINEL)
    assert S.set_launch_cap(0) == 0
    assert S.same(entry.run(host, packed, fill=S.SENTINEL), want)


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
