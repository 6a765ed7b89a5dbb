"""What the budget sweeps of tests/test_gpu_{cavity,pores,affinity,rigid,passage,hop}.py share: three jobs of tiny
grids laid out so that the planner of a grid entry (pywindow_amd/csrc/pw_grid_host.hpp) meets no zero -- padding that
nobody reads before the first job and between jobs in every input array, so every first is positive and every uploaded
span starts past 0, and the outputs handed to the jobs in reverse order -- and the sweep itself: every budget of the
workspace from one word to the jobs' words and eight more, under the poison switch, against the host context."""
import _stat_edges as S

DIMS = ((3, 2, 2), (4, 3, 2), (2, 2, 3))                             # the three jobs' grids
ATOMS = (0, 1, 5)                                                    # and their atoms


def interleaved(pads, jobs):
    """([pad, last job, pad, ..., pad, first job], the places of the jobs in their own order): packed in this order and
    cut down to the records at those places, a call has the pads' inputs as padding and the pads' outputs as holes, and
    its jobs own their inputs and outputs from the back to the front."""
    assert len(pads) == len(jobs)
    order = [c for pair in zip(pads, reversed(jobs)) for c in pair]
    return order, [len(order) - 1 - 2 * q for q in range(len(jobs))]


def budget_sweep(C, hip_ctx, host, packed, words):
    """The device returns the host context's bytes at every workspace_bytes that is a multiple of 8 from 8 to
    8 * (sum(words) + 8), with the workspace and the compact result poisoned; `words`: what each job takes of the
    budget.  C: the entry's cases module (raw, same, first_difference)."""
    rc, want = C.raw(host, packed)
    assert rc == 0
    budgets = range(8, 8 * (sum(words) + 8) + 1, 8)
    assert 20 < len(budgets) < 200
    S.set_poison(True)
    try:
        for workspace_bytes in budgets:
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
            assert rc == 0 and C.same(got, want), (workspace_bytes, C.first_difference(got, want))
    finally:
        S.set_poison(False)
