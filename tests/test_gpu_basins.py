"""Energy basins on the device: pw_basins on gfx950 against the host path (device = -1) and against the definition
(tests/_basins_cases.py), EXACTLY -- every sum is taken in the written association, everything else is a comparison of
doubles or an integer count, so neither the launch geometry, the races of the pointer jumping, the order in which the
hash table filled, how the jobs are gathered into launches nor what the workspace held before may show.  numpy only;
tests/test_basins.py holds the host path to the definition."""
import numpy as np
import pytest

import _basins_cases as B
import _percolation_cases as P
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
    """Device == host path == definition, job by job -- fields and atoms, the 64^3 among them -- and as one batch with
    holes, forwards and with the outputs handed out from the back; two consecutive device calls agree."""
    for c in B.cases() + B.atom_cases() + B.big_cases():
        packed = B.pack([c])
        rc, got = B.raw(hip_ctx, packed)
        want = B.expected([c])
        assert rc == 0 and B.same(got, want), (c.name, B.first_difference(got, want))
        assert B.same(got, B.raw(host, packed)[1]), c.name
    jobs = B.cases() + B.atom_cases()
    for reverse in (False, True):
        packed = B.pack(jobs, hole=3, reverse=reverse)
        rc, got = B.raw(hip_ctx, packed)
        want = B.expected(jobs, hole=3, reverse=reverse)
        assert rc == 0 and B.same(got, want), B.first_difference(got, want)
        assert B.same(got, B.raw(host, packed)[1]) and B.same(got, B.raw(hip_ctx, packed)[1])
    rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert (rows == B.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, workspace_bytes):
    """Through pw_internal_basins with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact results filled with 0xFF before the first kernel or not; right after a call of other shapes
    and values: the same bytes, and entries nobody owns untouched."""
    jobs = B.cases() + B.atom_cases()
    packed = B.pack(jobs, hole=1)
    want = B.expected(jobs, hole=1)
    for poison in (False, True):
        assert B.raw(hip_ctx, B.pack(B.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = B.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and B.same(got, want), (workspace_bytes, poison, B.first_difference(got, want))


def test_a_batch_of_mixed_grids_with_the_largest(hip_ctx, host):
    jobs = B.mixed_batch()
    assert (64, 64, 64) in [c.dims for c in jobs] and len({c.dims for c in jobs}) > 8
    packed = B.pack(jobs, hole=1)
    diagnostics = []
    rc, got = B.raw(hip_ctx, packed, diagnostics=diagnostics)
    want = B.expected(jobs, hole=1)
    assert rc == 0 and B.same(got, want), B.first_difference(got, want)
    assert B.same(got, B.raw(host, packed)[1])
    n_rounds, n_faces = diagnostics[0]
    assert (n_rounds >= 1).all() and (n_rounds <= 20).all() and (n_faces >= 0).all()   # ceil(log2 V) + 1 and the last
    rc, again = B.raw(hip_ctx, packed, workspace_bytes=300_000)
    assert rc == 0 and B.same(again, want)


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in B.bad_batches():
        for budget in (None, 1):
            rc, got = B.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and B.same(got, B.blank(*packed[4:9])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_basins: job 1: ") and what in message, (what, message)
    packed = B.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        hip_ctx.basins(packed[0], packed[1], packed[2], packed[3])


def test_against_pw_percolation(hip_ctx):
    """Library against library on the device: the union-find over the returned edges gives pw_percolation's six levels --
    on the mazes, the random fields and the map of the CC3 cell; the double helix winds over the integers where
    pw_percolation reads never."""
    import pywindow_amd as pw
    from pywindow_amd import diffusion as DF

    def check(U):
        out, basins, edges = B.run_field(hip_ctx, U)
        levels, _ = P.run_field(hip_ctx, U)
        assert not out["flags"] and B.percolation_keys_from_edges(out, basins, edges) == P.keys(levels).tolist()
        return levels, basins, edges

    for c in P.cases():
        if c.name.startswith(("channel", "staircase", "slab", "pocket", "two-interleaved", "cubic", "ties", "normal")):
            check(c.field)
    (c,) = [c for c in P.cases() if c.name == "double-helix"]
    levels, basins, edges = check(c.field)
    vectors = np.array([v for _, v in DF.winding_vectors(len(basins), edges["a"], edges["b"], edges["d"])[1]])
    assert (levels["flags"] == 1).all() and np.linalg.matrix_rank(vectors) == 1
    elements, xyz, lattice = P.cc3_cell()
    check(pw.guest_percolation(xyz, elements, lattice, guest="Xe", spacing=1.0, cutoff=8.0, maps=True, device=0).maps)


def test_the_public_layer_on_the_cc3_cell(hip_ctx):
    """pw.guest_diffusion with Xe on the CC3 cell of tests/golden/rebuild.npz at spacing 1.0 and cutoff 8.0, two
    temperatures, with map and labels: device against host, the raw rows and the tensor as bytes."""
    import pywindow_amd as pw

    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="Xe", temperatures=[250.0, 350.0], spacing=1.0, cutoff=8.0, maps=True, labels=True)
    dev = pw.guest_diffusion(xyz, elements, lattice, device=0, **kw)
    ref = pw.guest_diffusion(xyz, elements, lattice, device=-1, **kw)
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.tensor.tobytes() == ref.tensor.tobytes()
    assert dev.maps.tobytes() == ref.maps.tobytes() and dev.labels.tobytes() == ref.labels.tobytes() and dev.maps.shape == (25, 25, 25)
    assert dev.populations.tobytes() == ref.populations.tobytes() and dev.rates.tobytes() == ref.rates.tobytes()
    assert dev.hops.tobytes() == ref.hops.tobytes() and dev.tensor.shape == (2, 3, 3) and dev.n_basins > 1


def job_words(c):
    """What the planner of pw_basins.hip takes for a job, in 8-byte words: the map, the words, the table, the list, the
    faces and the rows."""
    V = c.voxels
    b_cap, e_cap = min(c.b_cap, V), min(c.e_cap, 3 * V)
    table = 64
    while table <= 3 * V:
        table *= 2
    slots = 1
    while slots < e_cap:
        slots *= 2
    return 2 * V + table + slots + (3 * V + 1) // 2 + 19 * b_cap + 30 * e_cap + (2 * V if c.labels else 0)


def test_budgets_round_every_place_where_a_launch_group_can_close(hip_ctx, host):
    """Three jobs of tiny grids -- a field of the caller's, 1 atom without a map and 5 atoms with one -- laid out by
    tests/_grid_sweep.py (padding in every input, outputs from the back to the front) at the budgets of a launch round
    every sum of consecutive jobs' words, and at a regular stride from one word to all their words and eight more, under
    the poison switch.  (_grid_sweep.budget_sweep itself steps by one word and asks for fewer than 200 budgets; a job of
    pw_basins takes some hundreds of words.)"""
    import _grid_sweep as G

    rng = np.random.default_rng(70)
    step = (1.0, 0.25, 1.0, 0.0, -0.25, 1.0)

    def atoms(n, d, seed):
        xyz, _ = P.CC.random_atoms(n, d, seed, step)
        return dict(dims=d, xyz=xyz, coef=rng.uniform(0.5, 2.0, (n, 2)), core2=0.04, cutoff2=9.0, step=step, b_cap=8, e_cap=40)

    jobs = [B.Case("sweep-0", rng.integers(-2, 3, G.DIMS[0][::-1]).astype(np.float64), map=True, labels=True, b_cap=8, e_cap=40),
            B.Case("sweep-1", **atoms(G.ATOMS[1], G.DIMS[1], 71)),
            B.Case("sweep-2", map=True, labels=True, **atoms(G.ATOMS[2], G.DIMS[2], 72))]
    pads = [B.Case("pad-0", **atoms(2, (2, 2, 2), 80)), B.Case("pad-1", **atoms(2, (2, 2, 2), 81)),
            B.Case("pad-2", rng.normal(size=(2, 2, 2)), map=True, labels=True)]
    order, at = G.interleaved(pads, jobs)
    packed = list(B.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert rec["field_first"][0] > 0 and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert (np.diff(rec["out"]) < 0).all() and (np.diff(rec["basin_first"]) < 0).all() and (np.diff(rec["edge_first"]) < 0).all()
    assert rec["map_first"][0] > rec["map_first"][2] > 0 and rec["map_first"][1] == -1 and rec["label_first"][1] == -1
    rc, want = B.raw(host, tuple(packed))
    assert rc == 0 and not (want[0]["flags"][rec["out"]] & B.OVERFLOW).any()
    words = [job_words(c) for c in jobs]
    sums = {sum(words[a:b]) for a in range(3) for b in range(a + 1, 4)}
    budgets = sorted({8 * (w + d) for w in sums for d in (-1, 0, 1)} | set(range(8, 8 * (sum(words) + 8) + 1, 8 * (sum(words) // 90))))
    assert 40 < len(budgets) < 200
    S.set_poison(True)
    try:
        for workspace_bytes in budgets:
            rc, got = B.raw(hip_ctx, tuple(packed), workspace_bytes=workspace_bytes)
            assert rc == 0 and B.same(got, want), (workspace_bytes, B.first_difference(got, want))
    finally:
        S.set_poison(False)
