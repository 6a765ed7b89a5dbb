"""Rigid guests in a periodic cell on the device: pw_rigid_cell on gfx950 against the host path (device = -1) and against
the definition (tests/_rigid_cell_cases.py: reference, over ALL atoms), as BYTES -- the order of every sum is part of the
definition and the atom skip is proved to change none, so neither the launch geometry, which kernel instance serves a
job, how the jobs are gathered into launches, what the workspace held before, the near list's capacity nor whether the
skip is on may show.  numpy only; tests/test_rigid_cell.py holds the host path to the definition."""
import numpy as np
import pytest

import _rigid_cell_cases as C
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
    """Device == host path == definition, job by job and as one batch with holes forwards and reversed; two consecutive
    device calls agree; every instance of the main kernel (1, 2, 3 sites and the guarded one) was launched."""
    ran = 0
    for c in C.cases():
        packed = C.pack([c])
        d = []
        rc, got = C.raw(hip_ctx, packed, diagnostics=d)
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]), c.name
        assert d[0][1] == 1 << min(len(c.offsets) - 1, 3), c.name
        ran |= d[0][1]
    assert ran == 15
    jobs = C.cases() + C.shared_batch()
    for reverse in (False, True):
        packed = C.pack(jobs, hole=3, reverse=reverse)
        rc, got = C.raw(hip_ctx, packed)
        want = C.expected(jobs, host, hole=3, reverse=reverse)
        assert rc == 0 and C.same(got, want), (reverse, C.first_difference(got, want))
        assert C.same(got, C.raw(host, packed)[1]) and C.same(got, C.raw(hip_ctx, packed)[1])
        rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
        assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


@pytest.mark.parametrize("workspace_bytes", (1, 100_000, 0))
def test_workspaces_poison_and_a_call_of_other_shapes_before(hip_ctx, host, workspace_bytes):
    """Through pw_internal_rigid_cell with every job a launch of its own, with 100 kB a launch and with the default; the
    workspace and the compact result filled with 0xFF before the first kernel or not; right after a call of other shapes
    and values: the same bytes, and entries nobody owns untouched."""
    jobs = C.cases() + C.shared_batch()
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, host, hole=1)
    for poison in (False, True):
        assert C.raw(hip_ctx, C.pack(C.other_shapes()))[0] == 0
        S.set_poison(poison)
        rc, got = C.raw(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert rc == 0 and C.same(got, want), (workspace_bytes, poison, C.first_difference(got, want))


def test_the_skip_changes_no_byte_and_saves_pairs(hip_ctx, host):
    """The skip disabled and enabled: the same bytes on every case; on the cutoff's edge fewer pair terms with it, and
    without it every pair term of the job."""
    for c in C.cases():
        packed = C.pack([c])
        on, off = [], []
        rc_on, got_on = C.raw(hip_ctx, packed, diagnostics=on)
        rc_off, got_off = C.raw(hip_ctx, packed, diagnostics=off, skip=False)
        assert rc_on == 0 and rc_off == 0 and C.same(got_on, got_off), c.name
        assert int(off[0][0][0]) == c.voxels * len(c.dirs) * len(c.offsets) * len(c.xyz), c.name
        assert int(on[0][0][0]) <= int(off[0][0][0]), c.name
        if c.name.startswith("cutoff2="):
            assert int(on[0][0][0]) < int(off[0][0][0]) // 4, c.name


def test_budgets_where_the_planner_closes_a_group_with_padded_inputs_and_outputs_in_reverse(hip_ctx, host):
    """Three jobs of tiny grids with 0, 1 and 5 atoms and one, two and three sites (tests/_grid_sweep.py's layout: nothing
    of the inputs starts at 0, the outputs go to the jobs from the back to the front) at every budget within two words
    of a sum of consecutive jobs' words, and at a stride of 24 words in between, poisoned: the host path's bytes.  A job
    takes its (2L + 2) V record words and 2L + 6 words a chunk."""
    import _grid_sweep as G

    sites, n_dirs, betas = (1, 2, 3), (1, 3, 2), ((0.4,), (0.2, 0.9), (0.3,))
    jobs = [C.Case(f"sweep-{k}", d, *C.box_atoms(n, sites[k], d, C.ortho(1.0), 70 + k, pad=1.0), offsets=C.line(sites[k], 0.3),
                   dirs=C.dirs_of(n_dirs[k], 70 + k), betas=betas[k], map=k != 2) for k, (d, n) in enumerate(zip(G.DIMS, G.ATOMS))]
    pads = [C.Case(f"pad-{k}", (2, 2, 2), *C.box_atoms(2, 2, (2, 2, 2), C.ortho(1.0), 80 + k, pad=1.0), offsets=C.line(2, 0.3),
                   dirs=C.dirs_of(2, 80 + k), betas=(0.1, 0.2)) for k in range(3)]
    order, at = G.interleaved(pads, jobs)
    packed = list(C.pack(order, hole=1))
    rec = packed[0] = np.ascontiguousarray(packed[0][at])
    assert (rec["n"] == G.ATOMS).all() and (rec["atom_first"][1:] > 0).all() and (rec["coef_first"][1:] > 0).all()
    assert all((rec[name] > 0).all() for name in ("beta_first", "site_first", "dir_first"))
    assert all((np.diff(rec[name]) < 0).all() for name in ("out", "level_first")) and rec["map_first"][0] > rec["map_first"][1] > 0
    words = [(2 * len(c.betas) + 2) * c.voxels + -(-c.voxels // 64) * (2 * len(c.betas) + 6) for c in jobs]
    edges = {sum(words[a:b]) + e for a in range(3) for b in range(a + 1, 4) for e in (-2, -1, 0, 1, 2)}
    budgets = sorted(w for w in edges | set(range(1, sum(words) + 8, 24)) if w > 0)
    assert 20 < len(budgets) < 80
    rc, want = C.raw(host, tuple(packed))
    assert rc == 0
    S.set_poison(True)
    for w in budgets:
        rc, got = C.raw(hip_ctx, tuple(packed), workspace_bytes=8 * w)
        assert rc == 0 and C.same(got, want), (w, C.first_difference(got, want))


def test_bad_arguments_never_launch(hip_ctx):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        for budget in (None, 1):
            rc, got = C.raw(hip_ctx, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank(packed[8], packed[7], packed[6])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_rigid_cell: job 1: ") and what in message, (what, message)


def test_the_public_layer_on_the_cc3_cell(hip_ctx):
    """rigid_guest_field, rigid_guest_percolation and rigid_guest_diffusion on the CC3 cell at spacing 1.0, cutoff 8.0 and
    8 directions: the device's bytes are the host path's."""
    import _percolation_cases as P
    import pywindow_amd as pw

    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="CO2", temperatures=[250.0, 350.0], spacing=1.0, cutoff=8.0, directions=pw.sphere_directions(8))
    dev, ref = (pw.rigid_guest_field(xyz, elements, lattice, device=d, **kw) for d in (0, -1))
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.levels.tobytes() == ref.levels.tobytes()
    assert dev.zbar.tobytes() == ref.zbar.tobytes() and dev.u_min_map.tobytes() == ref.u_min_map.tobytes()
    assert dev.zbar.shape[0] == 2 and (dev.zbar > 0.0).any() and dev.n_dead > 0
    dev, ref = (pw.rigid_guest_percolation(xyz, elements, lattice, device=d, **kw) for d in (0, -1))
    assert [p.levels.tobytes() for p in dev] == [p.levels.tobytes() for p in ref]
    dev, ref = (pw.rigid_guest_diffusion(xyz, elements, lattice, device=d, **kw) for d in (0, -1))
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.tensor.tobytes() == ref.tensor.tobytes()
