"""The periodic pre-processing on the device at its edges (tests/_rebuild_cases.py; the coverage of the sweep is asserted
in tests/test_rebuild_edges.py, which also holds the host build to the oracle and to the reference).  Here every frame
of every launch equals the host build's result EXACTLY - molecule count, offsets, source atoms and images, coordinate
bits:
  * the cases of one topology in one launch, forwards and backwards, with one team per CU and three times as many
    frames as teams: a team takes several different frames one after the other (all but the 15 625-atom block,
    one frame, which goes once through each of the two device walks);
  * in each memory layout the test hook pw_internal_rebuild_layout leaves (visit bit sets and the one-wave walk, with
    and without the scan arrays in team-shared memory; stamp arrays and the four-barrier team loop);
  * with the team slabs and the device outputs as the pool hands them out after a launch of another topology, and
    filled with 0xFF (pw_internal_poison_scratch).
No comparison carries a tolerance."""
import contextlib
import ctypes

import numpy as np
import pytest

import _rebuild_cases as RC
import _stat_edges as S

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::PendingDeprecationWarning")]

LAYOUTS = (1, 3, 0)
REFUSALS = RC.constants()["RB_ST_NB_OVERFLOW"] | RC.constants()["RB_ST_SEG_OVERFLOW"] | RC.constants()["RB_ST_THIN_CELL"]
GROUPS = RC.topologies()


def set_layout(layout):
    from pywindow_amd import _lib

    L = _lib.load()
    L.pw_internal_rebuild_layout.argtypes = [ctypes.c_int]
    L.pw_internal_rebuild_layout.restype = None
    L.pw_internal_rebuild_layout(layout)


@contextlib.contextmanager
def forced_layout(layout):
    set_layout(layout)
    try:
        yield
    finally:
        set_layout(-1)


@pytest.fixture(scope="module", autouse=True)
def hooks_off_afterwards():
    yield
    S.set_poison(False)
    set_layout(-1)


@pytest.fixture(scope="module")
def host(hostsim):
    """The host build's result of a case, computed once (its three layouts agree: tests/test_rebuild_edges.py)."""
    cache = {}

    def get(case):
        if case["name"] not in cache:
            cache[case["name"]] = RC.host_raw(hostsim, case, 1)
        return cache[case["name"]]

    return get


def teams(monkeypatch):
    """One team per CU: the grid of a launch, which the number of frames has to exceed three times over."""
    import torch

    monkeypatch.setenv("PW_RB_TEAMS_PER_CU", "1")
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(ctx, frames, host):
    """pw_discrete_molecules on `frames` (cases of one topology); per frame (status, n_mol, offsets, src, image, xyz),
    cut to what the frame says it wrote.  Capacities from the host build's results, so no frame overflows."""
    from pywindow_amd import _lib
    from pywindow_amd import rebuild as RB

    first = frames[0]
    topo = RC.topology_of(first)
    rebuild = first["rebuild"]
    periodic = "lattice" in first["system"]
    coords, lat, inv = RB.pack_frames(np.array([c["system"]["coordinates"] for c in frames]),
                                      np.array([c["system"]["lattice"] for c in frames]) if periodic else None)
    f, n = len(frames), topo.n
    want = [host(c) for c in {c["name"]: c for c in frames}.values()]
    cap = max(max(len(w[3]) for w in want), 1) + 3
    mols = max(max(w[1] for w in want), 1) + 2
    n_mol, status = np.full(f, -7, np.int32), np.full(f, -7, np.int32)
    off, src = np.full((f, mols + 1), -7, np.int32), np.full((f, cap), -7, np.int32)
    img, xyz = np.full((f, cap), -7, np.int8), np.full((f, cap, 3), np.nan)
    cin = _lib.CellIn(f, n, 1 if rebuild else 0, coords.ctypes.data, None if lat is None else lat.ctypes.data,
                      None if inv is None else inv.ctypes.data, topo.cov.ctypes.data, topo.mass.ctypes.data,
                      topo.terminal.ctypes.data, topo.max_dist, topo.tol)
    cout = _lib.CellOut(cap, mols, n_mol.ctypes.data, status.ctypes.data, off.ctypes.data, src.ctypes.data,
                        img.ctypes.data, xyz.ctypes.data)
    rc = _lib.load().pw_discrete_molecules(ctx._h, ctypes.byref(cin), ctypes.byref(cout))
    assert rc == 0, _lib.load().pw_last_error()
    out = []
    for k in range(f):
        m = int(n_mol[k])
        assert 0 <= m <= mols, (k, m)
        a = int(off[k, m])
        assert 0 <= a <= cap, (k, a)
        out.append((int(status[k]), m, off[k, :m + 1], src[k, :a], img[k, :a], xyz[k, :a]))
    return out


def frames_as_the_host_build(ctx, frames, host, where):
    got = launch(ctx, frames, host)
    for k, (c, g) in enumerate(zip(frames, got)):
        w = host(c)
        assert g[0] == w[0] == c["status"], f"{where} frame {k} ({c['name']}): status {g[0]}, host build {w[0]}"
        # a refused frame says so and nothing more: which candidates a full list keeps depends on the order the
        # atoms of a grid cell were dealt in
        if w[0] & REFUSALS:
            continue
        assert RC.same_raw(g, w), f"{where} frame {k} ({c['name']})"


def other_topology(group):
    name = "star16" if group[0]["name"] != "star16" else "block3"
    return [RC.case(name)] * 5


ONCE = 10000           # above this size (the 15 625-atom block) a frame goes through each device walk once


@pytest.mark.parametrize("group", [g for g in GROUPS if g[0]["n"] <= ONCE], ids=lambda g: g[0]["name"])
def test_every_frame_equals_the_host_build(hip_ctx, host, monkeypatch, group):
    grid = teams(monkeypatch)
    forwards = [group[k % len(group)] for k in range(3 * grid + 1)]
    for layout in LAYOUTS:
        with forced_layout(layout):
            for poison in (False, True):
                S.set_poison(False)
                launch(hip_ctx, other_topology(group), host)          # what the pool holds next is another topology's
                S.set_poison(poison)
                frames_as_the_host_build(hip_ctx, forwards, host, f"layout {layout} poison {poison} forwards")
                frames_as_the_host_build(hip_ctx, forwards[::-1], host, f"layout {layout} poison {poison} backwards")
    S.set_poison(False)


def test_the_largest_block_once_through_each_walk(hip_ctx, host, monkeypatch):
    """15 625 carbons, layers past RB_LWORK and a molecule past RB_LFINAL: one poisoned launch of one frame with the
    layout the device chooses (bit sets, the one-wave walk) and one with the bit sets forbidden (stamp arrays, the
    four-barrier team loop, whose list tails in global memory no smaller case reaches on the device)."""
    teams(monkeypatch)
    group = next(g for g in GROUPS if g[0]["n"] > ONCE)
    assert len(group) == 1 and RC.device_layout(group[0]["n"], False) == (True, False)
    for layout in (-1, 0):
        with forced_layout(layout):
            S.set_poison(False)
            launch(hip_ctx, other_topology(group), host)
            S.set_poison(True)
            frames_as_the_host_build(hip_ctx, group, host, f"layout {layout}")
    S.set_poison(False)


@pytest.mark.parametrize("name, bit", [("star17", "RB_ST_NB_OVERFLOW"), ("thin_below", "RB_ST_THIN_CELL"),
                                       ("thin_sheared_below", "RB_ST_THIN_CELL"), ("thin_reproducer", "RB_ST_THIN_CELL")])
def test_a_refused_frame_raises_and_names_its_status(hip_ctx, name, bit):
    from pywindow_amd import _lib
    from pywindow_amd import element_data as E
    from pywindow_amd import rebuild as RB

    c = RC.case(name)
    value = RC.constants()[bit]
    with pytest.raises(_lib.PwHipError, match=rf"status bits {value}: {value} = ") as err:
        RB.discrete_molecules(dict(c["system"]), rebuild=True if c["rebuild"] else None)
    assert _lib.rb_status_text(value) in str(err.value)
    topo = RC.topology_of(c)
    s = c["system"]
    coords, lat, inv = RB.pack_frames(s["coordinates"][None], s["lattice"][None] if "lattice" in s else None)
    with pytest.raises(_lib.PwHipError, match=rf"status bits {value}: {value} = "):
        hip_ctx.resident_from_cells(topo, E.VDW[E.element_ids(s["elements"])], coords, lat, inv, c["rebuild"])


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_resident_batches_with_different_molecule_counts(hip_ctx, host, hostsim, count):
    """pw_resident_from_cells on frames of one topology that hold one molecule or two: the unit and atom offsets of
    rb_scan_kernel (a run of frames per thread: 1, 1, 2 and 3 frames long here, the last runs short or empty) put
    every molecule where the host-marshalled batch has it."""
    from pywindow_amd import _lib, engine
    from pywindow_amd import element_data as E
    from pywindow_amd import rebuild as RB

    rng = np.random.default_rng(count)
    pool = [RC.case(n) for n in ("block7_cubic_1", "block7_split", "block7_cubic_3", "block7_split")]
    frames = [pool[int(k)] for k in rng.integers(0, len(pool), count)]
    assert {host(c)[1] for c in frames} == {1, 2}
    topo = RC.topology_of(frames[0])
    vdw = E.VDW[E.element_ids(frames[0]["system"]["elements"])]
    coords, lat, inv = RB.pack_frames(np.array([c["system"]["coordinates"] for c in frames]), np.array([c["system"]["lattice"] for c in frames]))
    res, n_mol = hip_ctx.resident_from_cells(topo, vdw, coords, lat, inv, True)
    try:
        assert list(n_mol) == [host(c)[1] for c in frames] and res.n_units == int(n_mol.sum())
        stages = _lib.STAGE_BASIC | _lib.STAGE_AVG
        res.launch(stages)
        got = res.download()
    finally:
        res.free()
    want = {}
    for c in pool:
        if c["name"] not in want:
            w = host(c)
            mols = RB.molecules_from_output(c["system"], w[1], w[2], w[3], w[5])
            assert min(len(m["elements"]) for m in mols) >= 20
            want[c["name"]] = engine.analyse([(m["elements"], m["coordinates"]) for m in mols], stages)
    at = 0
    for k, c in enumerate(frames):
        w = want[c["name"]]
        part = got[at:at + len(w)]
        for key in ("n_atoms", "mw", "com", "maxd", "pore_d", "avg_d"):
            assert np.array_equal(part[key], w[key]), (k, c["name"], key)
        at += len(w)
    assert at == len(got)
