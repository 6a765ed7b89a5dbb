"""The wave-level bracket scan (wave_path_bracket behind the guard of path_steps, pw_unit.hpp): lanes over atoms, each atom
at the two points of a path that bracket it, for the refined path of a window (from point 0: is every gap > 0, the
smallest gap, the FIRST point that has it) and for the left-over paths of the sampling stage (from point 1: ok and the
smallest gap).  (a) one path by the plain walk and by the scan -- ok, the bits of the smallest gap and, from point 0, its
position -- on atoms placed at the edges of the bracket, on the path, tying at different points, lattice fragments along
lattice directions, every chunk count and atom count at which a wave takes another pass; (b) the unit pipeline compiled with
and without it (-DPW_NO_PATH_BRACKETS): records and stage captures byte for byte, at five steps of the refined path, and
with team memory pre-filled with 0xff and with zeros."""
import ctypes
import importlib.util
import pathlib
import subprocess

import numpy as np
import pytest

from pywindow_amd import _lib, element_data as E, synth

ROOT = pathlib.Path(__file__).resolve().parents[1]
HOSTSIM = ROOT / "tests" / "hostsim"
CHUNKS = (1, 2, 15, 16, 17, 127, 128, 129, 300)
SIZES = (1, 2, 63, 64, 65, 128, 129, 300)
RADII = np.array([1.2, 1.7, 1.55, 1.52, 1.8, 1.47, 1.75, 1.85, 1.98, 2.1, 1.1])


def _flags():
    spec = importlib.util.spec_from_file_location("hostsim_build_flags", HOSTSIM / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refined")
    libs = []
    for so, extra in (("librefined_brackets.so", []), ("librefined_nobrackets.so", ["-DPW_NO_PATH_BRACKETS"])):
        subprocess.check_call(["g++", *_flags(), *extra, "-o", str(tmp / so), str(HOSTSIM / "refined_probe.cpp")])
        libs.append(ctypes.CDLL(str(tmp / so)))
    return libs


class Path:
    def __init__(self, lib, xyz, vdw, v, inc, k_first):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        vdw = np.ascontiguousarray(vdw, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert len(vdw) == len(xyz)
        res = np.zeros(16, dtype=np.int64)
        vp = ctypes.c_void_p
        rc = lib.hs_refined_both(ctypes.c_int(len(xyz)), xyz.ctypes.data_as(vp), vdw.ctypes.data_as(vp), v.ctypes.data_as(vp),
                                 ctypes.c_double(inc), ctypes.c_int(k_first), res.ctypes.data_as(vp))
        assert rc == 0
        self.n = len(xyz)
        self.plain = (int(res[0]), int(res[1]), int(res[2]))
        self.stage = (int(res[3]), int(res[4]), int(res[5]))
        self.ok, self.gap, self.pos = bool(res[0]), float(np.int64(res[1]).view(np.float64)), int(res[2])
        self.guard, self.terms, self.chunks, self.groups = bool(res[6]), int(res[7]), int(res[8]), int(res[9])


class Tally:
    def __init__(self):
        self.cases = self.guarded = self.ok = 0
        self.reached = set()


def _check(lib, xyz, vdw, v, inc, tally, expect_guard=None, note=None, cls=None):
    """One path from point 0 and from point 1 by both forms; the Path from point 0."""
    out = None
    for k_first in (0, 1):
        p = Path(lib, xyz, vdw, v, inc, k_first)
        # ok, the bits of the smallest gap; the position where it is wanted (from point 0)
        assert p.stage[:2] == p.plain[:2], (note, k_first, p.plain, p.stage, p.guard, p.chunks)
        if k_first == 0:
            assert p.stage[2] == p.plain[2], (note, p.plain, p.stage, p.guard, p.chunks)
        if p.guard:
            assert 0 < p.terms <= 2 * p.n and p.chunks >= 1 and p.groups > 0
        else:
            assert p.terms == 0
        if expect_guard is not None:
            assert p.guard == expect_guard, (note, k_first, p.chunks, p.groups)
        tally.cases += 1
        tally.guarded += p.guard
        tally.ok += p.ok and p.guard
        if cls and p.guard:
            tally.reached.add(cls)
            tally.reached.add(("chunks", p.chunks))
            tally.reached.add(("n", p.n))
        if k_first == 0:
            out = p
    return out


def _cloud(rng, n, kind, spacing=1.6):
    p = rng.normal(size=(n, 3))
    if kind == 0:          # a shell
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(3.0, 12.0) + rng.normal(scale=rng.uniform(0.0, 0.5), size=(n, 3))
    elif kind == 1:        # a blob
        p = p * rng.uniform(0.5, 6.0)
    else:                  # a lattice fragment with a hole: many equal distances
        g = np.array([(x, y, z) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)], dtype=np.float64) * spacing
        g = g[np.linalg.norm(g, axis=1) > 3.0]
        p = g[rng.permutation(len(g))[: min(n, len(g))]]
    return np.ascontiguousarray(p)


def test_atoms_at_the_edges_of_the_bracket_and_on_the_path(builds):
    probe = builds[0]
    tally = Tally()
    far = [(-9.0, 0.0, 0.0), (0.0, 0.0, 9.0)]
    negative = 0
    for chunks in CHUNKS:
        inc = 0.25 if chunks <= 17 else 0.0625          # (a path of 0.3 to 19 A)
        length = chunks * inc + 0.25 * inc
        c = length / chunks                          # the step along the axis
        mid = chunks // 2
        for r in (1.2, 1.7):
            for off in (2.5, 4.0, r, 0.5 * r, 0.0):      # beside the path, touching it, inside the atom, on its centre
                ts = [(0.0, "integer"), (1.0, "integer"), (float(chunks), "integer"), (float(mid + 1), "integer"),
                      (0.5, "half"), (1.5, "half"), (chunks - 0.5, "half"), (mid + 0.5, "half"),
                      (0.999, "near"), (1.0 - 1e-15, "near"), (1.0 + 1e-15, "near"), (np.nextafter(mid + 1.0, 0.0), "near"),
                      (np.nextafter(mid + 1.0, 1e9), "near"), (np.nextafter(mid + 0.5, 0.0), "near"),
                      (-1e-300, "below"), (-0.5, "below"), (-3.0, "below"), (-1e6 * inc, "below"),
                      (chunks * (1.0 + 1e-15), "beyond"), (chunks + 0.5, "beyond"), (chunks + 3.0, "beyond"), (chunks + 1e6 * inc, "beyond")]
                for t, where in ts:
                    for axis in range(3):
                        atom = np.roll(np.array([t * c, off, 0.0]), axis)
                        v = np.roll(np.array([length, 0.0, 0.0]), axis)
                        xyz = np.array([atom] + [np.roll(np.array(f), axis) for f in far])
                        p = _check(probe, xyz, np.array([r, 1.7, 1.2]), v, inc, tally, expect_guard=True,
                                   note=("edge", chunks, r, off, t), cls=where)
                        if off < r and 0.0 <= t <= chunks:
                            assert not p.ok and p.gap < 0.0          # (an atom ON the path: the window is dropped)
                            negative += 1
                            tally.reached.add("on the path")
    assert tally.guarded == tally.cases and tally.ok >= tally.cases // 4 and negative >= 100
    for cls in ("integer", "half", "near", "below", "beyond", "on the path"):
        assert cls in tally.reached, cls
    assert {("chunks", k) for k in CHUNKS} <= tally.reached


def test_two_atoms_of_different_radii_tie_at_different_points(builds):
    probe = builds[0]
    tally = Tally()
    # steps of 0.25 A along an axis, atoms 3.0 and 3.25 A beside points ka and kb with radii 1.5 and 1.75: every number is
    # exact, both gaps are 1.5 -- the FIRST of the two points is wanted whichever atom comes first
    for chunks in (2, 16, 17, 129):
        for ka, kb in ((0, 1), (1, 0), (1, chunks), (chunks, 1), (chunks // 2, chunks // 2 + 1), (chunks, 0), (0, chunks), (1, 1)):
            for axis in range(3):
                for flip in (False, True):
                    a = np.roll(np.array([ka * 0.25, 3.0, 0.0]), axis)
                    b = np.roll(np.array([kb * 0.25, 0.0, 3.25]), axis)
                    farther = np.roll(np.array([-9.0, 0.0, 0.0]), axis)
                    xyz, vdw = np.array([a, b, farther]), np.array([1.5, 1.75, 1.2])
                    if flip:
                        xyz, vdw = xyz[[1, 0, 2]], vdw[[1, 0, 2]]
                    v = np.roll(np.array([chunks * 0.25, 0.0, 0.0]), axis)
                    p = _check(probe, xyz, vdw, v, 0.25, tally, expect_guard=True, note=("tie", chunks, ka, kb, axis, flip), cls="tie")
                    assert p.ok and p.gap == 1.5 and p.pos == min(ka, kb) and p.chunks == chunks
    assert tally.guarded == tally.cases == tally.ok


def test_random_shells_blobs_and_lattices_give_the_bits_and_the_place_of_the_plain_walk(builds):
    probe = builds[0]
    rng = np.random.default_rng(9)
    tally = Tally()
    ungrouped = lattice_ties = 0
    for case in range(216):
        n = SIZES[case % len(SIZES)]
        kind = case % 3
        # (a lattice of 1.5 A with steps of 0.375 or 0.75 A along its axes: exact ties at different points)
        xyz = _cloud(rng, n, kind, spacing=1.5)
        n = len(xyz)
        n_radii = (1, 3, 8, 9, 11)[(case // 3) % 5]
        vdw = RADII[np.arange(n) % n_radii] if n >= n_radii else RADII[rng.integers(0, n_radii, size=n)]
        chunks = CHUNKS[(case // 8) % len(CHUNKS)]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        inc = rng.uniform(1.0, 6.0) / (chunks + 0.5)
        length = (chunks + 0.5) * inc
        v = d * length
        along = kind == 2 and case % 2 == 1
        if along:
            # (the diagonal's steps do not divide the lattice: near ties instead of exact ones)
            d = np.array([(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0)][(case // 2) % 4])
            inc = (0.375, 0.75)[(case // 6) % 2]
            v = d * ((2, 8, 16)[(case // 12) % 3] * inc)
        p = _check(probe, xyz, vdw, v, inc, tally, note=("random", case), cls="lattice" if along else "random")
        grouped = len(set(vdw)) <= 8
        assert p.guard == grouped, (case, p.groups, p.chunks)          # (nine radii or more are not grouped)
        ungrouped += not grouped
        lattice_ties += along and p.guard
    print(f"paths {tally.cases}, by brackets {tally.guarded}, of them ok {tally.ok}")
    assert tally.guarded >= tally.cases // 2 and tally.ok >= 20 and ungrouped >= 20 and lattice_ties >= 20
    assert {("n", n) for n in SIZES if n <= 300} <= tally.reached and {"random", "lattice"} <= tally.reached
    assert {("chunks", k) for k in CHUNKS} <= tally.reached


def test_guard_refuses_where_the_margin_is_not_proven(builds):
    probe = builds[0]
    rng = np.random.default_rng(4)
    xyz0 = _cloud(rng, 60, 0)
    vdw = RADII[rng.integers(0, 3, size=60)]
    d = np.array([0.6, -0.64, 0.48])
    tally = Tally()
    held = []
    for e in range(0, 13):                       # a molecule 10^e A from the origin, a path of 34 steps of 0.1 A
        xyz = xyz0 + np.array([1.0, 1.0, 1.0]) * (10.0 ** e if e else 0.0)
        held.append(_check(probe, xyz, vdw, d * 3.45, 0.1, tally, note=("scaled", e)).guard)
    # 0.01 (1 - 1e-6) > 64 * 2^-53 * 3e(2 e): up to 1e5 A it holds, from 1e6 A on it cannot
    assert held == [True] * 6 + [False] * 7, held
    for v in ((np.inf, 0.0, 0.0), (1e200, 1e200, 0.0), (0.0, 0.0, 0.0), (0.05, 0.0, 0.0)):      # not finite, no length, no step
        _check(probe, xyz0, vdw, np.array(v), 0.1, tally, expect_guard=False, note=("odd", v))
    for n_radii in (9, 10, 11):
        _check(probe, xyz0, RADII[np.arange(60) % n_radii], d * 3.45, 0.1, tally, expect_guard=False, note="ungrouped")
    _check(probe, xyz0, RADII[np.arange(60) % 8], d * 3.45, 0.1, tally, expect_guard=True, note="eight radii")


# ---- (b) the pipeline with and without ------------------------------------------------------------------------------
def _run(lib, mols, prm, stages=_lib.STAGE_WINDOWS):
    """Records and stage captures of a batch of (elements, coordinates) under prm."""
    off = np.zeros(len(mols) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(el) for el, _ in mols])
    ids = [E.element_ids(el) for el, _ in mols]
    xyz = np.ascontiguousarray(np.concatenate([p for _, p in mols]))
    vdw = np.ascontiguousarray(np.concatenate([E.VDW[i] for i in ids]))
    mass = np.ascontiguousarray(np.concatenate([E.MASS[i] for i in ids]))
    out = np.zeros(len(mols), dtype=_lib.UNIT_OUT_DTYPE)
    dbg = np.zeros(len(mols), dtype=_lib.UNIT_DEBUG_DTYPE)
    assert lib.hs_sizeof_unit_debug() == dbg.dtype.itemsize and lib.hs_sizeof_unit_out() == out.dtype.itemsize
    vp = ctypes.c_void_p
    rc = lib.hs_analysis_debug_params(ctypes.c_long(len(mols)), off.ctypes.data_as(vp), xyz.ctypes.data_as(vp), vdw.ctypes.data_as(vp),
                                      mass.ctypes.data_as(vp), ctypes.c_uint(stages), out.ctypes.data_as(vp), ctypes.byref(prm),
                                      dbg.ctypes.data_as(vp))
    assert rc == 0
    return out, dbg


def _units():
    from test_cliffs import load_cliffs

    elements, frames = synth.synthetic_units(6)
    cliffs, calls = load_cliffs()
    plain = [(elements, np.ascontiguousarray(f)) for f in frames] + [cliffs[k] for k in ("cc3", "windows_case_2", "windows_case_5", "shell20")]
    odd = [(cliffs[c["mol"]], c["kwargs"]) for c in calls if c["dropped"] or c["negative"]]
    assert len(odd) == 5
    return plain, odd


@pytest.fixture(scope="module")
def settings(builds):
    plain, odd = _units()
    r = _run(builds[0], plain, _lib.Params())[0]["sphere_r"]
    assert (r > 0).all()
    # 0.1, 0.05 and 0.37; one that gives every refined path of the smallest sphere a single step; one larger than every sphere
    return (0.1, 0.05, 0.37, float(r.min()) / 1.5, 2.0 * float(r.max()))


def test_records_and_captures_with_and_without_the_brackets_are_the_same_bytes(builds, settings):
    plain, odd = _units()
    fitted = dropped = negative = 0
    for k, inc2 in enumerate(settings):
        a, da = _run(builds[0], plain, _lib.Params(increment2=inc2))
        b, db = _run(builds[1], plain, _lib.Params(increment2=inc2))
        differ = [u for u in range(len(plain)) if a[u].tobytes() != b[u].tobytes() or da[u].tobytes() != db[u].tobytes()]
        assert not differ, (inc2, differ)
        assert a.tobytes() == b.tobytes() and da.tobytes() == db.tobytes()
        assert (a["n_clusters"] > 0).all()
        if k < 3:
            assert (a["n_windows"] > 0).all()
            fitted += int(a["n_windows"].sum())
        if k == 4:                                   # no step: every window is dropped
            assert (a["n_windows"] == 0).all() and (a["status"] & _lib.ST_WINDOW_DROPPED).all()
    assert fitted >= 60
    # the units with dropped and negative windows, under their own steps and under the others
    for (el, xyz), kw in odd:
        for inc2 in (kw.get("increment2", 0.1),) + tuple(settings):
            prm = _lib.Params(increment=kw["increment"], increment2=inc2)
            a, da = _run(builds[0], [(el, xyz)], prm)
            b, db = _run(builds[1], [(el, xyz)], prm)
            assert a.tobytes() == b.tobytes() and da.tobytes() == db.tobytes(), (kw, inc2)
            dropped += bool(a["status"][0] & _lib.ST_WINDOW_DROPPED)
            negative += bool(a["status"][0] & _lib.ST_WINDOW_NEGATIVE)
    assert dropped >= 3 and negative >= 2


def test_records_and_captures_do_not_depend_on_what_team_memory_held(builds, settings, monkeypatch):
    plain, odd = _units()
    sub = plain[:2] + plain[6:8] + [odd[0][0], odd[3][0]]
    for inc2 in settings[:1] + settings[3:4]:
        prm = _lib.Params(increment2=inc2)
        monkeypatch.delenv("HS_LDS_FILL", raising=False)
        want = _run(builds[0], sub, prm)
        for fill in ("0xff", "0x00"):
            monkeypatch.setenv("HS_LDS_FILL", fill)
            for lib in builds:
                got = _run(lib, sub, prm)
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (fill, inc2)
