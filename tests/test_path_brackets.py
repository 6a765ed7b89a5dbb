"""The sampling stage's path scans from the two points that bracket each atom (path_bracket_thread behind the guard of
path_steps, pw_unit.hpp) against the scan of every point (path_scan_thread): (a) one path by both forms -- ok and 2 * best
must be the same bits, with at most two evaluations per listed atom where the guard holds -- on atoms placed at the
edges of the bracket; (b) the unit pipeline compiled with and without it (-DPW_NO_PATH_BRACKETS): every byte of every
record the same; (c) the same with team memory pre-filled with 0xff and with zeros."""
import ctypes
import importlib.util
import os
import pathlib
import subprocess

import numpy as np
import pytest

from pywindow_amd import element_data as E, synth

ROOT = pathlib.Path(__file__).resolve().parents[1]
HOSTSIM = ROOT / "tests" / "hostsim"
INCREMENTS = (0.3, 0.7, 1.0, 2.5)
CHUNKS = (0, 1, 2, 11, 17, 40)


def _flags():
    spec = importlib.util.spec_from_file_location("hostsim_build_flags", HOSTSIM / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS


def _compile(tmp, so, src, *extra):
    out = tmp / so
    subprocess.check_call(["g++", *_flags(), *extra, "-o", str(out), str(HOSTSIM / src)])
    return ctypes.CDLL(str(out))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("paths"), "libpathprobe.so", "path_probe.cpp")


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("units")
    return (_compile(tmp, "libunitprobe_brackets.so", "unit_probe.cpp"),
            _compile(tmp, "libunitprobe_nobrackets.so", "unit_probe.cpp", "-DPW_NO_PATH_BRACKETS"))


class Path:
    def __init__(self, lib, xyz, vdw, v, inc, use_list):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        vdw = np.ascontiguousarray(vdw, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert len(vdw) == len(xyz)
        res = np.zeros(16, dtype=np.int64)
        vp = ctypes.c_void_p
        rc = lib.hs_path_both(ctypes.c_int(len(xyz)), xyz.ctypes.data_as(vp), vdw.ctypes.data_as(vp), v.ctypes.data_as(vp),
                              ctypes.c_double(inc), ctypes.c_int(use_list), res.ctypes.data_as(vp))
        assert rc == 0
        self.plain = (int(res[0]), int(res[1]))
        self.stage = (int(res[2]), int(res[3]))
        self.guard, self.terms, self.listed, self.chunks = bool(res[4]), int(res[5]), int(res[6]), int(res[7])
        self.n_eval = (int(res[8]), int(res[9]))
        self.groups = int(res[10])
        self.ok = bool(res[0])


class Tally:
    def __init__(self):
        self.cases = self.guarded = self.ok = self.terms = self.listed = 0


def _check(lib, xyz, vdw, v, inc, tally, expect_guard=None, note=None):
    out = []
    for use_list in (0, 1):
        p = Path(lib, xyz, vdw, v, inc, use_list)
        assert p.stage == p.plain, (note, use_list, p.plain, p.stage, p.guard, p.chunks)
        assert p.n_eval[0] == p.n_eval[1]
        if p.guard:
            assert p.terms <= 2 * p.listed and p.chunks >= 1 and p.groups > 0
        else:
            assert p.terms == 0
        if expect_guard is not None:
            assert p.guard == expect_guard, (note, use_list, p.chunks, p.groups)
        tally.cases += 1
        tally.guarded += p.guard
        tally.ok += p.ok and p.guard
        tally.terms += p.terms
        tally.listed += p.listed if p.guard else 0
        out.append(p)
    return out


RADII = np.array([1.2, 1.7, 1.55, 1.52, 1.8, 1.47, 1.75, 1.85, 1.98, 2.1, 1.1])


def _cloud(rng, n, kind):
    p = rng.normal(size=(n, 3))
    if kind == 0:          # a shell
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(3.0, 12.0) + rng.normal(scale=rng.uniform(0.0, 0.5), size=(n, 3))
    elif kind == 1:        # a blob
        p = p * rng.uniform(0.5, 6.0)
    else:                  # a lattice fragment with a hole: many equal distances
        g = np.array([(x, y, z) for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)], dtype=np.float64) * 1.6
        g = g[np.linalg.norm(g, axis=1) > 3.0]
        p = g[rng.permutation(len(g))[: min(n, len(g))]]
    return np.ascontiguousarray(p)


def test_random_shells_blobs_and_lattices_give_the_bits_of_the_plain_scan(probe):
    rng = np.random.default_rng(8)
    tally = Tally()
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 113, 168, 300]
    for case in range(252):
        n = sizes[case % len(sizes)] if case % 3 else int(rng.integers(1, 301))
        kind = case % 3
        xyz = _cloud(rng, n, kind)
        n = len(xyz)
        n_radii = (1, 3, 10)[(case // 3) % 3]
        vdw = RADII[rng.integers(0, n_radii, size=n)]
        if case % 7 == 0:
            xyz = xyz + rng.normal(scale=500.0, size=3)          # a molecule 500 A from the origin
        inc = INCREMENTS[case % 4]
        chunks = CHUNKS[(case // 4) % 6]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        # (along the lattice's axes and diagonals too: there many atoms tie)
        if kind == 2 and case % 2:
            d = np.array([(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 1.0, 1.0)][(case // 2) % 4])
            d /= np.linalg.norm(d)
        for length in ((chunks + 0.5) * inc, chunks * inc, np.nextafter(chunks * inc, 0.0)):
            ps = _check(probe, xyz, vdw, d * length, inc, tally, note=("random", case, length))
            for p in ps:
                # (more than PW_KCLS radii are not grouped, a path without a second point has no bracket: the plain scan)
                if p.chunks < 1 or p.groups == 0:
                    assert not p.guard
                elif np.abs(xyz).max() < 2000.0:
                    assert p.guard
    print(f"paths {tally.cases}, by brackets {tally.guarded}, of them ok {tally.ok}, evaluations per listed atom "
          f"{tally.terms / max(tally.listed, 1):.3f}")
    assert tally.guarded >= tally.cases // 2 and tally.ok >= 50            # (the bracket form had work to do)


def test_atoms_at_the_edges_of_the_bracket(probe):
    tally = Tally()
    far = [(-9.0, 0.0, 0.0), (0.0, 0.0, 9.0)]          # (a molecule around the origin, so that m0 > 0)
    for inc, chunks in ((1.0, 11), (0.7, 17), (2.5, 2), (0.3, 40), (1.0, 1), (1.0, 2)):
        length = chunks * inc + 0.25 * inc
        c = length / chunks                          # the step along x
        for r in (1.2, 1.7):
            for off in (2.5, 4.0, r, 0.5 * r, 0.0):      # beside the path, touching it, on it
                ts = [1.0, 2.0, float(chunks), float(chunks // 2 + 1),            # t* an integer
                      1.5, chunks - 0.5, chunks // 2 + 0.5,                       # a half-integer: two points tie
                      0.999, 0.5, 1.0 - 1e-15, 1.0 + 1e-15,                       # below 1 and at it
                      chunks + 1e-15 * chunks, chunks + 0.5, chunks + 3.0, 1e6,   # above chunks
                      -1e-300, -0.5, -3.0, -1e6,                                  # negative
                      np.nextafter(3.0, 0.0), np.nextafter(3.0, 9.0), np.nextafter(2.5, 0.0), np.nextafter(2.5, 9.0)]
                for t in ts:
                    if np.hypot(t * c, off) <= r + 0.05:
                        continue                     # (the origin is not inside the atom: m0 > 0)
                    for axis in range(3):
                        atom = np.roll(np.array([t * c, off, 0.0]), axis)
                        v = np.roll(np.array([length, 0.0, 0.0]), axis)
                        xyz = np.array([atom] + [np.roll(np.array(f), axis) for f in far])
                        _check(probe, xyz, np.array([r, 1.7, 1.2]), v, inc, tally, expect_guard=True, note=("edge", inc, chunks, r, off, t))
    # two atoms of one group at the same distance from two different points of the path, and a third tying with both
    for inc, length in ((1.0, 11.5), (0.7, 9.0), (2.5, 26.0)):
        chunks = int(length // inc)
        c = length / chunks
        for ka, kb in ((3, chunks - 1), (1, chunks), (2, 3)):
            for h in (4.0, 1.0):
                xyz = np.array([(ka * c, h, 0.0), (kb * c, 0.0, h), (kb * c, -h, 0.0), (-9.0, 0.0, 0.0)])
                ps = _check(probe, xyz, np.array([1.7, 1.7, 1.7, 1.7]), (length, 0.0, 0.0), inc, tally, expect_guard=True, note=("tie", ka, kb, h))
                assert all(p.ok == (h > 1.7) for p in ps)
    assert tally.guarded == tally.cases and tally.ok >= tally.cases // 4
    assert tally.terms <= 2 * tally.listed


def test_guard_refuses_where_the_margin_is_not_proven(probe):
    rng = np.random.default_rng(3)
    xyz0 = _cloud(rng, 60, 0)
    vdw = RADII[rng.integers(0, 3, size=60)]
    d = np.array([0.6, -0.64, 0.48])
    held = []
    tally = Tally()
    for e in range(0, 13):                       # a molecule 10^e A from the origin, a path of eleven steps of 0.3 A
        xyz = xyz0 + np.array([1.0, 1.0, 1.0]) * (10.0 ** e if e else 0.0)
        ps = _check(probe, xyz, vdw, d * 3.4, 0.3, tally, note=("scaled", e))
        held.append(all(p.guard for p in ps))
        assert all(p.guard for p in ps) or not any(p.guard for p in ps)
    # 0.09 (1 - 1e-6) > 64 * 2^-53 * 3e(2 e): up to 1e6 A it holds, from 1e7 A on it cannot
    assert held[:7] == [True] * 7 and held[7:] == [False] * 6, held
    # a path a step of which is not finite, and one of no length
    for v in ((np.inf, 0.0, 0.0), (1e200, 1e200, 0.0), (0.0, 0.0, 0.0)):
        _check(probe, xyz0, vdw, np.array(v), 0.3, tally, expect_guard=False, note=("odd", v))
    # eleven radii: not grouped
    _check(probe, xyz0, RADII[np.arange(60) % 11], d * 3.4, 0.3, tally, expect_guard=False, note="ungrouped")


def _mols():
    from test_scan_lists import _molecules

    elements, frames = synth.synthetic_units(6)
    return [(elements, np.ascontiguousarray(f)) for f in frames] + _molecules(400, 2026)


@pytest.fixture(scope="module")
def records(builds):
    from test_scan_lists import _run

    mols = _mols()
    return mols, _run(builds[0], mols), _run(builds[1], mols)


def test_records_with_and_without_the_brackets_are_the_same_bytes(records):
    mols, a, b = records
    assert (a["n_windows"] > 0).sum() >= 60 and (a["n_survivors"] > 0).sum() >= 120      # (the scans had work to do)
    differ = [u for u in range(len(mols)) if a[u].tobytes() != b[u].tobytes()]
    assert not differ, differ[:10]
    assert a.tobytes() == b.tobytes()


def test_records_do_not_depend_on_what_team_memory_held(builds, records, monkeypatch):
    from test_scan_lists import _run

    mols, a, _ = records
    sub = mols[:6] + mols[6::5]
    want = np.concatenate([a[:6], a[6::5]])
    for fill in ("0xff", "0x00"):
        monkeypatch.setenv("HS_LDS_FILL", fill)
        assert os.environ["HS_LDS_FILL"] == fill
        for lib in builds:
            assert _run(lib, sub).tobytes() == want.tobytes(), fill
