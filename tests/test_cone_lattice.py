"""The ray tests' cone lattice (team_ray_tests, pw_unit.hpp): a narrowed atom's candidates are enumerated on the golden
spiral's lattice instead of walking its band.  (a) the enumeration against the brute-force set of the band -- every k
with dot >= thr, the kernel's own expression -- over sphere sizes, directions and half-angles made to sit on its edges;
(b) the unit pipeline compiled with and without it (-DPW_NO_CONE_LATTICE): every byte of every record the same."""
import ctypes
import importlib.util
import pathlib
import subprocess

import numpy as np
import pytest

from pywindow_amd import element_data as E, synth

import _cone_cases

ROOT = pathlib.Path(__file__).resolve().parents[1]
HOSTSIM = ROOT / "tests" / "hostsim"


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
    lib = _compile(tmp_path_factory.mktemp("cone"), "libconeprobe.so", "cone_probe.cpp")
    lib.hs_cone_candidates.restype = ctypes.c_int
    return lib


class Cone:
    def __init__(self, lib, P, R, rel, vr, cn):
        rel = np.ascontiguousarray(rel, dtype=np.float64)
        cand = np.zeros(P + 8, dtype=np.int32)
        info = np.zeros(8, dtype=np.int32)
        brute = np.zeros(P, dtype=np.uint8)
        vp = ctypes.c_void_p
        m = lib.hs_cone_candidates(ctypes.c_int(P), ctypes.c_double(R), rel.ctypes.data_as(vp), ctypes.c_double(vr),
                                   ctypes.c_double(cn), cand.ctypes.data_as(vp), ctypes.c_int(len(cand)), info.ctypes.data_as(vp),
                                   brute.ctypes.data_as(vp))
        assert 0 <= m <= len(cand)
        self.cand = cand[:m]
        self.klo, self.khi, self.narrowed, self.pieces, self.iters, self.two_sided = (int(x) for x in info[:6])
        self.hits = np.flatnonzero(brute)


def test_table_is_the_fibonacci_residues_of_the_golden_angle(probe):
    q = np.zeros(64, dtype=np.int32)
    s = np.zeros(64, dtype=np.float64)
    n = probe.hs_cone_table(q.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p))
    q, s = q[:n], s[:n]
    assert q[0] == 1 and q[1] == 2 and np.array_equal(q[2:], q[1:-1] + q[:-2]) and q[-1] >= 65536
    g = (3.0 - np.sqrt(5.0)) / 2.0
    exact = q * g - np.rint(q * g)
    assert np.all(np.abs(s - exact) <= 1e-10) and np.all(np.sign(s) == np.where(np.arange(n) % 2 == 0, 1.0, -1.0))
    assert np.allclose(np.abs(s[:-2]), np.abs(s[1:-1]) + np.abs(s[2:]), rtol=0, atol=1e-10)


def _directions():
    out = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    tiny = [0.0, 1e-300, 1e-12, 1e-7, 1e-3]
    for e in tiny[1:]:                          # beside the poles
        out += [(e, 0.0, 1.0), (0.0, -e, -1.0), (-e, e, 1.0)]
    for theta in np.linspace(0.05, np.pi - 0.05, 9):          # a grid
        for phi in np.linspace(-np.pi, np.pi, 7, endpoint=False) + 0.1:
            out.append((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)))
    for z in (0.0, 0.3, -0.7, 0.97):            # the equator and three latitudes: azimuth 0, +-pi and just either side
        r = np.sqrt(1.0 - z * z)
        for e in tiny:
            out += [(r, e, z), (r, -e, z), (-r, e, z), (-r, -e, z)]
        out += [(-r, -0.0, z), (0.0, r, z), (0.0, -r, z)]
    return [np.array(d) / np.linalg.norm(d) for d in out]


@pytest.mark.parametrize("P", [32, 33, 64, 100, 797, 947, 2100, 8448, 65535])
def test_candidates_hold_every_ray_of_the_band_that_passes_the_dot_test(probe, P):
    R, dist = 7.0, 9.0
    dirs = _directions()
    if P > 3000:                                # (the brute-force side is P sines and cosines per case)
        dirs = dirs[:: 4 if P < 10000 else 16] + dirs[:2]
    n_cases = n_narrowed = n_hits = 0
    for d in dirs:
        colat = float(np.arccos(np.clip(d[2], -1.0, 1.0)))
        to_pole = min(colat, np.pi - colat)
        # from a cone that holds no ray, to one that just misses the nearer pole, to ones that contain it
        alphas = [1e-7, 0.3 / P, 2.0 / np.sqrt(P), 0.05, 0.15, 0.4, 1.0, 1.5]
        alphas += [to_pole * f for f in (0.5, 1.0 - 1e-3, 1.0 - 1e-6, 1.0 - 1e-9, 1.0, 1.0 + 1e-9, 1.0 + 1e-6, 1.0 + 1e-3, 1.5) if 0.0 < to_pole * f < 1.55]
        for alpha in alphas:
            for cn in (0.0, 2.0):
                c = Cone(probe, P, R, d * dist, dist * np.sin(alpha), cn)
                missing = np.setdiff1d(c.hits, c.cand)
                assert missing.size == 0, (P, tuple(d), alpha, cn, missing[:8], c.klo, c.khi, c.narrowed)
                assert c.cand.size == np.unique(c.cand).size and (c.cand.size == 0 or (c.klo <= c.cand.min() and c.cand.max() <= c.khi))
                n_cases += 1
                n_narrowed += c.narrowed
                n_hits += c.hits.size
    assert n_narrowed >= n_cases // 3 and n_hits > 0            # (the enumeration had work to do)


def test_synthetic_cc3_frames_are_narrowed(probe):
    elements, frames = synth.synthetic_units(4)
    ids = E.element_ids(elements)
    vdw, mass = E.VDW[ids], E.MASS[ids]
    atoms = whole = cand = pairs = iters = 0
    for xyz in frames:
        com = (xyz * mass[:, None]).sum(axis=0) / mass.sum()
        rel = xyz - com
        R = float(np.linalg.norm(rel, axis=1).max())
        P = int(np.log10(4.0 * np.pi * R * R) * 250.0)
        for i in range(len(rel)):
            c = Cone(probe, P, R, rel[i], float(vdw[i]), 0.0)          # (the unit pipeline shifts a molecule to its centre)
            assert np.setdiff1d(c.hits, c.cand).size == 0
            atoms += 1
            if c.narrowed:
                cand += c.cand.size
                pairs += c.hits.size
                iters += c.iters
            else:
                whole += 1
    print(f"atoms {atoms}, not narrowed {whole} ({100.0 * whole / atoms:.1f} %), candidates / pairs on the narrowed "
          f"{cand} / {pairs} = {cand / pairs:.3f}, loop iterations per narrowed atom {iters / (atoms - whole):.1f}")
    assert whole <= 0.20 * atoms          # (a numpy model of the enumeration gives 10 %: the cones that hold a pole)
    assert cand <= 2.0 * pairs            # (the model gives 1.35)


def test_records_with_and_without_the_cone_lattice_are_the_same_bytes(tmp_path):
    from test_scan_lists import _molecules, _run

    with_lattice = _compile(tmp_path, "libunitprobe_lattice.so", "unit_probe.cpp")
    without = _compile(tmp_path, "libunitprobe_nolattice.so", "unit_probe.cpp", "-DPW_NO_CONE_LATTICE")
    elements, frames = synth.synthetic_units(6)
    mols = [(elements, np.ascontiguousarray(f)) for f in frames] + _molecules(400, 2026) + _cone_cases.special_molecules(48, 7)
    a, b = _run(with_lattice, mols), _run(without, mols)
    assert (a["n_windows"] > 0).sum() >= 60 and (a["n_survivors"] > 0).sum() >= 120      # (the ray tests had work to do)
    differ = [u for u in range(len(mols)) if a[u].tobytes() != b[u].tobytes()]
    assert not differ, differ[:10]
    assert a.tobytes() == b.tobytes()
