"""Guest affinity on the host path (device = -1): pw_affinity against the definition (tests/_affinity_cases.py: reference)
as BYTES, case by case and as one batch with entries nobody owns; ties at the core and at the cutoff, tied minima, the
clamp, regions that are empty or all blocked; the refusals; pw_exp on (0, 700] against a long-double exp; the accuracy
of the sums against a long-double evaluation; and the Python layers above the entry (pywindow_amd.affinity,
Molecule.calculate_guest_affinity on CC3, DLPOLY.affinity).  tests/test_gpu_affinity.py holds the device to the same.

Measured here (host path):
    pw_exp on (0, 700]: 0.5063 ulp at most over 1.39e6 arguments, the neighbours of every reduction boundary among
    them (bar 1 ulp)
    jittered CC3, Xe at 298 K, 1139 voxels: Z off by 2.9e-16 and E by 2.2e-17 of the long-double values; plain float64
    numpy with numpy.sum by 7.9e-17 and 2.2e-17 (bar max(4 E_numpy, 64 * 2^-53 = 7.1e-15))
"""
import numpy as np
import pytest

import _affinity_cases as C
import _kde_cases as K
import pywindow_amd as pw
from pywindow_amd import _lib, affinity, engine, synth

LD = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


@pytest.fixture()
def on_the_host():
    engine.set_default_device(-1)
    yield
    engine.set_default_device(None)


def by_name(name):
    return [c for c in C.cases() if c.name == name][0]


def run(host, c):
    rc, got = C.raw(host, C.pack([c]))
    assert rc == 0
    return got


def test_every_case_one_job_at_a_time(host):
    """The first test of this file: it fails where the library has no pw_affinity."""
    assert hasattr(_lib.load(), "pw_affinity")
    for c in C.cases() + C.big_cases():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    names = {c.name for c in C.cases()}
    assert {f"V={v}" for v in (0, 1, 63, 64, 65, 128, 129)} <= names
    assert {f"n={n}" for n in (0, 1, C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1)} <= names
    assert len(C.big_cases()[0].xyz) == 5000 and C.big_cases()[1].dims == (64, 64, 64)


def test_regions(host):
    for v in (0, 1, 63, 64, 65, 128, 129):
        out = run(host, by_name(f"V={v}"))[0]
        assert out["n_voxels"][0] == v
    out, levels, _, _ = run(host, by_name("V=0"))
    assert out["u_min"][0] == np.inf and (out["min_voxel"][0] == -1).all() and levels["z"].tolist() == [0.0, 0.0]
    assert not np.signbit(levels["z"]).any() and not np.signbit(levels["e"]).any()
    for bit in (0, 63):
        out = run(host, by_name(f"bit-{bit}-alone"))[0]
        assert out["n_voxels"][0] == 1 and out["min_voxel"][0].tolist() == [bit, 0, 1]
    for nx in (5, 63, 64):
        assert run(host, by_name(f"nx={nx}-junk-bits"))[0]["n_voxels"][0] == nx * 6
    assert run(host, by_name("no-mask-3x2x2"))[0]["n_voxels"][0] == 12
    assert run(host, by_name("no-mask-64x1x1"))[0]["n_voxels"][0] == 64


def test_without_atoms_z_is_the_count(host):
    out, levels, hist, energies = run(host, by_name("n=0"))
    assert levels["z"].tolist() == [100.0, 100.0] and levels["e"].tolist() == [0.0, 0.0]
    assert hist.tolist() == [0, 0, 100] and (energies == 0.0).all() and out["u_min"][0] == 0.0 and out["n_blocked"][0] == 0
    l, j, i = (v[0] for v in np.nonzero(C.region(by_name("n=0"))))
    assert out["min_voxel"][0].tolist() == [i, j, l]


def test_ties_at_the_core_and_at_the_cutoff(host):
    """The atom sits on voxel 2: r2 = 0 there and r2 == core2 at voxels 1 and 3, all blocked; voxel 5 is exactly at
    r2 == cutoff2 and counts, voxel 6 is the next one out and does not."""
    out, levels, hist, energies = run(host, by_name("ties"))
    assert np.isinf(energies[[1, 2, 3]]).all() and out["n_blocked"][0] == 3
    assert energies[5] == (1.0 / 729.0) * (3.0 * (1.0 / 729.0) - 2.0) and energies[5] != 0.0
    assert energies[6] == 0.0 and energies[7] == 0.0 and not np.signbit(energies[6])
    assert energies[0] == energies[4] == (1.0 / 64.0) * (3.0 / 64.0 - 2.0)
    assert hist[0] == 3                                              # voxels 0, 4, 5; U == 0.0 is not below the edge 0.0


def test_a_tied_minimum_goes_to_the_lower_rank_and_a_clamped_job_says_so(host):
    out, levels, _, energies = run(host, by_name("tied-minimum"))
    assert energies[2] == energies[3] == -64.0 == out["u_min"][0] and out["min_voxel"][0].tolist() == [2, 0, 0]
    assert out["flags"][0] == C.CLAMPED and np.isfinite(levels["z"]).all()
    assert run(host, by_name("ties"))[0]["flags"][0] == 0


def test_all_blocked(host):
    out, levels, hist, energies = run(host, by_name("all-blocked"))
    assert out["n_blocked"][0] == out["n_voxels"][0] == 24 and out["u_min"][0] == np.inf
    assert (out["min_voxel"][0] == -1).all() and np.isinf(energies).all() and hist[0] == 0
    assert levels["z"][0] == 0.0 and levels["e"][0] == 0.0 and out["flags"][0] == 0


def test_an_energy_equal_to_an_edge_is_not_below_it(host):
    c, value = C.with_edge_on_a_voxel(host)
    rc, got = C.raw(host, C.pack([c]))
    want = C.expected([c], host)
    assert rc == 0 and C.same(got, want)
    energies, hist = got[3], got[2]
    assert (energies == value).sum() >= 1 and hist[1] == (energies < value).sum() == 40
    assert hist[2] > hist[1] >= hist[0]


def test_betas_and_edges_at_their_limits(host):
    out, levels, hist, _ = run(host, by_name("L=8,E=16"))
    assert len(levels) == 8 and len(hist) == 16 and (np.diff(hist) >= 0).all() and hist[-1] > hist[0]
    assert levels["z"][0] == out["n_voxels"][0] - out["n_blocked"][0]            # beta = 0: every weight is 1
    assert len(run(host, by_name("L=1,E=0"))[2]) == 0


def test_one_batch_with_holes_the_number_of_threads_and_the_budget():
    jobs = C.cases() + C.big_cases()[:1]
    packed = C.pack(jobs, hole=2)
    want = C.expected(jobs, _lib.Context(-1, host_threads=8), hole=2)
    for threads in (1, 3, 16):
        ctx = _lib.Context(-1, host_threads=threads)
        rc, got = C.raw(ctx, packed)
        assert rc == 0 and C.same(got, want), (threads, C.first_difference(got, want))
        rc, got = C.raw(ctx, packed, workspace_bytes=1)              # (every job a launch of its own on a device)
        assert rc == 0 and C.same(got, want)
    packed = C.pack(jobs, hole=1, energies=False)
    rc, got = C.raw(_lib.Context(-1, host_threads=3), packed)
    assert rc == 0 and C.same(got, C.expected(jobs, None, hole=1, energies=False))


def test_a_batch_of_64_mixed_jobs_that_share_atoms(host):
    jobs = C.mixed_batch()
    packed = C.pack(jobs, hole=1)
    assert len(np.unique(packed[0]["atom_first"])) < len(jobs)
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, host, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)


def test_bad_arguments_are_refused_and_nothing_is_written(host):
    batches = C.bad_batches()
    assert len(batches) >= 40
    for packed, sizes, what in batches:
        rc, got = C.raw(host, packed, sizes=sizes)
        assert rc == -2 and C.same(got, C.blank_of(packed)), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_affinity: job 1: ") and what in message, (what, message)


def test_no_jobs_and_the_wrapper(host):
    assert C.raw(host, C.pack([]))[0] == 0
    c = by_name("n=1")
    packed = C.pack([c])
    out, levels, hist, energies = host.affinity(packed[0], packed[1], packed[2], packed[4], packed[3], packed[5],
                                                energies=np.zeros(packed[6]))
    want = C.expected([c], host)
    assert C.same((out, levels, hist, energies), want)
    bad = C.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        host.affinity(bad[0], bad[1], bad[2], bad[4], bad[3], bad[5], energies=np.zeros(bad[6]))


# ---- pw_exp above zero ------------------------------------------------------------------------------------------------

def test_pw_exp_within_one_ulp_up_to_700(host):
    """A dense sweep of (0, 700] and both neighbours of every reduction boundary (i + 1/2) ln2 / 128 in it."""
    assert np.finfo(LD).nmant >= 63
    rng = np.random.default_rng(7)
    step = np.log(LD(2.0)) / LD(128.0)
    i = np.arange(0, int(700.0 / float(step)) + 1)
    edge = ((i.astype(LD) + LD(0.5)) * step).astype(np.float64)
    x = np.concatenate([np.linspace(0.0, 700.0, 500_001)[1:], rng.uniform(0.0, 700.0, 500_000), edge,
                        np.nextafter(edge, 0.0), np.nextafter(edge, 1000.0), [700.0, np.nextafter(700.0, 0.0)]])
    x = x[(x > 0.0) & (x <= 700.0)]
    assert len(x) >= 1_200_000 and len(edge) > 129_000
    y = K.internal_exp(host, x)
    exact = np.exp(x.astype(LD))
    err = np.abs(y.astype(LD) - exact) / np.spacing(exact.astype(np.float64)).astype(LD)
    worst = float(err.max())
    print(f"pw_exp on (0, 700]: {len(x)} arguments, largest error {worst:.4f} ulp at x = {x[int(err.argmax())]!r}")
    assert worst <= 1.0


# ---- CC3 ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cc3():
    return synth.load_cc3_base()


def _molecule(cc3, xyz=None):
    return pw.Molecule({"elements": cc3[0], "coordinates": cc3[1] if xyz is None else xyz}, "cc3", 0)


def test_accuracy_of_the_sums_on_jittered_cc3(cc3, on_the_host):
    """Z and E of Xe at 298 K over the cavity of a jittered CC3 against a long-double evaluation of the same voxels."""
    xyz = synth.noisy_frame(cc3[1], 77, sigma=0.05)
    mol = _molecule(cc3, xyz)
    mol.calculate_cavity(probe=0.0, mask=True)
    cav = mol.cavity
    coef = affinity.lj_coefficients(cc3[0], "Xe")
    af = pw.guest_affinity(xyz, coef, None, [298.0], cavity=cav, energies=True, device=-1)
    beta = 1.0 / (affinity.R * 298.0)
    l, j, i = np.nonzero(cav.mask)
    live = np.isfinite(af.energies)
    assert live.sum() > 500
    centres = [cav.origin[a] + np.asarray(v, dtype=np.float64) * cav.spacing for a, v in enumerate((i, j, l))]

    def sums(dtype, exp, total):
        U = np.zeros(len(i), dtype=dtype)
        for (X, Y, Z), (A, B) in zip(xyz.astype(dtype), coef.astype(dtype)):
            dx, dy, dz = centres[0].astype(dtype) - X, centres[1].astype(dtype) - Y, centres[2].astype(dtype) - Z
            q = dtype(1.0) / ((dx * dx + dy * dy) + dz * dz)
            s = (q * q) * q
            U = U + s * (A * s - B)
        w = exp(-(dtype(beta) * U[live]))
        return total(w), total(w * U[live])

    z_true, e_true = sums(LD, np.exp, lambda v: v.sum())
    z_numpy, e_numpy = sums(np.float64, np.exp, np.sum)
    z_ours, e_ours = af.levels["z"][0], af.levels["e"][0]
    rel = lambda v, t: float(abs(LD(v) - t) / abs(t))
    print(f"CC3 Xe 298 K, {int(live.sum())} voxels: Z ours {rel(z_ours, z_true):.3e} numpy {rel(z_numpy, z_true):.3e}; "
          f"E ours {rel(e_ours, e_true):.3e} numpy {rel(e_numpy, e_true):.3e}")
    assert rel(z_ours, z_true) <= max(4.0 * rel(z_numpy, z_true), 64.0 * EPS)
    assert rel(e_ours, e_true) <= max(4.0 * rel(e_numpy, e_true), 64.0 * EPS)


def test_lj_coefficients():
    sigma_c, eps_c = 3.851 / 2.0 ** (1.0 / 6.0), 4.184 * 0.105
    sigma, eps = (sigma_c + 4.10) / 2.0, np.sqrt(eps_c * affinity.R * 221.0)
    A, B = affinity.lj_coefficients(["C", "h"], "Xe")[0]
    assert np.isclose(A, 4.0 * eps * sigma ** 12, rtol=1e-14) and np.isclose(B, 4.0 * eps * sigma ** 6, rtol=1e-14)
    assert np.allclose(affinity.lj_coefficients(["C"], (4.10, affinity.R * 221.0)), [[A, B]], rtol=1e-14)
    with pytest.raises(KeyError):
        affinity.lj_coefficients(["C", "Zn"], "Xe")
    with pytest.raises(KeyError):
        affinity.lj_coefficients(["C"], "SF6")


def test_cc3_holds_xenon_more_strongly_than_krypton(cc3, on_the_host):
    mol = _molecule(cc3)
    before = dict(_molecule(cc3).full_analysis())
    found = {}
    for guest in ("He", "Kr", "Xe"):
        af = mol.calculate_guest_affinity(guest=guest, temperature=298.0)
        props = mol.properties["guest_affinity"]
        assert af is mol.affinity and af.closed and not af.clamped and props["closed"] is True and props["guest"] == guest
        assert af.n_voxels == mol.cavity.n_voxels > 0 and props["boltzmann_volume"] == float(af.boltzmann_volume[0])
        assert props["heat"] == float(affinity.R * 298.0 - af.mean_energy[0]) and props["min_energy"] == af.min_energy
        assert np.linalg.norm(props["min_position"] - mol.pore_opt_COM) < 4.0
        found[guest] = af
        print(f"CC3 {guest} at 298 K: V_B {props['boltzmann_volume']:.2f} A^3, K_H {props['henry']:.4g} /bar, "
              f"<U> {props['mean_energy']:.2f}, q_st {props['heat']:.2f}, U_min {props['min_energy']:.2f} kJ/mol, "
              f"{af.n_blocked} of {af.n_voxels} voxels blocked")
    he = found["He"]
    beta = 1.0 / (affinity.R * 298.0)
    n_live = int(he.n_voxels - he.n_blocked)
    # the Boltzmann volume is positive and below the cavity's voxel volume plus what attraction adds
    assert 0.0 < he.boltzmann_volume[0] <= n_live * 0.125 * np.exp(-beta * he.min_energy)
    assert he.boltzmann_volume[0] < mol.cavity.volume * np.exp(-beta * he.min_energy)
    assert found["Xe"].min_energy < found["Kr"].min_energy < he.min_energy < 0.0
    assert found["Xe"].selectivity(found["Kr"])[0] > 1.0
    assert found["Xe"].heat[0] > found["Kr"].heat[0] > he.heat[0] > 0.0
    again = _molecule(cc3).full_analysis()
    assert "guest_affinity" not in again and list(again) == list(before) and repr(again) == repr(before)


def _history(tmp_path, cc3, n=6, cell=None):
    elements, base = cc3
    rng = np.random.default_rng(12)
    frames = [base + rng.normal(0.0, 0.03, base.shape) for _ in range(n)]
    return pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=cell)), frames


def test_affinity_of_a_trajectory_and_its_series(tmp_path, cc3, on_the_host):
    traj, _ = _history(tmp_path, cc3)
    with pytest.raises(ValueError, match="no frame has been analysed"):
        traj.affinity()
    traj.analysis(frames=[0, 1, 2, 4, 5])
    edges = np.linspace(-30.0, 10.0, 9)
    af = traj.affinity("Xe", [298.0, 195.0], edges=edges, energies=True)
    assert list(af.frames) == [0, 1, 2, 4, 5] and af.raw.shape == (5,) and af.levels.shape == (5, 2)
    assert af.counts.shape == (5, 9) and af.histogram.shape == (5, 8) and (af.histogram >= 0).all()
    cav = traj.cavity(mask=True)
    coords = traj._read_selected([0, 1, 2, 4, 5], False)[0]
    for t in range(5):
        one_cav = pw.Cavity(cav.raw[t], cav.origin[t], cav.shape[t], cav.spacing, cav.probe, cav.mask[t], None, cav.words[t])
        one = pw.guest_affinity(coords[t], traj.elements(), "Xe", [298.0, 195.0], cavity=one_cav, edges=edges,
                                energies=True, device=-1)
        assert one.raw.tobytes() == af.raw[t].tobytes() and one.levels.tobytes() == af.levels[t].tobytes()
        assert np.array_equal(one.counts, af.counts[t]) and np.array_equal(one.energies, af.energies[t])
        assert len(af.energies[t]) == cav.n_voxels[t] and np.array_equal(one.min_position, af.min_position[t])
    assert (af.boltzmann_volume[:, 1] > af.boltzmann_volume[:, 0]).all()          # colder: held more strongly
    two = traj.affinity("Xe", [298.0, 195.0], frames=[4, 1])
    assert list(two.frames) == [4, 1] and two.raw.tobytes() == af.raw[[3, 1]].tobytes()
    values, valid = af.series("boltzmann_volume", level=1)
    assert valid.all() and np.array_equal(values, af.boltzmann_volume[:, 1]) and values.dtype == np.float64
    for name in ("henry", "mean_energy", "heat", "min_energy", "n_voxels", "n_blocked"):
        assert af.series(name)[0].shape == (5,) and np.isfinite(af.series(name)[0]).all()
    with pytest.raises(KeyError):
        af.series("colour")
    leaky = traj.affinity("Xe", close=None)
    assert not leaky.series("heat")[1].any()
    assert pw.time_correlation(values, max_lag=2, valid_a=valid, device=-1) is not None
    kr = traj.affinity("Kr", [298.0, 195.0])
    assert (af.selectivity(kr) > 1.0).all()
    with pytest.raises(ValueError, match="different temperatures"):
        af.selectivity(traj.affinity("Kr", 250.0))


def test_a_clamped_frame_is_not_valid():
    """A single strongly attractive atom at 1 K: the exponent passes 700."""
    af = pw.guest_affinity([[0.0, 0.0, 0.0]], [[0.0, 1e3]], None, [1.0], grid=([-2.0, -2.0, -2.0], 1.0, (5, 5, 5)), device=-1)
    assert af.clamped and not af.series("boltzmann_volume")[1].any() and af.closed is None and af.n_blocked == 1
    ok = pw.guest_affinity([[0.0, 0.0, 0.0]], [[0.0, 1e3]], None, [1e4], grid=([-2.0, -2.0, -2.0], 1.0, (5, 5, 5)), device=-1)
    assert not ok.clamped and ok.series("boltzmann_volume")[1].all()


def test_a_periodic_trajectory_is_refused(tmp_path, cc3, on_the_host):
    traj, _ = _history(tmp_path, cc3, n=2, cell=np.eye(3) * 40.0)
    with pytest.raises(ValueError, match="affinity: a periodic or modular trajectory is not supported yet"):
        traj.affinity()
