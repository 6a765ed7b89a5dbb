"""Rigid linear guests on the host path (device = -1): pw_rigid_affinity against the definition (tests/_rigid_cases.py:
reference) as BYTES, case by case and as one batch with entries nobody owns; blocked second sites, ties at the core and
at the cutoff, dead voxels, tied minima, the clamp; the reduction to pw_affinity; the refusals; the accuracy of the sums
against a long-double evaluation; and the Python layers above the entry (pywindow_amd.rigid,
Molecule.calculate_rigid_guest_affinity on CC3, DLPOLY.rigid_affinity).  tests/test_gpu_rigid.py holds the device to
the same.

Measured here (host path):
    jittered CC3, CO2 at 298 K, 64 orientations, 1139 voxels: Z off by 1.7e-16 and E by 2.3e-16 of the long-double
    values; plain float64 numpy with numpy.sum by 3.7e-16 and 4.4e-16 (bar max(4 E_numpy, 64 * 2^-53 = 7.1e-15))
"""
import numpy as np
import pytest

import _affinity_cases as A
import _rigid_cases as C
import pywindow_amd as pw
from pywindow_amd import _lib, affinity, engine, rigid, synth

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
    """The first test of this file: it fails where the library has no pw_rigid_affinity."""
    assert hasattr(_lib.load(), "pw_rigid_affinity")
    for c in C.cases() + C.grid_case():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    names = {c.name for c in C.cases()}
    assert {f"V={v}" for v in (0, 1, 63, 64, 65, 129)} <= names and {f"M={m}" for m in (1, 2, 63, 64, 65, 1024)} <= names
    assert {f"n={n}" for n in (0, 1, C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1)} <= names
    assert {f"S={s},charged={q}" for s in (1, 2, 3, 8) for q in (0, 1)} <= names
    assert {c.map_level for c in C.cases()} >= {-1, 0, 7} and {len(c.betas) for c in C.cases()} >= {1, 8}
    g = C.grid_case()[0]
    assert g.dims == (64, 64, 4) and g.words is None and len(g.dirs) == 8 and len(g.offsets) == 2 and len(g.xyz) == 8


def test_regions(host):
    for v in (0, 1, 63, 64, 65, 129):
        assert run(host, by_name(f"V={v}"))[0]["n_voxels"][0] == v
    out, levels, _ = run(host, by_name("V=0"))
    assert out["u_min"][0] == np.inf and (out["min_voxel"][0] == -1).all() and out["min_dir"][0] == -1
    assert levels["z"].tolist() == [0.0, 0.0] and not np.signbit(levels["z"]).any() and not np.signbit(levels["e"]).any()
    for bit in (0, 63):
        out = run(host, by_name(f"bit-{bit}-alone"))[0]
        assert out["n_voxels"][0] == 1 and out["min_voxel"][0].tolist() == [bit, 0, 1]
    for nx in (5, 64):
        assert run(host, by_name(f"nx={nx}-junk-bits"))[0]["n_voxels"][0] == nx * 6
    assert run(host, by_name("no-mask-3x2x2"))[0]["n_voxels"][0] == 12


def test_without_atoms_z_is_the_count(host):
    out, levels, maps = run(host, by_name("n=0"))
    assert levels["z"].tolist() == [100.0, 100.0] and levels["e"].tolist() == [0.0, 0.0]
    assert out["u_min"][0] == 0.0 and out["min_dir"][0] == 0 and out["n_blocked_poses"][0] == 0 and out["n_dead"][0] == 0
    assert (maps.reshape(-1, 2)[:, 0] == 1.0).all() and (maps.reshape(-1, 2)[:, 1] == 0.0).all()


def test_blocked_second_sites_ties_at_the_core_and_at_the_cutoff_and_dead_voxels(host):
    """The case "ties" of tests/_rigid_cases.py: see the comment there."""
    out, levels, maps = run(host, by_name("ties"))
    zbar, umin = maps.reshape(-1, 2).T

    def pair(r2, a, b):
        q = 1.0 / r2
        s = (q * q) * q
        return s * (a * s - b)

    assert out["n_dead"][0] == 3 and np.isinf(umin[[1, 2, 3]]).all() and (zbar[[1, 2, 3]] == 0.0).all()
    assert out["n_blocked_poses"][0] == 3 * 2 + 1 + 1                # the dead voxels, voxel 0 along +x, voxel 4 along -x
    assert umin[0] == pair(4.0, 3.0, 2.0) + pair(9.0, 5.0, 1.0)      # voxel 0 along -x: the second site at r2 == cutoff2
    assert umin[4] == pair(4.0, 3.0, 2.0) + pair(9.0, 5.0, 1.0)      # voxel 4 along +x: the same distances
    # voxel 5: along +x the second site is beyond the cutoff (adds nothing), along -x it is at r2 == 4
    assert umin[5] == min(pair(9.0, 3.0, 2.0) + 0.0, pair(9.0, 3.0, 2.0) + pair(4.0, 5.0, 1.0))
    assert out["flags"][0] == 0 and zbar[0] > 0.0


def test_all_voxels_dead(host):
    out, levels, maps = run(host, by_name("all-dead"))
    assert out["n_dead"][0] == out["n_voxels"][0] == 24 and out["n_blocked_poses"][0] == 24 * 3 and out["u_min"][0] == np.inf
    assert (out["min_voxel"][0] == -1).all() and out["min_dir"][0] == -1 and out["flags"][0] == 0
    assert levels["z"][0] == 0.0 and levels["e"][0] == 0.0 and not np.signbit(levels["z"][0])
    assert (maps.reshape(-1, 2)[:, 0] == 0.0).all() and np.isinf(maps.reshape(-1, 2)[:, 1]).all()


def test_tied_minima_go_to_the_lower_orientation_and_the_lower_rank(host):
    c = by_name("tied-orientations")
    U, blocked = C.pose_energies(c)
    assert not blocked.any() and (U[:, 0] == U[:, 1]).all() and (U != 0.0).all()   # d and -d: equal pose energies
    out = run(host, c)[0]
    assert out["min_dir"][0] == 0 and out["u_min"][0] == U.min()
    out, levels, _ = run(host, by_name("tied-voxels"))
    assert out["u_min"][0] == -64.0 and out["min_voxel"][0].tolist() == [2, 0, 0] and out["min_dir"][0] == 0
    assert out["flags"][0] == C.CLAMPED and np.isfinite(levels["z"]).all()


def test_at_beta_zero_zbar_counts_the_poses_that_are_not_blocked(host):
    c = by_name("M=65")
    assert c.betas[0] == 0.0
    one = C.Case("beta0", c.dims, c.xyz, c.coef, offsets=c.offsets, dirs=c.dirs, h=c.h, betas=(0.0,), charged=c.charged,
                 map_level=0, core2=0.6)
    out, levels, maps = run(host, one)
    _, blocked = C.pose_energies(one)
    assert 0 < blocked.sum() < blocked.size and out["n_blocked_poses"][0] == blocked.sum()
    assert np.array_equal(maps.reshape(-1, 2)[:, 0], (65 - blocked.sum(axis=1)).astype(np.float64) * (1.0 / 65.0))


def test_zero_charges_give_the_uncharged_bytes(host):
    plain, charged = by_name("zero-charges,charged=0"), by_name("zero-charges,charged=1")
    terms = []
    C.pose_energies(plain, terms)
    every = np.concatenate(terms)
    assert len(every) > 1000 and not (np.signbit(every) & (every == 0.0)).any()    # no pair term is -0.0
    assert C.same(run(host, plain), run(host, charged))


def test_one_batch_with_holes_and_the_number_of_threads():
    jobs = C.cases() + C.grid_case()
    packed = C.pack(jobs, hole=2)
    want = C.expected(jobs, _lib.Context(-1, host_threads=8), hole=2)
    for threads in (1, 3, 16):
        ctx = _lib.Context(-1, host_threads=threads)
        rc, got = C.raw(ctx, packed)
        assert rc == 0 and C.same(got, want), (threads, C.first_difference(got, want))
        rc, got = C.raw(ctx, packed, workspace_bytes=1)              # (every job a launch of its own on a device)
        assert rc == 0 and C.same(got, want)
    packed = C.pack(jobs, hole=1, maps=False)
    rc, got = C.raw(_lib.Context(-1, host_threads=3), packed)
    assert rc == 0 and len(got[2]) == 0 and C.same(got, C.expected(jobs, None, hole=1, maps=False))


def test_a_batch_of_64_mixed_jobs_that_share_atoms_and_directions(host):
    jobs = C.mixed_batch()
    packed = C.pack(jobs, hole=1)
    assert len(np.unique(packed[0]["atom_first"])) < len(jobs) and len(np.unique(packed[0]["dir_first"])) == 2
    assert set(packed[0]["n_sites"].tolist()) >= {1, 2, 3, 5, 8} and set(packed[0]["charged"].tolist()) == {0, 1}
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, host, hole=1)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)


def test_one_site_one_direction_is_pw_affinity(host):
    """Every job of tests/_affinity_cases.py as S = 1, t = 0, M = 1, uncharged: pw_affinity's bytes in every shared field."""
    for c in A.cases():
        rc, (out, levels, _) = C.raw(host, C.pack([C.from_affinity(c)]))
        rc_a, (out_a, levels_a, _, _) = A.raw(host, A.pack([c], energies=False))
        assert rc == 0 and rc_a == 0 and levels.tobytes() == levels_a.tobytes(), c.name
        for name in ("n_voxels", "u_min", "min_voxel", "flags"):
            assert out[name].tobytes() == out_a[name].tobytes(), (c.name, name)
        assert out["n_blocked_poses"][0] == out_a["n_blocked"][0] == out["n_dead"][0], c.name
        assert out["min_dir"][0] == (0 if out["u_min"][0] < np.inf else -1)


def test_bad_arguments_are_refused_and_nothing_is_written(host):
    batches = C.bad_batches()
    assert len(batches) >= 50
    for packed, sizes, what in batches:
        rc, got = C.raw(host, packed, sizes=sizes)
        assert rc == -2 and C.same(got, C.blank_of(packed)), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_rigid_affinity: job 1: ") and what in message, (what, message)


def test_no_jobs_and_the_wrapper(host):
    assert C.raw(host, C.pack([]))[0] == 0
    c = by_name("S=3,charged=1")
    p = C.pack([c])
    out, levels, maps = host.rigid_affinity(p[0], p[1], p[2], p[3], p[4], p[6], p[5], maps=np.zeros(p[7]))
    assert C.same((out, levels, maps), C.expected([c], host))
    bad = C.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: n_sites outside"):
        host.rigid_affinity(bad[0], bad[1], bad[2], bad[3], bad[4], bad[6], bad[5], maps=np.zeros(bad[7]))


# ---- CC3 ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cc3():
    return synth.load_cc3_base()


def _molecule(cc3, xyz=None):
    return pw.Molecule({"elements": cc3[0], "coordinates": cc3[1] if xyz is None else xyz}, "cc3", 0)


def test_accuracy_of_the_sums_on_jittered_cc3(cc3, on_the_host):
    """Z and E of CO2 at 298 K over the cavity of a jittered CC3 against a long-double evaluation of the same poses."""
    xyz = synth.noisy_frame(cc3[1], 77, sigma=0.05)
    mol = _molecule(cc3, xyz)
    mol.calculate_cavity(probe=0.0, mask=True)
    cav = mol.cavity
    guest = rigid.RIGID_GUESTS["CO2"]
    coef = rigid.rigid_coefficients(cc3[0], guest)
    dirs = pw.sphere_directions(rigid.M_DEFAULT)
    af = pw.rigid_guest_affinity(xyz, coef, guest, [298.0], cavity=cav, directions=dirs, device=-1)
    assert not af.charged
    beta = 1.0 / (affinity.R * 298.0)
    l, j, i = np.nonzero(cav.mask)
    centres = [cav.origin[a] + np.asarray(v, dtype=np.float64) * cav.spacing for a, v in enumerate((i, j, l))]
    # which poses are blocked is decided in float64, as the entry decides it: the comparison is of the sums
    blocked = np.zeros((len(i), len(dirs)), dtype=bool)
    for t in guest.offsets:
        p = [centres[a][:, None] + (t * dirs[:, a])[None, :] for a in range(3)]
        for X, Y, Z in xyz:
            blocked |= ((p[0] - X) ** 2 + (p[1] - Y) ** 2) + (p[2] - Z) ** 2 <= 0.25
    live = ~blocked
    assert live.sum() > 30000 and af.n_blocked_poses == blocked.sum()

    def sums(dtype, exp, total):
        U = np.zeros(blocked.shape, dtype=dtype)
        for s, t in enumerate(guest.offsets):
            p = [(centres[a][:, None] + (t * dirs[:, a])[None, :]).astype(dtype) for a in range(3)]   # the defined positions
            for (X, Y, Z), (a, b, _) in zip(xyz.astype(dtype), coef[s].astype(dtype)):
                dx, dy, dz = p[0] - X, p[1] - Y, p[2] - Z
                q = dtype(1.0) / ((dx * dx + dy * dy) + dz * dz)
                s6 = (q * q) * q
                U = U + s6 * (a * s6 - b)
        w = exp(-(dtype(beta) * U[live]))
        return total(w) / dtype(len(dirs)), total(w * U[live]) / dtype(len(dirs))

    z_true, e_true = sums(LD, np.exp, lambda v: v.sum())
    z_numpy, e_numpy = sums(np.float64, np.exp, np.sum)
    z_ours, e_ours = af.levels["z"][0], af.levels["e"][0]
    rel = lambda v, t: float(abs(LD(v) - t) / abs(t))
    print(f"CC3 CO2 298 K, {len(i)} voxels x {len(dirs)}: Z ours {rel(z_ours, z_true):.3e} numpy {rel(z_numpy, z_true):.3e}; "
          f"E ours {rel(e_ours, e_true):.3e} numpy {rel(e_numpy, e_true):.3e}")
    assert rel(z_ours, z_true) <= max(4.0 * rel(z_numpy, z_true), 64.0 * EPS)
    assert rel(e_ours, e_true) <= max(4.0 * rel(e_numpy, e_true), 64.0 * EPS)


def test_rigid_coefficients():
    sigma_c, eps_c = 3.851 / 2.0 ** (1.0 / 6.0), 4.184 * 0.105
    sigma, eps = (sigma_c + 3.05) / 2.0, np.sqrt(eps_c * affinity.R * 79.0)
    rows = rigid.rigid_coefficients(["C", "h"], "CO2", charges=[0.25, -0.1])
    assert rows.shape == (3, 2, 3)
    assert np.isclose(rows[0, 0, 0], 4.0 * eps * sigma ** 12, rtol=1e-14) and np.isclose(rows[2, 0, 1], 4.0 * eps * sigma ** 6, rtol=1e-14)
    assert np.isclose(rows[0, 0, 2], 1389.35457644382 * 0.25 * -0.35, rtol=1e-14)
    assert np.isclose(rows[1, 1, 2], 1389.35457644382 * -0.1 * 0.70, rtol=1e-14)
    n2 = rigid.rigid_coefficients(["C"], "N2", charges=[0.5])
    assert n2[1, 0, 0] == 0.0 and n2[1, 0, 1] == 0.0 and n2[1, 0, 2] > 0.0 and n2[0, 0, 0] > 0.0    # the centre: a charge only
    assert (rigid.rigid_coefficients(["C", "H"], "CO2")[:, :, 2] == 0.0).all()
    with pytest.raises(KeyError):
        rigid.rigid_coefficients(["C", "Zn"], "CO2")
    with pytest.raises(KeyError):
        rigid.rigid_coefficients(["C"], "SF6")


def test_a_one_site_guest_is_guest_affinity(cc3, on_the_host):
    mol = _molecule(cc3)
    mol.calculate_cavity(probe=0.0, mask=True)
    sigma, eps_k = affinity.GUESTS["Xe"]
    xe = pw.RigidGuest("Xe", (0.0,), (sigma,), (eps_k,), (0.0,))
    one = pw.rigid_guest_affinity(cc3[1], cc3[0], xe, [298.0, 195.0], cavity=mol.cavity, directions=[[0.0, 0.0, 1.0]], device=-1)
    ref = pw.guest_affinity(cc3[1], cc3[0], "Xe", [298.0, 195.0], cavity=mol.cavity, device=-1)
    assert one.levels.tobytes() == ref.levels.tobytes() and one.min_energy == ref.min_energy
    assert np.array_equal(one.min_position, ref.min_position) and one.n_dead == ref.n_blocked
    assert np.array_equal(one.selectivity(ref), [1.0, 1.0]) and np.array_equal(one.min_direction, [0.0, 0.0, 1.0])


def test_cc3_holds_co2_more_strongly_than_n2(cc3, on_the_host):
    mol = _molecule(cc3)
    before = dict(_molecule(cc3).full_analysis())
    found = {}
    for guest in ("CO2", "N2"):
        af = mol.calculate_rigid_guest_affinity(guest=guest, temperature=298.0)
        props = mol.properties["rigid_guest_affinity"]
        assert af is mol.rigid_affinity and af.closed and not af.clamped and not af.charged and props["guest"] == guest
        assert af.n_voxels == mol.cavity.n_voxels > 0 and props["henry"] == float(af.henry[0])
        assert len(af.directions) == rigid.M_DEFAULT and props["min_energy"] == af.min_energy < 0.0
        assert abs(np.linalg.norm(props["min_direction"]) - 1.0) < 1e-12
        found[guest] = af
        print(f"CC3 {guest} at 298 K: K_H {props['henry']:.4g} /bar, q_st {props['heat']:.2f}, U_min {props['min_energy']:.2f} kJ/mol")
    assert found["CO2"].heat[0] > found["N2"].heat[0] > 0.0 and found["CO2"].selectivity(found["N2"])[0] > 1.0
    charged = mol.calculate_rigid_guest_affinity("CO2", charges=np.where(cc3[0] == "N", -0.4, 0.4 * (cc3[0] == "N").sum() / (cc3[0] != "N").sum()))
    assert charged.charged and charged.levels.tobytes() != found["CO2"].levels.tobytes()
    again = _molecule(cc3).full_analysis()
    assert "rigid_guest_affinity" not in again and list(again) == list(before) and repr(again) == repr(before)


def test_the_free_energy_field_goes_through_passage_field(cc3, on_the_host):
    mol = _molecule(cc3)
    mol.full_analysis()
    centre = np.asarray(mol.pore_opt_COM, dtype=np.float64)
    half, h = 9.0, 1.0
    dims = (19, 19, 19)
    origin = centre - half
    af = pw.rigid_guest_affinity(cc3[1], cc3[0], "CO2", [298.0], grid=(origin, h, dims), directions=pw.sphere_directions(16),
                                 maps=True, device=-1)
    field = af.free_energy_field()
    assert field.shape == (19, 19, 19) and np.isinf(field).any() and np.isfinite(field).any() and af.n_dead > 0
    assert np.array_equal(np.isinf(field).reshape(-1), af.maps[:, 0] == 0.0)
    ps = pw.passage_field(field, (9, 9, 9), None, origin, h, device=-1)
    assert np.isfinite(ps.barrier).all() and (ps.barrier >= field[9, 9, 9]).all()
    with pytest.raises(ValueError, match="maps=True"):
        pw.rigid_guest_affinity(cc3[1], cc3[0], "CO2", [298.0], grid=(origin, h, dims), directions=pw.sphere_directions(2),
                                device=-1).free_energy_field()


def _history(tmp_path, cc3, n=5, cell=None):
    elements, base = cc3
    rng = np.random.default_rng(12)
    frames = [base + rng.normal(0.0, 0.03, base.shape) for _ in range(n)]
    return pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=cell)), frames


def test_rigid_affinity_of_a_trajectory_and_its_series(tmp_path, cc3, on_the_host):
    traj, _ = _history(tmp_path, cc3)
    with pytest.raises(ValueError, match="no frame has been analysed"):
        traj.rigid_affinity()
    traj.analysis()
    dirs = pw.sphere_directions(8)
    af = traj.rigid_affinity("CO2", [298.0, 195.0], directions=dirs)
    assert list(af.frames) == [0, 1, 2, 3, 4] and af.raw.shape == (5,) and af.levels.shape == (5, 2)
    cav = traj.cavity(mask=True)
    coords = traj._read_selected([0, 1, 2, 3, 4], False)[0]
    for t in range(5):
        one_cav = pw.Cavity(cav.raw[t], cav.origin[t], cav.shape[t], cav.spacing, cav.probe, cav.mask[t], None, cav.words[t])
        one = pw.rigid_guest_affinity(coords[t], traj.elements(), "CO2", [298.0, 195.0], cavity=one_cav, directions=dirs, device=-1)
        assert one.raw.tobytes() == af.raw[t].tobytes() and one.levels.tobytes() == af.levels[t].tobytes()
        assert np.array_equal(one.min_position, af.min_position[t]) and np.array_equal(one.min_direction, af.min_direction[t])
    values, valid = af.series("boltzmann_volume", level=1)
    assert valid.all() and np.array_equal(values, af.boltzmann_volume[:, 1]) and values.dtype == np.float64
    for name in ("henry", "mean_energy", "heat", "min_energy", "n_voxels", "n_dead"):
        assert af.series(name)[0].shape == (5,) and np.isfinite(af.series(name)[0]).all()
    with pytest.raises(KeyError):
        af.series("n_blocked")
    assert not traj.rigid_affinity("CO2", directions=dirs, close=None).series("heat")[1].any()
    xe = traj.affinity("Xe", [298.0, 195.0])
    assert af.selectivity(xe).shape == (5, 2) and (af.selectivity(xe) > 0.0).all()
    with pytest.raises(ValueError, match="different temperatures"):
        af.selectivity(traj.affinity("Xe", 250.0))


def test_a_clamped_frame_is_not_valid():
    guest = pw.RigidGuest("pair", (-0.2, 0.2), (1.0, 1.0), (1.0, 1.0), (0.0, 0.0))
    coef = np.tile([[[0.0, 1e3, 0.0]]], (2, 1, 1))
    grid = ([-2.0, -2.0, -2.0], 1.0, (5, 5, 5))
    af = pw.rigid_guest_affinity([[0.0, 0.0, 0.0]], coef, guest, [1.0], grid=grid, directions=[[0.0, 0.0, 1.0]], device=-1)
    assert af.clamped and not af.series("boltzmann_volume")[1].any() and af.closed is None and af.n_dead == 1
    ok = pw.rigid_guest_affinity([[0.0, 0.0, 0.0]], coef, guest, [1e4], grid=grid, directions=[[0.0, 0.0, 1.0]], device=-1)
    assert not ok.clamped and ok.series("boltzmann_volume")[1].all()


def test_a_periodic_trajectory_is_refused(tmp_path, cc3, on_the_host):
    traj, _ = _history(tmp_path, cc3, n=2, cell=np.eye(3) * 40.0)
    with pytest.raises(ValueError, match="rigid_affinity: a periodic or modular trajectory is not supported yet"):
        traj.rigid_affinity()
