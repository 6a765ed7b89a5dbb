"""Rigid guests in a periodic cell on the host path (device = -1): pw_rigid_cell against the definition over ALL atoms
(tests/_rigid_cell_cases.py: reference) as BYTES, case by case and as batches with entries nobody owns; the two reductions
(one site and one direction: pw_percolation's map; an orthorhombic cell: pw_rigid_affinity over the grid); the refusals;
properties of the result; and the Python layer above the entry (pywindow_amd.rigid_cell) on the CC3 cell.  The only
tolerance is that of the numpy layer's tensors, relative 1e-9 as in tests/test_diffusion.py.
tests/test_gpu_rigid_cell.py holds the device to the same."""
import numpy as np
import pytest

import _percolation_cases as P
import _rigid_cases as RC
import _rigid_cell_cases as C
import pywindow_amd as pw
from pywindow_amd import _lib
from pywindow_amd.affinity import R

RTOL = 1e-9


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


def by_name(name):
    return [c for c in C.cases() if c.name == name][0]


def run(ctx, c, **kw):
    rc, got = C.raw(ctx, C.pack([c]), **kw)
    assert rc == 0
    return got


def test_every_case_one_job_at_a_time(host):
    """The first test of this file: it fails where the library has no pw_rigid_cell."""
    assert hasattr(_lib.load(), "pw_rigid_cell")
    for c in C.cases():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
        assert c.voxels <= 400, c.name
    names = {c.name for c in C.cases()}
    assert {f"n={n}" for n in (0, 1, C.TILE, C.TILE + 1, C.NEAR_CAP + 150)} <= names
    assert {f"M={m}" for m in (1, 2, 3, 64, 1024)} <= names and {f"S={s}" for s in (1, 2, 3, 4, 8)} <= names
    assert {f"nx={n}" for n in (1, 2, 63, 64)} <= names and {len(c.betas) for c in C.cases()} >= {1, 8}
    assert any((c.step != 0.0).all() for c in C.cases()) and any(c.voxels % 64 and c.dims[0] % 4 for c in C.cases())


def test_batches_with_holes_forwards_and_reversed(host):
    jobs = C.cases() + C.shared_batch()
    assert C.pack(C.shared_batch())[1].shape == (30, 3)                 # (the three jobs hold one set of atoms)
    for reverse in (False, True):
        packed = C.pack(jobs, hole=2, reverse=reverse)
        rc, got = C.raw(host, packed)
        want = C.expected(jobs, host, hole=2, reverse=reverse)
        assert rc == 0 and C.same(got, want), (reverse, C.first_difference(got, want))
        rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
        assert (rows == C.SENTINEL).all(axis=1).sum() == 2 * len(jobs)


def test_threads_1_3_and_16_give_one_set_of_bytes(host):
    jobs = C.cases()
    packed = C.pack(jobs)
    want = C.raw(host, packed)[1]
    for threads in (1, 3, 16):
        rc, got = C.raw(_lib.Context(-1, host_threads=threads), packed)
        assert rc == 0 and C.same(got, want), threads


def test_the_skip_changes_no_byte_on_the_host(host):
    for c in C.cases():
        on, off = [], []
        assert C.same(run(host, c, diagnostics=on), run(host, c, diagnostics=off, skip=False)), c.name
        assert int(off[0][0][0]) == c.voxels * len(c.dirs) * len(c.offsets) * len(c.xyz) >= int(on[0][0][0]), c.name
    on, off = [], []
    run(host, by_name("cutoff2=25"), diagnostics=on), run(host, by_name("cutoff2=25"), diagnostics=off, skip=False)
    assert int(on[0][0][0]) < int(off[0][0][0]) // 4


def test_the_edges_of_the_cutoff_and_of_the_core(host):
    """r2 == 25 exactly from the second site of the pose +x of three voxels: the atom counts at cutoff2 = 25 and one ulp
    above, not one ulp below; the voxel whose centre is at r2 == core2 is dead although the site at it adds nothing."""
    zbar = {}
    for name in ("cutoff2=25", "cutoff2=25-ulp", "cutoff2=25+ulp"):
        out, _, maps = run(host, by_name(name))
        zbar[name] = maps.reshape(3, 5, 5, 5)[0]
        assert maps.reshape(3, 5, 5, 5)[2][0, 4, 4] == np.inf and out["n_dead"][0] >= 1
    assert zbar["cutoff2=25"].tobytes() == zbar["cutoff2=25+ulp"].tobytes()
    differ = zbar["cutoff2=25"] != zbar["cutoff2=25-ulp"]
    assert differ[0, 0, 0] and differ[2, 1, 2] and differ[3, 3, 3]
    out, _, maps = run(host, by_name("zero-site-blocks"))
    assert out["n_blocked_poses"][0] == 3 and out["n_dead"][0] == 1 and np.isinf(maps[3:]).tolist() == [False, False, True]


def test_degenerate_outputs(host):
    out, levels, maps = run(host, by_name("all-dead"))
    assert out["n_dead"][0] == 24 and out["u_min"][0] == np.inf and out["min_dir"][0] == -1 and (out["min_voxel"][0] == -1).all()
    assert levels["z"].tolist() == [0.0] and (maps[24:] == np.inf).all() and (maps[:24] == 0.0).all()
    out, levels, _ = run(host, by_name("one-live-pose"))
    assert out["n_blocked_poses"][0] == 2 and out["n_dead"][0] == 0 and out["min_dir"][0] == 2
    out, _, _ = run(host, by_name("tied-voxels-and-clamp"))
    assert out["flags"][0] == C.CLAMPED and out["min_voxel"][0].tolist() == [2, 0, 0] and out["min_dir"][0] == 0
    out, _, _ = run(host, by_name("tied-orientations"))
    assert out["min_dir"][0] == 0
    out, levels, _ = run(host, by_name("n=0"))
    assert levels["z"].tolist() == [210.0, 210.0] and out["u_min"][0] == 0.0 and out["min_voxel"][0].tolist() == [0, 0, 0]


def test_one_site_and_one_direction_is_the_map_of_pw_percolation(host):
    """S = 1, t_0 = 0, M = 1: the umin_v plane is pw_percolation's map byte for byte, on a skewed and an orthorhombic cell."""
    for name in ("n=129", "S=3", "direction-norms", "cutoff2=25"):
        one, ab = C.as_percolation_case(by_name(name))
        _, _, maps = run(host, one)
        pc = P.Case(name, dims=one.dims, xyz=one.xyz, coef=ab, core2=one.core2, cutoff2=one.cutoff2, origin=one.origin,
                    step=one.step, map=True)
        rc, (_, _, field) = P.raw(host, P.pack([pc]))
        assert rc == 0 and maps[len(one.betas) * one.voxels:].tobytes() == field.tobytes(), name


def test_the_public_one_site_field_is_guest_percolations_map():
    elements, xyz, lattice = P.cc3_cell()
    perc = pw.guest_percolation(xyz, elements, lattice, guest="Xe", spacing=2.0, cutoff=8.0, maps=True, device=-1)
    rows = pw.lj_coefficients(list(elements), "Xe")[None]
    one = pw.RigidGuest("Xe1", (0.0,), (0.0,), (0.0,), (0.0,))
    field = pw.rigid_guest_field(xyz, rows, lattice, guest=one, spacing=2.0, cutoff=8.0, directions=[[0.0, 0.0, 1.0]], device=-1)
    assert field.u_min_map.tobytes() == perc.maps.tobytes()


def test_an_orthorhombic_cell_is_pw_rigid_affinity_over_the_grid(host):
    """step = (h, 0, h, 0, 0, h): every output shared with rigid_guest_affinity(grid=..., maps=True) on the same listed
    atoms and the same cutoff2, level by level."""
    for name in ("M=3", "L=8", "n=129,S=8", "direction-norms"):
        c = by_name(name)
        h = float(c.step[0])
        assert c.step.tolist() == [h, 0.0, h, 0.0, 0.0, h]
        out, levels, maps = run(host, c)
        L = len(c.betas)
        planes = maps.reshape(L + 1, c.voxels)
        rows = np.concatenate([c.coef, np.zeros(c.coef.shape[:2] + (1,))], axis=2)
        for level in range(L):                                       # (pw_rigid_affinity keeps the zbar of one level a call)
            job = RC.Case(name, c.dims, c.xyz, rows, offsets=c.offsets, dirs=c.dirs, origin=c.origin, h=h, core2=c.core2,
                          cutoff2=c.cutoff2, betas=c.betas, map_level=level)
            rc, (out_a, levels_a, maps_a) = RC.raw(host, RC.pack([job]))
            assert rc == 0 and out_a.tobytes() == out.tobytes() and levels_a.tobytes() == levels.tobytes(), (name, level)
            pair = maps_a.reshape(c.voxels, 2)
            assert pair[:, 0].tobytes() == planes[level].tobytes() and pair[:, 1].tobytes() == planes[L].tobytes(), (name, level)
    # and through the public entry, whose temperatures become the betas
    c = by_name("M=3")
    guest = pw.RigidGuest("case", tuple(c.offsets), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))
    T = np.array([300.0, 400.0])
    d = C.Case("public", c.dims, c.xyz, c.coef, offsets=c.offsets, dirs=c.dirs, origin=c.origin, step=c.step, core2=c.core2,
               cutoff2=c.cutoff2, betas=1.0 / (R * T))
    out, levels, maps = run(host, d)
    got = pw.rigid_guest_affinity(c.xyz, np.concatenate([c.coef, np.zeros((2, len(c.xyz), 1))], axis=2), guest, T,
                                  grid=(c.origin, float(c.step[0]), c.dims), directions=c.dirs, maps=True, level=1, core2=c.core2,
                                  cutoff2=c.cutoff2, device=-1)
    assert got.raw.tobytes() == out[0].tobytes() and got.levels.tobytes() == levels.tobytes()
    assert got.maps[:, 0].tobytes() == maps.reshape(3, -1)[1].tobytes() and got.maps[:, 1].tobytes() == maps.reshape(3, -1)[2].tobytes()


def test_bad_arguments(host):
    reasons = set()
    for packed, sizes, what in C.bad_batches():
        rc, got = C.raw(host, packed, sizes=sizes)
        assert rc == -2 and C.same(got, C.blank(packed[8], packed[7], packed[6])), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_rigid_cell: job 1: ") and what in message, (what, message)
        reasons.add(what)
    assert len(reasons) >= 25
    jobs = np.zeros(1, dtype=_lib.RIGID_CELL_JOB_DTYPE)
    jobs[0] = (0, 0, 0, 0, 1, 0, 1, 0, 1, 0, -1, 0, (0.0, 0.0, 0.0), C.ortho(1.0), 0.25, 0.0, 2, 2, 2, 0)
    with pytest.raises(ValueError, match='pw_rigid_cell: job 0: cutoff2 is 0: a cell has no "no cutoff"'):
        host.rigid_cell(jobs, np.zeros((0, 3)), np.zeros((0, 2)), [0.0], [[0.0, 0.0, 1.0]], [0.4])


def test_permuting_the_directions_permutes_min_dir(host):
    c = by_name("S=2")
    perm = np.array([3, 0, 4, 1, 2])
    d = C.Case("permuted", c.dims, c.xyz, c.coef, offsets=c.offsets, dirs=c.dirs[perm], origin=c.origin, step=c.step, core2=c.core2,
               cutoff2=c.cutoff2, betas=c.betas)
    a, b = run(host, c)[0][0], run(host, d)[0][0]
    assert a["u_min"] == b["u_min"] and perm[b["min_dir"]] == a["min_dir"] and a["min_voxel"].tolist() == b["min_voxel"].tolist()
    assert a["n_blocked_poses"] == b["n_blocked_poses"] and a["n_dead"] == b["n_dead"]


def test_an_atom_beyond_the_reach_changes_no_byte(host):
    c = by_name("S=3")
    far = np.concatenate([c.xyz, [[80.0, -70.0, 90.0]]])
    coef = np.concatenate([c.coef, np.full((3, 1, 2), 7.0)], axis=1)
    d = C.Case("one-more", c.dims, far, coef, offsets=c.offsets, dirs=c.dirs, origin=c.origin, step=c.step, core2=c.core2,
               cutoff2=c.cutoff2, betas=c.betas)
    assert C.same(run(host, c), run(host, d))


def test_a_cyclic_shift_of_the_atoms_by_a_cell_vector_keeps_the_integers():
    """The CC3 cell with every atom moved by the cell vector a: the listed images change, the crystal does not."""
    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="N2", temperatures=300.0, spacing=2.0, cutoff=6.0, directions=pw.sphere_directions(4), device=-1)
    a = pw.rigid_guest_field(xyz, elements, lattice, **kw)
    b = pw.rigid_guest_field(xyz + np.asarray(lattice)[:, 0][None, :], elements, lattice, **kw)
    for name in ("n_voxels", "n_blocked_poses", "n_dead"):
        assert a.raw[name] == b.raw[name], name
    assert np.array_equal(np.isinf(a.u_min_map), np.isinf(b.u_min_map))


@pytest.fixture(scope="module")
def cc3():
    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="CO2", temperatures=[250.0, 350.0], spacing=1.0, cutoff=8.0, directions=pw.sphere_directions(8), device=-1)
    return elements, xyz, lattice, kw, pw.rigid_guest_field(xyz, elements, lattice, **kw)


def test_the_field_of_the_cc3_cell(cc3):
    elements, xyz, lattice, kw, field = cc3
    assert field.zbar.shape[0] == 2 and field.zbar.shape[1:] == field.u_min_map.shape == tuple(field.shape[::-1])
    for level in range(2):
        F = field.free_energy(level)
        assert np.array_equal(np.isfinite(F), field.zbar[level] > 0.0) and (F[field.zbar[level] == 0.0] == np.inf).all()
    assert field.n_dead == int(np.isinf(field.u_min_map).sum()) > 0 and not field.clamped
    assert field.min_energy == field.u_min_map.min() < 0.0 and np.isfinite(field.min_position).all()
    assert np.abs(np.linalg.norm(field.min_direction) - 1.0) < 1e-12
    assert (field.henry > 0.0).all() and (field.heat > 0.0).all() and field.series("henry", 1)[1].all()
    n2 = pw.rigid_guest_field(xyz, elements, lattice, **{**kw, "guest": "N2"})
    assert (field.selectivity(n2) > 1.0).all()                       # CO2 binds more strongly than N2
    with pytest.raises(ValueError, match="the largest cutoff that fits is"):
        pw.rigid_guest_field(xyz, elements, lattice, **{**kw, "cutoff": 40.0})
    with pytest.raises(ValueError, match="mass"):
        pw.rigid_guest_diffusion(xyz, elements, lattice, **{**kw, "guest": pw.RIGID_GUESTS["CO2"]})


def test_percolation_and_diffusion_of_the_cc3_cell(cc3):
    elements, xyz, lattice, kw, field = cc3
    perc = pw.rigid_guest_percolation(xyz, elements, lattice, **kw)
    diff = pw.rigid_guest_diffusion(xyz, elements, lattice, **kw)
    assert len(perc) == 2 and diff.tensor.shape == (2, 3, 3) and diff.mass == pw.RIGID_GUEST_MASSES["CO2"]
    merge = R * 250.0
    for level, T in enumerate((250.0, 350.0)):
        F = field.free_energy(level)
        want = pw.percolation_field(F, device=-1)
        assert perc[level].levels.tobytes() == want.levels.tobytes() and perc[level].raw.tobytes() == want.raw.tobytes()
        one = pw.diffusion_field(F, lattice, T, pw.RIGID_GUEST_MASSES["CO2"], cap=100.0, merge=merge, device=-1)
        assert diff.n_basins[level] == one.n_basins and diff.n_sites[level] == one.n_sites
        scale = max(float(np.abs(one.tensor).max()), 1e-300)
        assert np.abs(diff.tensor[level] - one.tensor[0]).max() <= RTOL * scale
    system = pw.MolecularSystem.load_system({"elements": elements, "coordinates": xyz, "lattice": lattice})
    del kw["guest"]
    assert system.calculate_rigid_guest_diffusion("CO2", **kw).tensor.tobytes() == diff.tensor.tobytes()
    assert [p.levels.tobytes() for p in system.calculate_rigid_guest_percolation("CO2", **kw)] == [p.levels.tobytes() for p in perc]


def test_a_periodic_trajectory(tmp_path):
    """DLPOLY.rigid_field, .rigid_percolation and .rigid_diffusion over two frames in one call each: the batch's bytes,
    frame by frame those of a frame on its own; a trajectory without a cell is refused."""
    from pywindow_amd import synth

    elements, xyz, lattice = P.cc3_cell()
    kw = dict(temperatures=[250.0, 350.0], spacing=2.0, cutoff=6.0, directions=pw.sphere_directions(4), device=-1)
    frames = [xyz + np.random.default_rng(40 + k).normal(0.0, 0.02, xyz.shape) for k in range(2)]
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=np.asarray(lattice).T))
    field = traj.rigid_field("N2", **kw)
    read, cells = traj._read_selected([0, 1], True)
    again = pw.rigid_guest_field_batch(read, elements, cells, "N2", **kw)
    assert field.raw.shape == (2,) and field.raw.tobytes() == again.raw.tobytes() and field.frames.tolist() == [0, 1]
    assert field.levels.shape == (2, 2) and field.henry.shape == (2, 2) and field.min_position.shape == (2, 3)
    assert field.free_energy(1, t=1).shape == field.u_min_map[1].shape and field.series("heat", 1)[0].shape == (2,)
    one = traj.rigid_field("N2", frames=[1], **kw)
    assert one.zbar[0].tobytes() == field.zbar[1].tobytes() and one.raw[0].tobytes() == field.raw[1].tobytes()
    perc = traj.rigid_percolation("N2", **kw)
    assert len(perc) == 2 and perc[0].levels.shape == (2, 6) and perc[1].frames.tolist() == [0, 1]
    assert perc[1].levels[1].tobytes() == pw.percolation_field(field.free_energy(1, t=1), device=-1).levels.tobytes()
    diff = traj.rigid_diffusion("N2", **kw)
    assert diff.tensor.shape == (2, 2, 3, 3) and diff.coefficient.shape == (2, 2) and diff.n_basins.shape == (2, 2)
    assert diff.series("coefficient", level=1)[0].shape == (2,) and diff.mass == pw.RIGID_GUEST_MASSES["N2"]
    assert traj.rigid_diffusion("N2", frames=[1], **kw).tensor[0].tobytes() == diff.tensor[1].tobytes()
    flat = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY_flat", elements, frames[:1]))
    with pytest.raises(ValueError, match=r"not periodic.*rigid_affinity\(\)"):
        flat.rigid_diffusion("N2", device=-1)


def test_a_one_site_guest_reproduces_guest_diffusion():
    elements, xyz, lattice = P.cc3_cell()
    want = pw.guest_diffusion(xyz, elements, lattice, guest="Xe", temperatures=298.0, spacing=2.0, cutoff=8.0, maps=True, device=-1)
    rows = pw.lj_coefficients(list(elements), "Xe")[None]
    one = pw.RigidGuest("Xe1", (0.0,), (0.0,), (0.0,), (0.0,))
    kw = dict(guest=one, temperatures=298.0, spacing=2.0, cutoff=8.0, directions=[[0.0, 0.0, 1.0]], device=-1)
    got = pw.rigid_guest_diffusion(xyz, rows, lattice, mass=131.293, **kw)
    assert got.n_basins[0] == want.n_basins
    assert pw.rigid_guest_field(xyz, rows, lattice, **kw).u_min_map.tobytes() == want.maps.tobytes()
