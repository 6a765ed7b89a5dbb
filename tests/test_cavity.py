"""The cavity of a cage as a voxel flood fill (pw_cavity) on the host path, Context(-1): every case of
tests/_cavity_cases.py equals, byte for byte, the definition written directly in numpy (C.reference), one job at a time
and as one batch with entries nobody owns; the definition itself against scipy.ndimage.label where scipy imports; ties,
closed seeds, degenerate grids, word edges and serpentines; the refusals; and the Python layers above the entry
(pywindow_amd.cavity, Molecule.calculate_cavity on CC3, DLPOLY.cavity).  Nothing here has a tolerance.
tests/test_gpu_cavity.py holds the device to the same."""
import numpy as np
import pytest

import _cavity_cases as C
import pywindow_amd as pw
from pywindow_amd import _lib, engine, synth


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=16)


@pytest.fixture()
def on_the_host():
    engine.set_default_device(-1)
    yield
    engine.set_default_device(None)


def by_name(name):
    return next(c for c in C.cases() + C.big_cases() if c.name == name)


def test_every_case_one_job_at_a_time(host):
    """The first test of this file: it fails where the library has no pw_cavity."""
    for c in C.cases() + C.big_cases():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_the_definition_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for c in C.cases() + C.big_cases():
        ok = C.open_voxels(c)
        labels, _ = ndimage.label(ok)                                # (the default structure: 6-connectivity)
        i, j, l = c.seed
        want = (labels == labels[l, j, i]) & ok if ok[l, j, i] else np.zeros_like(ok)
        assert np.array_equal(C.component(ok, c.seed), want), c.name


def test_a_tie_is_free_and_a_plane_through_centres_keeps_them(host):
    for name in ("tie", "tie-plane-through-centres", "tie-probe"):
        c = by_name(name)
        rc, (out, words) = C.raw(host, C.pack([c]))
        assert rc == 0 and out["flags"][0] == 0
        mask = pw.cavity.unpack_mask(words, *c.dims)                 # [l, j, i], voxel (i, j, l) at (i - 6, j - 6, l - 6)
        cut = name == "tie-plane-through-centres"
        assert mask[6, 10, 9] and mask[6, 2, 9] and not mask[6, 9, 9]    # (3, 4, 0) and (3, -4, 0) at 5 exactly; (3, 3, 0)
        assert mask[6, 9, 10] == mask[6, 6, 11] == (not cut) and not mask[6, 6, 10]   # (4, 3, 0), (5, 0, 0); (4, 0, 0)
        if name == "tie-plane-through-centres":
            assert mask[:, :, 9].any() and not mask[:, :, 10:].any() and out["box"][0][1] == 9  # x = 3 stays, x = 4 goes
            assert out["n_voxels"][0] == out["n_open"][0] == (C.open_voxels(by_name("tie"))[:, :, :10]).sum()
        else:
            g = np.arange(-6, 7)
            inside = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2 < 25).sum()   # (integers)
            assert out["n_voxels"][0] == out["n_open"][0] == 13 ** 3 - inside


def test_a_closed_seed(host):
    for name in ("seed-closed", "seed-behind-a-plane", "cut-in-two-(1, 1, 1)"):
        rc, (out, words) = C.raw(host, C.pack([by_name(name)]))
        o = out[0]
        assert rc == 0 and o["flags"] == _lib.CAV_SEED_CLOSED and o["n_voxels"] == o["n_surface"] == o["n_face"] == 0
        assert (o["box"] == -1).all() and not o["first"].any() and not o["second"].any() and not words.any()
        assert o["reserved"] == 0 and (o["n_open"] > 0) == (name != "cut-in-two-(1, 1, 1)")


def test_degenerate_grids_without_atoms(host):
    for dims in ((1, 1, 1), (64, 1, 1), (1, 64, 1), (1, 1, 64), (2, 2, 2), (3, 3, 3), (64, 64, 1)):
        rc, (out, words) = C.raw(host, C.pack([by_name(f"no-atoms-{dims}")]))
        nx, ny, nz = dims
        o = out[0]
        total = nx * ny * nz
        inner = max(nx - 2, 0) * max(ny - 2, 0) * max(nz - 2, 0)
        assert rc == 0 and o["n_voxels"] == o["n_open"] == total and o["n_face"] == o["n_surface"] == total - inner
        assert list(o["box"]) == [0, nx - 1, 0, ny - 1, 0, nz - 1] and (words == C.pack_words(np.ones((nz, ny, nx), bool))).all()
        assert o["first"][0] == ny * nz * nx * (nx - 1) // 2 and o["second"][0] == ny * nz * (nx - 1) * nx * (2 * nx - 1) // 6
    o = C.raw(host, C.pack([by_name("cut-in-two-(64, 1, 1)")]))[1][0][0]
    # (the atom at (31.75, 0.25, 0.25) with radius 0.8 takes voxel 32 alone: voxel 31 is at 0.6875 >= 0.64)
    assert o["n_voxels"] == 32 and list(o["box"][:2]) == [0, 31] and o["n_open"] == 63


def test_word_edges_and_bits_beyond_nx(host):
    for nx, bit in ((64, 0), (64, 63), (63, 0), (63, 62), (5, 4)):
        c = by_name(f"word-edge-nx={nx}-bit={bit}")
        rc, (out, words) = C.raw(host, C.pack([c]))
        o = out[0]
        assert rc == 0 and o["n_voxels"] == 12 and o["n_open"] == 14 and list(o["box"][:2]) == [bit, bit]
        assert (words == np.uint64(1) << np.uint64(bit)).all() and o["n_face"] == 12 and o["first"][0] == 12 * bit


def test_serpentines(host):
    for dims in ((8, 8, 8), (64, 5, 3)):
        ok, length, second = C.serpentine(*dims)
        for c in (by_name(f"serpentine-{dims}"), by_name(f"serpentine-from-its-last-voxel-{dims}")):
            rc, (out, words) = C.raw(host, C.pack([c]))
            assert rc == 0 and out["n_voxels"][0] == length and out["n_open"][0] == length + second
            mask = pw.cavity.unpack_mask(words, *dims)
            assert not mask[1, 1, 3:6].any() and mask.sum() == length and (mask <= ok).all()
            assert out["n_surface"][0] == length                   # one voxel wide: all of it is surface


def test_one_batch_with_holes_and_the_number_of_threads():
    jobs = C.cases() + C.big_cases()[:2]
    packed = C.pack(jobs, hole=2)
    want = C.expected(jobs, hole=2)
    for threads in (1, 16):
        rc, got = C.raw(_lib.Context(-1, host_threads=threads), packed)
        assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    untouched = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert ((untouched == C.SENTINEL).all(axis=1)).sum() == 2 * len(jobs)
    rc, got = C.raw(_lib.Context(-1, host_threads=3), C.pack(jobs, hole=1, mask=False), workspace_bytes=1)
    assert rc == 0 and C.same(got, C.expected(jobs, hole=1, mask=False)) and len(got[1]) == 0


def test_jobs_that_share_atoms_and_planes(host):
    c = by_name("planes-3")
    jobs = [c, by_name("tie"), c, c]
    rec = C.pack(jobs)[0]
    assert rec["atom_first"][0] == rec["atom_first"][2] == rec["atom_first"][3] and rec["plane_first"][2] == rec["plane_first"][0]
    rc, got = C.raw(host, C.pack(jobs))
    assert rc == 0 and C.same(got, C.expected(jobs)) and got[0][0].tobytes() == got[0][3].tobytes()


def test_bad_arguments_are_refused_and_nothing_is_written(host):
    batches = C.bad_batches()
    assert len(batches) >= 30
    for packed, sizes, what in batches:
        for budget in (None, 1):
            rc, got = C.raw(host, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and C.same(got, C.blank(packed[4], packed[5])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_cavity: job 1: ") and what in message, (what, message)
    packed, _, _ = batches[0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        host.cavity(packed[0], packed[1], packed[2], packed[3])
    words = C.pack([by_name("serpentine-(8, 8, 8)")] * 2)
    rc, got = C.raw(host, words[:6] + (words[6][:-1], words[7]))
    assert rc == -2 and "job 1: the open words are outside their array" in _lib.load().pw_last_error().decode()


def test_no_jobs_and_the_wrapper(host):
    assert C.raw(host, C.pack([]))[0] == 0
    c = by_name("probe")
    rec, xyz, radii, planes, *_ = C.pack([c])
    out, mask = host.cavity(rec, xyz, radii, planes)
    want = C.reference_cached(c)
    assert out[0].tobytes() == want[0].tobytes() and np.array_equal(mask, want[1])
    rec["mask_first"] = -1
    assert host.cavity(rec, xyz, radii, planes)[1] is None


# ---- pywindow_amd.cavity --------------------------------------------------------------------------------------------

def test_cavity_grid_box_and_derived_quantities():
    c = by_name("tie")
    cav = pw.cavity_grid([[0.0, 0.0, 0.0]], [1.0], [0.0, 0.0, 0.0], spacing=0.5, half_width=3.0, mask=True, device=-1)
    assert tuple(cav.shape) == (12, 12, 12) and np.array_equal(cav.origin, [-2.75] * 3) and cav.seed_closed and not cav.closed
    assert cav.n_voxels == 0 and cav.volume == 0.0 and np.isnan(cav.centroid).all() and not cav.mask.any()
    # a hollow shell of atoms: closed, the centroid in the middle by symmetry, an isotropic tensor
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float)
    cav = pw.cavity_grid(2.0 * g, np.full(26, 1.5), [0.0, 0.0, 0.0], spacing=0.25, half_width=4.0, mask=True, device=-1)
    assert cav.closed and cav.n_face == 0 and 0 < cav.n_voxels < cav.n_open and cav.mask.shape == (32, 32, 32)
    assert cav.mask.sum() == cav.n_voxels and cav.volume == cav.n_voxels * 0.25 ** 3
    assert np.array_equal(cav.centroid, [0.0, 0.0, 0.0])
    G = cav.gyration
    assert np.array_equal(G, G.T) and G[0, 0] == G[1, 1] == G[2, 2] > 0 and G[0, 1] == G[0, 2] == G[1, 2] == 0.0
    idx = np.argwhere(cav.mask)[:, ::-1] * 0.25 + cav.origin          # (i, j, l) -> coordinates
    assert np.allclose(np.cov(idx.T, bias=True), G, rtol=0, atol=1e-12)   # (the tensor's formula, not the kernel)
    assert abs(cav.asphericity) < 1e-12 and abs(cav.acylindricity) < 1e-12 and abs(cav.relative_shape_anisotropy) < 1e-12
    with pytest.raises(ValueError, match=r"more than 64: the smallest spacing that fits is 0\.5"):
        pw.cavity_grid(2.0 * g, np.full(26, 1.5), [0.0, 0.0, 0.0], spacing=0.25, half_width=16.0, device=-1)
    assert c.dims == (13, 13, 13)


def test_window_planes():
    from pywindow_amd.utilities import window_planes

    p = window_planes([1.0, 1.0, 1.0], [[4.0, 1.0, 1.0], [1.0, 1.0, -1.0]])
    assert np.array_equal(p, [[1.0, 0.0, 0.0, 4.0], [0.0, 0.0, -1.0, 1.0]])
    assert window_planes([0.0, 0.0, 0.0], None).shape == (0, 4) and window_planes([0.0, 0.0, 0.0], np.array([])).shape == (0, 4)
    with pytest.raises(ValueError, match="coincides"):
        window_planes([1.0, 2.0, 3.0], [[1.0, 2.0, 3.0]])


# ---- CC3: Molecule.calculate_cavity and DLPOLY.cavity ----------------------------------------------------------------

@pytest.fixture(scope="module")
def cc3():
    elements, base = synth.load_cc3_base()
    return elements, base


def _molecule(cc3):
    return pw.Molecule({"elements": cc3[0], "coordinates": cc3[1]}, "cc3", 0)


def _definition_of(mol, cav, planes):
    from pywindow_amd.element_data import VDW, element_ids

    c = C.Case("cc3", cav.shape, (int(cav.shape[0]) // 2 - 1,) * 3, mol.coordinates, VDW[element_ids(mol.elements)],
               cav.probe, cav.origin, cav.spacing, planes)
    return C.reference(c)


def test_cc3_cavity_is_closed_at_its_windows_and_exceeds_the_inscribed_sphere(cc3, on_the_host):
    from pywindow_amd.utilities import window_planes

    mol = _molecule(cc3)
    before = dict(_molecule(cc3).full_analysis())
    found = {}
    for probe in (0.0, 1.2):
        volume = mol.calculate_cavity(probe=probe)
        cav, props = mol.cavity, mol.properties["cavity"]
        assert cav.closed and cav.n_face == 0 and props["closed"] is True and tuple(cav.shape) == (46, 46, 46)
        assert props["volume"] == volume == cav.n_voxels * 0.125 and props["n_voxels"] == cav.n_voxels > 0
        assert props["spacing"] == 0.5 and props["probe"] == probe and set(props) == {
            "volume", "centre", "closed", "n_voxels", "spacing", "probe"}
        planes = window_planes(mol.pore_opt_COM, mol.properties["windows"]["centre_of_mass"])
        assert planes.shape == (4, 4)
        want, _ = _definition_of(mol, cav, planes)
        assert cav.raw.tobytes() == want.tobytes()
        assert np.linalg.norm(props["centre"] - mol.pore_opt_COM) < 1.0
        found[probe] = int(cav.n_voxels)
        print(f"CC3 probe {probe}: {cav.n_voxels} voxels, {volume} A^3, n_open {cav.n_open}, n_surface {cav.n_surface}")
    assert found[0.0] > found[1.2] > 0
    mol.calculate_cavity(probe=0.0)
    assert mol.properties["cavity"]["volume"] > mol.calculate_pore_volume_opt()
    # without planes the fill leaves through the windows and reaches the box
    mol.calculate_cavity(probe=0.0, close=None)
    assert not mol.cavity.closed and mol.cavity.n_face > 0 and mol.properties["cavity"]["closed"] is False
    assert mol.cavity.raw.tobytes() == _definition_of(mol, mol.cavity, None)[0].tobytes()
    print(f"CC3 without planes: {mol.cavity.n_face} face voxels of {mol.cavity.n_voxels}")
    # full_analysis does not call it, and its dict is what it was
    again = _molecule(cc3).full_analysis()
    assert "cavity" not in again and list(again) == list(before)
    assert repr(again) == repr(before)


def _history(tmp_path, cc3, n=6, cell=None):
    elements, base = cc3
    rng = np.random.default_rng(12)
    frames = [base + rng.normal(0.0, 0.03, base.shape) for _ in range(n)]
    return pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=cell)), frames


def test_cavity_of_a_trajectory_and_its_series(tmp_path, cc3, on_the_host):
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    traj, _ = _history(tmp_path, cc3)
    with pytest.raises(ValueError, match="no frame has been analysed"):
        traj.cavity()
    traj.analysis(frames=[0, 1, 2, 4, 5])
    cav = traj.cavity(mask=True)
    assert list(cav.frames) == [0, 1, 2, 4, 5] and cav.raw.shape == (5,) and len(cav.mask) == 5
    recs = traj.analysis_store.records
    coords = traj._read_selected([0, 1, 2, 4, 5], False)[0]
    radii = VDW[element_ids(traj.elements())]
    for t in range(5):
        win = engine.windows_of(recs[t])
        one = pw.cavity_grid(coords[t], radii, recs["pore_opt_c"][t], half_width=recs["maxd"][t] / 2.0,
                             planes=window_planes(recs["pore_opt_c"][t], win[1]), mask=True, device=-1)
        assert one.raw.tobytes() == cav.raw[t].tobytes() and np.array_equal(one.mask, cav.mask[t])
        assert np.array_equal(one.centroid, cav.centroid[t]) and np.array_equal(one.gyration, cav.gyration[t])
    assert cav.closed.all() and (cav.volume > recs["pore_vol_opt"]).all()
    two = traj.cavity(frames=[4, 1])
    assert list(two.frames) == [4, 1] and two.raw.tobytes() == cav.raw[[3, 1]].tobytes()
    with pytest.raises(ValueError, match="frame 3 has not been analysed"):
        traj.cavity(frames=[3])
    # without planes no frame is closed, and `valid` of a series says so
    leaky = traj.cavity(close=None)
    values, valid = leaky.series("volume")
    assert (leaky.n_face > 0).all() and not valid.any() and values.dtype == np.float64
    values, valid = cav.series("volume")
    assert np.array_equal(valid, cav.n_face == 0) and valid.all() and np.array_equal(values, cav.n_voxels * 0.125)
    for name in ("n_surface", "asphericity", "acylindricity", "relative_shape_anisotropy"):
        assert cav.series(name)[0].shape == (5,) and np.isfinite(cav.series(name)[0]).all()
    with pytest.raises(KeyError):
        cav.series("colour")
    assert pw.time_correlation(values, max_lag=2, valid_a=valid, device=-1) is not None


def test_series_is_invalid_exactly_where_the_cavity_reaches_a_face():
    """A shell of 26 atoms that holds its void in frames 0, 2, 3 and 5 and is blown up until it leaks in frames 1 and 4."""
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float)
    scale = np.array([2.0, 3.2, 1.9, 1.8, 3.4, 2.0])
    cav = pw.cavity_grid(g[None] * scale[:, None, None], np.full(26, 1.5), np.zeros((6, 3)), spacing=0.25, half_width=7.0,
                         device=-1)
    values, valid = cav.series("volume")
    assert np.array_equal(valid, cav.n_face == 0) and np.array_equal(valid, [True, False, True, True, False, True])
    assert not cav.seed_closed.any() and np.array_equal(cav.closed, valid) and (cav.n_voxels > 0).all()
    assert cav.raw[0].tobytes() == cav.raw[5].tobytes() and values[0] >= values[2] >= values[3] > 0 and values[0] > values[3]
    tc = pw.time_correlation(values, max_lag=2, valid_a=valid, device=-1)
    assert tc.n == 4 and tc.pairs[0] == 4
    assert pw.lomb_scargle(values, valid=valid, device=-1) is not None
    assert pw.gate_statistics(values, [float(values[0])], valid=valid, device=-1) is not None
    assert pw.transition_counts(values, [float(values[0])], 1, valid=valid, device=-1) is not None
    assert pw.gaussian_kde_1d(values[valid], np.linspace(0.0, 2.0 * values[0], 5), device=-1) is not None


def test_a_periodic_trajectory_is_refused(tmp_path, cc3, on_the_host):
    traj, _ = _history(tmp_path, cc3, n=2, cell=np.eye(3) * 40.0)
    with pytest.raises(ValueError, match="cavity: a periodic or modular trajectory is not supported yet"):
        traj.cavity()
