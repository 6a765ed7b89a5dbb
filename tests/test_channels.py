"""The pore network of a periodic cell on the host path (device = -1): pw_channels against the definition written twice
in numpy (tests/_channels_cases.py: by_rolls and by_search) as BYTES, the properties the definition implies, its
refusals, the periodic images of the public layer on the crystal cells of tests/golden/rebuild.npz, and the public
surface.  tests/test_gpu_channels.py holds the device to the same."""
import numpy as np
import pytest

import _channels_cases as C


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def solve(host, cases):
    """The host path's (out, comps, mask, labels) of a list of cases in one call."""
    rc, got = C.raw(host, C.pack(cases))
    assert rc == 0
    return got


def test_the_case_list_is_the_definition_byte_for_byte(host):
    """Every case alone, and all of them in one call with holes: the row, the table, the accessible words and the labels."""
    for c in C.cases() + C.big_cases():
        packed = C.pack([c])
        rc, got = C.raw(host, packed)
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    jobs = C.cases()
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    rows = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


def test_what_the_cases_are_for():
    """The properties the cases were built for, read from the definition."""
    ref = {c.name: C.reference_cached(c) for c in C.cases() + C.big_cases()}

    def comps(name):
        out, table = ref[name][:2]
        return table[:int(out["n_recorded"])]

    for bit, axis in enumerate("abc"):
        (row,) = comps(f"channel-along-{axis}")
        assert row["rank"] == 1 and row["wraps"] == sum(1 << (phi - 1) for phi in range(1, 8) if (phi >> bit) & 1)
        assert row["n_cross"].tolist() == [int(k == bit) for k in range(3)] and row["n_voxels"] == 8
    (row,) = comps("staircase-110")                                  # phi . (1, 1, 0) odd: phi = 1, 2, 5, 6
    assert (row["wraps"], row["rank"]) == (0b0110011, 1)
    (row,) = comps("staircase-111")                                  # every axis bit set, and still one dimension
    assert (row["wraps"], row["rank"]) == (0b1001011, 1) and all((row["wraps"] >> (phi - 1)) & 1 for phi in (1, 2, 4))
    assert comps("slab")["rank"].tolist() == [2] and comps("everything-open")["rank"].tolist() == [3]
    (row,) = comps("pocket-round-the-corner")                        # straddles all three faces, in one piece, and winds nowhere
    assert (row["n_voxels"], row["rank"], row["wraps"]) == (8, 0, 0) and (row["n_cross"] > 0).all()
    assert ref["pocket-round-the-corner"][2].any() == False and ref["slab"][2].any()   # noqa: E712
    assert comps("two-interleaved-channels")["rank"].tolist() == [1, 1]
    assert comps("double-helix")["rank"].tolist() == [0] and comps("double-helix")["n_cross"][0, 0] == 2
    assert comps("double-helix-tiled-twice")["rank"].tolist() == [1, 1]
    assert [c.limit for c in C.cases() if c.name == "double-helix"] == [True] and sum(c.limit for c in C.cases()) == 1
    out = ref["more-components-than-c_max=0"][0]
    assert out["n_components"] == 34 and out["n_recorded"] == 0 and out["flags"] == 1 and out["n_voxels_by_rank"].sum() == out["n_open"]
    assert set(np.unique(ref["more-components-than-c_max=0"][3])) == {254, 255}
    assert set(np.unique(ref["noise-(9, 8, 7)"][3])) == {0, 1, 2, 3, 4, 254, 255}
    assert ref["every-voxel-closed"][0]["n_components"] == 0 and (ref["every-voxel-closed"][3] == 255).all()
    assert sorted(comps("grid-64")["rank"].tolist()) == [0, 1, 3]
    for out, table, _, _ in ref.values():
        assert out["n_voxels_by_rank"].sum() == out["n_open"] and out["n_components_by_rank"].sum() == out["n_components"]
        firsts = table["first"][:int(out["n_recorded"])]
        assert (np.diff(firsts) > 0).all() and (table["first"][int(out["n_recorded"]):] == -1).all()


def shifted(c, axis, by):
    ok = np.roll(C.unpack_words(c.words, c.dims) if c.words is not None else C.open_voxels(c), by, axis)
    return C.Case(f"{c.name}-shifted", c.dims, words=C.pack_words(ok), c_max=254, labels=False)


def multiset(out, table):
    return sorted(zip(table["n_voxels"][:int(out["n_recorded"])].tolist(), table["wraps"][:int(out["n_recorded"])].tolist()))


def test_a_cyclic_shift_permutes_the_components(host):
    """The open words shifted by whole voxels along any axis, cyclically: another numbering, the same multiset of
    (n_voxels, wraps) -- on the library alone, no reference involved."""
    names = ("staircase-111", "pocket-round-the-corner", "double-helix", "noise-(63, 3, 4)", "noise-(64, 3, 4)",
             "noise-(9, 8, 7)", "rows=5x13", "skewed-cell")
    bases = [shifted(c, 0, 0) for c in C.cases() if c.name in names]
    assert len(bases) == len(names)
    moved = [shifted(b, axis, by) for b in bases for axis, by in ((2, 1), (2, -3), (1, 1), (0, 2), (0, -1))]
    got = solve(host, bases + moved)
    sets = [multiset(got[0][k], got[1][254 * k:254 * (k + 1)]) for k in range(len(bases) + len(moved))]
    assert not (got[0]["flags"] & 1).any()
    for q, m in enumerate(sets[len(bases):]):
        assert m == sets[q // 5], (bases[q // 5].name, q % 5)


def test_tiling_twice_doubles_what_winds_along_the_axis(host):
    """Open words tiled twice along an axis: a component whose bit of that axis is set comes back as one component of
    twice the voxels (its closed path of odd winding now takes both copies); one whose bit is clear comes back twice."""
    for c in [c for c in C.cases() if c.name in ("staircase-110", "slab", "two-interleaved-channels", "noise-(9, 8, 7)",
                                                  "noise-(6, 2, 5)", "rows=8x8", "double-helix")]:
        ok = C.unpack_words(c.words, c.dims) if c.words is not None else C.open_voxels(c)
        for bit, axis in enumerate(C.AXIS_OF_BIT):
            if 2 * ok.shape[axis] > 64:
                continue
            twice = np.concatenate([ok, ok], axis=axis)
            one, two = (C.Case("x", o.shape[::-1], words=C.pack_words(o), c_max=254, labels=False) for o in (ok, twice))
            got = solve(host, [one, two])
            a = got[1][:int(got[0][0]["n_recorded"])]
            b = got[1][254:254 + int(got[0][1]["n_recorded"])]
            winds = ((a["wraps"] >> (1 << bit) - 1) & 1).astype(bool)
            want = sorted((2 * a["n_voxels"][winds]).tolist() + 2 * a["n_voxels"][~winds].tolist())
            assert sorted(b["n_voxels"].tolist()) == want, (c.name, bit)


def test_n_open_never_rises_with_the_probe(host):
    base = [c for c in C.cases() if c.name == "skewed-cell"][0]
    ladder = [C.Case(f"probe-{p}", base.dims, base.xyz, base.radii, p, base.origin, base.step, c_max=0, mask=False, labels=False)
              for p in (0.0, 0.1, 0.3, 0.5, 0.9, 1.4)]
    n_open = solve(host, ladder)[0]["n_open"]
    assert (np.diff(n_open) <= 0).all() and n_open[0] > n_open[-1] >= 0


def test_refusals_name_job_1_and_leave_the_outputs_untouched(host):
    from pywindow_amd import _lib

    for packed, sizes, what in C.bad_batches():
        rc, got = C.raw(host, packed, sizes=sizes)
        assert rc == -2 and C.same(got, C.blank(*packed[3:7])), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_channels: job 1: ") and what in message, (what, message)
    packed = C.bad_batches()[0][0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        host.channels(packed[0], packed[1], packed[2])


def test_threads_do_not_show(host):
    from pywindow_amd import _lib

    jobs = C.mixed_batch()[:12]
    packed = C.pack(jobs, hole=1)
    want = C.raw(host, packed)[1]
    for threads in (1, 3):
        assert C.same(C.raw(_lib.Context(-1, host_threads=threads), packed)[1], want)


# ---- the crystal cells ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, probe", (("cc3_cell", 1.2), ("cc3_cell", 1.6), ("EPIRUR", 1.2), ("TATVER", 1.2)))
def test_crystal_cells_the_images_and_the_definition(host, name, probe):
    """The job pw.channel_network makes of a cell: the open words of the culled image list are those of all 27 images,
    the job is the definition, and the answers a prototype gave hold -- CC3 is a 3-dimensional network for a probe of
    1.2 A and a set of pockets at 1.6 A; the big voids of EPIRUR straddle the cell faces and wind nowhere."""
    culled, everything = C.crystal_case(name, probe), C.crystal_case(name, probe, cull=False)
    assert len(culled.xyz) < len(everything.xyz) == 27 * len(C.crystal(name)[1])
    packed = C.pack([culled])
    rc, got = C.raw(host, packed)
    want = C.expected([culled])
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    # (all 27 images of every atom against every voxel is the library's work, not numpy's: its closed voxels, label 255)
    closed = [C.raw(host, C.pack([C.Case(c.name, c.dims, c.xyz, c.radii, c.probe, c.origin, c.step, c_max=0, mask=False)]))[1][3] == 255
              for c in (culled, everything)]
    assert np.array_equal(closed[0], closed[1]) and (~closed[0]).sum() == want[0][0]["n_open"]
    out, table = got[0][0], got[1][:int(got[0][0]["n_recorded"])]
    top = int(np.flatnonzero(out["n_components_by_rank"])[-1])
    if name == "cc3_cell":
        assert culled.dims == (50, 50, 50) and top == (3 if probe == 1.2 else 0)
    if name == "EPIRUR":
        assert culled.dims == (33, 33, 47) and top == 0
        largest = table[np.argsort(-table["n_voxels"])[:3]]
        assert (largest["n_voxels"] > 1000).all() and (largest["n_cross"].sum(axis=1) > 0).all()
    if name == "TATVER":
        assert culled.dims == (40, 44, 46) and top == 3


def test_the_public_layer(host, tmp_path):
    """pw.channel_network on CC3 against the raw job; a ladder and its limiting probe; component_of; a rotated lattice
    gives the same integers; MolecularSystem.calculate_channels; a synthetic periodic HISTORY through DLPOLY.channels;
    the refusals."""
    import pywindow_amd as pw
    from pywindow_amd import channels as CN
    from pywindow_amd import synth

    elements, xyz, lattice = C.crystal("cc3_cell")
    one = pw.channel_network(xyz, elements, lattice, probe=1.2, c_max=254, mask=True, labels=True, device=-1)
    want = C.reference_cached(C.crystal_case("cc3_cell", 1.2))
    assert one.raw.tobytes() == want[0].tobytes() and one.components.tobytes() == want[1].tobytes()
    assert np.array_equal(one.accessible_words, want[2]) and one.dimensionality == 3 and not one.truncated
    volume = float(np.linalg.det(lattice))
    assert np.isclose(one.accessible_volume, 5860 * (volume / 50 ** 3), rtol=1e-12, atol=0.0)
    assert np.isclose(one.inaccessible_volume, 68 * (volume / 50 ** 3), rtol=1e-12, atol=0.0)
    assert one.void_fraction == 5928 / 50 ** 3 and one.accessible.sum() == 5860 and one.limiting_probe == 1.2
    # two points in the network carry one label, a point inside an atom 255
    inside = np.argwhere(one.accessible)[[0, -1]][:, ::-1]
    points = (inside + 0.5) / 50.0 @ np.asarray(lattice).T
    here = one.component_of(points)
    assert here[0] == here[1] < 254 and one.components[here[0]]["rank"] == 3 and one.component_of(xyz[:1]).tolist() == [255]
    ladder = pw.channel_network(xyz, elements, lattice, probe=[1.2, 1.6, 1.82], device=-1)
    assert ladder.dimensionality.tolist() == [3, 0, 0] and ladder.limiting_probe == 1.2 and ladder.truncated.tolist() == [False, True, True]
    assert (np.diff(ladder.n_open) < 0).all() and ladder.accessible_volume[1] == 0.0
    assert ladder.raw[0].tobytes() == one.raw.tobytes()
    # the same crystal turned: QR on the host brings it back to the triangular form, with the same voids up to rounding
    turn = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0]
    R, Q = CN.triangular_lattice(turn @ lattice)
    assert np.allclose(Q @ R, turn @ lattice) and np.allclose(np.tril(R, -1), 0.0) and (np.diag(R) > 0).all()
    turned = pw.channel_network(xyz @ turn.T, elements, turn @ lattice, probe=1.2, device=-1)
    assert turned.dimensionality == 3 and abs(int(turned.n_open) - 5928) < 60
    system = pw.MolecularSystem.load_system({"elements": elements, "coordinates": xyz, "lattice": lattice})
    assert system.calculate_channels(probe=1.2, c_max=254, device=-1).raw.tobytes() == one.raw.tobytes()
    with pytest.raises(ValueError, match="no unit cell"):
        pw.MolecularSystem.load_system({"elements": elements, "coordinates": xyz}).calculate_channels(device=-1)
    # a periodic HISTORY of three frames (the file keeps four decimals of a coordinate: compare with what was read)
    frames = [xyz + np.random.default_rng(40 + k).normal(0.0, 0.02, xyz.shape) for k in range(3)]
    path = synth.write_history(tmp_path / "HISTORY", elements, frames, cell=np.asarray(lattice).T)
    traj = pw.DLPOLY(path)
    got = traj.channels(probe=[1.2, 1.6], spacing=0.5, device=-1)
    read, cells = traj._read_selected([0, 1, 2], True)
    again = pw.channel_network_batch(read, elements, cells, probe=[1.2, 1.6], device=-1)
    assert got.raw.shape == (3, 2) and got.raw.tobytes() == again.raw.tobytes() and got.frames.tolist() == [0, 1, 2]
    assert got.dimensionality[:, 0].tolist() == [3, 3, 3] and (got.limiting_probe >= 1.2).all()
    values, valid = got.series("accessible_volume")
    assert values.shape == (3,) and valid.all() and (values > 500.0).all()
    assert traj.channels(probe=1.2, frames=[2], device=-1).raw[0, 0].tobytes() == got.raw[2, 0].tobytes()
    flat = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY_flat", elements, frames[:1]))
    with pytest.raises(ValueError, match="not periodic"):
        flat.channels(device=-1)
    # what the public layer refuses itself
    with pytest.raises(ValueError, match=r"smallest spacing that fits is 0\.3"):
        pw.channel_network(xyz, elements, lattice, spacing=0.3, device=-1)
    with pytest.raises(ValueError, match="thin cell"):
        pw.channel_network(xyz[:4], [30.0] * 4, lattice, device=-1)
    with pytest.raises(ValueError, match="c_max"):
        pw.channel_network(xyz, elements, lattice, c_max=255, device=-1)
    with pytest.raises(KeyError):
        one.series("volume")
    with pytest.raises(ValueError, match="labels=True"):
        ladder.component_of(points)
