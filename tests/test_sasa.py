"""The accessible surface of a cage by test points (pw_sasa) on the host path, Context(-1): every case of
tests/_sasa_cases.py equals, byte for byte, the definition written directly in numpy without culling (C.reference), one
job at a time and as batches with entries nobody owns; ties, exclusion by index, the analytic count of two spheres, the
grid's edges; the refusals; and the Python layers above the entry (pywindow_amd.surface,
Molecule.calculate_surface_area on CC3, DLPOLY.surface).  Only the areas' formulas have floating point, and they are
compared with the same formulas.  tests/test_gpu_sasa.py holds the device to the same."""
import math

import numpy as np
import pytest

import _sasa_cases as C
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
    return next(c for c in C.cases() if c.name == name)


def counts(host, name):
    rc, (out, exposed, inside) = C.raw(host, C.pack([by_name(name)]))
    assert rc == 0
    return out[0], exposed, inside


def test_every_case_one_job_at_a_time(host):
    """The first test of this file: it fails where the library has no pw_sasa."""
    for c in C.cases() + [C.big_case()]:
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_batches_with_holes_and_the_number_of_threads():
    groups = C.by_directions(C.cases() + [C.big_case()])
    assert len(groups) > 5 and any(len(g) > 3 and any(c.dims for c in g) and any(not c.dims for c in g) for g in groups)
    for jobs in groups:
        packed = C.pack(jobs, hole=2)
        want = C.expected(jobs, hole=2)
        results = []
        for threads in (1, 16):
            rc, got = C.raw(_lib.Context(-1, host_threads=threads), packed)
            assert rc == 0 and C.same(got, want), (jobs[0].name, threads, C.first_difference(got, want))
            results.append(got)
        assert C.same(results[0], results[1])
        untouched = np.frombuffer(got[0].tobytes(), dtype=np.uint8).reshape(len(got[0]), -1)
        assert ((untouched == C.SENTINEL).all(axis=1)).sum() == 2 * len(jobs)
        first = packed[0]["count_first"]
        for k in range(len(jobs)):
            assert (got[1][first[k] - 2:first[k]].view(np.uint8) == C.SENTINEL).all()
            assert (got[2][first[k] - 2:first[k]].view(np.uint8) == C.SENTINEL).all()


def test_no_atoms_one_atom_and_the_hook_on_the_host(host):
    o, exposed, inside = counts(host, "no-atoms")
    assert o["exposed"] == o["inside"] == o["flags"] == o["reserved"] == 0 and len(exposed) == 0
    o, exposed, inside = counts(host, "one-atom")
    assert o["exposed"] == 64 and list(exposed) == [64] and list(inside) == [0] and o["flags"] == 0
    assert C.raw(host, C.pack([]))[0] == 0
    packed = C.pack([by_name("n=130")])
    rc, got = C.raw(host, packed, hook=dict(list_capacity=-1, lds_words=-1, block_atoms=7))
    assert rc == 0 and C.same(got, C.expected([by_name("n=130")]))


def test_equality_is_exposed_and_one_ulp_more_buries(host):
    for name in ("tie", "tie-probe"):
        o, exposed, _ = counts(host, name)
        # atom 0: all six points, (1, 0, 0) at distance 2 exactly from atom 1 of reach 2 among them; atom 1: its point
        # (1, 0, 0) is at distance 1 = the reach of atom 0 exactly, exposed as well
        assert list(exposed) == [6, 6], name
        o, exposed, _ = counts(host, name + "-one-ulp-more")
        # (atom 1 has grown by an ulp as well: its point 3 - R is now nearer to atom 0 than 1, and buried too)
        assert list(exposed) == [5, 5], name


def test_exclusion_is_by_index(host):
    o, exposed, _ = counts(host, "same-position-unequal")
    assert list(exposed) == [0, 65]                                  # the smaller is buried, the larger does not bury itself
    o, exposed, _ = counts(host, "same-position-equal")
    assert exposed[0] == exposed[1] and np.array_equal(exposed, C.reference(by_name("same-position-equal"))[1])
    o, exposed, _ = counts(host, "zero-radius")
    # atom 0 (radius 0, its points are its centre) is inside atom 1; atom 2 (radius 0, far away) is exposed and, with
    # R * R = 0, buries nothing: atom 1 loses no point to either
    assert list(exposed) == [0, 65, 65]
    o, exposed, _ = counts(host, "inside-another")
    assert list(exposed) == [65, 0]


def test_culling_cannot_show(host):
    for name, want in (("far", [129, 129]), ("just-outside", [129, 129])):
        assert list(counts(host, "culling-" + name)[1]) == want
    for name in ("touching", "in-the-margin", "overlapping-a-hair", "far", "just-outside"):
        c = by_name("culling-" + name)
        assert np.array_equal(counts(host, c.name)[1], C.reference(c)[1])
    for name in ("huge", "tiny"):
        assert 0 < counts(host, name)[0]["exposed"] < 3 * 65


def test_two_spheres_have_the_analytic_count(host):
    """The count of atom 0 is P minus the k with z_k > c: the chain from the spiral through the test point and the
    exposure test to the ballot's count, tied to a closed form and not to a restatement of itself."""
    for args in ((1.5, 1.25, 2.0, 129), (1.0, 1.0, 1.0, 960), (2.0, 0.75, 2.25, 65)):
        case, want = C.two_spheres(*args)
        assert 0 < want < args[3]
        o, exposed, _ = counts(host, case.name)
        assert exposed[0] == want == C.reference(case)[1][0], args
        # the area of the cap that is left, 2 pi a^2 (1 + c), to the resolution of the points
        s = pw.surface_area(case.xyz, case.radii, points=args[3], device=-1)
        a, b, d = args[:3]
        c = (a * a + d * d - b * b) / (2.0 * a * d)
        assert abs(s.area_atoms[0] - 2.0 * math.pi * a * a * (1.0 + c)) <= 4.0 * math.pi * a * a / args[3]


def test_the_grid_at_its_edges(host):
    """The atom at (1, 1, 1) with radius 1 has the six points +x, -x, +y, -y, +z, -z, all exposed; voxel coordinates are
    0, 0.5, 1, ..."""
    def inside_points(name):
        """Which of the six points is inside: one direction a call."""
        c = by_name(name)
        found = []
        for k in range(6):
            one = C.Case(name, c.xyz, c.radii, np.ascontiguousarray(C.AXES[k:k + 1]), dims=c.dims, origin=c.origin, h=c.h, words=c.words)
            found.append(int(C.raw(host, C.pack([one]))[1][2][0]))
        o, exposed, inside = counts(host, name)
        assert list(exposed) == [6] and o["flags"] == _lib.SASA_GRID and inside[0] == sum(found) == C.reference(c)[2][0], name
        return found

    # (2, 1, 1) lies ON the coordinate of voxel 4: its cell starts there, voxel 5 is a corner of it and voxel 3 is not
    assert inside_points("on-a-coordinate-upper-corner") == [1, 0, 0, 0, 0, 0]
    assert inside_points("on-a-coordinate-not-the-cell-below")[0] == 0
    assert inside_points("left-of-voxel-0") == [0, 1, 0, 0, 0, 0]     # (0, 1, 1): i0 = -1, the corner 0 alone
    assert inside_points("left-of-voxel-0-next-voxel")[1] == 0
    assert inside_points("right-of-the-last-voxel")[0] == 1           # (2, 1, 1): i0 = 2 = nx - 1, the corner 2 alone
    assert inside_points("right-of-the-last-voxel-garbage-bits") == [0] * 6          # bits at i >= nx are not voxels
    # far from the grid on every axis: i0 is n - 1 (or -1) on each, so the voxel at that corner of the grid decides
    assert inside_points("far-from-the-grid-corner-voxel-set") == [1] * 6
    assert inside_points("far-from-the-grid-corner-voxel-clear") == [0] * 6
    assert inside_points("far-below-the-grid") == [1] * 6
    assert inside_points("nx=64-bit-63")[0] == 1 and inside_points("nx=64-bit-62-is-no-corner")[0] == 0
    # nx = 1: voxel 0 is the corner of every cell along x; (0, 2, 2) serves +x and -x, (0, 4, 2) serves +y
    assert inside_points("nx=1") == [1, 1, 1, 0, 0, 0]
    # ny = nz = 1: row 0 is every point's; voxel 4 is a corner for (2, 1, 1) alone, the others have i0 = 0 or 2
    assert inside_points("ny=1-nz=1") == [1, 0, 0, 0, 0, 0]
    assert inside_points("one-corner-of-one-cell") == [1, 0, 0, 0, 0, 0]


def test_bad_arguments_are_refused_and_nothing_is_written(host):
    batches = C.bad_batches()
    assert len(batches) >= 40
    for packed, sizes, null, what in batches:
        for hook in (None, dict(block_atoms=2)):
            rc, got = C.raw(host, packed, hook=hook, sizes=sizes, null=null)
            assert rc == -2 and C.same(got, C.blank(packed[6], packed[5])), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_sasa: job 1: ") and what in message, (what, message)
    packed = next(b for b in batches if b[3] == "a coordinate is not finite")[0]
    with pytest.raises(ValueError, match="job 1: a coordinate is not finite"):
        host.sasa(packed[0], packed[1], packed[2], packed[3], packed[4])


def sweep_of_rows(outs):
    """The job named for a shared row of out, or -1: the sweep of sasa_check restated -- rows sorted by (row, job), of
    equal neighbours the lowest later one."""
    rows, bad = sorted((o, k) for k, o in enumerate(outs)), -1
    for i in range(1, len(rows)):
        if rows[i][0] == rows[i - 1][0] and (bad < 0 or rows[i][1] < bad):
            bad = rows[i][1]
    return bad


def sweep_of_counts(jobs):
    """The job named for shared entries of exposed and inside, or -1: the sweep of sasa_check restated -- the jobs
    (count_first, n) with atoms sorted by (count_first, job), each against the furthest end so far and its owner."""
    bad = end = owner = -1
    for first, k in sorted((first, k) for k, (first, n) in enumerate(jobs) if n > 0):
        if first < end and (bad < 0 or max(k, owner) < bad):
            bad = max(k, owner)
        if first + jobs[k][1] > end:
            end, owner = first + jobs[k][1], k
    return bad


def test_the_job_named_for_shared_outputs_is_the_sweeps():
    """Which job a refusal for shared outputs names -- or that there is none -- for every sequence of up to four jobs
    with count_first in 0 .. 3 and n in 0 .. 3 atoms, and for every assignment of rows of out in 0 .. 2.  The rows are
    swept first and the counts only when no row is shared, so the two are not crossed in full (5.7 million calls):
    every sequence of jobs has a row of its own each (69904 calls, the counts' sweep alone); every assignment of rows
    goes with counts that are apart and with counts that all overlap (240 calls: the rows' sweep, and that it comes
    first); and up to two jobs are crossed in full (2352 calls).  The sweeps above are sasa_check's own, restated."""
    import itertools

    L = _lib.load()
    ctx = _lib.Context(-1, host_threads=1)
    xyz, radii, u = np.array([[0.0, 0.0, 0.0], [9.0, 0.0, 0.0], [0.0, 9.0, 0.0]]), np.ones(3), np.array([[0.0, 0.0, 1.0]])
    exposed, inside = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    out = np.zeros(4, dtype=_lib.SASA_OUT_DTYPE)
    recs = {N: np.zeros(N, dtype=_lib.SASA_JOB_DTYPE) for N in range(1, 5)}
    for rec in recs.values():
        rec["word_first"] = -1

    def named(jobs, outs):
        rec = recs[len(jobs)]
        rec["count_first"], rec["n"] = [j[0] for j in jobs], [j[1] for j in jobs]
        rec["out"] = outs
        rc = L.pw_sasa(ctx._h, rec.ctypes.data, len(rec), xyz.ctypes.data, 3, radii.ctypes.data, 3, u.ctypes.data, 1, None, 0,
                       exposed.ctypes.data, inside.ctypes.data, 8, out.ctypes.data, 4)
        return "" if rc == 0 else L.pw_last_error().decode()

    def want(jobs, outs):
        bad = sweep_of_rows(outs)
        if bad >= 0:
            return f"pw_sasa: job {bad}: shares its row of out with an earlier job"
        bad = sweep_of_counts(jobs)
        return f"pw_sasa: job {bad}: shares entries of exposed and inside with an earlier job" if bad >= 0 else ""

    shapes = list(itertools.product(range(4), range(4)))             # (count_first, n)
    calls = 0
    for N in range(1, 5):
        for jobs in itertools.product(shapes, repeat=N):
            outs = list(range(N))
            assert named(jobs, outs) == want(jobs, outs), (jobs, outs)
            calls += 1
        for outs in itertools.product(range(3), repeat=N):
            for jobs in ([(k, 1) for k in range(N)], [(0, 2)] * N):
                assert named(jobs, list(outs)) == want(jobs, list(outs)), (jobs, outs)
                calls += 1
    for N in (1, 2):
        for jobs in itertools.product(shapes, repeat=N):
            for outs in itertools.product(range(3), repeat=N):
                assert named(jobs, list(outs)) == want(jobs, list(outs)), (jobs, outs)
                calls += 1
    assert calls == 69904 + 240 + 2352
    # (a case that decides between the orders: sorted by length, job 2 would be named)
    assert want([(0, 1), (0, 3), (0, 2)], [0, 1, 2]).startswith("pw_sasa: job 1: shares entries")


def test_the_wrapper(host):
    c = by_name("random-directions-and-words")
    rec, xyz, radii, directions, words, *_ = C.pack([c])
    out, exposed, inside = host.sasa(rec, xyz, radii, directions, words)
    want = C.reference_cached(c)
    assert out[0].tobytes() == want[0].tobytes() and np.array_equal(exposed, want[1]) and np.array_equal(inside, want[2])
    assert exposed.dtype == inside.dtype == np.int32 and 0 < inside.sum() < exposed.sum()


# ---- pywindow_amd.surface -------------------------------------------------------------------------------------------

def test_sphere_directions_is_its_formula():
    for P in (1, 2, 65, 960, 4096):
        u = pw.sphere_directions(P)
        k = np.arange(P, dtype=np.float64)
        z = 1.0 - (2.0 * k + 1.0) / P
        phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
        assert u.shape == (P, 3) and u.dtype == np.float64 and np.array_equal(u[:, 2], z)
        assert np.array_equal(u[:, 0], np.sqrt(1.0 - z * z) * np.cos(phi)) and np.array_equal(u[:, 1], np.sqrt(1.0 - z * z) * np.sin(phi))
        assert (np.abs(((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) - 1.0) <= 1e-12).all()
    for P in (0, 4097):
        with pytest.raises(ValueError, match="points"):
            pw.sphere_directions(P)


def test_surface_areas_are_the_counts_formulas():
    R = 1.7
    s = pw.surface_area([[3.0, -2.0, 0.5]], [R], device=-1)
    assert s.area == 4.0 * math.pi * R * R and s.points == 960 and list(s.exposed) == [960] and s.internal_area == 0.0
    assert s.external_area == s.area and s.closed is None
    s = pw.surface_area([[3.0, -2.0, 0.5]], [1.2], probe=0.5, points=100, device=-1)
    assert s.area == 4.0 * math.pi * (1.2 + 0.5) * (1.2 + 0.5) and s.probe == 0.5
    c = by_name("P=129")
    s = pw.surface_area(c.xyz, c.radii, probe=c.probe, points=129, device=-1)
    want = C.reference_cached(c)
    assert np.array_equal(s.exposed, want[1]) and s.raw["exposed"] == want[0]["exposed"]
    reach = c.radii + c.probe
    assert np.array_equal(s.area_atoms, 4.0 * math.pi * reach * reach * (want[1] / 129))
    assert s.area == s.area_atoms.sum() and 0 < s.area < (4.0 * math.pi * reach * reach).sum()
    many = pw.surface_area(np.stack([c.xyz, c.xyz + 1.0, c.xyz * 1.1]), c.radii, probe=c.probe, points=129, device=-1)
    assert many.exposed.shape == (3, 12) and many.area.shape == (3,) and np.array_equal(many.exposed[0], s.exposed)
    assert many.area[0] == s.area and many.area[2] >= many.area[0]
    values, valid = many.series("area")
    assert np.array_equal(values, many.area) and valid.all() and valid.dtype == bool and values.dtype == np.float64
    assert np.array_equal(many.series("exposed")[0], many.raw["exposed"])
    with pytest.raises(KeyError):
        many.series("colour")


def test_a_cavity_tells_the_sides_apart_and_its_probe_must_match():
    # a hollow shell of 26 atoms: the cavity in the middle is closed, and the points that face it are inside
    g = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float)
    xyz, radii = 2.0 * g, np.full(26, 1.5)
    cav = pw.cavity_grid(xyz, radii, [0.0, 0.0, 0.0], spacing=0.25, half_width=4.0, mask=True, device=-1)
    assert cav.closed
    s = pw.surface_area(xyz, radii, cavity=cav, device=-1)
    assert s.closed is True and 0 < s.internal_area < s.area and s.external_area == s.area - s.internal_area
    assert (s.inside <= s.exposed).all() and s.raw["flags"] == _lib.SASA_GRID and s.raw["inside"] == s.inside.sum()
    # by symmetry the six face atoms have the same counts, and so have the eight corner atoms
    face = [i for i, v in enumerate(g) if np.abs(v).sum() == 1]
    assert len(face) == 6 and s.inside[face].min() > 0
    # the definition, with the cavity's words
    words = C.pack_words(cav.mask)
    c = C.Case("shell", xyz, radii, C.spiral(960), dims=tuple(cav.shape), origin=cav.origin, h=cav.spacing, words=words)
    want = C.reference(c)
    assert np.array_equal(s.exposed, want[1]) and np.array_equal(s.inside, want[2])
    with pytest.raises(ValueError, match="made for the probe 0.0, not 0.5"):
        pw.surface_area(xyz, radii, probe=0.5, cavity=cav, device=-1)
    with pytest.raises(ValueError, match="mask=True"):
        pw.surface_area(xyz, radii, cavity=pw.cavity_grid(xyz, radii, [0.0, 0.0, 0.0], spacing=0.25, half_width=4.0, device=-1), device=-1)
    # frames: 0 and 2 hold their void, 1 is blown up until it leaks -- `valid` of a series is the cavity's `closed`
    scale = np.array([2.0, 3.2, 1.9])
    frames = g[None] * scale[:, None, None]
    cavs = pw.cavity_grid(frames, radii, np.zeros((3, 3)), spacing=0.25, half_width=7.0, mask=True, device=-1)
    many = pw.surface_area_batch(frames, radii, cavity=cavs, device=-1)
    values, valid = many.series("internal_area")
    assert np.array_equal(valid, [True, False, True]) and np.array_equal(valid, cavs.closed) and (values[valid] > 0).all()
    assert np.array_equal(values, many.internal_area) and many.inside.shape == (3, 26)
    assert pw.time_correlation(values, max_lag=1, valid_a=valid, device=-1) is not None
    with pytest.raises(ValueError, match="one cavity per frame"):
        pw.surface_area_batch(frames[:2], radii, cavity=cavs, device=-1)


# ---- CC3: Molecule.calculate_surface_area and DLPOLY.surface ---------------------------------------------------------

@pytest.fixture(scope="module")
def cc3():
    return synth.load_cc3_base()


def test_cc3_has_an_internal_surface_until_the_probe_is_too_large(cc3, on_the_host):
    mol = pw.Molecule({"elements": cc3[0], "coordinates": cc3[1]}, "cc3", 0)
    before = dict(pw.Molecule({"elements": cc3[0], "coordinates": cc3[1]}, "cc3", 0).full_analysis())
    total = mol.calculate_surface_area()
    props = mol.properties["surface_area"]
    assert total == props["area"] == mol.surface.area > 0 and props["internal_area"] is None and props["closed"] is None
    assert set(props) == {"area", "internal_area", "external_area", "closed", "probe", "points"} and props["points"] == 960
    assert "cavity" not in mol.properties                            # (no side: no analysis and no cavity)
    internal = mol.calculate_surface_area(side="internal")
    props = mol.properties["surface_area"]
    assert 0 < internal == props["internal_area"] < props["area"] == total and props["closed"] is True
    assert props["external_area"] == props["area"] - props["internal_area"] == mol.calculate_surface_area(side="external")
    assert mol.cavity.mask is not None and mol.cavity.closed and mol.properties["cavity"]["probe"] == 0.0
    print(f"CC3 probe 0: area {total}, internal {internal}, exposed {int(mol.surface.raw['exposed'])}, "
          f"inside {int(mol.surface.raw['inside'])}")
    # a probe too large to enter the cage: no cavity, no internal surface
    assert mol.calculate_surface_area(probe=3.0, side="internal") == 0.0
    assert mol.properties["surface_area"]["area"] > total and mol.properties["surface_area"]["closed"] is False
    with pytest.raises(ValueError, match="side"):
        mol.calculate_surface_area(side="left")
    again = pw.Molecule({"elements": cc3[0], "coordinates": cc3[1]}, "cc3", 0).full_analysis()
    assert "surface_area" not in again and repr(again) == repr(before)


def test_surface_of_a_trajectory_and_its_series(tmp_path, cc3, on_the_host):
    from pywindow_amd.element_data import VDW, element_ids

    elements, base = cc3
    rng = np.random.default_rng(12)
    frames = [base + rng.normal(0.0, 0.03, base.shape) for _ in range(5)]
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames))
    whole = traj.surface(cavity=False, points=200)
    assert list(whole.frames) == [0, 1, 2, 3, 4] and whole.exposed.shape == (5, len(base)) and not whole.inside.any()
    assert whole.closed is None and whole.series("area")[1].all()
    with pytest.raises(ValueError, match="no frame has been analysed"):
        traj.surface()
    traj.analysis(frames=[0, 1, 3])
    s = traj.surface(points=200)
    cav = traj.cavity(mask=True)
    assert list(s.frames) == [0, 1, 3] and np.array_equal(s.exposed, whole.exposed[[0, 1, 3]])
    coords = traj._read_selected([0, 1, 3], False)[0]
    one = pw.surface_area(coords[1], VDW[element_ids(traj.elements())], points=200, device=-1,
                          cavity=pw.Cavity(cav.raw[1], cav.origin[1], cav.shape[1], cav.spacing, cav.probe, cav.mask[1]))
    assert np.array_equal(one.inside, s.inside[1]) and one.internal_area == s.internal_area[1]
    values, valid = s.series("internal_area")
    assert valid.all() and np.array_equal(valid, cav.closed) and (0 < values).all() and (values < s.area).all()
    assert len(set(values.tolist())) == 3
    two = traj.surface(points=200, frames=[3, 0])
    assert list(two.frames) == [3, 0] and np.array_equal(two.inside, s.inside[[2, 0]])
