"""The free-energy profile of a guest through a window on the host path: pw_hop on a device = -1 context against the
definition by another algorithm (tests/_hop_cases.py: a breadth-first search a slab, the energy by a loop over the
atoms), as BYTES; the rule that turns a profile into a rate against hand-made profiles.  numpy only, no GPU;
tests/test_gpu_hop.py holds the device to both."""
import math

import numpy as np
import pytest

import _hop_cases as C


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def by_name(name):
    return [c for c in C.cases() if c.name == name][0]


def test_the_layouts_and_the_symbol():
    from pywindow_amd import _lib

    assert _lib.HOP_JOB_DTYPE.itemsize == 176 and _lib.HOP_SLAB_DTYPE.itemsize == 32 and _lib.HOP_OUT_DTYPE.itemsize == 16
    assert hasattr(_lib.load(), "pw_hop") and "pw_hop" in _lib.EXPORTED_SYMBOLS and _lib.HOP_CLAMPED == C.CLAMPED


def test_the_case_list(host):
    """Host path == definition, job by job and as one batch with holes."""
    for c in C.cases():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c], host)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    jobs = C.cases()
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, host, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    rows = np.frombuffer(got[2].tobytes(), dtype=np.uint8).reshape(len(got[2]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)
    assert (got[3] == np.uint64(0xA5A5A5A5A5A5A5A5)).sum() >= 3 * sum(c.words for c in jobs)


def test_what_the_cases_are_meant_to_show(host):
    """The definition itself on the hand-made cases: the cases hit what their names say."""
    r = lambda name: C.reference_cached(by_name(name), host)
    s, z, o, w = r("1x1x1")
    assert s["n"][0] == 1 == s["n_face"][0] and s["u_min"][0] == 3.0 and (s["min_i"][0], s["min_j"][0]) == (0, 0)
    assert o["n"] == 1 and o["flags"] == 0 and w[0] == 1
    for name in ("serpentine-horizontal", "serpentine-vertical"):
        s = r(name)[0]
        assert s["n"][0] == 32 * 64 + 32 and s["u_min"][0] == 1.0
    s, z, o, w = r("ring")
    assert s["n"][0] == 9 and s["n_face"][0] == 0 and s["u_min"][0] == 1.0       # (the 56 voxels outside are not counted)
    s = r("two-components")[0]
    assert s["n"].tolist() == [3, 0] and s["n_face"].tolist() == [1, 0] and s["u_min"][0] == 1.0
    for name in ("seed-blocked", "seed-above-the-cap", "seed-outside-a-plane"):
        s, z, o, w = r(name)
        assert s["n"][0] == 0 == s["n_face"][0] and s["u_min"][0] == np.inf and (s["min_i"][0], s["min_j"][0]) == (-1, -1)
        assert z["z"][0] == 0.0 and not np.signbit(z["z"][0]) and not np.signbit(z["e"][0]) and w.sum() == 0 and o["n"] == 0
    for name in ("face-i0", "face-i-top", "face-j0", "face-j-top"):
        s = r(name)[0]
        assert s["n"][0] == 3 and s["n_face"][0] == 1, name
    assert r("corner-alone")[0]["n_face"][0] == 1 and r("all-of-3x3")[0]["n_face"][0] == 8
    assert r("n-ladder")[0]["n"].tolist() == [1, 63, 64, 65, 128, 129, 4096] and r("n-ladder")[2]["n"] == 4546
    assert r("U-equals-the-cap")[0]["n"][0] == 2
    assert np.signbit(r("zeros-minus-first")[0]["u_min"][0]) and r("zeros-minus-first")[0]["min_i"][0] == 1
    assert not np.signbit(r("zeros-plus-first")[0]["u_min"][0]) and r("zeros-plus-first")[0]["min_i"][0] == 1
    s = r("tied-minimum")[0]
    assert s["u_min"][0] == -2.0 and (s["min_i"][0], s["min_j"][0]) == (1, 0) and s["n"][0] == 12
    s, z, o, w = r("1e300-beta-0")
    assert s["n"].tolist() == [5, 5] and z["z"].tolist() == [5.0, 5.0] and o["flags"] == 0 and np.isfinite(z["e"]).all()
    s, z, o, w = r("clamped")
    assert o["flags"] == C.CLAMPED and z["z"][0] < z["z"][1] and np.isfinite(z["e"]).all() and s["n"][0] == 5
    assert len(r("L=8")[1]) == 8 * 5 and len(r("L=1")[1]) == 5 and not by_name("L=1").words
    assert r("m=1")[2]["n"] < r("m=0")[2]["n"] and 0 < r("m=65")[2]["n"] < r("m=0")[2]["n"]
    s = r("voxel-on-a-plane")[0]
    assert s["n"].tolist() == [7 * 8, 7 * 8, 7 * 8, 0]                           # (x == 6.0 and z == 2.0 are held)
    assert 0 < r("planes-off-axis")[2]["n"] < r("m=0")[2]["n"] and len(set(r("planes-off-axis")[0]["n"].tolist())) > 1
    for c in C.lj_cases():
        assert C.reference_cached(c, host)[2]["n"] > 0, c.name
    U = C.field_of(by_name("ties"))[0, 0]
    assert np.isinf(U[1:4]).all() and np.isfinite(U[0]) and U[5] != 0.0 and U[6] == 0.0
    assert r("ties")[0]["n"][0] == 4 and r("A=B=0")[1]["z"].tolist() == [r("A=B=0")[0]["n"][l // 2] for l in range(4)]


def test_lennard_jones_jobs_equal_the_jobs_given_the_map_of_pw_affinity(host):
    for c in C.lj_cases():
        packed = C.pack([c], fields=[C.affinity_map(host, c)])
        assert packed[0]["field_first"][0] == 0
        rc, got = C.raw(host, packed)
        want = C.raw(host, C.pack([c]))[1]
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_the_sums_are_pw_affinitys_with_the_slab_as_a_mask(host):
    """Six jobs: every slab's returned words fed to pw_affinity as a one-slab mask; (Z, E) equal as bytes."""
    chosen = [c for c in C.lj_cases() if c.words][:6]
    assert len(chosen) == 6
    for c in chosen:
        rc, (slabs, sums, out, words) = C.raw(host, C.pack([c]))
        assert rc == 0
        assert sums.tobytes() == C.affinity_of_the_words(host, c, words).tobytes(), c.name


def test_a_batch_of_64_mixed_jobs_at_1_3_and_16_threads(host):
    from pywindow_amd import _lib

    jobs = C.mixed_batch()
    assert len(jobs) == 64 and len({c.dims for c in jobs}) > 10 and {0, 5} <= {len(c.planes) for c in jobs}
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, host, hole=1)
    assert len(packed[1]) < sum(len(c.xyz) for c in jobs) and len(packed[3]) < sum(len(c.planes) for c in jobs)
    assert len(packed[5]) < sum(len(c.betas) for c in jobs)
    for threads in (1, 3, 16):
        rc, got = C.raw(_lib.Context(-1, host_threads=threads), packed)
        assert rc == 0 and C.same(got, want), (threads, C.first_difference(got, want))


def test_bad_arguments_write_nothing(host):
    from pywindow_amd import _lib

    batches = C.bad_batches()
    assert len(batches) > 50
    for packed, told, what in batches:
        rc, got = C.raw(host, packed, told=told)
        assert rc == -2 and C.same(got, C.blank(packed[6])), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_hop: job 1: ") and what in message, (what, message)


def test_the_rule_that_turns_a_profile_into_a_well_and_a_dividing_surface():
    from pywindow_amd.hopping import hopping_profile

    q = [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
    n, shut = [5] * 7, [0] * 7
    # a well at slab 1, a neck at slab 4, open ground beyond: the plain case
    p = hopping_profile([1.0, 9.0, 4.0, 2.0, 0.5, 3.0, 8.0], n, [0, 0, 0, 0, 0, 0, 2], q, 2)
    assert (p["l_w"], p["l_t"], p["first"], p["last"]) == (1, 4, 0, 5) and not p["seed_closed"] and not p["free_exit"]
    assert p["well_truncated"] and p["z_area"] == 0.5 and p["z_well"] == 1.0 + 9.0 + 4.0 + 2.0
    # ties: the lowest index wins both the well and the neck
    p = hopping_profile([9.0, 9.0, 0.5, 0.5, 0.5, 7.0, 7.0], [0] + [5] * 6, [0, 0, 0, 0, 0, 0, 1], q, 1)
    assert (p["l_w"], p["l_t"], p["first"], p["last"]) == (1, 2, 1, 5) and not p["well_truncated"] and p["z_well"] == 9.0
    # the well is sought at q <= 0 only, the neck from the well onwards
    p = hopping_profile([0.1, 2.0, 1.0, 1.5, 9.0, 0.7, 9.0], n, [0, 0, 0, 0, 0, 0, 1], q, 1)
    assert (p["l_w"], p["l_t"]) == (1, 5) and p["z_well"] == 0.1 + 2.0 + 1.0 + 1.5 + 9.0
    # a run that ends at the last slab, still falling: free_exit
    p = hopping_profile([5.0, 4.0, 3.0, 2.0, 1.0, 0.9, 0.8], n, shut, q, 2)
    assert p["l_t"] == 6 == p["last"] and p["free_exit"] and p["well_truncated"]
    # a run that starts at slab 0
    assert hopping_profile([5.0, 4.0, 3.0], [1, 1, 1], [0, 0, 1], [-1.0, 0.0, 1.0], 0)["well_truncated"]
    # a centre slab that is not closed: empty, or open to the side
    for counts, faces in (([5, 5, 0, 5, 5, 5, 5], shut), (n, [0, 0, 1, 0, 0, 0, 0])):
        p = hopping_profile([1.0] * 7, counts, faces, q, 2)
        assert p["seed_closed"] and p["l_w"] == -1 == p["l_t"] and math.isnan(p["z_area"])


def test_window_frame():
    import pywindow_amd as pw

    rng = np.random.default_rng(5)
    for w in (rng.normal(size=3), [0.0, 0.0, 2.0], [1.0, 1.0, 1.0], [-3.0, 0.0, 0.0]):
        c = rng.normal(size=3)
        f = pw.window_frame(c, c + np.asarray(w))
        assert np.allclose(f @ f.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(f), 1.0)
        assert np.allclose(f @ np.asarray(w), [0.0, 0.0, np.linalg.norm(w)], atol=1e-14)
    assert np.allclose(pw.window_frame([0, 0, 0], [1.0, 1.0, 1.0])[0], np.array([0.0, 1.0, -1.0]) / math.sqrt(2.0), atol=1e-15)
    with pytest.raises(ValueError):
        pw.window_frame([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])


def test_the_python_layer_on_the_host_path():
    """guest_hopping and Hopping on a hand-made tube of atoms, device = -1: a ring of atoms round the axis is the neck."""
    import pywindow_amd as pw
    from pywindow_amd import _lib
    from pywindow_amd.hopping import GUEST_MASSES

    angles = np.linspace(0.0, 2.0 * np.pi, 12, endpoint=False)
    ring = lambda z, r: np.stack([r * np.cos(angles), r * np.sin(angles), np.full(12, z)], axis=1)
    xyz = np.concatenate([ring(z, 4.5) for z in (-2.0, -1.0, 0.0, 1.0, 2.0)] + [ring(3.0, 3.4), ring(-3.0, 1.5)])
    coef = np.tile([[4.0 * 0.4 * 3.4 ** 12, 4.0 * 0.4 * 3.4 ** 6]], (len(xyz), 1))
    kw = dict(spacing=0.5, half_width=6.0, back=2.0, ahead=2.0, mass=40.0, device=-1)
    hp = pw.guest_hopping(xyz, coef, None, [0.0, 0.0, 0.0], [[0.0, 0.0, 3.0]], [300.0, 600.0], **kw)
    assert hp.slabs.shape == (1, 1, 15) and hp.Z.shape == (1, 1, 15, 2) and hp.rate.shape == (1, 2) and hp.q.shape == (1, 15)
    assert hp.q[0, 4] == -3.0 and hp.q[0, 10] == 0.0 and hp.valid.all() and not hp.free_exit.any()
    assert abs(hp.q[0, hp.l_t[0, 0]]) <= 0.5 and hp.q[0, hp.l_w[0, 0]] < -1.0
    assert hp.rate[0, 1] > hp.rate[0, 0] > 0.0 and hp.free_barrier[0, 0] > 0.0
    F = hp.free_energy
    assert np.isclose(F[0, hp.l_t[0, 0], 0] - F[0, hp.l_w[0, 0], 0], hp.free_barrier[0, 0])
    assert np.isclose(hp.area[0, 0], 0.25 * hp.Z[0, 0, hp.l_t[0, 0], 0])
    two = pw.guest_hopping_batch(np.stack([xyz, xyz]), coef, None, np.zeros((2, 3)), [[[0.0, 0.0, 3.0]], None], [300.0, 600.0], **kw)
    assert two.slabs.shape == (2, 1, 15) and two.n_windows.tolist() == [1, 0] and two.padding.tolist() == [[False], [True]]
    assert two.slabs[0].tobytes() == hp.slabs[0].tobytes() and (two.slabs["n"][1] == -1).all() and np.isnan(two.Z[1]).all()
    assert np.array_equal(two.escape_rate, [hp.rate[0], [0.0, 0.0]]) and np.array_equal(two.mean_rate()[0], hp.rate[0])
    values, valid = two.series("rate", level=1)
    assert values[0] == hp.rate[0, 1] and valid.tolist() == [True, False] and two.series("escape_rate")[1].tolist() == [True, False]
    assert np.array_equal(two.diffusion(6.0), two.escape_rate * 6.0)
    with pytest.raises(ValueError, match="spacing"):
        pw.guest_hopping(xyz, coef, None, [0.0, 0.0, 0.0], [[0.0, 0.0, 3.0]], [300.0], spacing=0.1, mass=40.0, device=-1)
    with pytest.raises(ValueError, match="spacing"):
        pw.guest_hopping(xyz, coef, None, [0.0, 0.0, 0.0], [[0.0, 0.0, 30.0]], [300.0], mass=40.0, device=-1)
    with pytest.raises(ValueError, match="mass"):
        pw.guest_hopping(xyz, coef, None, [0.0, 0.0, 0.0], [[0.0, 0.0, 3.0]], [300.0], device=-1)
    assert GUEST_MASSES["Xe"] == 131.293 and _lib.AFF_MAX_LEVELS == 8
