"""The probe-swept cavity for a ladder of probes (pw_pore_sizes) on the host path, Context(-1): every case of
tests/_pores_cases.py equals, byte for byte, the definition written directly in numpy (P.reference), one job at a time
and as one batch with entries nobody owns; the definition's sweep against scipy.ndimage.binary_dilation where scipy
imports; the K rule, the ball, the corner distance, word edges, row ownership, attribution and closed seeds by known
answers; the refusals; and the Python layers above the entry (pywindow_amd.pores, Molecule.
calculate_pore_size_distribution on CC3, DLPOLY.pore_sizes).  Nothing the entry returns is compared with a tolerance.
tests/test_gpu_pores.py holds the device to the same."""
import math

import numpy as np
import pytest

import _cavity_cases as C
import _pores_cases as P
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
    return next(c for c in P.cases() if c.name == name)


def run(host, case, masks=True):
    rc, got = P.raw(host, P.Packed([case], masks=masks))
    assert rc == 0, _lib.load().pw_last_error().decode()
    return got


def test_every_case_one_job_at_a_time(host):
    """The first test of this file: it fails where the library has no pw_pore_sizes."""
    for c in P.cases():
        packed = P.Packed([c])
        rc, got = P.raw(host, packed)
        want = packed.expected()
        assert rc == 0 and P.same(got, want), (c.name, P.first_difference(got, want))
        levels, out, _ = got
        assert out["n_domain"][0] == out["n_none"][0] + levels["n_largest"].sum() and out["n_levels"][0] == c.L
        assert levels["n_swept"][0] == out["n_domain"][0] == levels["n_reach"][0]


def test_the_definitions_sweep_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for shape, K in (((9, 9, 9), 0), ((9, 9, 9), 5), ((7, 12, 30), 6), ((7, 12, 30), 7), ((3, 1, 20), 50), ((6, 5, 4), 200)):
        reach = rng.random(shape) < 0.02
        reach[tuple(s // 2 for s in shape)] = True
        R = math.isqrt(K)
        g = np.arange(-R, R + 1)
        ball = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2 <= K
        assert np.array_equal(P.sweep(reach, K), ndimage.binary_dilation(reach, structure=ball)), (shape, K)
        dense = rng.random(shape) < 0.7                              # (more voxels than offsets: the other branch)
        assert np.array_equal(P.sweep(dense, K), ndimage.binary_dilation(dense, structure=ball)), (shape, K)


def test_the_k_rule(host):
    below_one = np.nextafter(1.0, 0.0)
    assert P.k2_rule(1.0, 0.5) == 4 and P.k2_rule(below_one, 0.5) == 3 and P.k2_rule(0.0, 0.5) == 0
    assert P.k2_rule(0.25, 0.5) == 0 and P.k2_rule(1e6, 0.5) == P.MAX_K2 == _lib.PORES_MAX_K2 == 11907
    ladders = ((0.5, [0.0, 0.25, below_one, 1.0, 1e6]),
               (0.1, [0.0, 0.05, 0.1, 0.2, 0.3, np.nextafter(0.3, 1.0), 0.7, 1.0, 1.1, 10.9, 11.0]),
               (1.0, [P.probe_for(k) for k in (0, 1, 2, 11906, 11907, 11908)]))
    for h, probes in ladders:
        levels, _, _ = run(host, P.Case("k", (1, 1, 1), (0, 0, 0), probes, h))
        assert list(levels["k2"]) == [P.k2_rule(p, h) for p in probes], (h, list(levels["k2"]))
    levels, _, _ = run(host, P.Case("k", (1, 1, 1), (0, 0, 0), ladders[0][1], 0.5))
    assert list(levels["k2"]) == [0, 0, 3, 4, 11907]
    # h = 0.1, whose square is not exact: k * fl(0.01) <= fl(p * p) decides, and for p = 0.3 that is k = 8, not 9
    inexact = [P.k2_rule(p, 0.1) for p in ladders[1][1]]
    h2 = np.float64(0.1) * np.float64(0.1)
    for p, k in zip(ladders[1][1], inexact):
        assert k * h2 <= np.float64(p) * np.float64(p) and (k == P.MAX_K2 or (k + 1) * h2 > np.float64(p) * np.float64(p))
    assert inexact[:5] == [0, 0, 1, 4, 8] and inexact[5] == 9
    assert list(run(host, P.Case("k", (1, 1, 1), (0, 0, 0), ladders[2][1], 1.0))[0]["k2"]) == [0, 1, 2, 11906, 11907, 11907]


def test_the_ball(host):
    levels, out, mask = run(host, by_name("ball"))
    g = np.arange(-4, 5)
    d2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    assert list(levels["k2"][1:]) == list(P.BALL_K2) and out["n_domain"][0] == 729
    assert list(levels["n_swept"][1:]) == [int((d2 <= k).sum()) for k in P.BALL_K2] == [1, 7, 19, 27, 33, 57, 81, 93, 123]
    assert (levels["n_reach"][1:] == 1).all() and (levels["n_face"][1:] == 0).all() and levels["n_face"][0] == 729 - 343
    for q, k in enumerate(P.BALL_K2):
        assert np.array_equal(pw.cavity.unpack_mask(mask[(q + 1) * 81:(q + 2) * 81], 9, 9, 9), d2 <= k), k
    # the shells: what the ball of a level has that the next one up has not
    assert list(levels["n_largest"]) == [729 - 123, 0, 0, 0, 0, 0, 0, 0, 0, 123]
    levels, _, mask = run(host, by_name("ball-6-and-7"))
    assert list(levels["k2"]) == [0, 6, 7] and np.array_equal(mask[81:162], mask[162:]) and levels["n_swept"][1] == 81
    assert list(levels["n_largest"]) == [729 - 81, 0, 81]           # (the larger of two equal levels takes them)


def test_the_corner_distance(host):
    levels, out, mask = run(host, by_name("corner"))
    assert list(levels["k2"]) == [0, 11906, 11907] and out["n_domain"][0] == 64 ** 3
    assert list(levels["n_swept"]) == [64 ** 3, 64 ** 3 - 1, 64 ** 3] and list(levels["n_largest"]) == [0, 0, 64 ** 3]
    assert (mask[2 * 4096:] == P.ALL).all() and mask[2 * 4096 - 1] == P.ALL >> np.uint64(1) and (mask[4096:2 * 4096 - 1] == P.ALL).all()


def test_word_edges_and_bits_beyond_nx(host):
    for nx, bit in ((64, 0), (64, 63), (63, 62), (63, 0), (5, 4), (5, 0), (1, 0)):
        c = by_name(f"word-edge-nx={nx}-bit={bit}")
        levels, out, mask = run(host, c)
        rowmask = P.ALL if nx == 64 else (np.uint64(1) << np.uint64(nx)) - np.uint64(1)
        assert out["n_domain"][0] == 12 * nx and not (mask & ~rowmask).any()
        swept = pw.cavity.unpack_mask(mask[12:24], nx, 4, 3)        # K = 1: the centre, its x neighbours inside the row
        assert swept.sum() == 5 + (bit > 0) + (bit < nx - 1) and swept[1, 1, bit] and not swept[1, 1, nx - 1 - bit] or nx < 3
        swept = pw.cavity.unpack_mask(mask[24:36], nx, 4, 3)        # K = 5: |di| <= 2 in the centre's row
        assert swept[1, 1].sum() == 1 + min(bit, 2) + min(nx - 1 - bit, 2)
        assert levels["n_swept"][3] == 12 * min(nx, 9)               # K = 70: |di| <= 8 in every row (70 - 4 - 1 >= 64)


def test_row_ownership(host):
    for ny, nz in P.ROW_GRIDS:
        for end, (j, l) in (("first", (0, 0)), ("last", (ny - 1, nz - 1))):
            levels, out, mask = run(host, by_name(f"rows={ny}x{nz}-{end}"))
            jj, ll = np.arange(ny)[None, :, None], np.arange(nz)[:, None, None]
            d2 = (np.arange(9)[None, None, :] - 4) ** 2 + (jj - j) ** 2 + (ll - l) ** 2
            assert out["n_domain"][0] == 9 * ny * nz and list(levels["n_swept"][1:]) == [(d2 <= 5).sum(), (d2 <= 27).sum()]
            assert np.array_equal(pw.cavity.unpack_mask(mask[2 * ny * nz:], 9, ny, nz), d2 <= 27)
    for dims in ((64, 1, 1), (1, 64, 1), (1, 1, 64)):
        levels, out, _ = run(host, by_name(f"line-{dims}"))
        assert list(levels["k2"]) == [0, 0, 9, 500, 11907] and list(levels["n_swept"]) == [64, 1, 7, 21 + 1 + 22, 64]   # (the centre is voxel 21)
    levels, out, mask = run(host, by_name("line-(1, 1, 1)"))
    assert list(levels["n_swept"]) == [1] * 5 and list(levels["n_largest"]) == [0, 0, 0, 0, 1] and list(mask) == [1] * 5


def test_the_sweep_is_of_the_cavity(host):
    c = by_name("second-component")
    levels, out, mask = run(host, c)
    assert list(levels["n_reach"]) == [12 * 9 * 7, 1, 1] and list(levels["n_swept"][1:]) == [19, 33]
    swept = pw.cavity.unpack_mask(mask[2 * 63:], 12, 9, 7)
    assert not swept[:, :, 6:].any() and swept[3, 4, 0] and swept[3, 4, 4]     # nothing near (9, 4, 3) or (6, 0, 0)
    for dims in ((8, 8, 8), (64, 5, 3)):
        ok, length, second = C.serpentine(*dims)
        levels, out, mask = run(host, by_name(f"serpentine-{dims}"))
        assert list(levels["k2"]) == [0, 1] and list(levels["n_reach"]) == [length] * 2 == list(levels["n_swept"])
        assert out["n_domain"][0] == length and list(levels["n_largest"]) == [0, length]


def test_attribution_follows_the_largest_level(host):
    levels, out, mask = run(host, by_name("not-nested"))
    rows = 49
    s1, s2 = (pw.cavity.unpack_mask(mask[q * rows:(q + 1) * rows], 11, 7, 7) for q in (1, 2))
    assert (s1 & ~s2).any() and (s2 & ~s1).any() and s1[3, 3, 0] and not s2[3, 3, 0] and s2[4, 4, 5] and not s1[4, 4, 5]
    assert list(levels["n_swept"]) == [539, 11 * 5, 19] and list(levels["n_largest"]) == [539 - 40 - 19, 55 - 15, 19]   # (15 of the ball's 19 are in the tube)
    assert out["n_domain"][0] == 539 == out["n_none"][0] + levels["n_largest"].sum() and out["n_none"][0] == 0
    levels, out, mask = run(host, by_name("closed-between"))
    assert list(levels["flags"]) == [0, 0, _lib.CAV_SEED_CLOSED, 0] and list(levels["k2"]) == [0, 1, 4, 9]
    assert levels[2].tobytes() == np.array((0, 0, 0, 0, 4, 1), dtype=_lib.PORES_LEVEL_DTYPE).tobytes() and not mask[2 * rows:3 * rows].any()
    assert levels["n_reach"][3] == 2 and levels["n_swept"][3] > 123 and levels["n_largest"][3] == levels["n_swept"][3]
    for name in ("no-domain", "no-domain-words"):
        c = by_name(name)
        levels, out, mask = run(host, c)
        assert out.tobytes() == np.array([(0, 0, c.L)], dtype=_lib.PORES_OUT_DTYPE).tobytes() and not mask.any()
        assert levels["flags"][0] == _lib.CAV_SEED_CLOSED and not levels["n_swept"].any() and not levels["n_largest"].any()
        if name == "no-domain":                                      # (a seed inside an atom stays closed: all zeros)
            assert (levels["flags"] == _lib.CAV_SEED_CLOSED).all() and not levels["n_reach"].any() and not levels["n_face"].any()
        else:                                                        # (ready-made levels are each computed: 11 voxels)
            assert list(levels["n_reach"]) == [0, 11] and levels["flags"][1] == 0


def test_the_classification_path_against_pw_cavity(host):
    for name in ("atoms-0", "atoms-1", "atoms-5", "atoms-200", "tie", "ladder-1", "ladder-2", "ladder-63", "ladder-64"):
        c = by_name(name)
        levels, out, mask = run(host, c)
        packed = C.pack([c.level(q) for q in range(c.L)])
        cav, words = host.cavity(*packed[:4])
        assert np.array_equal(levels["n_reach"], cav["n_voxels"]) and np.array_equal(levels["n_face"], cav["n_face"]), name
        assert np.array_equal(levels["flags"], cav["flags"]) and np.array_equal(mask[:len(mask) // c.L], words[:len(words) // c.L])
        assert list(levels["k2"]) == [P.k2_rule(p, c.h) for p in c.probes]
        if name.startswith("atoms"):
            assert (levels["n_reach"] > 0).all() and (np.diff(levels["n_reach"]) <= 0).all()
            assert (levels["n_reach"][4] < levels["n_reach"][0]) == (len(c.xyz) > 0)
    tie = run(host, by_name("tie"))[0]
    g = np.arange(-6, 7)
    inside = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2 < 25).sum()
    assert tie["n_reach"][1] == 13 ** 3 - inside and list(tie["k2"]) == [0, 1]     # (distance 5 exactly is free at probe 1.25)
    for L in (63, 64):
        levels = run(host, by_name(f"ladder-{L}"))[0]
        closed = levels["flags"] == _lib.CAV_SEED_CLOSED
        assert not closed[0] and closed[-5:].all() and (np.diff(closed.astype(int)) >= 0).all() and not levels["n_reach"][closed].any()
        assert (levels["n_reach"][~closed] > 0).all() and len(levels) == L


def test_one_batch_with_holes_masks_for_some_and_the_number_of_threads():
    jobs = P.mixed_batch()
    some = [k % 3 != 1 for k in range(len(jobs))]
    for masks in (True, some, False):
        packed = P.Packed(jobs, hole=2, masks=masks)
        want = packed.expected()
        for threads, budget in ((1, None), (3, 1), (16, 0)):
            rc, got = P.raw(_lib.Context(-1, host_threads=threads), packed, workspace_bytes=budget)
            assert rc == 0 and P.same(got, want), (masks, threads, P.first_difference(got, want))
    untouched = np.frombuffer(got[1].tobytes(), dtype=np.uint8).reshape(len(got[1]), -1)
    assert ((untouched == P.SENTINEL).all(axis=1)).sum() == 2 * len(jobs) and len(got[2]) == 0


def test_jobs_that_share_atoms_planes_and_probes(host):
    c = by_name("atoms-5")
    packed = P.Packed([c, by_name("tie"), c, c])
    assert packed.rec["atom_first"][0] == packed.rec["atom_first"][3] and packed.rec["probe_first"][2] == packed.rec["probe_first"][0]
    rc, got = P.raw(host, packed)
    assert rc == 0 and P.same(got, packed.expected()) and got[0][:5].tobytes() == got[0][-5:].tobytes()


def test_bad_arguments_are_refused_and_nothing_is_written(host):
    batches = P.bad_batches()
    assert len(batches) >= 40
    for packed, sizes, what in batches:
        for budget in (None, 1):
            rc, got = P.raw(host, packed, workspace_bytes=budget, sizes=sizes)
            assert rc == -2 and P.same(got, packed.blank()), what
            message = _lib.load().pw_last_error().decode()
            assert message.startswith("pw_pore_sizes: job 1: ") and what in message, (what, message)
    packed = batches[2][0]
    with pytest.raises(ValueError, match="job 1: the probes are not strictly ascending"):
        host.pore_sizes(packed.rec, packed.xyz, packed.radii, packed.probes, packed.planes)
    words = P.Packed([by_name("not-nested")] * 2)
    words.words = words.words[:-1]
    rc, got = P.raw(host, words)
    assert rc == -2 and "job 1: the open words are outside their array" in _lib.load().pw_last_error().decode()


def test_no_jobs_and_the_wrapper(host):
    assert P.raw(host, P.Packed([]))[0] == 0
    c = by_name("atoms-5")
    packed = P.Packed([c])
    levels, out, mask = host.pore_sizes(packed.rec, packed.xyz, packed.radii, packed.probes, packed.planes)
    want = P.reference_cached(c)
    assert levels.tobytes() == want[0].tobytes() and out[0].tobytes() == want[1].tobytes() and np.array_equal(mask, want[2])
    packed.rec["mask_first"] = -1
    assert host.pore_sizes(packed.rec, packed.xyz, packed.radii, packed.probes, packed.planes)[2] is None


# ---- pywindow_amd.pores ---------------------------------------------------------------------------------------------

SHELL = 2.0 * np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float)


def test_pore_size_distribution_of_a_shell_of_atoms():
    """26 atoms of radius 1.5 on a cube of edge 4 around the origin: a closed void."""
    kw = dict(spacing=0.25, half_width=4.0, device=-1)
    ps = pw.pore_size_distribution(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], masks=True, **kw)
    assert ps.closed and len(ps.probes) == 33 and np.array_equal(ps.probes, 0.125 * np.arange(33))   # 0, h/2, .. half width
    assert np.array_equal(ps.diameter, 2.0 * ps.probes) and np.array_equal(ps.k2, [P.k2_rule(p, 0.25) for p in ps.probes])
    h3 = 0.25 ** 3
    assert np.array_equal(ps.reach_volume, ps.levels["n_reach"] * h3) and np.array_equal(ps.occupiable_volume, ps.levels["n_swept"] * h3)
    assert np.array_equal(ps.histogram, ps.levels["n_largest"] * h3) and ps.occupiable_volume[0] == ps.reach_volume[0] == ps.domain_volume
    assert np.array_equal(ps.cumulative, np.cumsum(ps.histogram[::-1])[::-1]) and (np.diff(ps.cumulative) <= 0).all()
    assert ps.cumulative[0] + ps.raw["n_none"] * h3 == ps.domain_volume and ps.raw["n_none"] == 0
    # the cumulative curve is the occupiable volume wherever the levels are nested, which on a grid they need not be
    assert (ps.cumulative >= ps.occupiable_volume).all() and ps.cumulative[0] == ps.occupiable_volume[0]
    # the void's inscribed sphere: the nearest atoms are the six at distance 2, so radius 0.5 -- to the voxel
    top = int(np.flatnonzero(ps.levels["n_reach"] > 0)[-1])
    assert ps.largest_probe == ps.probes[top] and 0.5 - 0.25 * math.sqrt(3) / 2 <= ps.largest_probe <= 0.5
    assert ps.histogram[top + 1:].sum() == 0 and (ps.levels["flags"][top + 1:] == _lib.CAV_SEED_CLOSED).all()
    width = np.diff(np.append(ps.diameter, 2 * ps.diameter[-1] - ps.diameter[-2]))
    assert np.array_equal(ps.distribution, ps.histogram / width)
    assert 0.0 < ps.mean_diameter <= 2 * ps.largest_probe and ps.diameter[0] <= ps.median_diameter <= 2 * ps.largest_probe
    assert ps.mean_diameter == (ps.histogram * ps.diameter).sum() / ps.histogram.sum()
    assert len(ps.masks) == 33 and ps.masks[0].shape == (32, 32, 32) and [int(m.sum()) for m in ps.masks] == list(ps.levels["n_swept"])
    # level l's reach is pw_cavity's at that probe
    for q in (0, 3, top, top + 1):
        cav = pw.cavity_grid(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], probe=float(ps.probes[q]), **kw)
        assert cav.volume == ps.reach_volume[q] and cav.n_face == ps.levels["n_face"][q]
    # a ladder that does not start at 0: the domain is the reach at its first probe
    two = pw.pore_size_distribution(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], probes=[0.375, 0.75], **kw)
    assert two.domain_volume == ps.reach_volume[3] and two.occupiable_volume[0] == two.domain_volume and two.masks is None
    with pytest.raises(ValueError, match="at most 64"):
        pw.pore_size_distribution(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], probes=np.arange(65.0), **kw)
    with pytest.raises(ValueError, match="strictly ascending"):
        pw.pore_size_distribution(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], probes=[0.5, 0.5], **kw)


def test_series_shapes_and_validity():
    """The shell holds its void in frames 0, 2, 3 and 5 and is blown up until it leaks in frames 1 and 4."""
    scale = np.array([1.0, 1.6, 0.95, 0.9, 1.7, 1.0])
    ps = pw.pore_size_distribution_batch(SHELL[None] * scale[:, None, None], np.full(26, 1.5), np.zeros((6, 3)),
                                         probes=[0.0, 0.25, 0.5, 0.75], spacing=0.25, half_widths=np.full(6, 7.0), device=-1)
    assert ps.levels.shape == (6, 4) and ps.raw.shape == (6,) and ps.reach_volume.shape == ps.cumulative.shape == (6, 4)
    assert np.array_equal(ps.closed, [True, False, True, True, False, True]) and ps.mean_diameter.shape == (6,)
    assert np.array_equal(ps.closed, (ps.levels["n_face"][:, 0] == 0) & (ps.levels["flags"][:, 0] == 0))
    for name in ("occupiable_volume", "reach_volume", "histogram", "cumulative", "distribution"):
        values, valid = ps.series(name, level=2)
        assert values.shape == (6,) and values.dtype == np.float64 and np.array_equal(valid, ps.closed)
        assert np.array_equal(values, getattr(ps, name)[:, 2])
        with pytest.raises(ValueError, match="level"):
            ps.series(name)
    for name in ("mean_diameter", "median_diameter", "largest_probe", "domain_volume"):
        values, valid = ps.series(name)
        assert values.shape == (6,) and np.array_equal(valid, ps.closed) and np.array_equal(values, getattr(ps, name))
    with pytest.raises(KeyError):
        ps.series("colour")
    assert ps.levels[0].tobytes() == ps.levels[5].tobytes() and ps.largest_probe.shape == (6,)
    values, valid = ps.series("occupiable_volume", level=1)
    tc = pw.time_correlation(values, max_lag=2, valid_a=valid, device=-1)
    assert tc.n == 4 and pw.lomb_scargle(values, valid=valid, device=-1) is not None
    assert pw.gate_statistics(values, [float(values[0])], valid=valid, device=-1) is not None
    assert pw.transition_counts(values, [float(values[0])], 1, valid=valid, device=-1) is not None
    assert pw.gaussian_kde_1d(values[valid], np.linspace(0.0, 2.0 * values[0], 5), device=-1) is not None
    one = pw.pore_size_distribution(SHELL, np.full(26, 1.5), [0.0, 0.0, 0.0], probes=[0.0, 0.25, 0.5, 0.75], spacing=0.25,
                                    half_width=7.0, device=-1)
    assert one.levels.tobytes() == ps.levels[0].tobytes() and one.series("histogram", level=0)[0].shape == (1,)


# ---- CC3: Molecule.calculate_pore_size_distribution and DLPOLY.pore_sizes -------------------------------------------

@pytest.fixture(scope="module")
def cc3():
    return synth.load_cc3_base()


def _molecule(cc3):
    return pw.Molecule({"elements": cc3[0], "coordinates": cc3[1]}, "cc3", 0)


def test_cc3_pore_size_distribution(cc3, on_the_host):
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    mol = _molecule(cc3)
    before = dict(_molecule(cc3).full_analysis())
    ps = mol.calculate_pore_size_distribution()
    props = mol.properties["pore_size_distribution"]
    assert ps is mol.pore_sizes and ps.closed and props["closed"] is True and tuple(ps.shape) == (46, 46, 46)
    assert len(ps.probes) == 45 and ps.probes[1] == 0.25 and ps.spacing == 0.5                 # 0, 0.25, .. 11.0
    # the definition, from the same atoms, planes and grid
    planes = window_planes(mol.pore_opt_COM, mol.properties["windows"]["centre_of_mass"])
    case = P.Case("cc3", ps.shape, (22, 22, 22), ps.probes, 0.5, ps.origin, mol.coordinates, VDW[element_ids(mol.elements)], planes)
    want = P.reference(case)
    assert ps.levels.tobytes() == want[0].tobytes() and ps.raw.tobytes() == want[1].tobytes()
    # every level's reach is the cavity of calculate_cavity at that probe, and level 0's occupiable volume too
    for q in range(0, 14):
        assert ps.reach_volume[q] == mol.calculate_cavity(probe=float(ps.probes[q])), q
    assert ps.occupiable_volume[0] == mol.calculate_cavity(probe=0.0) == ps.domain_volume == 143.0
    assert (np.diff(ps.cumulative) <= 0).all() and ps.cumulative[0] + ps.raw["n_none"] * 0.125 == ps.domain_volume
    assert np.array_equal(props["cumulative"], ps.cumulative) and props["largest_probe"] == ps.largest_probe
    # the largest level with a reach against the optimised inscribed sphere: the seed voxel's centre is within half a
    # voxel diagonal of the optimised centre (no probe of this ladder is within 1e-9 of the bound)
    bound = mol.calculate_pore_diameter_opt() / 2.0 - 0.5 * math.sqrt(3.0) / 2.0
    assert (np.abs(ps.probes - bound) > 1e-9).all() and ps.largest_probe >= ps.probes[ps.probes <= bound].max()
    print(f"CC3: largest probe {ps.largest_probe} (bound {bound:.4f}), mean diameter {ps.mean_diameter:.4f}, "
          f"median {ps.median_diameter}, swept voxels {list(ps.levels['n_swept'][:14])}, largest {list(ps.levels['n_largest'][:14])}")
    assert ps.largest_probe == 2.25 and ps.median_diameter == 4.5 and list(ps.levels["n_swept"][:11]) == [
        1144, 930, 951, 1005, 894, 984, 942, 882, 636, 624, 0]       # (not monotone on a grid; the cumulative curve is)
    assert list(ps.levels["n_largest"][:11]) == [79, 0, 0, 69, 0, 54, 60, 222, 36, 624, 0]
    coarse = mol.calculate_pore_size_distribution(probes=[0.0, 1.0, 2.0, 3.0], close=None)
    assert not coarse.closed and len(coarse.probes) == 4 and mol.properties["pore_size_distribution"]["closed"] is False
    again = _molecule(cc3).full_analysis()
    assert "pore_size_distribution" not in again and repr(again) == repr(before)


def test_pore_sizes_of_the_golden_trajectory(tmp_path, cc3, on_the_host):
    """DLPOLY.pore_sizes on the reference's own 20-frame HISTORY file (tests/golden/history20.npz) equals the batch
    function on its frames."""
    from _util import GOLDEN
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    path = tmp_path / "HISTORY_singlemol_short"
    path.write_bytes(np.load(GOLDEN / "history20.npz")["file_bytes"].tobytes())
    traj = pw.DLPOLY(path)
    names = dict(swap_atoms={"he": "H"}, forcefield="opls")
    with pytest.raises(ValueError, match="no frame has been analysed"):
        traj.pore_sizes(**names)
    sel = [0, 1, 7, 19]
    traj.analysis(frames=sel, **names)
    probes = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    ps = traj.pore_sizes(probes=probes, masks=True, **names)
    assert list(ps.frames) == sel and ps.levels.shape == (4, 7) and len(ps.masks) == 4 and len(ps.masks[0]) == 7
    recs = traj.analysis_store.records
    coords = traj._read_selected(sel, False)[0]
    radii = VDW[element_ids(traj.elements(**names))]
    planes = [window_planes(recs["pore_opt_c"][t], engine.windows_of(recs[t])[1]) for t in range(4)]
    batch = pw.pore_size_distribution_batch(coords, radii, recs["pore_opt_c"], probes, 0.5, recs["maxd"] / 2.0, planes, True, -1)
    assert batch.levels.tobytes() == ps.levels.tobytes() and batch.raw.tobytes() == ps.raw.tobytes()
    assert all(np.array_equal(a, b) for x, y in zip(batch.masks, ps.masks) for a, b in zip(x, y))
    cav = traj.cavity(probe=1.0, **names)
    assert np.array_equal(ps.reach_volume[:, 2], cav.volume) and np.array_equal(ps.closed, cav.closed)
    assert (ps.levels["n_reach"][:, 0] > 0).all() and (np.diff(ps.cumulative, axis=1) <= 0).all()
    two = traj.pore_sizes(probes=probes, frames=[19, 1], **names)
    assert list(two.frames) == [19, 1] and two.levels.tobytes() == ps.levels[[3, 1]].tobytes()
    values, valid = ps.series("occupiable_volume", level=3)
    assert values.shape == (4,) and np.array_equal(valid, ps.closed) and len(set(values.tolist())) > 1
    with pytest.raises(ValueError, match="frame 2 has not been analysed"):
        traj.pore_sizes(frames=[2], **names)
    elements, base = cc3
    periodic = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY2", elements, [base, base], cell=np.eye(3) * 40.0))
    with pytest.raises(ValueError, match="pore_sizes: a periodic or modular trajectory is not supported yet"):
        periodic.pore_sizes()
