"""The barrier a guest crosses at every window on the host path: pw_passage on a device = -1 context against the
definition by another algorithm (tests/_passage_cases.py: a bottleneck Dijkstra and breadth-first fills), as BYTES.
numpy only, no GPU; tests/test_gpu_passage.py holds the device to both."""
import numpy as np
import pytest

import _passage_cases as C


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


def by_name(name):
    return [c for c in C.cases() if c.name == name][0]


def test_the_layouts_and_the_symbol():
    from pywindow_amd import _lib

    assert _lib.PASSAGE_JOB_DTYPE.itemsize == 128 and _lib.PASSAGE_OUT_DTYPE.itemsize == 72
    assert hasattr(_lib.load(), "pw_passage") and "pw_passage" in _lib.EXPORTED_SYMBOLS


def test_the_case_list(host):
    """Host path == definition, job by job and as one batch with holes."""
    for c in C.cases():
        rc, got = C.raw(host, C.pack([c]))
        want = C.expected([c])
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    jobs = C.cases()
    packed = C.pack(jobs, hole=3)
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, hole=3)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    rows = np.frombuffer(got.tobytes(), dtype=np.uint8).reshape(len(got), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 3 * len(jobs)


def test_what_the_cases_are_meant_to_show():
    """The definition itself on the hand-made cases: the cases hit what their names say."""
    r = lambda name: C.reference_cached(by_name(name))
    o = r("1x1x1")[0]
    assert o["barrier"] == 3.0 == o["u_seed"] and o["n_basin"] == 0 and o["n_fill"] == 1 and o["flags"] == 0
    o = r("single-ridge")[0]
    assert o["barrier"] == 5.0 and tuple(o["saddle"]) == (2, 1, 1) and o["n_fill"] == 4 and o["n_basin"] == 1
    assert o["well"] == 0.0 and tuple(o["well_voxel"]) == (0, 1, 1)
    assert tuple(r("two-equal-ridges")[0]["saddle"]) == (1, 1, 1)
    o = r("constant")[0]
    assert o["barrier"] == 2.5 and o["n_fill"] == 120 and o["n_basin"] == 0 and tuple(o["saddle"]) == (0, 0, 0)
    for name in ("one-ulp-apart", "one-ulp-apart-mirrored"):
        assert r(name)[0]["barrier"] == 2.5
    assert r("one-ulp-apart")[0]["n_fill"] == 5
    assert r("sign-change-negative-B")[0]["barrier"] == -0.5 and r("sign-change-positive-B")[0]["barrier"] == 1e-3
    assert np.signbit(r("zeros-minus-first")[0]["barrier"]) and not np.signbit(r("zeros-plus-first")[0]["barrier"])
    assert r("zeros-minus-first")[0]["n_fill"] == 5
    assert np.signbit(r("zero-wells-minus-first")[0]["well"]) and not np.signbit(r("zero-wells-plus-first")[0]["well"])
    assert r("denormals")[0]["barrier"] == 5e-324 and r("1e300")[0]["barrier"] == 1e299
    o = r("B-is-the-seed")[0]
    assert o["barrier"] == 5.0 == o["u_seed"] and o["n_basin"] == 0
    assert r("B-is-the-largest")[0]["barrier"] == 7.0
    assert r("nearer-exit-higher")[0]["barrier"] == 2.0 and tuple(r("nearer-exit-higher")[0]["saddle"]) == (6, 1, 1)
    assert tuple(r("well-ties")[0]["well_voxel"]) == (1, 1, 1)
    o = r("seed-blocked")[0]
    assert o["flags"] == C.SEED_CLOSED and o["u_seed"] == np.inf == o["barrier"] and o["n_fill"] == 0
    for name in ("closed-shell", "shell-of-98-atoms"):
        o = r(name)[0]
        assert o["flags"] == C.NO_EXIT and o["n_fill"] == 27 == o["n_basin"] and o["barrier"] == np.inf and np.isfinite(o["well"])
    o = r("m=4-low-exit-cut")
    assert o["barrier"][0] == 2.0 and o["barrier"][1] == 5.0 and (o["flags"][2:] == C.NO_EXIT).all()
    o = r("seed-outside-a-plane")
    assert o["flags"][0] == 0 and o["flags"][1] == C.SEED_CLOSED and np.isfinite(o["u_seed"][1])
    o = r("voxel-on-a-plane")
    assert o["flags"][0] == 0 and o["barrier"][0] == 4.0 and tuple(o["saddle"][0]) == (6, 1, 1) and o["barrier"][1] == 4.0
    assert len(r("m=65")) == 65 and len({o.tobytes() for o in r("m=65")}) > 2
    assert len({o.tobytes() for o in r("planes-off-axis")}) == 3
    closed = [c.name for c in C.lj_cases() if (C.reference_cached(c)["flags"] & C.SEED_CLOSED).all()]
    assert closed == []
    U = C.field_of(by_name("ties"))[0, 0]
    assert np.isinf(U[1:4]).all() and np.isfinite(U[0]) and U[5] != 0.0 and U[6] == 0.0
    o = r("ties")[0]
    assert o["u_seed"] == U[5] == o["barrier"] and o["n_fill"] == 2 and o["well"] == U[4] < U[5] < 0.0


def test_lennard_jones_jobs_equal_the_jobs_given_the_map_of_pw_affinity(host):
    for c in C.lj_cases():
        packed = C.pack([c], fields=[C.affinity_map(host, c)])
        assert packed[0]["field_first"][0] == 0
        rc, got = C.raw(host, packed)
        want = C.raw(host, C.pack([c]))[1]
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))


def test_one_64_cubed_grid(host):
    c = C.big_cases()[0]
    rc, got = C.raw(host, C.pack([c]))
    want = C.expected([c])
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    assert (got["flags"] == 0).all() and got["n_fill"].min() > 1000


def test_a_batch_of_64_mixed_jobs_at_1_3_and_16_threads():
    from pywindow_amd import _lib

    jobs = C.mixed_batch()
    assert len(jobs) == 64 and len({c.dims for c in jobs}) > 10 and {0, 5} <= {len(c.planes) for c in jobs}
    packed = C.pack(jobs, hole=1)
    want = C.expected(jobs, hole=1)
    assert len(packed[1]) < sum(len(c.xyz) for c in jobs) and len(packed[3]) < sum(len(c.planes) for c in jobs)
    for threads in (1, 3, 16):
        rc, got = C.raw(_lib.Context(-1, host_threads=threads), packed)
        assert rc == 0 and C.same(got, want), (threads, C.first_difference(got, want))


def test_bad_arguments_write_nothing(host):
    from pywindow_amd import _lib

    batches = C.bad_batches()
    assert len(batches) > 50
    for packed, sizes, what in batches:
        rc, got = C.raw(host, packed, sizes=sizes)
        assert rc == -2 and C.same(got, C.blank(packed[5])), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_passage: job 1: ") and what in message, (what, message)


def test_the_python_layer_on_the_host_path():
    """passage_field, guest_passage and Passage's derived quantities, device = -1."""
    import pywindow_amd as pw

    c = by_name("m=4-low-exit-cut")
    p = pw.passage_field(c.field, c.seed, c.planes, device=-1)
    assert p.raw.tobytes() == C.reference_cached(c).tobytes() and p.n_windows == 4
    assert p.activation[0] == 2.0 and p.activation[1] == 5.0 and p.no_exit.tolist() == [False, False, True, True]
    assert p.free_exit.tolist() == [False, False, False, False]
    assert np.array_equal(p.saddle_position[1], [5.0, 1.0, 1.0]) and np.isnan(p.saddle_position[2]).all()
    values, valid = p.series("activation")
    assert values.tolist() == [2.0] and valid.tolist() == [True]
    assert p.series("barrier", window=1)[0].tolist() == [5.0] and p.series("barrier", window=2)[1].tolist() == [False]
    assert p.transmission(300.0)[2] == 0.0 and 0.0 < p.transmission(300.0)[1] < p.transmission(300.0)[0] < 1.0
    assert pw.passage_field(by_name("B-is-the-largest").field, (1, 1, 1), device=-1).free_exit.tolist() == [True]
    lj = by_name("n=128")
    one = pw.guest_passage(lj.xyz, lj.coef, None, [3.2, 2.4, 1.6], lj.planes, spacing=0.8, half_width=2.0, device=-1)
    two = pw.guest_passage_batch(np.stack([lj.xyz, lj.xyz + 0.01]), lj.coef, None, [[3.2, 2.4, 1.6]] * 2, [lj.planes, None],
                                 spacing=0.8, half_widths=[2.0, 2.0], device=-1)
    assert one.raw.shape == (2,) and two.raw.shape == (2, 2) and two.raw[0].tobytes() == one.raw.tobytes()
    assert two.n_windows.tolist() == [2, 0] and np.isnan(two.barrier[1, 1]) and two.n_basin[1, 1] == -1
    assert two.padding.tolist() == [[False, False], [False, True]] and two.series("well")[0].shape == (2,)
