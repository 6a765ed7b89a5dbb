"""pw_math.hpp at its edges, on the host path (device = -1, the library's own build of the header): the sets of
tests/_math_cases.py -- every threshold of the range reductions, every table entry, the wrappers' fall-backs --
against independent references: the C library (math.sin / cos / pow), numpy's arccos, log10, sqrt and division.
Exact where the reference is the one the header restates (glibc 2.35; AVX-512 numpy for arccos), one ulp elsewhere;
sqrt and division exact everywhere.  tests/test_gpu_math.py holds gfx950 to this host path bit for bit."""
import math
import platform

import numpy as np
import pytest

import _math_cases as M

GLIBC_235 = platform.libc_ver() == ("glibc", "2.35")


def _svml_arccos() -> bool:
    from numpy._core._multiarray_umath import __cpu_features__ as feats

    return bool(feats.get("AVX512_SKX"))


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1)


@pytest.fixture(scope="module")
def sets():
    return M.sets()


def ulps(got, ref) -> np.ndarray:
    """|got - ref| in units of ref's last place; 0 where the two are the same value (infinities included) or both NaN."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got - ref) / np.spacing(np.abs(ref))
    d = np.where(same, 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


def same_bits_or_nan(got, ref) -> np.ndarray:
    return (M.bits(got) == M.bits(ref)) | (np.isnan(got) & np.isnan(ref))


def check(name, x, got, ref, exact: bool):
    """<= 1 ulp always, the same value where `exact`; the message names the first offending argument."""
    d = ulps(got, ref)
    bad = d > 1.0
    if exact:
        bad |= ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {len(x)} arguments differ from the reference (exact={exact}); first: "
                             f"x = {float(x[k]).hex()} got {float(got[k]).hex()} want {float(ref[k]).hex()}")


def c_pow(x: float, y: float) -> float:
    try:
        return math.pow(x, y)
    except OverflowError:               # (the C library returns the infinity; Python raises on its ERANGE)
        return -math.inf if x < 0 and y % 2 == 1 else math.inf


def test_the_sets_cover_what_they_claim(sets):
    M.coverage(sets)                        # (sets() has asserted it already: here it is a test of its own)
    assert sum(len(x) for _, x, _ in sets.values()) < 2_000_000


@pytest.mark.parametrize("name", ["sin", "cos"])
def test_sin_cos_equal_the_c_library(host, sets, name):
    which, x, _ = sets[name]
    got = M.internal_math(host, which, x)
    f = math.sin if which == M.SIN else math.cos
    ref = np.array([f(v) for v in x.tolist()])
    check(M.NAMES[which], x, got, ref, GLIBC_235)
    assert np.array_equal(np.signbit(got), np.signbit(ref))       # (-0.0 == 0.0: the sign of a zero is compared here)


@pytest.mark.parametrize("name", ["pow-2", "pow-3", "pow-0.5"])
def test_pow_equals_the_c_library(host, sets, name):
    which, x, y = sets[name]
    got = M.internal_math(host, which, x, y)
    # pw_math.hpp above pw_pow_np: "x positive and normal, the result normal with room to spare:
    # 2^-1020 <= x^y < 2^1020 ... otherwise the caller's plain expression is used" -- outside it nothing is promised
    # (the wrappers below are what the path calls, and they are held to the C library everywhere)
    inside = M.pow_in_domain(x, float(y[0]))
    assert inside.sum() > len(x) // 2          # (40 exponent fields up to the wrappers' limit: the lowest underflow)
    xi, gi = x[inside], got[inside]
    ref = np.array([c_pow(v, float(y[0])) for v in xi.tolist()])
    check(f"pw_pow_np(x, {y[0]:g})", xi, gi, ref, GLIBC_235)
    if GLIBC_235:                             # numpy's scalar ** is the same function
        step = max(1, len(xi) // 2000)
        assert all(np.float64(v) ** np.float64(y[0]) == g for v, g in zip(xi[::step], gi[::step]))


@pytest.mark.parametrize("name", ["square", "cube"])
def test_square_and_cube_wrappers(host, sets, name, capsys):
    which, x, _ = sets[name]
    y = 2.0 if which == M.SQUARE else 3.0
    got = M.internal_math(host, which, x)
    main = M.wrapper_main_path(which, x)
    assert main.sum() > 20000 and (~main).sum() > 100
    ref = np.array([c_pow(v, y) for v in x.tolist()])
    # main path: pow's bits (with the sign of an odd power)
    check(f"{M.NAMES[which]} (pow path)", x[main], got[main], ref[main], GLIBC_235)
    # fall-back: the plain product is what the header promises, bit for bit ...
    with np.errstate(over="ignore", under="ignore"):
        product = x * x if which == M.SQUARE else x * x * x
    fb, gf, rf = x[~main], got[~main], ref[~main]
    assert same_bits_or_nan(gf, product[~main]).all()
    # ... and it may differ from pow in the last bit
    differing = int((gf != rf).sum())
    with capsys.disabled():
        print(f"\n{M.NAMES[which]}: {differing} of {len(fb)} fall-back arguments differ from pow(x, {y:g}) in the last bit")
    check(f"{M.NAMES[which]} (fall-back)", fb, gf, rf, False)


def test_arccos_equals_numpy(host, sets):
    which, x, _ = sets["acos"]
    got = M.internal_math(host, which, x)
    with np.errstate(invalid="ignore"):
        ref = np.arccos(x)
    check(M.NAMES[which], x, got, ref, _svml_arccos())
    beyond = np.abs(x) > 1.0
    assert beyond.sum() == 2 and np.isnan(ref[beyond]).all() and np.isnan(got[beyond]).all()
    assert not np.isnan(got[~beyond]).any()


def test_log10_floors_as_numpy(host, sets):
    which, x, _ = sets["log10"]
    got = M.internal_math(host, which, x)
    ref = np.log10(x)
    bad = np.floor(got * 250) != np.floor(ref * 250)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"pw_log10: floor(lg * 250) differs for {int(bad.sum())} of {len(x)} arguments; first: x = {float(x[k]).hex()}"
                             f" got {float(got[k]).hex()} numpy {float(ref[k]).hex()}")
    k, tens, exact = M.powers_of_ten()
    lg = M.internal_math(host, which, tens[exact])
    assert np.array_equal(lg, k[exact].astype(np.float64)), (lg, k[exact])
    check(M.NAMES[which], x, got, ref, False)


def test_sqrt_and_division_are_exact(host, sets):
    which, x, _ = sets["sqrt"]
    got = M.internal_math(host, which, x)
    with np.errstate(invalid="ignore"):
        assert same_bits_or_nan(got, np.sqrt(x)).all()
    sub = x[(x > 0) & (x < M.SMALLEST_NORMAL)]
    assert len(sub) >= 4096
    which, a, b = sets["div"]
    got = M.internal_math(host, which, a, b)
    with np.errstate(all="ignore"):
        ref = a / b
    assert same_bits_or_nan(got, ref).all()
    tiny = np.abs(ref) < M.SMALLEST_NORMAL
    assert (tiny & (ref != 0)).sum() >= 2048                      # subnormal quotients are in the set
    assert ((np.abs(a) < M.SMALLEST_NORMAL) & (a != 0)).sum() >= 2048 and (np.abs(b) < M.SMALLEST_NORMAL).sum() >= 2048


def test_arguments_are_checked(host):
    x = np.ones(4)
    out = np.full(4, -77.0)
    assert M.internal_math_rc(host, M.SIN, None, None, 0, None) == 0
    for rc in (M.internal_math_rc(host, M.SIN, None, None, 4, out), M.internal_math_rc(host, M.SIN, x, None, 4, None),
               M.internal_math_rc(host, M.POW, x, None, 4, out), M.internal_math_rc(host, M.DIV, x, None, 4, out),
               M.internal_math_rc(host, 9, x, x, 4, out), M.internal_math_rc(host, -1, x, x, 4, out),
               M.internal_math_rc(host, M.SIN, x, None, -1, out)):
        assert rc == M.PW_E_BAD_ARG
    assert (out == -77.0).all()
