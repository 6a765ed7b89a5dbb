"""Arguments of the elementary functions of csrc/pw_math.hpp, shared by tests/test_math_edges.py (host path against
the C library and numpy) and tests/test_gpu_math.py (gfx950 against the host path, bit for bit): every threshold of the
range reductions, every entry of every table, the fall-backs of the wrappers.  numpy only, fixed seeds.

Thresholds and table geometry are read from the sources; where a figure is restated, a comment names its line.  The
builder asserts by itself (coverage()) that the sets reach what they claim: the indices are recomputed here, in numpy,
as the source defines them -- nothing of the code under test is involved."""
import decimal
import functools
import re

import numpy as np

from _util import ROOT

CSRC = ROOT / "pywindow_amd" / "csrc"

# pw_math.hpp: `enum { PW_MATH_SIN = 0, ... }`
SIN, COS, POW, SQUARE, CUBE, ACOS, LOG10, SQRT, DIV = range(9)
NAMES = ("pw_sin_np", "pw_cos_np", "pw_pow_np", "pw_square_np", "pw_cube_np", "pw_acos_np", "pw_log10", "pw_sqrt", "x / y")

U = np.uint64
SIGN = U(0x8000000000000000)


@functools.lru_cache(maxsize=None)
def _text(name: str) -> str:
    return (CSRC / name).read_text()


def _function(name: str) -> str:
    """The body of `name` in pw_math.hpp (up to the closing brace in column 0)."""
    m = re.search(rf"inline \w+ {name}\(.*?\n}}\n", _text("pw_math.hpp"), re.S)
    assert m, name
    return m.group(0)


def source_double(name: str, file: str = "pw_sincos_data.hpp") -> float:
    m = re.search(rf"constexpr double {name} = (-?[0-9a-fx.p+-]+);", _text(file))
    assert m, name
    s = m.group(1)
    return float.fromhex(s) if "x" in s else float(s)


def _enum_matches() -> bool:
    m = re.search(r"enum \{\s*(PW_MATH_SIN.*?)\};", _text("pw_math.hpp"), re.S)
    got = {k.strip(): int(v) for k, v in (kv.split("=") for kv in m.group(1).replace("\n", " ").split(",") if "=" in kv)}
    want = dict(PW_MATH_SIN=SIN, PW_MATH_COS=COS, PW_MATH_POW=POW, PW_MATH_SQUARE=SQUARE, PW_MATH_CUBE=CUBE,
                PW_MATH_ACOS=ACOS, PW_MATH_LOG10=LOG10, PW_MATH_SQRT=SQRT, PW_MATH_DIV=DIV, PW_MATH_COUNT=9)
    return got == want


assert _enum_matches()

# ---- geometry read from the sources ------------------------------------------------------------------------------
SC_TAYLOR_MAX = source_double("SC_TAYLOR_MAX")
SC_BIG = source_double("SC_BIG")
SC_HP0 = source_double("SC_HP0")
SC_HPINV = source_double("SC_HPINV")
SC_MP1, SC_MP2, SC_PP3 = source_double("SC_MP1"), source_double("SC_MP2"), source_double("SC_PP3")
SC_ENTRIES = int(re.search(r"SC_TAB\[(\d+)\]", _text("pw_sincos_data.hpp")).group(1)) // 4
#: high-word thresholds of pw_sin_np and pw_cos_np (`if (k < 0x...u)`), ascending
SIN_HI = sorted(int(h, 16) for h in re.findall(r"k < 0x([0-9a-f]+)u", _function("pw_sin_np")))
COS_HI = sorted(int(h, 16) for h in re.findall(r"k < 0x([0-9a-f]+)u", _function("pw_cos_np")))
assert len(SIN_HI) == 3 and len(COS_HI) == 3 and SIN_HI[1:] == COS_HI[1:]
#: "Arguments beyond 1.05e8 never occur on the path" (pw_math.hpp, the comment above sc_copysign); pw_math_probe's guard
SC_LIMIT = float(re.search(r"pw_abs\(x\) <= ([0-9.e]+)\)", _function("pw_math_probe")).group(1))
assert SC_LIMIT == 1.05e8
GOLDEN_ANGLE = source_double("GOLDEN_ANGLE", "pw_unit.hpp")
#: PW_NB_PMAX = PW_P_MAX (pw_unit.hpp), the largest sampling-sphere point count the engine tabulates
assert re.search(r"constexpr int PW_NB_PMAX = PW_P_MAX;", _text("pw_unit.hpp"))
PW_NB_PMAX = int(re.search(r"#define PW_P_MAX (\d+)", (ROOT / "include" / "pywindow_amd.h").read_text()).group(1))

_pow = _function("pw_pow_np")
POW_OFF = int(re.search(r"ix - 0x([0-9a-f]+)ull;", _pow).group(1), 16)
_m = re.search(r"\(tmp >> (\d+)\) & 0x([0-9a-f]+)\)", _pow)
POW_I_SHIFT, POW_I_MASK = int(_m.group(1)), int(_m.group(2), 16)
POW_KI_MASK = int(re.search(r"\(ki & 0x([0-9a-f]+)\)", _pow).group(1), 16)
POW_LOG_ENTRIES = int(re.search(r"POW_LOG_TAB\[(\d+)\]", _text("pw_pow_data.hpp")).group(1)) // 4
POW_EXP_ENTRIES = int(re.search(r"POW_EXP_TAB\[(\d+)\]", _text("pw_pow_data.hpp")).group(1)) // 2
assert POW_I_MASK + 1 == POW_LOG_ENTRIES == 128 and POW_KI_MASK + 1 == POW_EXP_ENTRIES == 128


def _wrapper_bounds(name: str):
    m = re.search(r"a >= ([0-9a-fx.p+-]+) && a < ([0-9.e+-]+)\)", _function(name))
    assert m, name
    lo = m.group(1)
    return (float.fromhex(lo) if "x" in lo else float(lo)), float(m.group(2))


#: pw_square_np / pw_cube_np take pw_pow_np for lo <= |x| < hi and the plain product elsewhere
SQUARE_LO, SQUARE_HI = _wrapper_bounds("pw_square_np")
CUBE_LO, CUBE_HI = _wrapper_bounds("pw_cube_np")
assert (SQUARE_HI, CUBE_HI) == (1e150, 1e100)
SMALLEST_NORMAL = 2.2250738585072014e-308
LARGEST = 1.7976931348623157e308
#: pw_pow_np's domain (pw_math.hpp, the comment above it): x positive and normal, 2^-1020 <= x^y < 2^1023
POW_RESULT_LOG2 = 1020.0

#: sqrt(2) rounded up: where a logarithm that normalises the significand to [sqrt(1/2), sqrt(2)) switches exponents (the
#: fdlibm-style kernel pw_log10 was built on did; today's switches at pw_pow_np's POW_OFF, see log10_arguments)
LOG_SWITCH = 1.4142135623730951
assert "0x%xull" % POW_OFF in _function("pw_log10") and "POW_LOG_TAB[4 * i]" in _function("pw_log10")
_m = re.search(r"\(h - 0x([0-9a-f]+)u\) <= 0x([0-9a-f]+)u", _text("pw_common.hpp"))
#: pw_plain_exponent: biased exponents PLAIN_LO .. PLAIN_HI
PLAIN_LO = int(_m.group(1), 16) >> 20
PLAIN_HI = PLAIN_LO + (int(_m.group(2), 16) >> 20)
PW_E_BAD_ARG = int(re.search(r"#define PW_E_BAD_ARG \((-?\d+)\)", (ROOT / "include" / "pywindow_amd.h").read_text()).group(1))
RSQ_ENTRIES = 65536              # pw_math.hpp: rsqrt14_decode, "65536 entries"
assert "tab[p * 32768 + (int)((u >> 37) & 0x7fff)]" in _function("pw_rsqrt14")


# ---- bit helpers ---------------------------------------------------------------------------------------------------
def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(U)


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=U).view(np.float64)


def around(x, k: int) -> np.ndarray:
    """x and its k neighbours on each side in magnitude (positive, finite, away from zero by more than k ulp): the
    doubles whose bit patterns are bits(|x|) - k .. bits(|x|) + k, with x's sign."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    b = bits(np.abs(x)).astype(np.int64)
    assert (b > k).all() and (b + k < 0x7ff0000000000000).all()
    out = (b[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).astype(U)
    return (from_bits(out) * np.sign(x)[:, None]).ravel()


def both_signs(x) -> np.ndarray:
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return np.concatenate([x, -x])


def cat(*parts) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in parts]))


# pi to 70 decimals, as an integer scaled by 2^240 (exact integer arithmetic: the nearest double to n pi/2)
_PI = decimal.Decimal("3.1415926535897932384626433832795028841971693993751058209749445923078164")
_PI_SCALE = 240
with decimal.localcontext() as _c:
    _c.prec = 120
    _PI_INT = int(_PI * (1 << _PI_SCALE))


def multiple_of_half_pi(n: int) -> float:
    return (n * _PI_INT) / (1 << (_PI_SCALE + 1))      # int / int: correctly rounded


# ---- sin / cos -------------------------------------------------------------------------------------------------------
def sincos_arguments() -> np.ndarray:
    rng = np.random.default_rng(20261)
    hi = sorted(set(SIN_HI + COS_HI))
    assert hi == [0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd]      # pw_math.hpp: pw_sin_np, pw_cos_np
    thresholds = from_bits(np.array([h << 32 for h in hi], dtype=U))
    parts = [both_signs(around(thresholds, 16)), both_signs(around(SC_TAYLOR_MAX, 16))]
    # steps of the table index k = low word of (SC_BIG + |x|): |x| = (2 j + 1) / 256, j = 0 .. SC_ENTRIES - 1
    steps = (2.0 * np.arange(SC_ENTRIES) + 1.0) / 256.0
    parts.append(both_signs(around(steps, 4)))
    # multiples of pi/2
    n_max = int(SC_LIMIT / (np.pi / 2))
    while multiple_of_half_pi(n_max) >= SC_LIMIT:
        n_max -= 1
    ns = set(range(1, 2049))
    m = 0
    while (1 << m) - 1 <= n_max:
        ns.update(v for v in ((1 << m) - 1, 1 << m, (1 << m) + 1) if 1 <= v <= n_max)
        m += 1
    ns.add(n_max)
    half_pi = np.array([multiple_of_half_pi(n) for n in sorted(ns)])
    half_pi = around(half_pi, 3)
    parts.append(both_signs(half_pi[np.abs(half_pi) < SC_LIMIT]))
    parts.append(GOLDEN_ANGLE * np.arange(PW_NB_PMAX + 1, dtype=np.float64))      # pw_unit.hpp: Sphere::point
    parts.append(rng.uniform(-2.5 * np.pi, 2.5 * np.pi, 20000))
    # the ranges of tests/test_math.py
    sign = lambda n: rng.choice([-1.0, 1.0], n)
    parts += [rng.uniform(-0.126, 0.126, 20000), rng.uniform(-0.8555, 0.8555, 20000), rng.uniform(0.85, 2.43, 20000) * sign(20000),
              rng.uniform(2.4, 7, 20000) * sign(20000), rng.uniform(7, 3000, 20000), rng.uniform(3000, 1.05e8, 20000),
              rng.uniform(-1e-7, 1e-7, 20000),
              (np.arange(1, 2001) * np.pi / 2)[:, None].repeat(10, 1).ravel() + rng.normal(0, 1e-9, 20000)]
    parts.append(both_signs([0.0, 5e-324, 2.2e-308, 1e-300]))
    x = cat(*parts)
    assert (np.abs(x) < SC_LIMIT).all()
    return x


def _sc_index(ax) -> np.ndarray:
    """k of sc_do_sin / sc_do_cos: the low word of SC_BIG + |x|."""
    return (bits(SC_BIG + ax) & U(0xffffffff)).astype(np.int64)


def _sc_reduce(x):
    """(n mod 4, a) of sc_reduce in plain doubles: x n MP1 and x n MP2 are exact products, so a is good to ~1e-16 --
    enough to count arguments per branch, not to decide an argument that sits on a step."""
    xn = np.rint(x * SC_HPINV)
    a = ((x - xn * SC_MP1) - xn * SC_MP2) - xn * SC_PP3
    return xn.astype(np.int64) & 3, a


def sincos_paths(which: int, x):
    """(branch label of every argument, table entries read with an exactly known index)."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    hw = ((bits(x) >> U(32)) & U(0x7fffffff)).astype(np.int64)
    t0, t1, t2 = SIN_HI if which == SIN else COS_HI
    label = np.empty(len(x), dtype=object)
    entries = set()
    tiny = hw < t0
    label[tiny] = "tiny"
    direct = ~tiny & (hw < t1)
    if which == SIN:
        taylor = direct & (ax < SC_TAYLOR_MAX)
        label[taylor] = "direct-taylor"
        label[direct & ~taylor] = "direct-table"
        entries.update(_sc_index(ax[direct & ~taylor]).tolist())
    else:
        label[direct] = "direct-table"
        entries.update(_sc_index(ax[direct]).tolist())
    mid = ~tiny & ~direct & (hw < t2)
    t = SC_HP0 - ax[mid]
    if which == SIN:                                   # sc_do_cos(t, SC_HP1): k from |t| alone
        label[mid] = "mid-table"
        entries.update(_sc_index(np.abs(t)).tolist())
    else:                                              # sc_do_sin(t + SC_HP1, ...)
        small = np.abs(t) < SC_TAYLOR_MAX
        lab = np.where(small, "mid-taylor", "mid-table")
        label[mid] = lab
    red = ~tiny & ~direct & ~mid
    n, a = _sc_reduce(x[red])
    if which == COS:
        n = (n + 1) & 3
    sub = np.where(n & 1, "cos", np.where(np.abs(a) < SC_TAYLOR_MAX, "sin-taylor", "sin-table"))
    label[red] = np.array([f"reduced-{q}-{s}" for q, s in zip(n.tolist(), sub.tolist())], dtype=object)
    return label, entries


# ---- pow and its wrappers --------------------------------------------------------------------------------------------
def _exponent_fields(hi: float, count: int = 40) -> np.ndarray:
    """`count` biased exponents from the smallest normal's (1) to that of `hi`, both included."""
    top = int(bits(hi)[0] >> U(52))
    e = np.unique(np.round(np.linspace(1, top, count)).astype(np.int64))
    assert len(e) == count and e[0] == 1 and e[-1] == top
    return e


def pow_boundaries(hi: float) -> np.ndarray:
    """For 40 exponent fields up to hi's: the 128 arguments at which i = ((ix - POW_OFF) >> 45) & 0x7f steps, +-2 ulp."""
    step = 1 << POW_I_SHIFT
    out = []
    for e in _exponent_fields(hi):
        lo = int(e) << 52
        first = lo + ((POW_OFF - lo) % step)
        b = first + step * np.arange(POW_LOG_ENTRIES, dtype=np.int64)
        assert b[-1] < lo + (1 << 52)
        out.append(around(from_bits(b.astype(U)), 2))
    x = cat(*out)
    return x[(x >= SMALLEST_NORMAL) & (x < hi)]


def pow_exp_arguments(y: float, hi: float) -> np.ndarray:
    """Arguments with 128 y log2(x) an integer t (to ~1e-13), t mod 128 taking every value, around 40 exponents: ki of
    pw_pow_np is Shift + the nearest integer to that product, so ki & 0x7f takes each of its values."""
    e = _exponent_fields(hi).astype(np.float64) - 1023.0
    t = np.round(e[:, None] * 128.0 * y) + np.arange(POW_EXP_ENTRIES, dtype=np.float64)[None, :]
    x = np.exp2(t.ravel() / (128.0 * y))
    return x[(x >= SMALLEST_NORMAL) & (x < hi)]


def pow_ki(x, y: float) -> np.ndarray:
    """ki & 0x7f as numpy sees it: the nearest integer to 128 y log2(x) -- exact for the arguments built on an
    integer, where the product is ~1e-13 from it."""
    return np.rint(128.0 * y * np.log2(x)).astype(np.int64) & POW_KI_MASK


def pow_i(x) -> np.ndarray:
    return (((bits(x) - U(POW_OFF)) >> U(POW_I_SHIFT)) & U(POW_I_MASK)).astype(np.int64)


def pow_arguments(y: float) -> np.ndarray:
    """x of pw_pow_np(x, y): positive and normal."""
    rng = np.random.default_rng(20262 + int(y * 2))
    hi = CUBE_HI if y == 3.0 else SQUARE_HI
    return cat(pow_boundaries(hi), pow_exp_arguments(y, hi), 10.0 ** rng.uniform(-3, 4, 20000))


def pow_in_domain(x, y: float) -> np.ndarray:
    """pw_math.hpp, above pw_pow_np: "x positive and normal, the result normal with room to spare:
    2^-1020 <= x^y < 2^1020"."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x >= SMALLEST_NORMAL) & (x <= LARGEST) & (np.abs(y * np.log2(x)) < POW_RESULT_LOG2)


def wrapper_arguments(which: int) -> np.ndarray:
    lo, hi = (SQUARE_LO, SQUARE_HI) if which == SQUARE else (CUBE_LO, CUBE_HI)
    y = 2.0 if which == SQUARE else 3.0
    rng = np.random.default_rng(20263 + which)
    subnormal = from_bits(rng.integers(1, 1 << 52, 64, dtype=np.uint64))
    edges = cat(0.0, 5e-324, subnormal, from_bits(np.array([(1 << 52) - 1], dtype=U)), around(SMALLEST_NORMAL, 1),
                around([1e150, 1e100], 2), around(lo, 2), LARGEST)
    body = cat(pow_boundaries(hi), pow_exp_arguments(y, hi), 10.0 ** rng.uniform(-3, 4, 20000))
    # the stretch between the smallest normal and the wrapper's lower bound, where the product replaces pow
    low = 10.0 ** rng.uniform(np.log10(SMALLEST_NORMAL), np.log10(lo), 2000)
    return both_signs(cat(edges, body, low))


def wrapper_main_path(which: int, x) -> np.ndarray:
    lo, hi = (SQUARE_LO, SQUARE_HI) if which == SQUARE else (CUBE_LO, CUBE_HI)
    a = np.abs(np.asarray(x, dtype=np.float64))
    return (a >= lo) & (a < hi)


# ---- arccos ----------------------------------------------------------------------------------------------------------
def rsq_index(x) -> np.ndarray:
    """Entry of the reciprocal-square-root table pw_acos_np reads for x (pw_rsqrt14 of y = (1 - |x|) / 2; the product
    by a half is exact, so the fused form rounds as this one does)."""
    y = 0.5 - 0.5 * np.abs(np.asarray(x, dtype=np.float64))
    u = bits(y)
    p = (u >> U(52)) & U(1)
    return (p * U(32768) + ((u >> U(37)) & U(0x7fff))).astype(np.int64)


def acos_table_arguments() -> np.ndarray:
    """x = +-(1 - 2 y), y over [1/16, 1/4) at every value of the top 15 mantissa bits: one per table entry, each on the
    2 asin(sqrt(y)) branch (x^2 > y), which is the one that uses the estimate."""
    m = np.arange(32768, dtype=np.float64) / 32768.0
    y = np.concatenate([(1.0 + m) / 16.0, (1.0 + m) / 8.0])
    x = 1.0 - 2.0 * y
    assert np.array_equal(0.5 - 0.5 * x, y) and (x * x > y).all()
    sign = np.where(np.arange(len(x)) % 2 == 0, 1.0, -1.0)
    return x * sign


def acos_arguments() -> np.ndarray:
    rng = np.random.default_rng(20264)
    below_one = np.nextafter(1.0, 0.0)
    return cat(acos_table_arguments(), both_signs(around(0.5, 8)), both_signs([1.0, below_one, 0.0]), 1e-300,
               1.0 - 10.0 ** -np.arange(1, 17, dtype=np.float64), rng.uniform(-1, 1, 50000), both_signs(np.nextafter(1.0, 2.0)))


# ---- log10 -----------------------------------------------------------------------------------------------------------
def powers_of_ten():
    """(k, nearest double to 10^k, exactly representable?) for k = -300 .. 300."""
    k = np.arange(-300, 301)
    v = np.array([float(f"1e{int(q)}") for q in k])
    exact = np.array([0 <= int(q) <= 22 for q in k])        # 5^22 < 2^53 < 5^23
    return k, v, exact


def log10_steps() -> np.ndarray:
    """Nearest doubles to 10^(m / 250), m = 400 .. 1300."""
    with decimal.localcontext() as c:
        c.prec = 60
        return np.array([float(decimal.Decimal(10) ** (decimal.Decimal(m) / 250)) for m in range(400, 1301)])


def log10_arguments() -> np.ndarray:
    rng = np.random.default_rng(20265)
    _, tens, _ = powers_of_ten()
    e = np.round(np.linspace(-1000, 1000, 40)).astype(np.int64)
    switch = np.ldexp(around(LOG_SWITCH, 4)[None, :], e[:, None]).ravel()
    # (pow_boundaries: the steps of pw_log10's own table index, which is pw_pow_np's i)
    return cat(around(tens, 2), switch, around(log10_steps(), 2), 10.0 ** rng.uniform(-300, 300, 20000),
               rng.uniform(100, 60000, 20000), pow_boundaries(LARGEST))


# ---- sqrt and division -----------------------------------------------------------------------------------------------
def _plain_exponent_classes(rng, n_each: int) -> np.ndarray:
    """Random significands on the biased exponents around pw_plain_exponent's two bounds (pw_common.hpp), both signs."""
    e = np.array([PLAIN_LO - 1, PLAIN_LO, PLAIN_LO + 1, PLAIN_HI - 1, PLAIN_HI, PLAIN_HI + 1], dtype=U)
    mant = rng.integers(0, 1 << 52, (len(e), n_each), dtype=np.uint64)
    sign = rng.integers(0, 2, (len(e), n_each), dtype=np.uint64) << U(63)
    return from_bits(((e[:, None] << U(52)) | mant | sign).ravel())


def sqrt_arguments() -> np.ndarray:
    rng = np.random.default_rng(20266)
    any_bits = from_bits(rng.integers(0, 1 << 63, 1 << 16, dtype=np.uint64))
    subnormal = from_bits(rng.integers(1, 1 << 52, 4096, dtype=np.uint64))
    return cat(any_bits, subnormal, np.abs(_plain_exponent_classes(rng, 256)), 0.0, 5e-324, SMALLEST_NORMAL, LARGEST, np.inf)


def div_arguments():
    """(dividends, divisors): any bit pattern over finite, non-zero divisors; subnormal operands; quotients that are
    subnormal; both operands on the exponents around pw_plain_exponent's bounds."""
    rng = np.random.default_rng(20267)
    n = 1 << 16
    a = from_bits(rng.integers(0, 1 << 64, n, dtype=np.uint64))
    b = from_bits(rng.integers(0, 1 << 64, n, dtype=np.uint64))
    sub = lambda k: from_bits(rng.integers(1, 1 << 52, k, dtype=np.uint64) | (rng.integers(0, 2, k, dtype=np.uint64) << U(63)))
    # subnormal operands on either side
    a = np.concatenate([a, sub(2048), from_bits(rng.integers(0, 1 << 64, 2048, dtype=np.uint64)), sub(1024)])
    b = np.concatenate([b, from_bits(rng.integers(0, 1 << 64, 2048, dtype=np.uint64)), sub(2048), sub(1024)])
    # subnormal quotients: |a / b| between 2^-1074 and 2^-1022
    ea = rng.integers(1, 1000, 4096)
    eb = np.minimum(ea + 1023 + rng.integers(0, 52, 4096), 2046)
    mant = lambda: rng.integers(0, 1 << 52, 4096, dtype=np.uint64)
    a = np.concatenate([a, from_bits((ea.astype(U) << U(52)) | mant())])
    b = np.concatenate([b, from_bits((eb.astype(U) << U(52)) | mant())])
    # the operand classes of pw_plain_exponent, each against each
    pa, pb = _plain_exponent_classes(rng, 512), _plain_exponent_classes(rng, 512)
    a = np.concatenate([a, pa, rng.permutation(pa), 2.0 ** rng.uniform(-40, 40, 3072)])
    b = np.concatenate([b, 2.0 ** rng.uniform(-40, 40, 3072), pb, rng.permutation(pb)])
    keep = np.isfinite(b) & (b != 0.0)
    a, b = np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep])
    return a, b


# ---- the sets --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sets():
    """{name: (which, x, y or None)}.  Built once; the arrays are read-only."""
    sc = sincos_arguments()
    out = {"sin": (SIN, sc, None), "cos": (COS, sc, None)}
    for y in (2.0, 3.0, 0.5):
        x = pow_arguments(y)
        out[f"pow-{y:g}"] = (POW, x, np.full_like(x, y))
    out["square"] = (SQUARE, wrapper_arguments(SQUARE), None)
    out["cube"] = (CUBE, wrapper_arguments(CUBE), None)
    out["acos"] = (ACOS, acos_arguments(), None)
    out["log10"] = (LOG10, log10_arguments(), None)
    out["sqrt"] = (SQRT, sqrt_arguments(), None)
    a, b = div_arguments()
    out["div"] = (DIV, a, b)
    for _, x, y in out.values():
        x.setflags(write=False)
        if y is not None:
            y.setflags(write=False)
    coverage(out)
    return out


SET_NAMES = ("sin", "cos", "pow-2", "pow-3", "pow-0.5", "square", "cube", "acos", "log10", "sqrt", "div")


def coverage(out) -> None:
    """What the sets claim to reach, asserted on indices recomputed here."""
    assert tuple(out) == SET_NAMES
    assert sum(len(x) for _, x, _ in out.values()) < 2_000_000
    # sin / cos: every entry of SC_TAB through an exactly known index, and >= 100 arguments on every branch
    for which, want in ((SIN, range(int(_sc_index(np.array([SC_TAYLOR_MAX]))[0]), SC_ENTRIES)), (COS, range(SC_ENTRIES))):
        label, entries = sincos_paths(which, out["sin"][1])
        assert entries <= set(range(SC_ENTRIES)), sorted(entries - set(range(SC_ENTRIES)))
        assert set(want) <= entries, sorted(set(want) - entries)
        names, counts = np.unique(label.astype(str), return_counts=True)
        expected = {"tiny", "direct-table", "mid-table", *(f"reduced-{q}-cos" for q in (1, 3)),
                    *(f"reduced-{q}-sin-{s}" for q in (0, 2) for s in ("taylor", "table"))}
        expected.add("direct-taylor" if which == SIN else "mid-taylor")
        assert set(names) == expected, set(names) ^ expected
        assert counts.min() >= 100, dict(zip(names, counts))
    # pow: every entry of POW_LOG_TAB (i) and of POW_EXP_TAB (ki & 0x7f), for every exponent y and both wrappers
    for name, y in (("pow-2", 2.0), ("pow-3", 3.0), ("pow-0.5", 0.5), ("square", 2.0), ("cube", 3.0)):
        which, x, _ = out[name]
        x = np.abs(x)
        x = x[pow_in_domain(x, y) & (wrapper_main_path(which, x) if which != POW else True)]
        assert len(np.unique(pow_i(x))) == POW_LOG_ENTRIES, name
        hi = CUBE_HI if y == 3.0 else SQUARE_HI
        built = pow_exp_arguments(y, hi)
        built = built[pow_in_domain(built, y) & (wrapper_main_path(which, built) if which != POW else True)]
        t = 128.0 * y * np.log2(built)
        assert np.abs(t - np.rint(t)).max() < 1e-6 and len(np.unique(pow_ki(built, y))) == POW_EXP_ENTRIES, name
        assert np.isin(built, x).all(), name
    # arccos: all 65536 entries of the reciprocal-square-root table, on the branch that uses them
    ax = out["acos"][1]
    root = ax[(ax * ax >= 0.5 - 0.5 * np.abs(ax)) & (np.abs(ax) < 1.0)]
    assert len(np.unique(rsq_index(root))) == RSQ_ENTRIES


# ---- the library's entry -----------------------------------------------------------------------------------------------
def _entry():
    import ctypes

    from pywindow_amd import _lib

    L = _lib.load()
    L.pw_internal_math.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.pw_internal_math.restype = ctypes.c_int
    return L


def internal_math_rc(ctx, which: int, x, y, n: int, out) -> int:
    """The raw return code; x, y, out: arrays or None (a null pointer)."""
    ptr = lambda a: None if a is None else a.ctypes.data
    return _entry().pw_internal_math(ctx._h, which, ptr(x), ptr(y), n, ptr(out))


def internal_math(ctx, which: int, x, y=None) -> np.ndarray:
    """f_which element by element through the library's test entry, on the context's device or host path."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    out = np.full_like(x, -77.0)
    rc = internal_math_rc(ctx, which, x, y, len(x), out)
    assert rc == 0, _entry().pw_last_error()
    return out
