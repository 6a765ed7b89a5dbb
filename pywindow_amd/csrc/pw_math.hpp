// pw_math.hpp -- the elementary functions of the path, restated so that host tests and
// gfx950 produce the SAME BITS as the reference's numpy calls (utilities.py:1097, 1261-1279,
// 1409-1423): numpy.sin / numpy.cos are the C library's (glibc 2.35, s_sin.c), numpy.arccos is
// Intel SVML's __svml_acos8_ha, numpy.log10 only feeds an int() and is reproduced through its
// floor.  None of them is correctly rounded, and the window optimisers amplify a last-bit
// difference in the rotation matrix to 1e-9..1e-6 in a window diameter, so "within one ulp" is
// not enough: each routine below follows the original operation by operation, fused
// multiply-adds included.  They are NOT the device's libm (ocml differs in the last bit).
#pragma once
#include "pw_common.hpp"
#include "pw_rsqrt14_data.hpp"
#include "pw_sincos_data.hpp"
#include "pw_pow_data.hpp"

namespace pw {

struct DD {
    double hi, lo;
};

PW_HD inline DD two_sum(double a, double b) {
    double s = a + b;
    double bb = s - a;
    double e = (a - (s - bb)) + (b - bb);
    return DD{s, e};
}
PW_HD inline DD quick_two_sum(double a, double b) {  // |a| >= |b|
    double s = a + b;
    double e = b - (s - a);
    return DD{s, e};
}
PW_HD inline DD two_prod(double a, double b) {
    double p = a * b;
    double e = pw_fma(a, b, -p);
    return DD{p, e};
}
PW_HD inline DD dd_add(DD a, DD b) {
    DD s = two_sum(a.hi, b.hi);
    DD t = two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return quick_two_sum(s.hi, s.lo);
}
PW_HD inline DD dd_add_d(DD a, double b) {
    DD s = two_sum(a.hi, b);
    s.lo = s.lo + a.lo;
    return quick_two_sum(s.hi, s.lo);
}
PW_HD inline DD dd_mul(DD a, DD b) {
    DD p = two_prod(a.hi, b.hi);
    p.lo = p.lo + (a.hi * b.lo + a.lo * b.hi);
    return quick_two_sum(p.hi, p.lo);
}
PW_HD inline DD dd_mul_d(DD a, double b) {
    DD p = two_prod(a.hi, b);
    p.lo = p.lo + a.lo * b;
    return quick_two_sum(p.hi, p.lo);
}
PW_HD inline DD dd_neg(DD a) { return DD{-a.hi, -a.lo}; }

PW_HD inline double pw_bits2d(uint64_t u) { union { double d; uint64_t u; } cv; cv.u = u; return cv.d; }
PW_HD inline uint64_t pw_d2bits(double d) { union { double d; uint64_t u; } cv; cv.d = d; return cv.u; }

// ---- numpy.sin / numpy.cos for float64 ------------------------------------------------------------
// numpy calls the C library for these; on the reference's platform that is glibc 2.35's
// s_sin.c (IBM Accurate Mathematical Library branch; < 0.55 ulp, i.e. NOT always correctly
// rounded: 0.2 % of the golden-spiral angles differ from the correctly rounded value).  The
// routine is restated with the fused multiply-adds exactly where the FMA build of glibc has
// them (x86-64 ifunc variant used on every AVX2 machine): table look-up of sin/cos(k/128),
// short Taylor polynomials for the remainder, Cody-Waite reduction in four parts for
// 2.43 < |x| < 1.05e8.  Checked against the C library on millions of arguments
// (tests/test_math.py).  Arguments beyond 1.05e8 never occur on the path.
PW_HD inline double sc_copysign(double mag, double sgn) {
    return pw_bits2d((pw_d2bits(mag) & 0x7fffffffffffffffull) | (pw_d2bits(sgn) & 0x8000000000000000ull));
}
// TAYLOR_SIN(xx, x, dx), s_sin.c
PW_HD inline double sc_taylor_sin(double x, double dx) {
    double xx = x * x;
    double p = pw_fma(xx, SC_S5, SC_S4);
    p = pw_fma(xx, p, SC_S3);
    p = pw_fma(xx, p, SC_S2);
    p = pw_fma(xx, p, SC_S1);
    double t = pw_fma(xx, pw_fma(p, x, -(0.5 * dx)), dx);
    return x + t;
}
// do_sin(x, dx), s_sin.c: sin(x + dx), |x| < 0.86
PW_HD inline double sc_do_sin(double x, double dx) {
    const double xold = x;
    if (pw_abs(x) < SC_TAYLOR_MAX) return sc_taylor_sin(x, dx);
    if (x <= 0.0) dx = -dx;
    const double u = SC_BIG + pw_abs(x);
    x = pw_abs(x) - (u - SC_BIG);
    const int k = (int)(unsigned)(pw_d2bits(u) & 0xffffffffull) * 4;
    const double xx = x * x;
    const double s = x + pw_fma(x * xx, pw_fma(xx, SC_SN5, SC_SN3), dx);
    const double c = pw_fma(x, dx, xx * pw_fma(xx, pw_fma(xx, SC_CS6, SC_CS4), SC_CS2));
    const double sn = SC_TAB[k], ssn = SC_TAB[k + 1], cs = SC_TAB[k + 2], ccs = SC_TAB[k + 3];
    const double cor = pw_fma(s, cs, pw_fma(-c, sn, pw_fma(s, ccs, ssn)));
    return sc_copysign(sn + cor, xold);
}
// do_cos(x, dx), s_sin.c: cos(x + dx), |x| < 0.86
PW_HD inline double sc_do_cos(double x, double dx) {
    if (x < 0.0) dx = -dx;
    const double u = SC_BIG + pw_abs(x);
    x = pw_abs(x) - (u - SC_BIG) + dx;
    const int k = (int)(unsigned)(pw_d2bits(u) & 0xffffffffull) * 4;
    const double xx = x * x;
    const double s = pw_fma(x * xx, pw_fma(xx, SC_SN5, SC_SN3), x);
    const double c = xx * pw_fma(xx, pw_fma(xx, SC_CS6, SC_CS4), SC_CS2);
    const double sn = SC_TAB[k], ssn = SC_TAB[k + 1], cs = SC_TAB[k + 2], ccs = SC_TAB[k + 3];
    const double cor = pw_fma(-s, sn, pw_fma(-c, cs, pw_fma(-s, ssn, ccs)));
    return cs + cor;
}
// reduce_sincos(x, &a, &da), s_sin.c: x = n*pi/2 + a + da; returns n mod 4
PW_HD inline int sc_reduce(double x, double* a, double* da) {
    const double t = pw_fma(x, SC_HPINV, SC_TOINT);
    const double xn = t - SC_TOINT;
    const double y = pw_fma(-xn, SC_MP2, pw_fma(-xn, SC_MP1, x));
    const int n = (int)(pw_d2bits(t) & 3ull);
    const double t2 = pw_fma(-xn, SC_PP3, y);
    double db = pw_fma(-xn, SC_PP3, y - t2);
    const double b = pw_fma(-xn, SC_PP4, t2);
    db = db + pw_fma(-xn, SC_PP4, t2 - b);
    *a = b;
    *da = db;
    return n;
}
PW_HD inline double sc_do_sincos(double a, double da, int n) {
    double r = (n & 1) ? sc_do_cos(a, da) : sc_do_sin(a, da);
    return (n & 2) ? -r : r;
}
// libm sin(x) as numpy.sin sees it
PW_NOINLINE PW_HD inline double pw_sin_np(double x) {
    const unsigned k = (unsigned)(pw_d2bits(x) >> 32) & 0x7fffffffu;
    if (k < 0x3e500000u) return x;
    if (k < 0x3feb6000u) return sc_do_sin(x, 0.0);
    if (k < 0x400368fdu) {
        double t = SC_HP0 - pw_abs(x);
        return sc_copysign(sc_do_cos(t, SC_HP1), x);
    }
    double a, da;
    int n = sc_reduce(x, &a, &da);
    return sc_do_sincos(a, da, n);
}
// libm cos(x) as numpy.cos sees it
PW_NOINLINE PW_HD inline double pw_cos_np(double x) {
    const unsigned k = (unsigned)(pw_d2bits(x) >> 32) & 0x7fffffffu;
    if (k < 0x3e400000u) return 1.0;
    if (k < 0x3feb6000u) return sc_do_cos(x, 0.0);
    if (k < 0x400368fdu) {
        double y = SC_HP0 - pw_abs(x);
        double a = y + SC_HP1;
        double da = (y - a) + SC_HP1;
        return sc_do_sin(a, da);
    }
    double a, da;
    int n = sc_reduce(x, &a, &da);
    return sc_do_sincos(a, da, n + 1);
}

PW_HD inline void pw_sincos(double x, double* s, double* c) {
    *s = pw_sin_np(x);
    *c = pw_cos_np(x);
}
PW_HD inline double pw_sin(double x) { return pw_sin_np(x); }
PW_HD inline double pw_cos(double x) { return pw_cos_np(x); }

// ---- float64 scalar ** (numpy -> the C library's pow) --------------------------------------------
// The reference writes x ** 2, r ** 3 and m ** 0.5 on numpy float64 SCALARS (utilities.py:93, 431,
// 1095, 1434); those go to glibc's pow() (e_pow.c: table-driven log to ~68 bits, then exp), which
// is within 0.52 ulp but not correctly rounded: pow(x, 2.0) != x*x for 0.08 % of the arguments.
// Main path of the FMA build, operation by operation; x positive and normal, the result normal with room to
// spare: 2^-1020 <= x^y < 2^1020 (everything on this path), otherwise the caller's plain expression is used --
// glibc's handling of a result that under- or overflows is not restated, and below 2^-1022 `scale` is meaningless.
PW_NOINLINE PW_HD inline double pw_pow_np(double x, double y) {
    const uint64_t ix = pw_d2bits(x);
    const uint64_t tmp = ix - 0x3fe6955500000000ull;
    const int i = (int)((tmp >> 45) & 0x7f);
    const int k = (int)((int64_t)tmp >> 52);
    const double z = pw_bits2d(ix - (tmp & 0xfff0000000000000ull));
    const double kd = (double)k;
    const double ln2hi = POW_LOG_HEAD[0], ln2lo = POW_LOG_HEAD[1];
    const double A0 = POW_LOG_HEAD[2], A1 = POW_LOG_HEAD[3], A2 = POW_LOG_HEAD[4], A3 = POW_LOG_HEAD[5],
                 A4 = POW_LOG_HEAD[6], A5 = POW_LOG_HEAD[7], A6 = POW_LOG_HEAD[8];
    const double invc = POW_LOG_TAB[4 * i], logc = POW_LOG_TAB[4 * i + 2], logctail = POW_LOG_TAB[4 * i + 3];
    // log(x) = k ln2 + log(c) + log1p(z/c - 1), as hi + lo
    const double t1 = pw_fma(kd, ln2hi, logc);
    const double r = pw_fma(z, invc, -1.0);
    const double ar = r * A0;
    const double lo1 = pw_fma(kd, ln2lo, logctail);
    const double p12 = pw_fma(r, A2, A1);
    const double p34 = pw_fma(r, A4, A3);
    const double t2 = r + t1;
    const double ar2 = r * ar;
    const double ar3 = r * ar2;
    const double lo3 = pw_fma(ar, r, -ar2);
    const double lo2 = (t1 - t2) + r;
    const double p56 = pw_fma(r, A6, A5);
    const double hi = t2 + ar2;
    const double lo4 = (t2 - hi) + ar2;
    const double inner = pw_fma(ar2, pw_fma(p56, ar2, p34), p12);
    double lo = lo1 + lo2;
    lo = lo + lo3;
    lo = lo + lo4;
    lo = pw_fma(ar3, inner, lo);
    const double lhi = hi + lo;
    const double llo = (hi - lhi) + lo;
    // exp(y * log x)
    const double ehi = y * lhi;
    const double elo = pw_fma(y, llo, pw_fma(lhi, y, -ehi));
    const double InvLn2N = POW_EXP_HEAD[0], Shift = POW_EXP_HEAD[1], NegLn2hiN = POW_EXP_HEAD[2],
                 NegLn2loN = POW_EXP_HEAD[3], C2 = POW_EXP_HEAD[4], C3 = POW_EXP_HEAD[5], C4 = POW_EXP_HEAD[6],
                 C5 = POW_EXP_HEAD[7];
    const double zz = pw_fma(ehi, InvLn2N, Shift);
    const uint64_t ki = pw_d2bits(zz);
    const double kdd = zz - Shift;
    double rr = pw_fma(kdd, NegLn2loN, pw_fma(kdd, NegLn2hiN, ehi));
    const int idx = 2 * (int)(ki & 0x7f);
    const uint64_t sbits = POW_EXP_TAB[idx + 1] + (ki << 45);
    rr = elo + rr;
    const double q23 = pw_fma(rr, C3, C2);
    const double tail_r = rr + pw_bits2d(POW_EXP_TAB[idx]);
    const double r2 = rr * rr;
    const double q45 = pw_fma(rr, C5, C4);
    const double acc = pw_fma(q23, r2, tail_r);
    const double r4 = r2 * r2;
    const double tmpv = pw_fma(q45, r4, acc);
    const double scale = pw_bits2d(sbits);
    return pw_fma(tmpv, scale, scale);
}

// ---- exp(x) for x <= 0 ---------------------------------------------------------------------------
// The Gaussian kernel of the trajectory distributions (pw_kde.hpp) is the one caller.  This is NOT a
// restatement of any library's exp: it is the project's own definition, and what matters is that the
// gfx950 build and the -ffp-contract=off host build return the SAME BITS (every operation below is
// written out, fused multiply-adds only where pw_fma stands) and that the value is accurate.
// Method: the table-driven scheme of pw_pow_np's second half, on the same 128-entry table of 2^(j/128)
// as {tail, bits} pairs: x = (128 k + j) ln2/128 + r with |r| <= ln2/256 (Cody-Waite in two parts), a
// degree-5 polynomial for exp(r) - 1, the result 2^k 2^(j/128) (1 + tail + p(r)) with one final fma.
// Reduction boundaries: x = (i + 1/2) ln2/128 for integer i (tests/test_kde.py straddles every one
// down to -745).
// Accuracy: measured maximum 0.506 ulp against a 64-bit-mantissa exp over the 2.8e6 arguments
// of tests/test_kde.py (bar: 1 ulp).
// Range: -inf <= x <= 0.  A result below the smallest normal (x < -708.396..., or a product that
// rounds below 2^-1022) is FLUSHED TO ZERO: gradual underflow would make the last bits depend on how a
// target treats subnormals, and 1e-308 of a density is nothing.  Elsewhere: 0 < x < 709 follows the
// same path and is as accurate, but nothing calls or tests it; x >= 709.78 and NaN give unspecified
// finite-or-not values, never a trap.
// `tab`: POW_EXP_TAB, or a copy of it (the device kernel keeps one in LDS -- a per-lane look-up in a
// 2 KB table is what LDS is for).
template <class Tab>
PW_HD inline double pw_exp_tab(double x, Tab tab) {
    const double InvLn2N = POW_EXP_HEAD[0], Shift = POW_EXP_HEAD[1], NegLn2hiN = POW_EXP_HEAD[2],
                 NegLn2loN = POW_EXP_HEAD[3], C2 = POW_EXP_HEAD[4], C3 = POW_EXP_HEAD[5], C4 = POW_EXP_HEAD[6],
                 C5 = POW_EXP_HEAD[7];
    const double zz = pw_fma(x, InvLn2N, Shift);
    const uint64_t ki = pw_d2bits(zz);
    const double kd = zz - Shift;
    const double r = pw_fma(kd, NegLn2loN, pw_fma(kd, NegLn2hiN, x));
    const int idx = 2 * (int)(ki & 0x7f);
    const uint64_t tbits = tab[idx];
    const uint64_t sbits = tab[idx + 1] + (ki << 45);
    const double q23 = pw_fma(r, C3, C2);
    const double tail_r = r + pw_bits2d(tbits);
    const double r2 = r * r;
    const double q45 = pw_fma(r, C5, C4);
    const double acc = pw_fma(q23, r2, tail_r);
    const double r4 = r2 * r2;
    const double tmp = pw_fma(q45, r4, acc);
    const double scale = pw_bits2d(sbits);
    const double res = pw_fma(tmp, scale, scale);
    // x below ln(2^-1022): `scale` would be meaningless (its exponent field wrapped)
    const bool gone = !(x >= -708.3964185322641) || res < 2.2250738585072014e-308;
    return gone ? 0.0 : res;
}
PW_HD inline double pw_exp(double x) { return pw_exp_tab(x, POW_EXP_TAB); }

// ---- erfc(x) for x >= 0 --------------------------------------------------------------------------
// The real-space Ewald term of pw_ewald.hpp is the one caller.  Like pw_exp this is the project's own definition: what
// matters is that the gfx950 build and the -ffp-contract=off host build return the SAME BITS and that the value is
// accurate.  Every operation is written out and none is fused.
// Method: the classical piecewise rational form (W. J. Cody, "Rational Chebyshev approximations for the error function",
// Math. Comp. 23 (1969), in the arrangement and with the coefficients published with Sun's freely distributable
// math library, 1993):
//     x < 2^-56              1 - x                                    (exactly 1.0 at 0)
//     x < 0.84375            erf(x) = x + x * P(x^2) / Q(x^2); 1 - erf(x), or 0.5 - ((x - 0.5) + x * P / Q) from 0.25 on
//     x < 1.25               1 - erx - P(x - 1) / Q(x - 1), erx = 0.845062911510467529297
//     x < 1 / 0.35           exp(-z*z - 0.5625) * exp((z - x) * (z + x) + R(1 / x^2) / S(1 / x^2)) / x
//     x < 28                 the same with a second pair (R, S)
//     otherwise              +0.0
// z is x with its low 32 bits cleared, so z * z is exact and the first exponential takes an argument without a
// rounding error: THE ARGUMENT SPLIT.  The exponentials are pw_exp_tab's, so a first factor below the smallest normal
// (x above 26.6) is +0.0: the true value is a denormal from x = 26.543 on, and there the result is +0.0 or a denormal.
// Never NaN for a finite argument; NaN and negative arguments are not the path's (a NaN gives +0.0).
// Piece boundaries: 2^-56, 0.25, 0.84375, 1.25, 1 / 0.35, 28 (tests/test_ewald_host.py sweeps each with both neighbours).
// Accuracy: measured maximum 3.0 ulp against the C library's erfc (documented below 1 ulp) over that sweep with 10^5
// log-spaced arguments, up to the last argument whose value is a normal number; the test allows twice that.  The
// largest errors are in 0.84375 <= x < 1.25, where 1 - erx and P / Q cancel to a value half their size.
template <class Tab>
PW_HD inline double pw_erfc_tab(double x, Tab tab) {
    const double erx = 8.45062911510467529297e-01;
    if (x < 1.3877787807814457e-17) return 1.0 - x;                  // 2^-56
    if (x < 0.84375) {
        const double pp0 = 1.28379167095512558561e-01, pp1 = -3.25042107247001499370e-01, pp2 = -2.84817495755985104766e-02,
                     pp3 = -5.77027029648944159157e-03, pp4 = -2.37630166566501626084e-05;
        const double qq1 = 3.97917223959155352819e-01, qq2 = 6.50222499887672944485e-02, qq3 = 5.08130628187576562776e-03,
                     qq4 = 1.32494738004321644526e-04, qq5 = -3.96022827877536812320e-06;
        const double z = x * x;
        const double r = pp0 + z * (pp1 + z * (pp2 + z * (pp3 + z * pp4)));
        const double s = 1.0 + z * (qq1 + z * (qq2 + z * (qq3 + z * (qq4 + z * qq5))));
        const double y = r / s;
        if (x < 0.25) return 1.0 - (x + x * y);
        const double t = x * y + (x - 0.5);
        return 0.5 - t;
    }
    if (x < 1.25) {
        const double pa0 = -2.36211856075265944077e-03, pa1 = 4.14856118683748331666e-01, pa2 = -3.72207876035701323847e-01,
                     pa3 = 3.18346619901161753674e-01, pa4 = -1.10894694282396677476e-01, pa5 = 3.54783043256182359371e-02,
                     pa6 = -2.16637559486879084300e-03;
        const double qa1 = 1.06420880400844228286e-01, qa2 = 5.40397917702171048937e-01, qa3 = 7.18286544141962662868e-02,
                     qa4 = 1.26171219808761642112e-01, qa5 = 1.36370839120290507362e-02, qa6 = 1.19844998467991074170e-02;
        const double s = x - 1.0;
        const double P = pa0 + s * (pa1 + s * (pa2 + s * (pa3 + s * (pa4 + s * (pa5 + s * pa6)))));
        const double Q = 1.0 + s * (qa1 + s * (qa2 + s * (qa3 + s * (qa4 + s * (qa5 + s * qa6)))));
        return (1.0 - erx) - P / Q;
    }
    if (!(x < 28.0)) return 0.0;
    const double s = 1.0 / (x * x);
    double R, S;
    if (x < 2.857142857142857) {                                     // 1 / 0.35
        const double ra0 = -9.86494403484714822705e-03, ra1 = -6.93858572707181764372e-01, ra2 = -1.05586262253232909814e+01,
                     ra3 = -6.23753324503260060396e+01, ra4 = -1.62396669462573470355e+02, ra5 = -1.84605092906711035994e+02,
                     ra6 = -8.12874355063065934246e+01, ra7 = -9.81432934416914548592e+00;
        const double sa1 = 1.96512716674392571292e+01, sa2 = 1.37657754143519042600e+02, sa3 = 4.34565877475229228821e+02,
                     sa4 = 6.45387271733267880336e+02, sa5 = 4.29008140027567833386e+02, sa6 = 1.08635005541779435134e+02,
                     sa7 = 6.57024977031928170135e+00, sa8 = -6.04244152148580987438e-02;
        R = ra0 + s * (ra1 + s * (ra2 + s * (ra3 + s * (ra4 + s * (ra5 + s * (ra6 + s * ra7))))));
        S = 1.0 + s * (sa1 + s * (sa2 + s * (sa3 + s * (sa4 + s * (sa5 + s * (sa6 + s * (sa7 + s * sa8)))))));
    } else {
        const double rb0 = -9.86494292470009928597e-03, rb1 = -7.99283237680523006574e-01, rb2 = -1.77579549177547519889e+01,
                     rb3 = -1.60636384855821916062e+02, rb4 = -6.37566443368389627722e+02, rb5 = -1.02509513161107724954e+03,
                     rb6 = -4.83519191608651397019e+02;
        const double sb1 = 3.03380607434824582924e+01, sb2 = 3.25792512996573918826e+02, sb3 = 1.53672958608443695994e+03,
                     sb4 = 3.19985821950859553908e+03, sb5 = 2.55305040643316442583e+03, sb6 = 4.74528541206955367215e+02,
                     sb7 = -2.24409524465858183362e+01;
        R = rb0 + s * (rb1 + s * (rb2 + s * (rb3 + s * (rb4 + s * (rb5 + s * rb6)))));
        S = 1.0 + s * (sb1 + s * (sb2 + s * (sb3 + s * (sb4 + s * (sb5 + s * (sb6 + s * sb7))))));
    }
    const double z = pw_bits2d(pw_d2bits(x) & 0xffffffff00000000ull);
    const double first = pw_exp_tab(-(z * z) - 0.5625, tab);
    const double second = pw_exp_tab((z - x) * (z + x) + R / S, tab);
    return (first * second) / x;
}
PW_HD inline double pw_erfc(double x) { return pw_erfc_tab(x, POW_EXP_TAB); }

// x ** 2 and x ** 3 for any finite x (pow's sign handling for integer exponents).  Outside pw_pow_np's domain -- a
// power below 2^-1020 or beyond 1e300, zero, infinities, NaN -- the plain product, which is within one ulp of pow.
PW_HD inline double pw_square_np(double x) {
    double a = pw_abs(x);
    if (!(a >= 0x1p-510 && a < 1e150)) return x * x;
    return pw_pow_np(a, 2.0);
}
PW_HD inline double pw_cube_np(double x) {
    double a = pw_abs(x);
    if (!(a >= 0x1p-340 && a < 1e100)) return x * x * x;
    double r = pw_pow_np(a, 3.0);
    return x < 0.0 ? -r : r;
}

// ---- numpy.arccos for float64 ------------------------------------------------------------------
// numpy evaluates arccos with Intel SVML (__svml_acos8_ha; also for scalars: the AVX-512 loop
// handles the tail with masks).  Its results differ from the correctly rounded arccos in 9 % of
// the arguments, so the routine is restated operation by operation (FMA placement included)
// from the vector code: for x^2 < y = (1-|x|)/2 a degree-12 polynomial in x^2, otherwise
// 2*asin(sqrt(y)) with sqrt(2y) as a hi/lo pair refined from the VRSQRT14PD estimate.  That
// instruction is a function of the exponent parity and the top 15 mantissa bits only; its 65536
// values (identical on Intel Xeon and AMD Zen 5) are in pw_rsqrt14_data.hpp.  Checked against
// numpy on 4e6 arguments without a mismatch (tests/test_math.py).
//
// `tab`: 65536 entries decoded by rsqrt14_decode(): (result bits >> 36) for operands in
// [0.5, 1) then [1, 2), indexed by the top 15 mantissa bits.
inline void rsqrt14_decode(unsigned* tab) {
    const unsigned start[2] = {RSQRT14_START_0, RSQRT14_START_1};
    const char* delta[2] = {RSQRT14_DELTA_0, RSQRT14_DELTA_1};
    for (int p = 0; p < 2; ++p) {
        unsigned v = start[p];
        for (int i = 0; i < 32768; ++i) {
            tab[p * 32768 + i] = v;
            if (i < 32767) {
                char c = delta[p][i];
                v -= (unsigned)(c <= '9' ? c - '0' : c - 'a' + 10);
            }
        }
    }
}
// VRSQRT14PD for a positive normal operand
PW_HD inline double pw_rsqrt14(double y, const unsigned* tab) {
    uint64_t u = pw_d2bits(y);
    int ef = (int)((u >> 52) & 0x7ff);
    int p = ef & 1;
    int k = (ef - (1022 + p)) / 2;                 // y = y' * 4^k with y' in [0.5, 2)
    unsigned v = tab[p * 32768 + (int)((u >> 37) & 0x7fff)];
    uint64_t rb = ((uint64_t)((int)(v >> 16) - k) << 52) | ((uint64_t)(v & 0xffffu) << 36);
    return pw_bits2d(rb);
}
// numpy.arccos(x) for |x| <= 1; NaN beyond, as numpy (|vx| / sqrt(vx ** 2) can round to 1 + 2^-52)
PW_NOINLINE PW_HD inline double pw_acos_np(double x, const unsigned* tab) {
    const double c4 = pw_bits2d(0xbf918000993b24c3ull), c3 = pw_bits2d(0x3fa400006f70d42dull),
                 c2 = pw_bits2d(0xbfb7fffffffffe97ull), c1 = pw_bits2d(0x3fcfffffffffff9dull);
    const double q12 = pw_bits2d(0x3fa07520c70eb909ull), q11 = pw_bits2d(0xbf90fb17f7dbb0edull),
                 q10 = pw_bits2d(0x3f943f44bfbc3baeull), q9 = pw_bits2d(0x3f7a583395d45ed5ull),
                 q8 = pw_bits2d(0x3f88f8dc2afccad6ull), q7 = pw_bits2d(0x3f8c6dbbcb88bd57ull),
                 q6 = pw_bits2d(0x3f91c6dcf538ad2eull), q5 = pw_bits2d(0x3f96e89cebdefaddull),
                 q4 = pw_bits2d(0x3f9f1c72e13ad8beull), q3 = pw_bits2d(0x3fa6db6db3b445f8ull),
                 q2 = pw_bits2d(0x3fb333333337e0deull), q1 = pw_bits2d(0x3fc555555555529cull);
    const double pi_lo = pw_bits2d(0x3ca1a62633145c07ull), pi_hi = pw_bits2d(0x400921fb54442d18ull),
                 pio2_lo = pw_bits2d(0x3c91a62633145c07ull), pio2_hi = pw_bits2d(0x3ff921fb54442d18ull);
    const uint64_t sign = pw_d2bits(x) & 0x8000000000000000ull;
    const double nax = pw_bits2d(pw_d2bits(x) | 0x8000000000000000ull);   // -|x|
    const double y = pw_fma(0.5, nax, 0.5);
    const double x2 = nax * nax;
    const bool tiny = y < pw_bits2d(0x3000000000000000ull);
    const double r = tiny ? 0.0 : pw_rsqrt14(y, tab);
    const double t = (x2 < y) ? x2 : y;
    const double y2 = y + y;
    const bool root = !(t < y);                    // 2*asin(sqrt(y)) branch
    const bool reflect = root && !(t < x);         // ... of a negative argument: pi - (...)
    const double rr = r * r;
    const double S = y2 * r;                       // ~ sqrt(2y) * sqrt(2): 2*sqrt(y), high part
    const double e = pw_fma(rr, y2, -2.0);
    const double Slo = pw_fma(r, y2, -S);
    double g = pw_fma(c4, e, c3);
    const double Se = S * e;
    g = pw_fma(e, g, c2);
    g = pw_fma(e, g, c1);
    const double a0 = pw_fma(q10, t, q9);
    double C = pw_fma(Se, g, -Slo);                // 2*sqrt(y) = S - C
    double a1 = pw_fma(q12, t, q11);
    const double a3 = pw_fma(q4, t, q3);
    const double t2 = t * t;
    double a2 = pw_fma(q8, t, q7);
    a1 = pw_fma(t2, a1, a0);
    const double t4 = t2 * t2;
    const double a4 = pw_fma(q6, t, q5);
    a2 = pw_fma(t2, a2, a4);
    a1 = pw_fma(t4, a1, a2);
    a1 = pw_fma(t2, a1, a3);
    if (!root) C = 0.0;
    a1 = pw_fma(t, a1, q2);
    a1 = pw_fma(t, a1, q1);
    const double Q = a1 * t;
    double lo = root ? 0.0 : pio2_lo, hi = root ? 0.0 : pio2_hi;
    if (reflect) { lo = pi_lo; hi = pi_hi; }
    const double slo = pw_bits2d(pw_d2bits(lo) ^ sign);
    const double H = root ? S : nax;
    const double z6 = slo - C;
    const double z3 = H - C;
    double z = pw_fma(z3, Q, z6);
    z = z + H;
    const double res = pw_bits2d(pw_d2bits(z) ^ sign) + hi;
    return nax < -1.0 ? pw_bits2d(0x7ff8000000000000ull) : res;
}

// ---- numpy.log10, through its floor ---------------------------------------------------------------------------
// The reference sizes the sampling sphere with int(numpy.log10(area) * 250 * adjust), and numpy.log10 (SVML) is
// correctly rounded on every argument it has been compared on -- among them the doubles next to 10^(m/250), where the
// product is within an ulp of the integer m and a logarithm that is one ulp off floors to the wrong count
// (tests/test_math_edges.py; the fdlibm-style kernel that stood here did on 689 of 47870).  So: log(x) as hi + lo to
// ~2^-66 by the table-driven first half of pw_pow_np (same table, same operations), times 1 / ln 10 as hi + lo,
// rounded once at the end.  x positive and normal.
PW_HD inline double pw_log10(double x) {
    const double ivln10_hi = 0.4342944819032518, ivln10_lo = 1.098319650216765e-17;
    const uint64_t ix = pw_d2bits(x);
    const uint64_t tmp = ix - 0x3fe6955500000000ull;
    const int i = (int)((tmp >> 45) & 0x7f);
    const double kd = (double)(int)((int64_t)tmp >> 52);
    const double z = pw_bits2d(ix - (tmp & 0xfff0000000000000ull));
    const double invc = POW_LOG_TAB[4 * i], logc = POW_LOG_TAB[4 * i + 2], logctail = POW_LOG_TAB[4 * i + 3];
    const double A0 = POW_LOG_HEAD[2], A1 = POW_LOG_HEAD[3], A2 = POW_LOG_HEAD[4], A3 = POW_LOG_HEAD[5],
                 A4 = POW_LOG_HEAD[6], A5 = POW_LOG_HEAD[7], A6 = POW_LOG_HEAD[8];
    const double r = pw_fma(z, invc, -1.0);
    const double t1 = pw_fma(kd, POW_LOG_HEAD[0], logc);
    const double t2 = r + t1;
    const double ar = r * A0, ar2 = r * ar, ar3 = r * ar2;
    const double hi = t2 + ar2;
    double lo = pw_fma(kd, POW_LOG_HEAD[1], logctail) + ((t1 - t2) + r);
    lo = lo + pw_fma(ar, r, -ar2);
    lo = lo + ((t2 - hi) + ar2);
    lo = pw_fma(ar3, pw_fma(ar2, pw_fma(pw_fma(r, A6, A5), ar2, pw_fma(r, A4, A3)), pw_fma(r, A2, A1)), lo);
    const double lhi = hi + lo;
    const double llo = (hi - lhi) + lo;
    DD p = two_prod(lhi, ivln10_hi);
    return p.hi + (p.lo + pw_fma(lhi, ivln10_lo, llo * ivln10_hi));
}

// ---- test instrumentation: one function of this header, chosen by number --------------------------
// pw_internal_math (pw_kernels.hip; pw_hostpath.cpp for a device == -1 context) applies this to arrays so that the
// gfx950 build and the host build can be compared bit for bit, argument by argument (tests/test_gpu_math.py,
// tests/_math_cases.py holds the numbers).  `y` is read by PW_MATH_POW and PW_MATH_DIV only.
enum {
    PW_MATH_SIN = 0, PW_MATH_COS = 1, PW_MATH_POW = 2, PW_MATH_SQUARE = 3, PW_MATH_CUBE = 4, PW_MATH_ACOS = 5,
    PW_MATH_LOG10 = 6, PW_MATH_SQRT = 7, PW_MATH_DIV = 8, PW_MATH_COUNT = 9
};
PW_HD inline bool pw_math_probe_binary(int which) { return which == PW_MATH_POW || which == PW_MATH_DIV; }
PW_HD inline double pw_math_probe(int which, double x, double y, const unsigned* rsq_tab) {
    // sin / cos beyond 1.05e8 (unspecified above, and the reduced argument would index past SC_TAB): not evaluated
    if (which <= PW_MATH_COS && !(pw_abs(x) <= 1.05e8)) return pw_bits2d(0x7ff8000000000000ull);
    switch (which) {
        case PW_MATH_SIN: return pw_sin_np(x);
        case PW_MATH_COS: return pw_cos_np(x);
        case PW_MATH_POW: return pw_pow_np(x, y);
        case PW_MATH_SQUARE: return pw_square_np(x);
        case PW_MATH_CUBE: return pw_cube_np(x);
        case PW_MATH_ACOS: return pw_acos_np(x, rsq_tab);
        case PW_MATH_LOG10: return pw_log10(x);
        case PW_MATH_SQRT: return pw_sqrt(x);
        default: return x / y;
    }
}

}  // namespace pw
