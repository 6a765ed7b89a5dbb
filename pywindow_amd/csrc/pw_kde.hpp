// pw_kde.hpp -- the raw sums of a one-dimensional Gaussian kernel density estimate
// (include/pywindow_amd.h: pw_kde_sums), single source for the gfx950 kernels (pw_kde.hip) and the
// host path (pw_hostpath.cpp).  What the reference's trajectory examples do with the analysis: every
// window / pore / maximum diameter of a trajectory goes through scipy.stats.gaussian_kde on a grid of
// 1000 points (examples/example_7.py:55-80, example_8.py:50-75).
//
// DEFINED RESULT.  For a job with samples x[0..n), points g[0..m) and r = inv_bandwidth (a double the
// CALLER computed once as 1 / h -- the division is not repeated here, so r is part of the definition):
//
//     term(j, i) = pw_exp(-0.5 * (z * z)),   z = (g[j] - x[i]) * r           (each operation rounded)
//     part(c, j) = ((0 + term(j, c L)) + term(j, c L + 1)) + ...             over chunk c, L = KDE_CHUNK samples
//     S[j]       = (part(0, j) + part(1, j)) + part(2, j) + ...              in chunk order
//
// The chunk length is a compile-time constant and the orders are written in the source, so S does not
// depend on the device, the launch geometry, the thread count of the host path or the run, and the two
// paths return the same bits.  No floating-point atomics anywhere.
#pragma once
#include "pw_math.hpp"

namespace pw {

constexpr int KDE_CHUNK = 512;         // samples of one partial sum
constexpr int KDE_LANE_POINTS = 2;     // grid points a lane keeps in registers
constexpr int KDE_WAVE = 64;
constexpr int KDE_TILE = KDE_WAVE * KDE_LANE_POINTS;   // grid points of one workgroup (one wavefront)

template <class Tab>
PW_HD inline double kde_term(double g, double x, double r, Tab tab) {
    const double z = (g - x) * r;
    const double t = z * z;
    return pw_exp_tab(-0.5 * t, tab);
}

// one point's partial sum over samples [0, len) of a chunk
template <class Xs, class Tab>
PW_HD inline double kde_chunk_sum(double g, Xs x, int len, double r, Tab tab) {
    double p = 0.0;
    for (int i = 0; i < len; ++i) p = p + kde_term(g, x[i], r, tab);
    return p;
}

PW_HD inline bool kde_finite(double v) { return (pw_d2bits(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

}  // namespace pw
