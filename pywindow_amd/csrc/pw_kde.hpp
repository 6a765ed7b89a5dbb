// pw_kde.hpp -- the raw sums of a one-dimensional Gaussian kernel density estimate
// (include/pywindow_amd.h: pw_kde_sums) and, further down, of a two-dimensional one (pw_kde2_sums) and of the
// one-dimensional one under many weight vectors (pw_kde_wsums),
// single source for the gfx950 kernels (pw_kde.hip, pw_kdew.hip) and the
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

// ---- two dimensions: the raw sums of a joint (two-quantity) Gaussian KDE (pw_kde2_sums) ----------------
// What the examples' scipy.stats.gaussian_kde does with a 2 x n dataset and a mesh of points.
//
// DEFINED RESULT.  For a job with samples (x0[i], x1[i]), points (g0[j], g1[j]) and the three doubles
// w00, w10, w11 -- the lower-triangular inverse of the Cholesky factor of the kernel's covariance, computed
// ONCE by the caller and part of the definition like r above:
//
//     dx = g0[j] - x0[i];  dy = g1[j] - x1[i]                                 (each operation rounded)
//     z0 = dx * w00;  z1 = fma(dx, w10, dy * w11);  t = fma(z1, z1, z0 * z0)
//     term(j, i) = pw_exp(-0.5 * t)
//
// (difference first, whitening second: whitening samples and points apart and subtracting afterwards loses
// a digit where the offset is large against the kernel width).  The sum over i is the one above: chunks of
// KDE_CHUNK samples added one after the other from zero, the chunks' sums added in chunk order.  How the
// points of a job are cut into slabs to bound the workspace (KDE2_WORKSPACE_BYTES) has no part in it:
// points are independent.
constexpr int KDE2_LANE_POINTS = 2;    // mesh points a lane keeps in registers
constexpr int KDE2_TILE = KDE_WAVE * KDE2_LANE_POINTS;
constexpr int KDE2_STAGE = 256;        // sample pairs staged in LDS at a time (a chunk goes through in two halves)
constexpr long KDE2_WORKSPACE_BYTES = 64l << 20;   // partial sums of one launch pair (see pw_kde.hip: kde2_plan)

template <class Tab>
PW_HD inline double kde2_term(double g0, double g1, double x0, double x1, double w00, double w10, double w11, Tab tab) {
    const double dx = g0 - x0, dy = g1 - x1;
    const double z0 = dx * w00;
    const double z1 = pw_fma(dx, w10, dy * w11);
    const double t = pw_fma(z1, z1, z0 * z0);
    return pw_exp_tab(-0.5 * t, tab);
}

// one point's partial sum over sample pairs [0, len) of a chunk; xy = x0, x1, x0, x1, ...
template <class Tab>
PW_HD inline double kde2_chunk_sum(double g0, double g1, const double* xy, int len, double w00, double w10, double w11,
                                   Tab tab) {
    double p = 0.0;
    for (int i = 0; i < len; ++i) p = p + kde2_term(g0, g1, xy[2 * i], xy[2 * i + 1], w00, w10, w11, tab);
    return p;
}

// ---- weights: the raw sums of a one-dimensional KDE under many weight vectors at once (pw_kde_wsums) -----
// scipy.stats.gaussian_kde(samples, bw_method, weights=w), and the replicas of a block bootstrap: a replica is
// the sample set with integer multiplicities, i.e. a weight vector, and all replicas share every exponential.
//
// DEFINED RESULT.  For a job with samples x[0..n), points g[0..m), R weight vectors w[i][b] (sample-major:
// weights[i * R + b]) and r = inv_bandwidth, with term(j, i) the kde_term above, unchanged:
//
//     part(c, b, j): p = +0;  p = pw_fma(w[i][b], term(j, i), p)  for i over chunk c in sample order
//     S[b][j]      = (part(0, b, j) + part(1, b, j)) + part(2, b, j) + ...       in chunk order
//
// with the chunks the KDE_CHUNK samples counted from sample 0, as above.  A replica's sum is its own: it does
// not depend on which other replicas the job carries, on how points and replicas are cut into tiles and slabs
// (KDEW_WORKSPACE_BYTES), on the launch geometry or on the host's threads.  With all weights 1.0 the bits are
// pw_kde_sums': fma(1, e, p) is p + e.  The caller divides by sum_i w[i][b] * h * sqrt(2 pi).
constexpr int KDEW_LANE_POINTS = 2;    // grid points a lane keeps in registers
constexpr int KDEW_TILE = KDE_WAVE * KDEW_LANE_POINTS;   // grid points of one work item
constexpr int KDEW_REPLICAS = 32;      // replicas of one work item: a lane holds KDEW_LANE_POINTS x KDEW_REPLICAS sums
constexpr int KDEW_GROUP = 8;          // replicas a cut-short replica tile goes through at a time
constexpr long KDEW_WORKSPACE_BYTES = 64l << 20;   // partial sums of one launch pair (see pw_kdew.hip: kdew_plan)

// one point's partial sums over samples [0, len) of a chunk under nb weight vectors: p[b], b < nb;
// w: the first sample's weights, stride doubles from one sample to the next
template <class Tab>
PW_HD inline void kdew_chunk_sums(double g, const double* x, const double* w, long stride, int len, long nb, double r,
                                  Tab tab, double* p) {
    for (long b = 0; b < nb; ++b) p[b] = 0.0;
    for (int i = 0; i < len; ++i) {
        const double e = kde_term(g, x[i], r, tab);
        const double* wi = w + (long)i * stride;
        for (long b = 0; b < nb; ++b) p[b] = pw_fma(wi[b], e, p[b]);
    }
}

}  // namespace pw
