// pw_cov.hpp -- the scatter matrix of the rows of a matrix, its column mean and projections on given vectors
// (include/pywindow_amd.h: pw_covariance, pw_project), single source for the gfx950 kernels (pw_cov.hip) and the
// host path (pw_hostpath.cpp).  The reference has no counterpart: it has no essential dynamics.
//
// DEFINED RESULT.  A job has the row-major matrix X of T rows and D columns and, optionally, T transform rows
// (pw_superpose_out; only rotation R, centre_mobile cm and centre_target ct are read).
//
//   VALUE.  Without transforms y_ta = X[t][a].  With them D = 3 n, row t is n points x_p = X[t][3p .. 3p + 2], and
//   for the point p = a / 3 and the component c = a % 3 (cov_y below)
//       d_0 = x_p0 - cm_0,  d_1 = x_p1 - cm_1,  d_2 = x_p2 - cm_2          (three subtractions)
//       r   = fma(R[c][2], d_2, fma(R[c][1], d_1, R[c][0] * d_0))          (one product, two fma)
//       y_ta = r + ct_c                                                    (one addition)
//   CHUNKS.  The rows are cut into chunks of PW_COV_CHUNK = 256 consecutive rows, chunk q the rows 256 q .. ; the
//   last chunk may be short.
//   MEAN.  The column sum of a chunk starts at +0.0 and takes s = s + y_ta in ascending t.  The total is the sum of
//   chunk 0, then total = total + (the sum of chunk q) for q = 1, 2, ...;  mean_a = total / (double)T.
//   SCATTER.  z_ta = y_ta - mean_a.  A chunk's partial of S[a][b] starts at +0.0 and takes acc = fma(z_ta, z_tb, acc)
//   in ascending t; S[a][b] is the partial of chunk 0, then S = S + (the partial of chunk q) for q = 1, 2, ....
//   fma(u, v, w) == fma(v, u, w) to the bit, so S[a][b] and S[b][a] have the same bits whether the lower triangle is
//   mirrored (the device) or computed; T = 1 gives z = y - y / 1 = +0.0 and S = +0.0 everywhere.  Nothing is divided
//   by T - 1.
//   PROJECTION.  P[t][j] is taken over the columns by COV_PROJ_ACC = 64 STRIDED accumulators folded as in sup_fold
//   (pw_superpose.hpp): accumulator l starts at +0.0 and takes acc = fma(z_ta, V[j][a], acc) for a = l, l + 64,
//   l + 128, ... in that order, with z_ta = y_ta - mean_a of the mean GIVEN to pw_project; then acc[l] = acc[l] +
//   acc[l + s] for l < s, s = 32, 16, 8, 4, 2, 1, and acc[0] is P[t][j].
//
// Only + - * / and fma occur, all of them correctly rounded on both paths (-ffp-contract=off), and the orders are
// written here: the result does not depend on the device, the launch geometry, how a job's tiles and chunks are cut
// into launches to bound the workspace (COV_WORKSPACE_BYTES), the thread count of the host path, the other jobs of the
// call or the run, and the two paths return the same bits.  No floating-point atomics, no MFMA (v_mfma_f64 sums four
// products in an order of its own).  A short last chunk and the last columns of a tile row are left out of the loops
// and the stores; no sum ever takes a padded term.  Products beyond the FP64 range overflow: not checked.
#pragma once
#include "pw_common.hpp"

namespace pw {

constexpr int COV_CHUNK = 256;                      // PW_COV_CHUNK: rows of a chunk
constexpr int COV_MAX_D = 3072;                     // PW_COV_MAX_D: columns of a job (S is 72 MiB there)
constexpr int COV_TILE = 128;                       // a workgroup's square tile of S (pw_cov.hip)
constexpr int COV_PROJ_ACC = 64;                    // accumulators of a projection: the lanes of a wave
constexpr long COV_WORKSPACE_BYTES = 256l << 20;    // chunk sums and [chunk][tile] partials of one launch
constexpr int COV_TRANSFORM_DOUBLES = 19;           // sizeof(pw_superpose_out) / 8: rotation 0, centres 9 and 12

// y_ta of VALUE: xrow the row t of X, tr the transform row t as doubles or null
PW_HD inline double cov_y(const double* xrow, const double* tr, long a) {
    if (!tr) return xrow[a];
    const long p = a / 3;
    const int c = (int)(a - 3 * p);
    const double* x = xrow + 3 * p;
    const double d0 = x[0] - tr[9], d1 = x[1] - tr[10], d2 = x[2] - tr[11];
    // (the row of R and the entry of ct by selects, not by an index: the transform row's address is the same in every
    // lane, so the device reads it with scalar loads)
    const double r0 = c == 0 ? tr[0] : c == 1 ? tr[3] : tr[6];
    const double r1 = c == 0 ? tr[1] : c == 1 ? tr[4] : tr[7];
    const double r2 = c == 0 ? tr[2] : c == 1 ? tr[5] : tr[8];
    const double ct = c == 0 ? tr[12] : c == 1 ? tr[13] : tr[14];
    const double r = pw_fma(r2, d2, pw_fma(r1, d1, r0 * d0));
    return r + ct;
}

// the upper-triangle tile `index` (row-major over ta <= tb) of a matrix of `nt` tile rows
PW_HD inline void cov_tile_of(long index, int nt, int& ta, int& tb) {
    int a = 0;
    while (index >= nt - a) {
        index -= nt - a;
        ++a;
    }
    ta = a;
    tb = a + (int)index;
}

}  // namespace pw
