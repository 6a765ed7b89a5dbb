// pw_corr.hpp -- the raw lagged sums of a time correlation (include/pywindow_amd.h: pw_corr_sums), single
// source for the gfx950 kernels (pw_corr.hip) and the host path (pw_hostpath.cpp).  The reference has no
// counterpart: its examples stop at the distribution of the values of a trajectory and never ask how long a
// value lasts.
//
// DEFINED RESULT.  For a job with series a[0..n), b[0..n) and n_lags <= n:
//
//     part(c, k) = fma(a[t], b[t + k], part)  from part = 0, t rising over chunk c:
//                  t in [c L, min((c + 1) L, n - k)),  L = CORR_CHUNK                  (one rounding per term)
//     S[k]       = (part(0, k) + part(1, k)) + part(2, k) + ...  over the chunks that have a term, in order
//
// The cut of the t axis starts at t = 0 and does not depend on k: a lag's last chunk is shorter, and chunks
// wholly beyond n - k do not exist for it.  The chunk length is a compile-time constant and the orders are
// written in the source, so S does not depend on the device, the launch geometry, how the lags of a job are
// cut into slabs to bound the workspace, the thread count of the host path or the run, and the two paths
// return the same bits.  No floating-point atomics anywhere.  The sums know nothing of means or gaps: the
// caller hands over centred series with zeros in the gaps and counts the valid pairs of a lag by correlating
// the two 0/1 masks (sums of ones are exact in any order).
#pragma once
#include "pw_common.hpp"

namespace pw {

constexpr int CORR_CHUNK = 512;        // times of one partial sum
constexpr int CORR_LANE_LAGS = 8;      // consecutive lags a lane keeps in registers (R of the register tile)
constexpr int CORR_WAVE = 64;
constexpr int CORR_TILE = CORR_WAVE * CORR_LANE_LAGS;   // lags of one workgroup (one wavefront)
constexpr long CORR_WORKSPACE_BYTES = 64l << 20;        // partial sums of one launch pair (pw_corr.hip: corr_plan)

// one lag's partial sum over `len` times of a chunk: a at the chunk's first time, b at that time + lag
PW_HD inline double corr_chunk_sum(const double* a, const double* b, int len) {
    double p = 0.0;
    for (int t = 0; t < len; ++t) p = pw_fma(a[t], b[t], p);
    return p;
}

// how many terms chunk c has for lag k (0 and below: the chunk does not exist for it)
PW_HD inline long corr_chunk_len(long n, long k, long c) {
    const long left = n - k - c * CORR_CHUNK;
    return left < CORR_CHUNK ? left : CORR_CHUNK;
}

}  // namespace pw
