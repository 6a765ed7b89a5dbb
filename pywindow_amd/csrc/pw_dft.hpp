// pw_dft.hpp -- the raw sums of a spectrum at rational frequencies (include/pywindow_amd.h: pw_dft_sums), single
// source for the gfx950 kernels (pw_dft.hip) and the host path (pw_hostpath.cpp).  The reference has no
// counterpart: it never asks at which frequency a cage breathes.
//
// DEFINED RESULT.  For a job with series a[0..n), period M and integer frequency numerators j (j / M cycles per
// sample):
//
//     phase(j, k)  = (c, s):  q = (j k) mod M in 64-bit integers;  q' = q - M when 2 q >= M;
//                    u = (double)q' / (double)M (one correctly rounded division);  ang = u * 6.283185307179586;
//                    (s, c) = pw_sincos(ang)                     (|ang| <= pi: the phases are EXACT integers)
//     chunk ch     = times [512 ch, min(512 (ch + 1), n)),  r = t - 512 ch,  (cA[r], sA[r]) = phase(j, r):
//                    pc = fma(a[t], cA[r], pc),  ps = fma(a[t], sA[r], ps)   from pc = ps = +0, in r order
//     rotation     (cB, sB) = phase(j, 512 ch):
//                    re_ch = fma(cB, pc, -(sB * ps)),  im_ch = fma(sB, pc, cB * ps)
//     re = ((+0 + re_0) + re_1) + ...,  im likewise, in chunk order
//
// The hot loop holds no sine or cosine: it is the product of the series with a table of 512 twiddles a frequency.
// The chunk length is a compile-time constant and every order is written in the source, so the sums do not depend
// on the device, the launch geometry, how the frequencies of a job are cut into slabs to bound the workspace, the
// thread count of the host path, the run, or which other jobs and frequencies share the call, and the two paths
// return the same bits.  No floating-point atomics anywhere.  The sums know nothing of means, gaps or
// normalisation: the caller hands over a centred series with zeros in the gaps and transforms the 0/1 mask
// with further jobs.
#pragma once
#include "pw_common.hpp"
#include "pw_math.hpp"

namespace pw {

constexpr int DFT_CHUNK = 512;           // times of one partial sum; twiddles of one frequency
constexpr int DFT_WAVE = 64;
constexpr int DFT_LANE_FREQS = 2;        // frequencies a lane keeps in registers
constexpr int DFT_WAVE_CHUNKS = 8;       // chunks a wavefront keeps in registers, side by side
constexpr int DFT_GROUP_WAVES = 4;       // wavefronts of a workgroup: the same frequencies, consecutive chunks
constexpr int DFT_TILE = DFT_WAVE * DFT_LANE_FREQS;                  // frequencies of one workgroup
constexpr int DFT_GROUP_CHUNKS = DFT_GROUP_WAVES * DFT_WAVE_CHUNKS;  // chunks of one workgroup
constexpr long DFT_WORKSPACE_BYTES = 64l << 20;   // twiddles and partial sums of one launch (pw_dft.hip: dft_plan)
constexpr long DFT_MAX = 1l << 31;       // largest n and largest period
constexpr double DFT_TWO_PI = 6.283185307179586;

// cosine and sine of 2 pi ((j k) mod M) / M;  0 <= j < M <= 2^31, 0 <= k <= 2^32 (the product stays below 2^63)
PW_HD inline void dft_phase(long j, long k, long M, double* c, double* s) {
    long q = (long)(((unsigned long long)j * (unsigned long long)k) % (unsigned long long)M);
    if (2 * q >= M) q -= M;
    const double u = (double)q / (double)M;
    const double ang = u * DFT_TWO_PI;
    pw_sincos(ang, s, c);
}

// the rotation of a chunk's partial sums by the phase of its first time
PW_HD inline void dft_rotate(double cB, double sB, double pc, double ps, double* re, double* im) {
    *re = pw_fma(cB, pc, -(sB * ps));
    *im = pw_fma(sB, pc, cB * ps);
}

}  // namespace pw
