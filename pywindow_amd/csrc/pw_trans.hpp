// pw_trans.hpp -- lagged state-transition counts of a series (include/pywindow_amd.h: pw_trans_counts), single source
// for the gfx950 kernels (pw_trans.hip) and the host path (pw_hostpath.cpp).  The reference has no counterpart.
//
// DEFINED RESULT.  A job has a series a[0..n), n_edges strictly increasing edges and lags k_q.  The state of an entry is
// the number of edges e with e <= a[t] (np.searchsorted(edges, a, side="right")); a NaN entry -- recognised on the
// bits, as pw_gate.hpp does -- is a GAP and has no state.  C_k[i][j] = #{t : 0 <= t, t + k < n, s[t] = i, s[t + k] = j},
// a pair with a gap at either end counted nowhere.
//
// Every output is an integer count, so the result is the definition itself whatever the order of the work.  Both paths
// take the bit-parallel form: the series is classified ONCE into one bit mask a state over the time axis (bit t % W of
// word t / W, W = 32 on the device, 64 on the host; gaps and entries past n are in no mask, and one word of zeros
// follows the last), and for a word w of W origins and a lag k the partner word of state j is the funnel shift of
// M_j[w + k / W + 1] : M_j[w + k / W] by k % W.  C[i][j] += popcount(M_i[w] & partner_j): t + k < n, gaps and states
// that the edges cannot reach need no branch.
#pragma once
#include "pw_common.hpp"
#include "pw_gate.hpp"

namespace pw {

constexpr int TRANS_MAX_STATES = 16;
constexpr int TRANS_CHUNK = 8192;        // entries of one chunk of the time axis: the origins of one work item
constexpr int TRANS_TILE = 256;          // lags of one workgroup, one a lane
constexpr int TRANS_WINDOW = 16640;      // entries of the partner window a work item can stage in LDS (520 words a state)
constexpr long TRANS_WORKSPACE_BYTES = 64l << 20;   // masks of one launch pair (pw_trans.hip: trans_plan)
constexpr long TRANS_MAX = 1l << 31;     // largest n
constexpr long TRANS_MAX_LAG = 1l << 62; // lag_first + (n_lags - 1) * lag_step stays below this

constexpr int TRANS_GAP = -1;

// the state of an entry against the job's edges, TRANS_GAP for a NaN (an infinity never reaches this: the entry
// refuses it, so all ones in the exponent is a NaN).  -0.0 >= 0.0 holds, so -0.0 at an edge 0.0 is in the upper state.
PW_HD inline int trans_state(double a, const double* edges, int n_edges) {
    union { double d; unsigned long long u; } c;
    c.d = a;
    if ((c.u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return TRANS_GAP;
    int s = 0;
    for (int e = 0; e < n_edges; ++e) s += edges[e] <= a ? 1 : 0;
    return s;
}

// the padded state count a kernel is instantiated for: 2, 4, 8 or 16
PW_HD inline int trans_padded(int n_states) { return n_states <= 2 ? 2 : n_states <= 4 ? 4 : n_states <= 8 ? 8 : 16; }

// bits [r, r + W) of the 2W-bit number hi : lo, 0 <= r < W
PW_HD inline unsigned trans_funnel(unsigned hi, unsigned lo, unsigned r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, r);                   // v_alignbit_b32
#else
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> r);
#endif
}
PW_HD inline unsigned long long trans_funnel(unsigned long long hi, unsigned long long lo, unsigned r) {
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
}
// acc += popcount(v).  On the device one v_bcnt_u32_b32, written out: left to itself the compiler counts into a fresh
// register and adds two counts at a time, a fifth instruction for every four.
PW_HD inline void trans_count(unsigned& acc, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(v));
#else
    acc += (unsigned)__builtin_popcount(v);
#endif
}
PW_HD inline void trans_count(long& acc, unsigned long long v) { acc += __builtin_popcountll(v); }

}  // namespace pw
