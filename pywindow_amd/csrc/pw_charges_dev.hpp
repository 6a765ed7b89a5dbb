// pw_charges_dev.hpp -- the wave-level sums of the charge equilibration kernels (pw_charges.hip, pw_charges_cell.hip): lane l
// of a wave is accumulator l of pw_charges.hpp's SUMS, and the folds below are sup_fold's order as a butterfly.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_charges.hpp"

namespace pw {
namespace {

// acc[l] and acc[l ^ S] (pw_superpose.hpp, SUMS): as in pw_superpose.hip
template <int S>
__device__ inline double chg_partner(double v) {
    if constexpr (S == 32) {
        return __shfl_xor(v, 32, 64);
    } else {
        union { double d; int i[2]; } a, b;
        a.d = v;
        constexpr int pattern = 0x1f | (S << 10);          // bit mode: and 0x1f, or 0, xor S
        b.i[0] = __builtin_amdgcn_ds_swizzle(a.i[0], pattern);
        b.i[1] = __builtin_amdgcn_ds_swizzle(a.i[1], pattern);
        return b.d;
    }
}

__device__ inline double chg_wave_fold(double v) {
    v = v + chg_partner<32>(v);
    v = v + chg_partner<16>(v);
    v = v + chg_partner<8>(v);
    v = v + chg_partner<4>(v);
    v = v + chg_partner<2>(v);
    v = v + chg_partner<1>(v);
    return v;
}

// the fold of q_min (LOW) and q_max: lane l < s holds what the tree of pw_charges.hpp holds in acc[l]; lane 0 the result
template <bool LOW, int S>
__device__ inline double chg_extreme_step(double v) {
    const double other = chg_partner<S>(v);
    return (LOW ? other < v : other > v) ? other : v;
}
template <bool LOW>
__device__ inline double chg_wave_extreme(double v) {
    v = chg_extreme_step<LOW, 32>(v);
    v = chg_extreme_step<LOW, 16>(v);
    v = chg_extreme_step<LOW, 8>(v);
    v = chg_extreme_step<LOW, 4>(v);
    v = chg_extreme_step<LOW, 2>(v);
    v = chg_extreme_step<LOW, 1>(v);
    return v;
}

// lane 0's value in scalar registers: what steers the solver is the same in every lane
__device__ inline double chg_uniform(double v) {
    union { double d; int i[2]; } a;
    a.d = v;
    a.i[0] = __builtin_amdgcn_readfirstlane(a.i[0]);
    a.i[1] = __builtin_amdgcn_readfirstlane(a.i[1]);
    return a.d;
}

template <class I>
__device__ inline double chg_dot(const double* a, const double* b, I n, int lane) {
    double acc = 0.0;
    for (I i = lane; i < n; i += SUP_ACC) acc = pw_fma(a[i], b[i], acc);
    return chg_uniform(chg_wave_fold(acc));
}

}  // namespace
}  // namespace pw
