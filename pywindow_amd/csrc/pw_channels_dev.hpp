// pw_channels_dev.hpp -- the parity fill of pw_channels.hpp on the device, one copy for pw_channels.hip and
// pw_percolate.hip: a workgroup of CAV_THREADS, the three bit grids in LDS.  Thread t owns rows t, t + 256, ...; a sweep
// gives a row the words of its four periodic neighbour rows, of the other parity where the step crosses a face of phi
// (channels_gather), and takes the x direction to its fixed point inside the word (channels_fill_words); neighbours are
// read while their owners may be storing them (relaxed atomics: either value is a subset of the fixed point), and the
// sweeps repeat while __syncthreads_or(changed), at most 2 * nx * ny * nz + 1 times.  Every thread of the workgroup
// calls it; the seed is in p0 and a barrier has passed since it was stored.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_cavity_dev.hpp"
#include "pw_channels.hpp"

namespace pw {

// the fill for phi of p0, p1 inside `open`: see the head of pw_channels.hip
__device__ inline void chan_fill(const cavity_word* s_open, cavity_word* s_p0, cavity_word* s_p1, int nx, int ny, int nz, int phi) {
    const int rows = ny * nz;
    const long max_sweeps = 2 * (long)nx * ny * nz + 1;
    auto load = [&](int q, int row) { return __hip_atomic_load((q ? s_p1 : s_p0) + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    for (long sweep = 0; sweep < max_sweeps; ++sweep) {
        int changed = 0;
        for (int r = threadIdx.x; r < rows; r += CAV_THREADS) {
            const cavity_word o = s_open[r];
            if (!o) continue;
            const cavity_word f0 = s_p0[r], f1 = s_p1[r];        // (only this thread stores them)
            cavity_word from0 = f0, from1 = f1, g0, g1;
            channels_gather(load, r % ny, r / ny, ny, nz, phi, from0, from1);
            if (!((from0 | from1) & o)) continue;
            channels_fill_words(from0, from1, o, nx, (phi & 1) != 0, g0, g1);
            if (g0 != f0) __hip_atomic_store(s_p0 + r, g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (g1 != f1) __hip_atomic_store(s_p1 + r, g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            changed |= g0 != f0 || g1 != f1;
        }
        if (!__syncthreads_or(changed)) break;                       // (the same answer in every thread)
    }
}

}  // namespace pw
