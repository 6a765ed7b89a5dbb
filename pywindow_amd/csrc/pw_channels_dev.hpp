// pw_channels_dev.hpp -- the component loop of pw_channels.hpp on the device, one copy for pw_channels.hip and
// pw_percolate.hip: a workgroup of CAV_THREADS, the bit grids in LDS, every function called by every thread of the
// workgroup.
//   chan_first  the seed pick: the first set bit of `todo` in rank order by an integer workgroup minimum.
//   chan_fill   the parity fill.  Thread t owns rows t, t + 256, ...; a sweep gives a row the words of its four periodic
//               neighbour rows, of the other parity where the step crosses a face of phi (channels_gather), and takes the
//               x direction to its fixed point inside the word (channels_fill_words); neighbours are read while their
//               owners may be storing them (relaxed atomics: either value is a subset of the fixed point), and the sweeps
//               repeat while __syncthreads_or(changed), at most 2 * nx * ny * nz + 1 times.
//   chan_walk   the component of a seed and how it winds: the fill for phi = 7, which is the component as p0 | p1, its
//               n_voxels and n_cross by integer LDS atomics, then only the fills that channels_next asks for.
// The callers keep the shared words the functions are handed -- sum[0 .. 3] and first -- where they keep their other
// scratch.  Every branch that leads to a barrier depends on values read from LDS after a barrier, the same in every thread.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_cavity_dev.hpp"
#include "pw_channels.hpp"

namespace pw {

constexpr unsigned CHAN_NONE = 0xFFFFFFFFu;                      // no set bit of todo

// the first set bit of s_todo in rank order as row * 64 + bit, or CHAN_NONE, the same in every thread; two barriers.
// cursor: the thread's own, tid before the first call -- no row of this thread before it has a bit of todo, so every
// thread scans its rows from where it stopped the last time (todo only loses bits)
__device__ inline unsigned chan_first(const cavity_word* s_todo, int rows, int& cursor, unsigned* s_first) {
    if (threadIdx.x == 0) *s_first = CHAN_NONE;
    __syncthreads();
    while (cursor < rows && !s_todo[cursor]) cursor += CAV_THREADS;
    if (cursor < rows) atomicMin(s_first, (unsigned)cursor * 64u + (unsigned)(__ffsll((long long)s_todo[cursor]) - 1));
    __syncthreads();
    return *s_first;
}

// the fill for phi of p0, p1 inside `open`; the seed is in p0 and a barrier has passed since it was stored
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

// The component of the bit seed_bit of row seed_row inside `open`, the same in every thread: up to seven fills for the
// phi that channels_next asks for, phi = 7 first, channels_learn after each; the first fill also counts the voxels and the
// crossings of the component into s_sum[0 .. 3].  On return p0 | p1 is the component, and nobody stores to it before the
// caller's next barrier.  A fill costs the barrier before p0, p1 are cleared, the one after, and chan_fill's; the first
// fill one more after the counts.
__device__ inline ChannelsWalk chan_walk(const cavity_word* s_open, cavity_word* s_p0, cavity_word* s_p1, unsigned long long* s_sum,
                                         int seed_row, cavity_word seed_bit, int nx, int ny, int nz) {
    const int tid = threadIdx.x, rows = ny * nz;
    ChannelsWalk W{0, 0, 0, {0, 0, 0}};
    int known = 0, cross = 0, phi = 7;
    bool measured = false;
    for (; W.fills < 7 && phi; ++W.fills) {                          // (seven bits to learn)
        __syncthreads();                                             // (everybody has read what the last fill left)
        for (int r = tid; r < rows; r += CAV_THREADS) {
            s_p0[r] = r == seed_row ? seed_bit : 0;
            s_p1[r] = 0;
        }
        if (!measured && tid < 4) s_sum[tid] = 0;
        __syncthreads();
        chan_fill(s_open, s_p0, s_p1, nx, ny, nz, phi);
        const bool reached = (s_p1[seed_row] & seed_bit) != 0;
        channels_learn(phi, reached, known, W.wraps);
        if (!measured) {
            for (int r = tid; r < rows; r += CAV_THREADS) {
                const cavity_word f = s_p0[r] | s_p1[r];
                if (!f) continue;
                const int j = r % ny, l = r / ny;
                const int rj = l * ny, rl = j;                       // the rows (0, l) and (j, 0)
                long c[3];
                channels_row_cross(f, s_p0[rj] | s_p1[rj], s_p0[rl] | s_p1[rl], nx, ny, nz, j, l, c);
                atomicAdd(s_sum + 0, (unsigned long long)cavity_popcount(f));
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (c[k]) atomicAdd(s_sum + 1 + k, (unsigned long long)c[k]);
            }
            __syncthreads();
            W.n_voxels = (long)s_sum[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                W.n_cross[k] = (long)s_sum[1 + k];
                cross |= (W.n_cross[k] > 0) << k;
            }
            if (cross) channels_learn(cross, reached, known, W.wraps);   // ((1): phi = 7 and phi = cross are one graph)
            measured = true;
        }
        phi = channels_next(cross, known, W.wraps);
    }
    return W;
}

}  // namespace pw
