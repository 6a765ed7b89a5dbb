// pw_cavity_dev.hpp -- the device steps that pw_cavity_kernel (pw_cavity.hip) and pw_pores_kernel (pw_pores.hip) share:
// the open words of a grid from the atoms and planes, and the flood fill of two bit grids in LDS.  A workgroup of
// CAV_THREADS threads a job, every thread of it calls each step; definitions and proofs in pw_cavity.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_cavity.hpp"

namespace pw {

constexpr int CAV_THREADS = 256;

// the value that lane `from` of the wave holds; `from` is the wave's
__device__ inline double cav_lane(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}

// classify: a wave takes rows (j, l), lane i is voxel i; s_open[r] gets the row's word and s_fill[r] 0
__device__ inline void cav_classify(const double* __restrict__ atoms, const double* __restrict__ reach, long n,
                                    const double* __restrict__ cuts, long m, double ox, double oy, double oz, double h,
                                    double probe, int nx, int ny, int rows, cavity_word* s_open, cavity_word* s_fill) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = cavity_coord(ox, lane, h);
    for (int r = wave; r < rows; r += CAV_THREADS / 64) {
        const double y = cavity_coord(oy, r % ny, h), z = cavity_coord(oz, r / ny, h);
        bool open = lane < nx;
        // 64 atoms at a time, lane a holding atom base + a: one ballot of the row test says which of them this row
        // has to look at -- a few of a cage's -- and those go to every lane through the lane-read
        for (long base = 0; base < n; base += 64) {
            if (!__ballot(open)) break;                          // (no voxel of the row is open any more)
            const long a = base + lane;
            double X = 0.0, Y = 0.0, Z = 0.0, r2 = 0.0;
            bool near = false;
            if (a < n) {
                X = atoms[3 * a]; Y = atoms[3 * a + 1]; Z = atoms[3 * a + 2];
                r2 = cavity_reach2(reach[a], probe);
                near = !cavity_row_clear(y - Y, z - Z, r2);
            }
            for (cavity_word todo = __ballot(near); todo; todo &= todo - 1) {   // (at most 64 bits, one fewer a turn)
                const int b = __ffsll((long long)todo) - 1;
                open = open && cavity_free(x - cav_lane(X, b), y - cav_lane(Y, b), z - cav_lane(Z, b), cav_lane(r2, b));
            }
        }
        for (long base = 0; base < m; base += 64) {
            const long q = base + lane;
            double pa = 0.0, pb = 0.0, pc = 0.0, pd = 0.0;
            if (q < m) {
                pa = cuts[4 * q]; pb = cuts[4 * q + 1]; pc = cuts[4 * q + 2]; pd = cuts[4 * q + 3];
            }
            const int count = m - base < 64 ? (int)(m - base) : 64;
            for (int b = 0; b < count; ++b)
                open = open && cavity_inside(cav_lane(pa, b), cav_lane(pb, b), cav_lane(pc, b), cav_lane(pd, b), x, y, z);
        }
        const cavity_word word = __ballot(open);
        if (lane == 0) {
            s_open[r] = word;
            s_fill[r] = 0;
        }
    }
}

// ready-made open words in place of the classification: loaded and masked to nx
__device__ inline void cav_load_open(const cavity_word* __restrict__ words, int nx, int rows, cavity_word* s_open,
                                     cavity_word* s_fill) {
    const cavity_word xmask = cavity_row_mask(nx);
    for (int r = threadIdx.x; r < rows; r += CAV_THREADS) {
        s_open[r] = words[r] & xmask;
        s_fill[r] = 0;
    }
}

// the seed: thread 0 sets its bit in s_fill if it is open and returns that (false in every other thread); the
// workgroup has passed a barrier after the classification, and passes one here
__device__ inline bool cav_seed(const int* seed, int ny, const cavity_word* s_open, cavity_word* s_fill) {
    bool seed_open = false;
    if (threadIdx.x == 0) {
        const int seed_row = seed[2] * ny + seed[1];
        const cavity_word seed_bit = 1ull << seed[0];
        seed_open = (s_open[seed_row] & seed_bit) != 0;
        if (seed_open) s_fill[seed_row] = seed_bit;
    }
    __syncthreads();
    return seed_open;
}

// fill: thread t owns rows t, t + CAV_THREADS, ...; sweeps repeat while one of them changed a word, at most
// nx * ny * nz + 1 times; every thread reaches every barrier the same number of times, the last one after the last store
__device__ inline void cav_fill(const cavity_word* s_open, cavity_word* s_fill, int nx, int ny, int nz) {
    const int rows = ny * nz;
    const long max_sweeps = (long)nx * ny * nz + 1;
    for (long sweep = 0; sweep < max_sweeps; ++sweep) {
        int changed = 0;
        for (int r = threadIdx.x; r < rows; r += CAV_THREADS) {
            const cavity_word o = s_open[r];
            if (!o) continue;
            const int j = r % ny, l = r / ny;
            const cavity_word f = s_fill[r];                         // (only this thread stores it)
            cavity_word from = f;
            if (j > 0) from |= __hip_atomic_load(s_fill + r - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (j + 1 < ny) from |= __hip_atomic_load(s_fill + r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (l > 0) from |= __hip_atomic_load(s_fill + r - ny, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (l + 1 < nz) from |= __hip_atomic_load(s_fill + r + ny, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const cavity_word g = cavity_fill_word(from, o);
            if (g != f) {
                __hip_atomic_store(s_fill + r, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;                       // (the same answer in every thread)
    }
}

}  // namespace pw
