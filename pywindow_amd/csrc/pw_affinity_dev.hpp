// pw_affinity_dev.hpp -- the prefix kernel that pw_affinity.hip and pw_rigid.hip share: the exclusive prefix of the
// popcounts of the ny * nz words of every job of a launch that has a mask (bits at i >= nx dropped), rows + 1 integers
// in the workspace.  A workgroup a job, a thread at most 16 consecutive rows.  `Job` is the entry's device job: it has
// nx, ny, nz, word_first (the job's words in the uploaded span) and prefix_first (an 8-byte word index into the
// workspace, or -1: no mask).
#pragma once
#include <hip/hip_runtime.h>

#include "pw_cavity.hpp"

namespace pw {

constexpr int AFF_PREFIX_THREADS = 256;

template <class Job>
__global__ void __launch_bounds__(AFF_PREFIX_THREADS)
pw_region_prefix_kernel(const Job* __restrict__ jobs, const cavity_word* __restrict__ words, cavity_word* __restrict__ ws) {
    __shared__ int s_sum[AFF_PREFIX_THREADS];
    const Job& J = jobs[blockIdx.x];
    if (J.prefix_first < 0) return;                                  // (the same in every thread)
    const int rows = J.ny * J.nz, t = threadIdx.x;
    const int per = (rows + AFF_PREFIX_THREADS - 1) / AFF_PREFIX_THREADS;   // <= 16
    const int begin = t * per < rows ? t * per : rows, end = begin + per < rows ? begin + per : rows;
    const cavity_word xmask = cavity_row_mask(J.nx);
    const cavity_word* w = words + J.word_first;
    int* prefix = (int*)(ws + J.prefix_first);
    int mine = 0;
    for (int r = begin; r < end; ++r) mine += cavity_popcount(w[r] & xmask);
    s_sum[t] = mine;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < t; ++q) base += s_sum[q];
    for (int r = begin; r < end; ++r) {
        prefix[r] = base;
        base += cavity_popcount(w[r] & xmask);
    }
    if (t == AFF_PREFIX_THREADS - 1) prefix[rows] = base;            // (the last thread's rows end at `rows`: the total)
}

}  // namespace pw
