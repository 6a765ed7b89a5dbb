// pw_field_cell_dev.hpp -- pw_field_dev.hpp's field_items on the skewed grid of a periodic cell: the Lennard-Jones energy
// of every voxel of the cells of the jobs of a launch, written to each job's map in the workspace.  The same body with
// channels_x / _y / _z (pw_channels.hpp) in place of cavity_coord; a header of its own, and not a coordinate functor in
// field_items, so that the kernels of pw_passage.hip and pw_hop.hip keep their code byte for byte.  A work item is (job,
// chunk of 64 ranks of the whole cell) and a wavefront (a workgroup of AFF_CHUNK threads) takes one item after the other,
// the job of an item found by binary search in the prefix of work items.  The atoms -- every periodic image that matters
// listed as an atom of its own -- go through LDS PAS_FIELD_TILE at a time and are read at one address per wave, so there
// is no capacity in n.  No atom is skipped.  The pair terms are pw_affinity.hpp's in pw_affinity_kernel's order; the lane
// writes U, +inf where blocked.
//
// Job: a record with atom_first, n, coef_first, map_first, item_first, V, o[3], s[6], core2, cutoff2, nx, ny.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_channels.hpp"
#include "pw_passage.hpp"
#include "pw_stat_host.hpp"

namespace pw {

template <class Job>
__device__ inline void field_items_cell(const Job* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                                        const double* __restrict__ coef, cavity_word* __restrict__ ws) {
    __shared__ double s_xyz[3 * PAS_FIELD_TILE];
    __shared__ double s_coef[2 * PAS_FIELD_TILE];
    const int lane = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {      // (the items of the launch)
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
        const Job& J = jobs[k];
        const long chunk = item - J.item_first, rank = chunk * AFF_CHUNK + lane;
        const bool valid = rank < J.V;
        const int nx = J.nx, ny = J.ny;
        const int row = valid ? (int)(rank / nx) : 0, i = valid ? (int)(rank - (long)row * nx) : 0;
        const int j = row % ny, l = row / ny;
        const double x = channels_x(J.o[0], i, J.s[0], j, J.s[1], l, J.s[3]), y = channels_y(J.o[1], j, J.s[2], l, J.s[4]),
                     z = channels_z(J.o[2], l, J.s[5]);
        const double core2 = J.core2, cutoff2 = J.cutoff2;
        const double* atoms = xyz + 3 * J.atom_first;
        const double* rows_ab = coef + 2 * J.coef_first;
        double U = 0.0;
        bool blocked = false;
        for (long a0 = 0; a0 < J.n; a0 += PAS_FIELD_TILE) {              // (the atoms, a tile a turn)
            const int len = (int)(J.n - a0 < PAS_FIELD_TILE ? J.n - a0 : PAS_FIELD_TILE);
            __syncthreads();                                         // (the atoms staged before are done with)
            for (int t = lane; t < 3 * len; t += AFF_CHUNK) s_xyz[t] = atoms[3 * a0 + t];
            for (int t = lane; t < 2 * len; t += AFF_CHUNK) s_coef[t] = rows_ab[2 * a0 + t];
            __syncthreads();
            for (int t = 0; t < len; ++t) {
                const double r2 = aff_r2(x - s_xyz[3 * t], y - s_xyz[3 * t + 1], z - s_xyz[3 * t + 2]);
                blocked = blocked || aff_blocked(r2, core2);
                const double u = aff_pair(r2, s_coef[2 * t], s_coef[2 * t + 1]);
                U = aff_counts(r2, cutoff2) ? U + u : U;
            }
        }
        if (valid) ws[J.map_first + rank] = pw_d2bits(blocked ? aff_inf() : U);
    }
}

}  // namespace pw
