// pw_ewald_dev.hpp -- what pw_rigid_cell.hip (the plan, the field kernel, the two C ABI entries) and pw_ewald.hip (the
// kernels of the reciprocal sum) share: a job as the kernels of a launch read it, and the launch of the reciprocal part.
#pragma once
#include <hip/hip_runtime.h>

#include "pw_ewald.hpp"

namespace pw {

// firsts are relative to the spans of the arrays that were uploaded; the fields from `alpha` on are pw_rigid_cell_ewald's
// and are zero (urec_first: -1) in a pw_rigid_cell job
struct RCellJobDev {
    long atom_first, n, coef_first;
    long rec_first;            // the job's (2L + 2) V record words in the workspace of its launch
    long part_first;           // the job's [chunks][stride] partials in that workspace
    long item_first;           // the job's first group among the work items of the main kernel
    long chunk_first;          // the job's first chunk among the work items of the sums kernel
    long chunks, V;
    long beta_first, site_first, dir_first;   // into the uploaded betas, offsets and directions
    long level_first;          // into the compact result of the call
    double o[3], s[6], core2, cutoff2, reach2;
    int nx, ny, nz, gx, gy, L, S, M, cls, charged;
    double alpha;
    long q_first, cell_first, n_cell, k_first, K;   // into the uploaded site charges, cell rows and (h, k, l, w) rows
    long table_first;          // the job's ewald_table_words in the workspace: (c0, s0) a row, then (P, Q) per (o, row)
    long urec_first;           // the job's M V words of Urec in the workspace, plane o at o * V; -1: nothing is added
    long krow_first;           // the job's first row among the work items of the tables kernel
    long tile_first;           // the job's first (group, tile of EWALD_OT orientations) among the items of the Urec kernel
};

// the tables and Urec of the jobs of a launch group that have rows (`rows` and `tiles`: the items of the two kernels);
// on the stream, before the group's field kernel
hipError_t ewald_launch(hipStream_t st, const RCellJobDev* jobs, int n_jobs, long rows, long tiles, const double* cell,
                        const double* kvecs, const double* site_q, const double* offsets, const double* dirs,
                        unsigned long long* ws);

}  // namespace pw
