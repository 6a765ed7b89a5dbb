// pw_ewald.hip -- gfx950 kernels of the reciprocal part of pw_rigid_cell_ewald (include/pywindow_amd.h; the definition in
// pw_ewald.hpp) and the test hook of pw_erfc.  Two kernels a launch group, ahead of pw_rigid_cell.hip's field kernel:
//   tables   a work item is (job, row k), one wavefront an item.  The lanes share out the cell atoms -- lane t takes j = t,
//            t + 64, ... in order, the 64 accumulators of the definition --, the structure factors come down the tree by
//            __shfl_down and go to every lane by __shfl; then a lane takes an orientation and writes (P, Q) of (o, k).
//            Lane 0 writes the phase of the origin, and the item of a job's row 0 writes the three axis tables.
//   urec     a work item is (job, group of 4 x 4 x 4 voxels, tile of EWALD_OT orientations), one wavefront an item, a lane a
//            voxel as in the field kernel.  Per row the lane builds (c_kv, s_kv) once from the axis tables (LDS, indexed by
//            exact integer residues) and uses it for the EWALD_OT accumulators of the tile, which are registers; the row's
//            indices, its phase and its (P, Q) are the same address in every lane.  V x M x K x 2 multiply-adds a job and
//            V x (M / EWALD_OT) x K angle additions, no sine or cosine.  The lane writes Urec(v, o) into the workspace,
//            plane o at o * V, where the field kernel reads it when the pose's sites are summed.
// Why the workspace and not LDS tiles inside the field kernel: the two loops want different register tiles (the pair loop
// holds positions and per-site sums of two orientations, this one an accumulator an orientation and nothing else), the
// field kernel stays the kernel it was, and M V doubles a job (64 MB for a CC3 frame at 64 orientations) are written
// and read once, coalesced, against 3e10 multiply-adds.  The jobs of a launch are grouped so that records, partials, tables
// and Urec fit RCELL_WORKSPACE_BYTES; a job larger than that is a launch of its own.
// Every loop is bounded by n_cell, M, S, K or a constant; a workgroup is one wavefront; nothing spins, no workgroup waits
// for another, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_ewald_dev.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" void pw_hostpath_erfc(const double* x, long n, double* out);   // pw_hostpath.cpp

namespace {

__global__ void __launch_bounds__(AFF_CHUNK)
pw_ewald_tables_kernel(const RCellJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ cell,
                       const double* __restrict__ kvecs, const double* __restrict__ site_q, const double* __restrict__ offsets,
                       const double* __restrict__ dirs, unsigned long long* __restrict__ ws) {
    const int lane = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {      // (the rows of the launch)
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].krow_first; });
        const RCellJobDev& J = jobs[k];
        const long row = item - J.krow_first, K = J.K;
        const int M = J.M;
        const double* kv = kvecs + 4 * (J.k_first + row);
        const EwaldK kk = ewald_kvec(J.s, J.nx, J.ny, J.nz, kv[0], kv[1], kv[2]);
        double sc = 0.0, ss = 0.0;
        for (long j = lane; j < J.n_cell; j += AFF_CHUNK) {              // (accumulator `lane` of the 64)
            const double* a = cell + 4 * (J.cell_first + j);
            const EwaldCS f = ewald_sincos(ewald_dot(kk, a[0], a[1], a[2]));
            sc = sc + a[3] * f.c;
            ss = ss + a[3] * f.s;
        }
        for (int s = 1; s < AFF_CHUNK; s <<= 1) {
            sc = sc + __shfl_down(sc, s);
            ss = ss + __shfl_down(ss, s);
        }
        const double Sc = __shfl(sc, 0), Ss = __shfl(ss, 0);
        double* T = (double*)(ws + J.table_first);
        if (row == 0) {                                              // (the same in every lane)
            if (lane < J.nx) {
                const EwaldCS e = ewald_axis(J.nx, lane);
                T[2 * lane] = e.c;
                T[2 * lane + 1] = e.s;
            }
            if (lane < J.ny) {
                const EwaldCS e = ewald_axis(J.ny, lane);
                T[2 * (EWALD_MAX_INDEX + lane)] = e.c;
                T[2 * (EWALD_MAX_INDEX + lane) + 1] = e.s;
            }
            if (lane < J.nz) {
                const EwaldCS e = ewald_axis(J.nz, lane);
                T[2 * (2 * EWALD_MAX_INDEX + lane)] = e.c;
                T[2 * (2 * EWALD_MAX_INDEX + lane) + 1] = e.s;
            }
        }
        T += EWALD_AXIS_WORDS;
        if (lane == 0) {
            const EwaldCS e0 = ewald_sincos(ewald_dot(kk, J.o[0], J.o[1], J.o[2]));
            T[2 * row] = e0.c;
            T[2 * row + 1] = e0.s;
        }
        const double* dd = dirs + 3 * J.dir_first;
        for (int o = lane; o < M; o += AFF_CHUNK) {
            double P, Q;
            ewald_pq(kk, kv[3], Sc, Ss, offsets + J.site_first, site_q + J.q_first, J.S, dd[3 * o], dd[3 * o + 1], dd[3 * o + 2], &P,
                     &Q);
            T[2 * K + 2 * ((long)o * K + row)] = P;
            T[2 * K + 2 * ((long)o * K + row) + 1] = Q;
        }
    }
}

__global__ void __launch_bounds__(AFF_CHUNK)
pw_ewald_urec_kernel(const RCellJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ kvecs,
                     unsigned long long* ws) {
    __shared__ double s_axis[EWALD_AXIS_WORDS];
    const int lane = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {      // (the (group, tile)s of the launch)
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].tile_first; });
        const RCellJobDev& J = jobs[k];
        const int M = J.M, nx = J.nx, ny = J.ny, nz = J.nz, tiles = (M + EWALD_OT - 1) / EWALD_OT;
        const long local = item - J.tile_first, g = local / tiles, grow = g / J.gx, K = J.K, V = J.V;
        const int o0 = EWALD_OT * (int)(local - g * tiles);
        const int i0 = RCELL_G * (int)(g - grow * J.gx), j0 = RCELL_G * (int)(grow % J.gy), l0 = RCELL_G * (int)(grow / J.gy);
        const int i = i0 + (lane & 3), j = j0 + ((lane >> 2) & 3), l = l0 + (lane >> 4);
        const bool valid = i < nx && j < ny && l < nz;
        // (a lane without a voxel computes the group's first voxel and writes nothing)
        const int iv = valid ? i : i0, jv = valid ? j : j0, lv = valid ? l : l0;
        const double* T = (const double*)(ws + J.table_first);
        __syncthreads();                                             // (the item before is done with the LDS)
        for (int t = lane; t < EWALD_AXIS_WORDS; t += AFF_CHUNK) {
            const int q = (t >> 1) & (EWALD_MAX_INDEX - 1), axis = t >> 7;
            s_axis[t] = q < (axis == 0 ? nx : axis == 1 ? ny : nz) ? T[t] : 0.0;   // (entries past a dimension were never written)
        }
        __syncthreads();
        const double* E0 = T + EWALD_AXIS_WORDS;
        const double* PQ = E0 + 2 * K;
        const double* kv = kvecs + 4 * J.k_first;
        double acc[EWALD_OT];                                        // (indexed by unrolled loops only: registers)
        long at[EWALD_OT];
#pragma unroll
        for (int q = 0; q < EWALD_OT; ++q) {
            acc[q] = 0.0;
            at[q] = (long)(o0 + q < M ? o0 + q : M - 1) * K;         // (past the end: the last one again, not written)
        }
        for (long r = 0; r < K; ++r) {                                   // (the rows, in list order)
            const int qx = ewald_residue((int)kv[4 * r], iv, nx), qy = ewald_residue((int)kv[4 * r + 1], jv, ny),
                      qz = ewald_residue((int)kv[4 * r + 2], lv, nz);
            EwaldCS e{E0[2 * r], E0[2 * r + 1]};
            e = ewald_add(e, EwaldCS{s_axis[2 * qx], s_axis[2 * qx + 1]});
            e = ewald_add(e, EwaldCS{s_axis[2 * (EWALD_MAX_INDEX + qy)], s_axis[2 * (EWALD_MAX_INDEX + qy) + 1]});
            e = ewald_add(e, EwaldCS{s_axis[2 * (2 * EWALD_MAX_INDEX + qz)], s_axis[2 * (2 * EWALD_MAX_INDEX + qz) + 1]});
#pragma unroll
            for (int q = 0; q < EWALD_OT; ++q) acc[q] = acc[q] + ewald_term(PQ[2 * (at[q] + r)], PQ[2 * (at[q] + r) + 1], e);
        }
        if (valid) {
            double* U = (double*)(ws + J.urec_first) + ((long)(l * ny + j) * nx + i);
#pragma unroll
            for (int q = 0; q < EWALD_OT; ++q)
                if (o0 + q < M) U[(long)(o0 + q) * V] = acc[q];
        }
    }
}

// pw_erfc element by element (test instrumentation)
__global__ void __launch_bounds__(256) pw_erfc_probe_kernel(long n, const double* __restrict__ x, double* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = pw_erfc(x[i]);
}

}  // namespace

hipError_t pw::ewald_launch(hipStream_t st, const RCellJobDev* jobs, int n_jobs, long rows, long tiles, const double* cell,
                            const double* kvecs, const double* site_q, const double* offsets, const double* dirs,
                            unsigned long long* ws) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(pw_ewald_tables_kernel, dim3((unsigned)launch_blocks(rows, 65536)), dim3(AFF_CHUNK), 0, st, jobs, n_jobs,
                       rows, cell, kvecs, site_q, offsets, dirs, ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pw_ewald_urec_kernel, dim3((unsigned)launch_blocks(tiles, 65536)), dim3(AFF_CHUNK), 0, st, jobs, n_jobs,
                       tiles, kvecs, ws);
    return hipGetLastError();
}

// test instrumentation (not part of the header): out[i] = pw_erfc(x[i]) on the context's device, or on the host path for
// a device == -1 context.  The two must agree to the bit (tests/test_ewald_gpu.py)
extern "C" int pw_internal_erfc(pw_context* ctx, const double* x, int64_t n, double* out) {
    if (!ctx || n < 0 || (n && (!x || !out))) return PW_E_BAD_ARG;
    if (n == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    if (pw_context_device(ctx) < 0) {
        pw_hostpath_erfc(x, (long)n, out);
        return PW_OK;
    }
    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    const size_t bytes = sizeof(double) * (size_t)n;
    {
        StreamBuffers buf(st);
        double *d_x, *d_out;
        STAT_TRY(buf.alloc(&d_x, bytes));
        STAT_TRY(buf.alloc(&d_out, bytes));
        STAT_TRY(hipMemcpyAsync(d_x, x, bytes, hipMemcpyHostToDevice, st));
        const long blocks = ((long)n + 255) / 256;
        hipLaunchKernelGGL(pw_erfc_probe_kernel, dim3((unsigned)launch_blocks(blocks, 65536)), dim3(256), 0, st, (long)n, d_x,
                           d_out);
        STAT_TRY(hipGetLastError());
        STAT_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    return PW_OK;
}
