// pw_superpose.hip -- gfx950 kernels and the C ABI entry of the least-squares superposition of point sets
// (include/pywindow_amd.h: pw_superpose; definition of the result in pw_superpose.hpp).  Three kernels per launch.
//
// pw_superpose_moments_kernel, passes (a) and (b): one wave a job, lane l is accumulator l of every sum and strides
// over the atoms l, l + 64, ... straight from global memory (a frame of 168 atoms is 4 KB and a thousand frames stay
// in L2, so the all-pairs matrix re-reads them from there).  The fold is a butterfly across the lanes, ds_swizzle for
// the strides 16 .. 1 and a ds_bpermute for 32; no LDS is allocated.  Lane 0 leaves M, the centroids and W in the
// workspace, [field][job of the launch].
//
// pw_superpose_solve_kernel: the eigen solve is a dependent chain of a few hundred FP64 operations, so it runs ONE
// LANE A JOB, 64 jobs a wave (a wave a job would idle 63 lanes for most of the run time of an all-pairs batch); the
// 4 x 4 and its eigenvectors are registers (compile-time indices, sup_rotate<P, Q>) and the [field][job] layout makes
// its loads and stores contiguous across the lanes.
//
// pw_superpose_residual_kernel, pass (c): a wave a job again, the rotation from the workspace, the direct residual
// sum, and lane 0 writes the job's row of the compact result.  Everything is queued on the context's stream, memory
// included.  No atomics of any kind.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_superpose.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_superpose(const pw_superpose_job* jobs, long n_jobs, const double* xyz, const double* weights,
                                     pw_superpose_out* out, int threads);   // pw_hostpath.cpp

static_assert(sizeof(pw_superpose_out) == 152, "rotation, two centres, rmsd, lambda[2], sweeps and padding");
static_assert(sizeof(pw_superpose_job) == 40, "five int64");

namespace {

constexpr int SUP_WAVES = 4;     // waves of a workgroup of the two wave-a-job kernels

// one job: rows relative to the uploaded spans of xyz and weights
struct SupJobDev {
    long mobile, target, weight;   // weight < 0: none
    long n;
};

// acc[l] + acc[l ^ S] in every lane (pw_superpose.hpp, SUMS)
template <int S>
__device__ inline double sup_partner(double v) {
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

__device__ inline double sup_wave_fold(double v) {
    v = v + sup_partner<32>(v);
    v = v + sup_partner<16>(v);
    v = v + sup_partner<8>(v);
    v = v + sup_partner<4>(v);
    v = v + sup_partner<2>(v);
    v = v + sup_partner<1>(v);
    return v;
}

__global__ void __launch_bounds__(64 * SUP_WAVES)
pw_superpose_moments_kernel(const SupJobDev* __restrict__ jobs, long count, const double* __restrict__ xyz,
                            const double* __restrict__ weights, double* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long j = (long)blockIdx.x * SUP_WAVES + wave; j < count; j += (long)gridDim.x * SUP_WAVES) {
        const SupJobDev J = jobs[j];
        const double* x = xyz + 3 * J.mobile;
        const double* y = xyz + 3 * J.target;
        const double* w = J.weight < 0 ? nullptr : weights + J.weight;
        SupSums s;
        sup_sums_zero(s);
        for (long i = lane; i < J.n; i += SUP_ACC) sup_sums_atom(s, x, y, w, i);
        s.w = sup_wave_fold(s.w);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s.x[a] = sup_wave_fold(s.x[a]);
            s.y[a] = sup_wave_fold(s.y[a]);
        }
        SupCentres c;
        sup_centres(s, c);
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = 0.0;
        for (long i = lane; i < J.n; i += SUP_ACC) sup_moment_atom(m, c, x, y, w, i);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = sup_wave_fold(m[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) ws[k * count + j] = m[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                ws[(9 + a) * count + j] = c.cx[a];
                ws[(12 + a) * count + j] = c.cy[a];
            }
            ws[15 * count + j] = c.W;
        }
    }
}

__global__ void __launch_bounds__(64)
pw_superpose_solve_kernel(long count, double* __restrict__ ws) {
    double* sol = ws + SUP_MOMENT_FIELDS * count;
    for (long j = (long)blockIdx.x * 64 + threadIdx.x; j < count; j += (long)gridDim.x * 64) {
        double m[9], r[9], lambda[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = ws[k * count + j];
        const int sweeps = sup_solve(m, r, lambda);
#pragma unroll
        for (int k = 0; k < 9; ++k) sol[k * count + j] = r[k];
        sol[9 * count + j] = lambda[0];
        sol[10 * count + j] = lambda[1];
        sol[11 * count + j] = (double)sweeps;
    }
}

__global__ void __launch_bounds__(64 * SUP_WAVES)
pw_superpose_residual_kernel(const SupJobDev* __restrict__ jobs, long count, const double* __restrict__ xyz,
                             const double* __restrict__ weights, const double* __restrict__ ws,
                             pw_superpose_out* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* sol = ws + SUP_MOMENT_FIELDS * count;
    for (long j = (long)blockIdx.x * SUP_WAVES + wave; j < count; j += (long)gridDim.x * SUP_WAVES) {
        const SupJobDev J = jobs[j];
        const double* x = xyz + 3 * J.mobile;
        const double* y = xyz + 3 * J.target;
        const double* w = J.weight < 0 ? nullptr : weights + J.weight;
        SupCentres c;
        double r[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = sol[k * count + j];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c.cx[a] = ws[(9 + a) * count + j];
            c.cy[a] = ws[(12 + a) * count + j];
        }
        c.W = ws[15 * count + j];
        double e = 0.0;
        for (long i = lane; i < J.n; i += SUP_ACC) e = sup_residual_atom(e, r, c, x, y, w, i);
        e = sup_wave_fold(e);
        if (lane == 0) {
            pw_superpose_out* o = out + j;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) o->rotation[a][b] = r[3 * a + b];
                o->centre_mobile[a] = c.cx[a];
                o->centre_target[a] = c.cy[a];
            }
            o->rmsd = pw_sqrt(e / c.W);
            o->lambda[0] = sol[9 * count + j];
            o->lambda[1] = sol[10 * count + j];
            o->sweeps = (int)sol[11 * count + j];
            o->reserved = 0;
        }
    }
}

// Everything is checked before anything is launched or written.  The entries a call reads are found once, by a
// difference array over the rows and one over the weights, so that an all-pairs batch -- millions of jobs over a few
// thousand frames -- is checked in the time of one pass over the arrays and one over the jobs.
int sup_check(const pw_superpose_job* jobs, long n_jobs, const double* xyz, const double* weights, long n_points,
              long& r_lo, long& r_hi, long& w_lo, long& w_hi) {
    r_lo = w_lo = -1;
    r_hi = w_hi = 0;
    for (long k = 0; k < n_jobs; ++k) {
        const pw_superpose_job& J = jobs[k];
        if (J.n < 1) return stat_bad("pw_superpose", k, "n < 1");
        if (J.out < 0) return stat_bad("pw_superpose", k, "a negative row of the result");
        if (J.mobile_first < 0 || J.target_first < 0 || J.n > n_points || J.mobile_first > n_points - J.n ||
            J.target_first > n_points - J.n)
            return stat_bad("pw_superpose", k, "points outside xyz");
        if (J.weight_first < -1 || (J.weight_first >= 0 && J.weight_first > n_points - J.n))
            return stat_bad("pw_superpose", k, "weights outside the array");
        if (!xyz || (J.weight_first >= 0 && !weights)) return stat_bad("pw_superpose", k, "null array");
        const long lo = (long)(J.mobile_first < J.target_first ? J.mobile_first : J.target_first);
        const long hi = (long)(J.mobile_first < J.target_first ? J.target_first : J.mobile_first) + (long)J.n;
        if (r_lo < 0 || lo < r_lo) r_lo = lo;
        if (hi > r_hi) r_hi = hi;
        if (J.weight_first >= 0) {
            if (w_lo < 0 || (long)J.weight_first < w_lo) w_lo = (long)J.weight_first;
            if ((long)(J.weight_first + J.n) > w_hi) w_hi = (long)(J.weight_first + J.n);
        }
    }
    if (w_lo < 0) w_lo = w_hi = 0;
    // which rows and weights are read
    std::vector<int> used((size_t)(r_hi - r_lo) + 1, 0), usedw((size_t)(w_hi - w_lo) + 1, 0);
    for (long k = 0; k < n_jobs; ++k) {
        const pw_superpose_job& J = jobs[k];
        used[J.mobile_first - r_lo] += 1; used[J.mobile_first + J.n - r_lo] -= 1;
        used[J.target_first - r_lo] += 1; used[J.target_first + J.n - r_lo] -= 1;
        if (J.weight_first >= 0) { usedw[J.weight_first - w_lo] += 1; usedw[J.weight_first + J.n - w_lo] -= 1; }
    }
    long bad_row = -1, bad_w = -1;
    for (long i = 0, depth = 0; i < r_hi - r_lo && bad_row < 0; ++i) {
        depth += used[i];
        if (depth > 0) {
            const double* p = xyz + 3 * (r_lo + i);
            if (!pw_finite(p[0]) || !pw_finite(p[1]) || !pw_finite(p[2])) bad_row = r_lo + i;
        }
    }
    // positive[i]: the weights > 0 before entry i of the span
    std::vector<long> positive((size_t)(w_hi - w_lo) + 1, 0);
    for (long i = 0, depth = 0; i < w_hi - w_lo; ++i) {
        depth += usedw[i];
        const double v = weights[w_lo + i];
        if (depth > 0 && bad_w < 0 && (!pw_finite(v) || v < 0.0)) bad_w = w_lo + i;
        positive[i + 1] = positive[i] + (v > 0.0 ? 1 : 0);
    }
    if (bad_row < 0 && bad_w < 0 && w_hi == w_lo) return PW_OK;
    for (long k = 0; k < n_jobs; ++k) {
        const pw_superpose_job& J = jobs[k];
        if (bad_row >= 0 && ((bad_row >= J.mobile_first && bad_row < J.mobile_first + J.n) ||
                             (bad_row >= J.target_first && bad_row < J.target_first + J.n)))
            return stat_bad("pw_superpose", k, "a coordinate is not finite");
        if (J.weight_first < 0) continue;
        if (bad_w >= J.weight_first && bad_w < J.weight_first + J.n)
            return stat_bad("pw_superpose", k, "a weight is negative or not finite");
        if (bad_row < 0 && bad_w < 0 && positive[J.weight_first + J.n - w_lo] == positive[J.weight_first - w_lo])
            return stat_bad("pw_superpose", k, "the weights sum to 0");
    }
    return PW_OK;
}

// workspace_bytes: the budget of moments and rotations of a launch (0: SUP_WORKSPACE_BYTES); kernel_ms: when not
// null, the time of all kernels of the call by HIP events on the context's stream
int superpose(pw_context* ctx, const pw_superpose_job* jobs, int64_t n_jobs, const double* xyz, const double* weights,
              int64_t n_points, pw_superpose_out* out, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    long r_lo, r_hi, w_lo, w_hi;
    const int rc = sup_check(jobs, (long)n_jobs, xyz, weights, (long)n_points, r_lo, r_hi, w_lo, w_hi);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_superpose(jobs, (long)n_jobs, xyz, weights, out, pw_context_host_threads(ctx, 0));

    const long N = (long)n_jobs;
    std::vector<SupJobDev> dev((size_t)N);
    for (long k = 0; k < N; ++k) {
        const pw_superpose_job& J = jobs[k];
        dev[k] = SupJobDev{(long)J.mobile_first - r_lo, (long)J.target_first - r_lo,
                           J.weight_first < 0 ? -1 : (long)J.weight_first - w_lo, (long)J.n};
    }
    // jobs go through in launches of `per`: nothing of a job's row depends on the cut
    long per = (long)(workspace_bytes ? workspace_bytes : SUP_WORKSPACE_BYTES) / SUP_JOB_WORKSPACE;
    per = per < 1 ? 1 : per > N ? N : per;
    const size_t ws_bytes = (size_t)per * SUP_JOB_WORKSPACE, out_bytes = sizeof(pw_superpose_out) * (size_t)N;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        SupJobDev* d_jobs;
        double *d_x, *d_w, *d_ws;
        pw_superpose_out* d_out;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(SupJobDev) * (size_t)N));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * 3 * (size_t)(r_hi - r_lo)));
        STAT_TRY(buf.alloc(&d_w, sizeof(double) * (size_t)(w_hi - w_lo)));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(hipMemcpyAsync(d_jobs, dev.data(), sizeof(SupJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_x, xyz + 3 * r_lo, sizeof(double) * 3 * (size_t)(r_hi - r_lo), hipMemcpyHostToDevice, st));
        if (w_hi > w_lo)
            STAT_TRY(hipMemcpyAsync(d_w, weights + w_lo, sizeof(double) * (size_t)(w_hi - w_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over; all three kernels
        // stride over their jobs -- tests/test_gpu_launch_cap.py sends them round again -- and count >= 1; each launch
        // asks for its own grid, so that the test hook counts launches)
        for (long first = 0; first < N; first += per) {
            const long count = N - first < per ? N - first : per;
            const long wave_blocks = (count + SUP_WAVES - 1) / SUP_WAVES;
            hipLaunchKernelGGL(pw_superpose_moments_kernel, dim3((unsigned)launch_blocks(wave_blocks, 1l << 16)), dim3(64 * SUP_WAVES), 0, st,
                               d_jobs + first, count, d_x, d_w, d_ws);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_superpose_solve_kernel, dim3((unsigned)launch_blocks((count + 63) / 64, 1l << 16)), dim3(64), 0, st, count, d_ws);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_superpose_residual_kernel, dim3((unsigned)launch_blocks(wave_blocks, 1l << 16)), dim3(64 * SUP_WAVES), 0, st,
                               d_jobs + first, count, d_x, d_w, d_ws, d_out + first);
            STAT_TRY(hipGetLastError());
        }
        STAT_TRY(ev.stop(st));
        // (the compact result is in job order: neighbours in the caller's array come back in one copy)
        for (long k = 0; k < N;) {
            long e = k + 1;
            while (e < N && jobs[e].out == jobs[e - 1].out + 1) ++e;
            STAT_TRY(hipMemcpyAsync(out + jobs[k].out, d_out + k, sizeof(pw_superpose_out) * (size_t)(e - k),
                                   hipMemcpyDeviceToHost, st));
            k = e;
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_superpose(pw_context* ctx, const pw_superpose_job* jobs, int64_t n_jobs, const double* xyz,
                            const double* weights, int64_t n_points, pw_superpose_out* out) {
    return superpose(ctx, jobs, n_jobs, xyz, weights, n_points, out, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_superpose with the budget of the workspace given (0: the
// default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_superpose(pw_context* ctx, const pw_superpose_job* jobs, int64_t n_jobs, const double* xyz,
                                     const double* weights, int64_t n_points, pw_superpose_out* out,
                                     int64_t workspace_bytes, float* kernel_ms) {
    return superpose(ctx, jobs, n_jobs, xyz, weights, n_points, out, workspace_bytes, kernel_ms);
}
