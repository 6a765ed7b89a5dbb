// pw_charges.hip -- gfx950 kernel and the C ABI entry of charge equilibration (include/pywindow_amd.h: pw_charges;
// definition of the result in pw_charges.hpp).  One kernel, two instances.
//
// pw_charges_kernel: one workgroup of four wavefronts a job.  The job's state -- coordinates (x, y and z apart), J, and
// x, r, z, p, Ap of both systems, CHG_VECTORS = 14 doubles an atom -- lives in dynamic LDS (instance <true>, up to
// CHG_LDS_ATOMS atoms; the launch sizes it for the largest job it serves) or in the job's part of a global workspace
// (instance <false>); nothing else differs, so where the state lives cannot show.  A product y = A p: wave w owns the rows
// w, w + 4, ..., lane l is accumulator l of the row's sum and takes the columns l, l + 64, ...; A_ij is recomputed by
// chg_pair() once an element and serves the products of both systems; the fold is the butterfly of pw_superpose.hip.
// The dot products of a step are taken by all four waves redundantly, each over the whole vectors: every wave then holds
// the same alpha, beta and freeze state in scalar registers and nothing is broadcast.  The element-wise updates are shared
// out among the 256 threads; three barriers a step.  Wave 0 writes the job's charges and row.  Every loop is bounded by
// n or max_iter; no workgroup waits for another; no atomics.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_charges_dev.hpp"       // the wave folds, shared with pw_charges_cell.hip
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_charges(const pw_charges_job* jobs, long n_jobs, const double* xyz, const double* params,
                                   double* charges, pw_charges_out* out, int threads);   // pw_hostpath.cpp

static_assert(sizeof(pw_charges_job) == 72 && sizeof(pw_charges_out) == 88, "the layouts of the header");
static_assert(PW_CHG_NOT_CONVERGED == CHG_NOT_CONVERGED && PW_CHG_BREAKDOWN == CHG_BREAKDOWN && PW_CHG_NO_SUM == CHG_NO_SUM,
              "the header's flags and the kernel's");

namespace {

constexpr int CHG_WAVES = 4, CHG_THREADS = 64 * CHG_WAVES;

// a job as the kernel reads it: firsts relative to the uploaded spans and to the compact result
struct ChgJobDev {
    long xyz_first, param_first, n, max_iter;
    long state_first;              // the job's CHG_VECTORS * n doubles in the workspace of its launch, or -1: LDS
    long charge_first;             // into the compact charges of the call
    double Q, K, tol;
};

template <bool IN_LDS>
__global__ void __launch_bounds__(CHG_THREADS)
pw_charges_kernel(const ChgJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ xyz,
                  const double* __restrict__ params, double* ws, double* __restrict__ charges,
                  pw_charges_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double s_state[];
    typedef typename std::conditional<IN_LDS, int, long>::type idx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const ChgJobDev J = jobs[job];
        if ((J.state_first < 0) != IN_LDS) continue;                 // (the same in every thread: the other instance's job)
        double* base;
        if constexpr (IN_LDS) base = s_state; else base = ws + J.state_first;
        const idx n = (idx)J.n;
        double *X = base, *Y = base + n, *Z = base + 2 * n, *Jd = base + 3 * n;
        const double* gx = xyz + 3 * J.xyz_first;
        const double* gp = params + 2 * J.param_first;
        __syncthreads();                                             // (the job before is done with the LDS)
        for (idx i = tid; i < n; i += CHG_THREADS) {
            X[i] = gx[3 * i];
            Y[i] = gx[3 * i + 1];
            Z[i] = gx[3 * i + 2];
            const double Ji = gp[2 * i + 1];
            Jd[i] = Ji;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                double* V = base + (4 + 5 * s) * n;                  // x, r, z, p, Ap of system s
                const double b = s == 0 ? -gp[2 * i] : 1.0, z = b / Ji;
                V[i] = 0.0;
                V[n + i] = b;
                V[2 * n + i] = z;
                V[3 * n + i] = z;
            }
        }
        __syncthreads();
        ChgSystem sys[2];                                            // (indexed by unrolled loops only: registers)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double* r = base + (5 + 5 * s) * n;
            sys[s].rz = chg_dot(r, r + n, n, lane);
            sys[s].rr = sys[s].bb = chg_dot(r, r, n, lane);
            sys[s].iterations = 0;
            sys[s].frozen = sys[s].broke = false;
        }
        const double K = J.K, tol2 = J.tol * J.tol;
        const int max_iter = (int)J.max_iter;
        bool ran_out = false;
        for (int k = 0;; ++k) {
            chg_freeze_check(sys[0], tol2, k);
            chg_freeze_check(sys[1], tol2, k);
            if (sys[0].frozen && sys[1].frozen) break;
            if (k == max_iter) {
                ran_out = true;
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (!sys[s].frozen) sys[s].iterations = k;
                break;
            }
            {
                const bool on0 = !sys[0].frozen, on1 = !sys[1].frozen;
                const double *p0 = base + 7 * n, *p1 = base + 12 * n;
                double *Ap0 = base + 8 * n, *Ap1 = base + 13 * n;
                for (idx i = wave; i < n; i += CHG_WAVES) {
                    const double xi = X[i], yi = Y[i], zi = Z[i], Ji = Jd[i];
                    double a0 = 0.0, a1 = 0.0;
                    for (idx c = lane; c < n; c += SUP_ACC) {
                        const double pair = chg_pair(xi, yi, zi, Ji, X[c], Y[c], Z[c], Jd[c], K);
                        const double a = c == i ? Ji : pair;
                        if (on0) a0 = pw_fma(a, p0[c], a0);
                        if (on1) a1 = pw_fma(a, p1[c], a1);
                    }
                    if (on0) {
                        a0 = chg_wave_fold(a0);
                        if (lane == 0) Ap0[i] = a0;
                    }
                    if (on1) {
                        a1 = chg_wave_fold(a1);
                        if (lane == 0) Ap1[i] = a1;
                    }
                }
            }
            __syncthreads();
            double alpha[2] = {0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (sys[s].frozen) continue;
                const double* p = base + (7 + 5 * s) * n;
                const double pAp = chg_dot(p, p + n, n, lane);
                if (chg_curvature_ok(sys[s], pAp, k)) alpha[s] = sys[s].rz / pAp;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (sys[s].frozen) continue;
                double* V = base + (4 + 5 * s) * n;
                const double al = alpha[s];
                for (idx i = tid; i < n; i += CHG_THREADS) {
                    V[i] = pw_fma(al, V[3 * n + i], V[i]);
                    const double r = pw_fma(-al, V[4 * n + i], V[n + i]);
                    V[n + i] = r;
                    V[2 * n + i] = r / Jd[i];
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (sys[s].frozen) continue;
                double* V = base + (4 + 5 * s) * n;
                const double rz_new = chg_dot(V + n, V + 2 * n, n, lane);
                sys[s].rr = chg_dot(V + n, V + n, n, lane);
                const double beta = rz_new / sys[s].rz;
                for (idx i = tid; i < n; i += CHG_THREADS) V[3 * n + i] = pw_fma(beta, V[3 * n + i], V[2 * n + i]);
                sys[s].rz = rz_new;
            }
            __syncthreads();
        }
        if (wave != 0) continue;                                     // (the barrier at the top keeps the state until wave 0 is done)
        const double *sv = base + 4 * n, *tv = base + 9 * n;
        double as = 0.0, at = 0.0;
        for (idx i = lane; i < n; i += SUP_ACC) {
            as = as + sv[i];
            at = at + tv[i];
        }
        const double S = chg_uniform(chg_wave_fold(as)), T = chg_uniform(chg_wave_fold(at));
        const int flags = chg_flags(sys[0], sys[1], ran_out, T);
        const bool lost = (flags & (CHG_BREAKDOWN | CHG_NO_SUM)) != 0;
        const double Q = J.Q, mu = (Q - S) / T, nan = chg_nan();
        double e = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, lo = PW_INF, hi = -PW_INF;
        double* q = charges + J.charge_first;
        for (idx i = lane; i < n; i += SUP_ACC) {
            const double qi = pw_fma(mu, tv[i], sv[i]);
            e = pw_fma(gp[2 * i], qi, e);
            d0 = pw_fma(qi, X[i], d0);
            d1 = pw_fma(qi, Y[i], d1);
            d2 = pw_fma(qi, Z[i], d2);
            lo = qi < lo ? qi : lo;
            hi = qi > hi ? qi : hi;
            q[i] = lost ? nan : chg_canon(qi);
        }
        e = chg_wave_fold(e);
        d0 = chg_wave_fold(d0);
        d1 = chg_wave_fold(d1);
        d2 = chg_wave_fold(d2);
        lo = chg_wave_extreme<true>(lo);
        hi = chg_wave_extreme<false>(hi);
        if (lane == 0) {
            pw_charges_out* o = out + job;
            o->mu = lost ? nan : chg_canon(mu);
            o->sum_s = chg_canon(S);
            o->sum_t = chg_canon(T);
            o->energy = lost ? nan : chg_canon(0.5 * (e + mu * Q));
            o->dipole[0] = lost ? nan : chg_canon(d0);
            o->dipole[1] = lost ? nan : chg_canon(d1);
            o->dipole[2] = lost ? nan : chg_canon(d2);
            o->q_min = lost ? nan : chg_canon(lo);
            o->q_max = lost ? nan : chg_canon(hi);
            o->iterations[0] = sys[0].iterations;
            o->iterations[1] = sys[1].iterations;
            o->flags = flags;
            o->reserved = 0;
        }
    }
}

const char* const ENTRY = "pw_charges";
int chg_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written
int chg_check(const pw_charges_job* jobs, long n_jobs, const double* xyz, const double* params, long n_points,
              const double* charges) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_charges_job& J = jobs[k];
        if (J.n < 1) return chg_bad(k, "n < 1");
        if (span_outside((long)J.xyz_first, (long)J.n, n_points)) return chg_bad(k, "atoms outside xyz");
        if (span_outside((long)J.param_first, (long)J.n, n_points)) return chg_bad(k, "parameters outside params");
        if (span_outside((long)J.charge_first, (long)J.n, n_points)) return chg_bad(k, "the entries are outside charges");
        if (J.out < 0) return chg_bad(k, "a negative row of the result");
        if (!xyz || !params || !charges) return chg_bad(k, "null array");
        if (!pw_finite(J.total_charge)) return chg_bad(k, "total_charge is not finite");
        if (!pw_finite(J.coulomb)) return chg_bad(k, "coulomb is not finite");
        if (!(J.coulomb > 0.0)) return chg_bad(k, "coulomb <= 0");
        if (!(J.tol >= CHG_TOL_MIN && J.tol <= CHG_TOL_MAX)) return chg_bad(k, "tol outside 1e-14 .. 1e-2");
        if (J.max_iter < 1 || J.max_iter > CHG_MAX_ITER) return chg_bad(k, "max_iter outside 1 .. 100000");
        GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, (long)J.xyz_first, (long)J.n));
        for (long i = (long)J.param_first; i < (long)(J.param_first + J.n); ++i) {
            if (!pw_finite(params[2 * i])) return chg_bad(k, "chi is not finite");
            if (!pw_finite(params[2 * i + 1])) return chg_bad(k, "J is not finite");
            if (!(params[2 * i + 1] > 0.0)) return chg_bad(k, "J <= 0");
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    return shared_output(ENTRY, n_jobs, "shares entries of charges with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].charge_first, (long)jobs[k].n}; });
}

// workspace_bytes: the budget of the state of the jobs of one launch that are too large for LDS (0:
// CHG_WORKSPACE_BYTES; at 1 every job is a launch of its own); kernel_ms: when not null, the time of the kernels of the
// call by HIP events on the context's stream
int charges_call(pw_context* ctx, const pw_charges_job* jobs, int64_t n_jobs, const double* xyz, const double* params,
                 int64_t n_points, double* charges, pw_charges_out* out, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = chg_check(jobs, N, xyz, params, (long)n_points, charges);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_charges(jobs, N, xyz, params, charges, out, pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while the state of
    // those that do not fit LDS fits the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : CHG_WORKSPACE_BYTES) / 8;
    Span atoms, rows;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].xyz_first, (long)jobs[k].n);
        rows.widen((long)jobs[k].param_first, (long)jobs[k].n);
    }
    std::vector<ChgJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long n_charges = 0;
    for (long k = 0; k < N; ++k) {
        const pw_charges_job& J = jobs[k];
        const bool in_lds = J.n <= CHG_LDS_ATOMS;
        const long need = in_lds ? 0 : CHG_VECTORS * (long)J.n;
        place(groups, cur, budget_words, need + 1);                  // (a word more a job: no job is free)
        ChgJobDev& D = devs[k];
        D.xyz_first = atoms.rel((long)J.xyz_first, (long)J.n);
        D.param_first = rows.rel((long)J.param_first, (long)J.n);
        D.n = (long)J.n;
        D.max_iter = (long)J.max_iter;
        D.state_first = in_lds ? -1 : cur.words;
        D.charge_first = n_charges;
        D.Q = J.total_charge; D.K = J.coulomb; D.tol = J.tol;
        n_charges += (long)J.n;
        cur.words += need; cur.cost += need + 1; cur.last += 1;
    }
    groups.push_back(cur);

    // the compact result of the call: the rows of out in job order, then the charges
    const size_t out_bytes = sizeof(pw_charges_out) * (size_t)N, res_bytes = out_bytes + sizeof(double) * (size_t)n_charges,
                 ws_bytes = sizeof(double) * (size_t)most_words(groups);
    std::vector<unsigned char> res(res_bytes);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        ChgJobDev* d_jobs;
        double *d_xyz, *d_params, *d_ws;
        unsigned char* d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(ChgJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(ChgJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows.upload(buf, &d_params, params, 2));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        pw_charges_out* d_out = (pw_charges_out*)d_res;
        double* d_charges = (double*)(d_res + out_bytes);
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over)
        for (const LaunchGroup& G : groups) {
            const long n_group = G.last - G.first;
            long lds_atoms = 0;
            bool any_global = false;
            for (long k = G.first; k < G.last; ++k) {
                if (devs[k].state_first < 0) lds_atoms = devs[k].n > lds_atoms ? devs[k].n : lds_atoms;
                else any_global = true;
            }
            if (lds_atoms) {
                hipLaunchKernelGGL(pw_charges_kernel<true>, dim3((unsigned)launch_blocks(n_group, 65536)), dim3(CHG_THREADS),
                                   sizeof(double) * CHG_VECTORS * (size_t)lds_atoms, st, d_jobs + G.first, (int)n_group, d_xyz,
                                   d_params, d_ws, d_charges, d_out + G.first);
                STAT_TRY(hipGetLastError());
            }
            if (any_global) {
                hipLaunchKernelGGL(pw_charges_kernel<false>, dim3((unsigned)launch_blocks(n_group, 65536)), dim3(CHG_THREADS), 0, st, d_jobs + G.first,
                                   (int)n_group, d_xyz, d_params, d_ws, d_charges, d_out + G.first);
                STAT_TRY(hipGetLastError());
            }
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's arrays, job by job
    const pw_charges_out* r_out = (const pw_charges_out*)res.data();
    const double* r_charges = (const double*)(res.data() + out_bytes);
    for (long k = 0; k < N; ++k) {
        out[jobs[k].out] = r_out[k];
        memcpy(charges + jobs[k].charge_first, r_charges + devs[k].charge_first, sizeof(double) * (size_t)jobs[k].n);
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_charges(pw_context* ctx, const pw_charges_job* jobs, int64_t n_jobs, const double* xyz, const double* params,
                          int64_t n_points, double* charges, pw_charges_out* out) {
    return charges_call(ctx, jobs, n_jobs, xyz, params, n_points, charges, out, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_charges with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_charges(pw_context* ctx, const pw_charges_job* jobs, int64_t n_jobs, const double* xyz,
                                   const double* params, int64_t n_points, double* charges, pw_charges_out* out,
                                   int64_t workspace_bytes, float* kernel_ms) {
    return charges_call(ctx, jobs, n_jobs, xyz, params, n_points, charges, out, workspace_bytes, kernel_ms);
}
