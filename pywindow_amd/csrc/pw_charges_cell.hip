// pw_charges_cell.hip -- gfx950 kernels and the C ABI entry of charge equilibration on a periodic cell
// (include/pywindow_amd.h: pw_charges_cell; definition of the result in pw_charges_cell.hpp).  Three kernels.
//
// chc_count_kernel: a wave a row of R; the candidates (j, m) of row i go through the wave 64 at a time in index order and
// the counting ones are counted by __ballot.  The host reads the counts back, lays the rows of every job out in the
// workspace of its launch and cuts the jobs into launches by the budget.
// chc_rows_kernel (phase one): the same walk, now compacting: a counting candidate's place in the row is the count so far
// plus the counting lanes below it, so the row is in index order whatever the geometry; its value (chc_term, the only
// pw_erfc of the call) and column go to the workspace.  The same launch fills the per-atom per-axis phase tables.
// chc_solve_kernel (phase two): one workgroup of eight wavefronts a job, pw_charges_kernel's shape.  The six vectors live in
// dynamic LDS (instance <true>, up to CHC_LDS_ATOMS atoms) or in the workspace (instance <false>); nothing else differs.  A
// product: the structure factors are summed a wave a row of k, lane l accumulator l over the atoms; then wave w owns the
// rows w, w + 8, ... of the matrix, lane l accumulator l of the row's list and then of the sum over k.  The scalars of a
// step are taken by all waves redundantly, so every wave holds the same state and nothing is broadcast.  Every loop is
// bounded by n, n_k, 27 n or max_iter; no workgroup waits for another; no atomics, no MFMA.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_charges_cell.hpp"
#include "pw_charges_dev.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_charges_cell(const pw_charges_cell_job* jobs, long n_jobs, const double* xyz, const double* params,
                                        const double* kvecs, double* charges, pw_charges_cell_out* out,
                                        int threads);   // pw_hostpath.cpp

static_assert(sizeof(pw_charges_cell_job) == 160 && sizeof(pw_charges_cell_out) == 40, "the layouts of the header");
static_assert(PW_EWALD_MAX_K == EWALD_MAX_K && PW_EWALD_MAX_INDEX == EWALD_MAX_INDEX, "the header's caps and the kernel's");

namespace {

constexpr int CHC_ROW_WAVES = 4, CHC_ROW_THREADS = 64 * CHC_ROW_WAVES;
constexpr int CHC_WAVES = 8, CHC_THREADS = 64 * CHC_WAVES;
constexpr int CHC_ROW_CHUNKS = 64;                    // workgroups a job of the count and rows kernels, at most
constexpr long CHC_MAX_ATOMS = 0x7fffffffl / CHC_IMAGES;   // 27 n is an int

// a job as the kernels read it: firsts relative to the uploaded spans, to the workspace of the launch (8-byte words) and to
// the compact result
struct ChcJobDev {
    long xyz_first, param_first, k_first, n, n_k, max_iter;
    long atom_first;               // the job's atoms among all atoms of the call: its entries of counts and firsts
    long value_first, column_first, table_first, factor_first;
    long state_first;              // the job's CHC_VECTORS * n doubles, or -1: LDS
    long charge_first;
    double e[6], K, alpha, cutoff2, on2, off2, tol;
    ChcTables T;
};

// the walk of row i: FILL false counts, true writes value and column in index order.  Returns the count (in every lane)
template <bool FILL>
__device__ inline int chc_row_walk(const ChcJobDev& J, const double* __restrict__ gx, const double* __restrict__ gp, int i,
                                   int lane, double* __restrict__ value, int* __restrict__ column) {
    const int n = (int)J.n, candidates = CHC_IMAGES * n;
    const double xi = gx[3 * i], yi = gx[3 * i + 1], zi = gx[3 * i + 2];
    const double Ji = FILL ? gp[2 * i + 1] : 0.0;
    int count = 0;
    for (int base = 0; base < candidates; base += 64) {
        const int c = base + lane;
        bool counts = false;
        int j = 0;
        double r2 = 0.0;
        if (c < candidates) {
            j = c / CHC_IMAGES;
            const int m = c - CHC_IMAGES * j;
            double tx, ty, tz;
            chc_shift(J.e, m, &tx, &ty, &tz);
            r2 = chc_r2(xi, yi, zi, gx[3 * j], gx[3 * j + 1], gx[3 * j + 2], tx, ty, tz);
            counts = !(j == i && m == CHC_SELF_IMAGE) && r2 <= J.cutoff2;
        }
        const unsigned long long mask = __ballot(counts);
        if constexpr (FILL) {
            if (counts) {
                const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
                value[at] = chc_term(r2, Ji, gp[2 * j + 1], J.K, J.alpha, J.on2, J.off2);
                column[at] = j;
            }
        }
        count += __popcll(mask);
    }
    return count;
}

__global__ void __launch_bounds__(CHC_ROW_THREADS)
chc_count_kernel(const ChcJobDev* __restrict__ jobs, const double* __restrict__ xyz, int* __restrict__ counts) {
    const ChcJobDev J = jobs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = (int)J.n;
    const double* gx = xyz + 3 * J.xyz_first;
    for (int i = blockIdx.y * CHC_ROW_WAVES + wave; i < n; i += gridDim.y * CHC_ROW_WAVES) {
        const int count = chc_row_walk<false>(J, gx, nullptr, i, lane, nullptr, nullptr);
        if (lane == 0) counts[J.atom_first + i] = count;
    }
}

__global__ void __launch_bounds__(CHC_ROW_THREADS)
chc_rows_kernel(const ChcJobDev* __restrict__ jobs, const double* __restrict__ xyz, const double* __restrict__ params,
                const long* __restrict__ firsts, double* __restrict__ ws) {
    const ChcJobDev J = jobs[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = (int)J.n;
    const double* gx = xyz + 3 * J.xyz_first;
    const double* gp = params + 2 * J.param_first;
    double* value = ws + J.value_first;
    int* column = (int*)(ws + J.column_first);
    for (int i = blockIdx.y * CHC_ROW_WAVES + wave; i < n; i += gridDim.y * CHC_ROW_WAVES) {
        const long first = firsts[J.atom_first + i];
        chc_row_walk<true>(J, gx, gp, i, lane, value + first, column + first);
    }
    // the tables: entry (a, m, j), axis by axis (unrolled: the axis is a constant wherever it indexes the job's arrays)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double* tab = ws + J.table_first + J.T.first[a];
        const long entries = (long)(J.T.top[a] + 1) * n;
        for (long t = (long)blockIdx.y * CHC_ROW_THREADS + threadIdx.x; t < entries; t += (long)gridDim.y * CHC_ROW_THREADS) {
            const int m = (int)(t / n), j = (int)(t - (long)m * n);
            const EwaldCS v = ewald_sincos(ewald_dot(chc_axis_kvec(J.e, a, m), gx[3 * j], gx[3 * j + 1], gx[3 * j + 2]));
            tab[2l * m * n + j] = v.c;
            tab[2l * m * n + n + j] = v.s;
        }
    }
}

// lambda of the residual r: every wave takes the whole sum
template <class I>
__device__ inline double chc_lambda(const double* r, const double* Jd, I n, int lane, double sJ) {
    double acc = 0.0;
    for (I i = lane; i < n; i += SUP_ACC) acc = acc + r[i] / Jd[i];
    return chg_uniform(chg_wave_fold(acc)) / sJ;
}

// r.z with the residual's constant part taken out (pw_charges_cell.hpp, SOLVER)
template <class I>
__device__ inline double chc_projected_dot(const double* r, const double* z, I n, int lane, double lambda) {
    double acc = 0.0;
    for (I i = lane; i < n; i += SUP_ACC) acc = pw_fma(r[i] - lambda, z[i], acc);
    return chg_uniform(chg_wave_fold(acc));
}

template <bool IN_LDS>
__global__ void __launch_bounds__(CHC_THREADS)
chc_solve_kernel(const ChcJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ params,
                 const double* __restrict__ kvecs, const long* __restrict__ firsts, const int* __restrict__ counts, double* ws,
                 double* __restrict__ charges, pw_charges_cell_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double s_state[];
    typedef typename std::conditional<IN_LDS, int, long>::type idx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const ChcJobDev J = jobs[job];
        if ((J.state_first < 0) != IN_LDS) continue;                 // (the same in every thread: the other instance's job)
        double* base;
        if constexpr (IN_LDS) base = s_state; else base = ws + J.state_first;
        const idx n = (idx)J.n;
        const int nk = (int)J.n_k;
        double *q = base, *r = base + n, *z = base + 2 * n, *p = base + 3 * n, *y = base + 4 * n, *Jd = base + 5 * n;
        const double* gp = params + 2 * J.param_first;
        const double* kv = kvecs + 4 * J.k_first;
        const double* value = ws + J.value_first;
        const int* column = (const int*)(ws + J.column_first);
        const double* tab = ws + J.table_first;
        double* factor = ws + J.factor_first;                        // Sc, then Ss
        const long* first = firsts + J.atom_first;
        const int* count = counts + J.atom_first;
        __syncthreads();                                             // (the job before is done with the LDS)
        for (idx i = tid; i < n; i += CHC_THREADS) {
            Jd[i] = gp[2 * i + 1];
            q[i] = 0.0;
            r[i] = -gp[2 * i];
        }
        __syncthreads();
        double sJ;
        {
            double acc = 0.0;
            for (idx i = lane; i < n; i += SUP_ACC) acc = acc + 1.0 / Jd[i];
            sJ = chg_uniform(chg_wave_fold(acc));
        }
        ChcState S;
        S.lambda = chc_lambda(r, Jd, n, lane, sJ);
        for (idx i = tid; i < n; i += CHC_THREADS) {
            const double zi = r[i] / Jd[i] - S.lambda / Jd[i];
            z[i] = zi;
            p[i] = zi;
        }
        __syncthreads();
        S.rz = S.rz0 = chc_projected_dot(r, z, n, lane, S.lambda);
        S.iterations = 0;
        S.ran_out = S.broke = false;
        const double tol2 = J.tol * J.tol, self = chc_self(J.K, J.alpha);
        const int max_iter = (int)J.max_iter;
        for (int k = 0;; ++k) {
            S.iterations = k;
            if (S.rz <= tol2 * S.rz0) break;
            if (k == max_iter) {
                S.ran_out = true;
                break;
            }
            for (int kr = wave; kr < nk; kr += CHC_WAVES) {
                const int hh = (int)kv[4 * kr], kk = (int)kv[4 * kr + 1], ll = (int)kv[4 * kr + 2];
                double ac = 0.0, as = 0.0;
                for (idx j = lane; j < n; j += SUP_ACC) {
                    const EwaldCS ph = chc_phase(tab, J.T, n, j, hh, kk, ll);
                    ac = pw_fma(p[j], ph.c, ac);
                    as = pw_fma(p[j], ph.s, as);
                }
                ac = chg_wave_fold(ac);
                as = chg_wave_fold(as);
                if (lane == 0) {
                    factor[kr] = ac;
                    factor[nk + kr] = as;
                }
            }
            __syncthreads();
            for (idx i = wave; i < n; i += CHC_WAVES) {
                const double* v = value + first[i];
                const int* c = column + first[i];
                const int entries = count[i];
                double real = 0.0, rec = 0.0;
                for (int e = lane; e < entries; e += SUP_ACC) real = pw_fma(v[e], p[c[e]], real);
                for (int kr = lane; kr < nk; kr += SUP_ACC) {
                    const EwaldCS ph = chc_phase(tab, J.T, n, i, (int)kv[4 * kr], (int)kv[4 * kr + 1], (int)kv[4 * kr + 2]);
                    rec = pw_fma(kv[4 * kr + 3], chc_rec_term(ph, factor[kr], factor[nk + kr]), rec);
                }
                real = chg_wave_fold(real);
                rec = chg_wave_fold(rec);
                if (lane == 0) y[i] = ((Jd[i] - self) * p[i] + real) + rec;
            }
            __syncthreads();
            const double pAp = chg_dot(p, y, n, lane);
            if (!(pAp > 0.0)) {
                S.broke = true;
                break;
            }
            const double al = S.rz / pAp;
            for (idx i = tid; i < n; i += CHC_THREADS) {
                q[i] = pw_fma(al, p[i], q[i]);
                r[i] = pw_fma(-al, y[i], r[i]);
            }
            __syncthreads();
            S.lambda = chc_lambda(r, Jd, n, lane, sJ);
            for (idx i = tid; i < n; i += CHC_THREADS) z[i] = r[i] / Jd[i] - S.lambda / Jd[i];
            __syncthreads();
            const double rz_new = chc_projected_dot(r, z, n, lane, S.lambda);
            const double beta = rz_new / S.rz;
            for (idx i = tid; i < n; i += CHC_THREADS) p[i] = pw_fma(beta, p[i], z[i]);
            S.rz = rz_new;
            __syncthreads();
        }
        if (wave != 0) continue;                                     // (the barrier at the top keeps the state until wave 0 is done)
        const int flags = chc_flags(S, sJ);
        const bool lost = (flags & (CHG_BREAKDOWN | CHG_NO_SUM)) != 0;
        const double nan = chg_nan();
        double e = 0.0, lo = PW_INF, hi = -PW_INF;
        double* Q = charges + J.charge_first;
        for (idx i = lane; i < n; i += SUP_ACC) {
            const double qi = q[i];
            e = pw_fma(gp[2 * i], qi, e);
            lo = qi < lo ? qi : lo;
            hi = qi > hi ? qi : hi;
            Q[i] = lost ? nan : chg_canon(qi);
        }
        e = chg_wave_fold(e);
        lo = chg_wave_extreme<true>(lo);
        hi = chg_wave_extreme<false>(hi);
        if (lane == 0) {
            pw_charges_cell_out* o = out + job;
            o->mu = lost ? nan : chg_canon(-S.lambda);
            o->energy = lost ? nan : chg_canon(0.5 * e);
            o->q_min = lost ? nan : chg_canon(lo);
            o->q_max = lost ? nan : chg_canon(hi);
            o->iterations = S.iterations;
            o->flags = flags;
        }
    }
}

const char* const ENTRY = "pw_charges_cell";
int chc_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written
int chc_check(const pw_charges_cell_job* jobs, long n_jobs, const double* xyz, const double* params, long n_points,
              const double* kvecs, long n_kvecs, const double* charges) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_charges_cell_job& J = jobs[k];
        if (J.n < 1) return chc_bad(k, "n < 1");
        if (J.n > CHC_MAX_ATOMS) return chc_bad(k, "n is above (2^31 - 1) / 27");
        if (span_outside((long)J.xyz_first, (long)J.n, n_points)) return chc_bad(k, "atoms outside xyz");
        if (span_outside((long)J.param_first, (long)J.n, n_points)) return chc_bad(k, "parameters outside params");
        if (span_outside((long)J.charge_first, (long)J.n, n_points)) return chc_bad(k, "the entries are outside charges");
        if (J.out < 0) return chc_bad(k, "a negative row of the result");
        if (J.n_k < 0 || J.n_k > EWALD_MAX_K) return chc_bad(k, "n_k outside 0 .. PW_EWALD_MAX_K (4096)");
        if (span_outside((long)J.k_first, (long)J.n_k, n_kvecs)) return chc_bad(k, "rows outside kvecs");
        if (!xyz || !params || !charges || (J.n_k && !kvecs)) return chc_bad(k, "null array");
        for (int a = 0; a < 6; ++a)
            if (!pw_finite(J.edges[a])) return chc_bad(k, "an edge is not finite");
        if (!(J.edges[0] > 0.0 && J.edges[2] > 0.0 && J.edges[5] > 0.0)) return chc_bad(k, "a1, b2 or c3 is not positive");
        if (!pw_finite(J.coulomb)) return chc_bad(k, "coulomb is not finite");
        if (!(J.coulomb > 0.0)) return chc_bad(k, "coulomb <= 0");
        if (!pw_finite(J.alpha)) return chc_bad(k, "alpha is not finite");
        if (J.alpha < 0.0) return chc_bad(k, "alpha < 0");
        if (!pw_finite(J.cutoff2)) return chc_bad(k, "cutoff2 is not finite");
        if (!(J.cutoff2 > 0.0)) return chc_bad(k, "cutoff2 <= 0");
        if (!pw_finite(J.shield_on2) || !pw_finite(J.shield_off2)) return chc_bad(k, "the switch is not finite");
        if (J.shield_on2 < 0.0) return chc_bad(k, "shield_on2 < 0");
        if (!(J.shield_on2 < J.shield_off2)) return chc_bad(k, "shield_on2 >= shield_off2");
        if (J.shield_off2 > J.cutoff2) return chc_bad(k, "shield_off2 > cutoff2");
        if (!(J.tol >= CHG_TOL_MIN && J.tol <= CHG_TOL_MAX)) return chc_bad(k, "tol outside 1e-14 .. 1e-2");
        if (J.max_iter < 1 || J.max_iter > CHG_MAX_ITER) return chc_bad(k, "max_iter outside 1 .. 100000");
        GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, (long)J.xyz_first, (long)J.n));
        for (long i = (long)J.param_first; i < (long)(J.param_first + J.n); ++i) {
            if (!pw_finite(params[2 * i])) return chc_bad(k, "chi is not finite");
            if (!pw_finite(params[2 * i + 1])) return chc_bad(k, "J is not finite");
            if (!(params[2 * i + 1] > 0.0)) return chc_bad(k, "J <= 0");
        }
        for (long r = (long)J.k_first; r < (long)(J.k_first + J.n_k); ++r) {
            const double* kv = kvecs + 4 * r;
            for (int a = 0; a < 3; ++a)
                if (!pw_finite(kv[a]) || pw_abs(kv[a]) > (double)EWALD_MAX_INDEX || kv[a] != (double)(int)kv[a])
                    return chc_bad(k, "an index of a row is not an integer within -PW_EWALD_MAX_INDEX .. PW_EWALD_MAX_INDEX (64)");
            if (!pw_finite(kv[3])) return chc_bad(k, "a weight is not finite");
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    return shared_output(ENTRY, n_jobs, "shares entries of charges with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].charge_first, (long)jobs[k].n}; });
}

unsigned chc_chunks(long n) {
    const long rows = (n + CHC_ROW_WAVES - 1) / CHC_ROW_WAVES;
    return (unsigned)(rows < CHC_ROW_CHUNKS ? rows : CHC_ROW_CHUNKS);
}

// workspace_bytes: the budget of the rows, tables, structure factors and (beyond LDS) vectors of the jobs of one launch
// (0: CHC_WORKSPACE_BYTES; at 1 every job is a launch of its own); times: when not null, three floats, the count kernel,
// the rows kernels and the solver kernels of the call in ms by HIP events on the context's stream
int charges_cell_call(pw_context* ctx, const pw_charges_cell_job* jobs, int64_t n_jobs, const double* xyz, const double* params,
                      int64_t n_points, const double* kvecs, int64_t n_kvecs, double* charges, pw_charges_cell_out* out,
                      int64_t workspace_bytes, float* times) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_kvecs < 0 ||
        workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (times) times[0] = times[1] = times[2] = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = chc_check(jobs, N, xyz, params, (long)n_points, kvecs, (long)n_kvecs, charges);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_charges_cell(jobs, N, xyz, params, kvecs, charges, out, pw_context_host_threads(ctx, 0));

    const long budget_words = (workspace_bytes ? (long)workspace_bytes : CHC_WORKSPACE_BYTES) / 8;
    Span atoms, rows, waves;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].xyz_first, (long)jobs[k].n);
        rows.widen((long)jobs[k].param_first, (long)jobs[k].n);
        waves.widen((long)jobs[k].k_first, (long)jobs[k].n_k);
    }
    std::vector<ChcJobDev> devs((size_t)N);
    long n_atoms = 0, n_largest = 0;
    for (long k = 0; k < N; ++k) {
        const pw_charges_cell_job& J = jobs[k];
        ChcJobDev& D = devs[k];
        D.xyz_first = atoms.rel((long)J.xyz_first, (long)J.n);
        D.param_first = rows.rel((long)J.param_first, (long)J.n);
        D.k_first = waves.rel((long)J.k_first, (long)J.n_k);
        D.n = (long)J.n;
        D.n_k = (long)J.n_k;
        D.max_iter = (long)J.max_iter;
        D.atom_first = n_atoms;
        D.charge_first = n_atoms;
        D.value_first = D.column_first = D.table_first = D.factor_first = 0;
        D.state_first = -1;
        for (int a = 0; a < 6; ++a) D.e[a] = J.edges[a];
        D.K = J.coulomb; D.alpha = J.alpha; D.cutoff2 = J.cutoff2; D.on2 = J.shield_on2; D.off2 = J.shield_off2; D.tol = J.tol;
        D.T.top[0] = D.T.top[1] = D.T.top[2] = 0;
        for (long r = (long)J.k_first; r < (long)(J.k_first + J.n_k); ++r)
            for (int a = 0; a < 3; ++a) {
                const int v = (int)kvecs[4 * r + a], mag = v < 0 ? -v : v;
                D.T.top[a] = mag > D.T.top[a] ? mag : D.T.top[a];
            }
        chc_tables_layout(D.T, D.n);
        n_atoms += D.n;
        n_largest = D.n > n_largest ? D.n : n_largest;
    }

    const size_t jobs_bytes = sizeof(ChcJobDev) * (size_t)N, out_bytes = sizeof(pw_charges_cell_out) * (size_t)N,
                 res_bytes = out_bytes + sizeof(double) * (size_t)n_atoms;
    std::vector<unsigned char> res(res_bytes);
    std::vector<int> counts((size_t)n_atoms);
    std::vector<long> firsts((size_t)n_atoms);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev_count(times), ev_rows(times), ev_solve(times);
    STAT_TRY(ev_count.create());
    STAT_TRY(ev_rows.create());
    STAT_TRY(ev_solve.create());
    float ms_count = 0.0f, ms_rows = 0.0f, ms_solve = 0.0f;
    ev_count.ms = times ? &ms_count : nullptr;
    ev_rows.ms = times ? &ms_rows : nullptr;
    ev_solve.ms = times ? &ms_solve : nullptr;
    {
        StreamBuffers buf(st);
        ChcJobDev* d_jobs;
        double *d_xyz, *d_params, *d_kvecs, *d_ws;
        int* d_counts;
        long* d_firsts;
        unsigned char* d_res;
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(buf.alloc(&d_jobs, jobs_bytes));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), jobs_bytes, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows.upload(buf, &d_params, params, 2));
        STAT_TRY(waves.upload(buf, &d_kvecs, kvecs, 4));
        STAT_TRY(buf.alloc(&d_counts, sizeof(int) * (size_t)n_atoms));
        STAT_TRY(buf.alloc(&d_firsts, sizeof(long) * (size_t)n_atoms));
        STAT_TRY(poison_scratch(poison, d_counts, sizeof(int) * (size_t)n_atoms, st));

        // the counts of every row, and from them the plan: jobs in order, gathered into launches while what they keep in
        // the workspace fits the budget
        STAT_TRY(ev_count.start(st));
        hipLaunchKernelGGL(chc_count_kernel, dim3((unsigned)N, chc_chunks(n_largest)), dim3(CHC_ROW_THREADS), 0, st, d_jobs, d_xyz,
                           d_counts);
        STAT_TRY(hipGetLastError());
        STAT_TRY(ev_count.stop(st));
        STAT_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * (size_t)n_atoms, hipMemcpyDeviceToHost, st));
        STAT_TRY(hipStreamSynchronize(st));
        STAT_TRY(ev_count.read());
        std::vector<LaunchGroup> groups;
        LaunchGroup cur;
        for (long k = 0; k < N; ++k) {
            ChcJobDev& D = devs[k];
            long entries = 0;
            for (long i = 0; i < D.n; ++i) {
                firsts[(size_t)(D.atom_first + i)] = entries;
                entries += counts[(size_t)(D.atom_first + i)];
            }
            const bool in_lds = D.n <= CHC_LDS_ATOMS;
            const long need = entries + (entries + 1) / 2 + chc_table_words(D.T.top, D.n) + 2 * D.n_k + (in_lds ? 0 : CHC_VECTORS * D.n);
            place(groups, cur, budget_words, need + 1);              // (a word more a job: no job is free)
            D.value_first = cur.words;
            D.column_first = D.value_first + entries;
            D.table_first = D.column_first + (entries + 1) / 2;
            D.factor_first = D.table_first + chc_table_words(D.T.top, D.n);
            D.state_first = in_lds ? -1 : D.factor_first + 2 * D.n_k;
            cur.words += need; cur.cost += need + 1; cur.last += 1;
        }
        groups.push_back(cur);
        const size_t ws_bytes = sizeof(double) * (size_t)most_words(groups);
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), jobs_bytes, hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_firsts, firsts.data(), sizeof(long) * (size_t)n_atoms, hipMemcpyHostToDevice, st));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        pw_charges_cell_out* d_out = (pw_charges_cell_out*)d_res;
        double* d_charges = (double*)(d_res + out_bytes);
        STAT_TRY(hipFuncSetAttribute((const void*)chc_solve_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(double) * CHC_VECTORS * CHC_LDS_ATOMS)));
        // (launches follow one another on the stream, so the next one may take the workspace over)
        for (const LaunchGroup& G : groups) {
            const long n_group = G.last - G.first;
            long lds_atoms = 0, most = 0;
            bool any_global = false;
            for (long k = G.first; k < G.last; ++k) {
                most = devs[k].n > most ? devs[k].n : most;
                if (devs[k].state_first < 0) lds_atoms = devs[k].n > lds_atoms ? devs[k].n : lds_atoms;
                else any_global = true;
            }
            if (times) STAT_TRY(hipEventRecord(ev_rows.a, st));
            hipLaunchKernelGGL(chc_rows_kernel, dim3((unsigned)n_group, chc_chunks(most)), dim3(CHC_ROW_THREADS), 0, st,
                               d_jobs + G.first, d_xyz, d_params, d_firsts, d_ws);
            STAT_TRY(hipGetLastError());
            if (times) {
                STAT_TRY(hipEventRecord(ev_rows.b, st));
                STAT_TRY(hipEventRecord(ev_solve.a, st));
            }
            if (lds_atoms) {
                hipLaunchKernelGGL(chc_solve_kernel<true>, dim3((unsigned)launch_blocks(n_group, 65536)), dim3(CHC_THREADS),
                                   sizeof(double) * CHC_VECTORS * (size_t)lds_atoms, st, d_jobs + G.first, (int)n_group, d_params,
                                   d_kvecs, d_firsts, d_counts, d_ws, d_charges, d_out + G.first);
                STAT_TRY(hipGetLastError());
            }
            if (any_global) {
                hipLaunchKernelGGL(chc_solve_kernel<false>, dim3((unsigned)launch_blocks(n_group, 65536)), dim3(CHC_THREADS), 0, st, d_jobs + G.first, (int)n_group,
                                   d_params, d_kvecs, d_firsts, d_counts, d_ws, d_charges, d_out + G.first);
                STAT_TRY(hipGetLastError());
            }
            if (times) {                                             // (a launch at a time: the events are used again)
                STAT_TRY(hipEventRecord(ev_solve.b, st));
                STAT_TRY(hipStreamSynchronize(st));
                float a = 0.0f, b = 0.0f;
                STAT_TRY(hipEventElapsedTime(&a, ev_rows.a, ev_rows.b));
                STAT_TRY(hipEventElapsedTime(&b, ev_solve.a, ev_solve.b));
                ms_rows += a;
                ms_solve += b;
            }
        }
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    if (times) {
        times[0] = ms_count;
        times[1] = ms_rows;
        times[2] = ms_solve;
    }
    // the caller's arrays, job by job
    const pw_charges_cell_out* r_out = (const pw_charges_cell_out*)res.data();
    const double* r_charges = (const double*)(res.data() + out_bytes);
    for (long k = 0; k < N; ++k) {
        out[jobs[k].out] = r_out[k];
        memcpy(charges + jobs[k].charge_first, r_charges + devs[k].charge_first, sizeof(double) * (size_t)jobs[k].n);
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_charges_cell(pw_context* ctx, const pw_charges_cell_job* jobs, int64_t n_jobs, const double* xyz,
                               const double* params, int64_t n_points, const double* kvecs, int64_t n_kvecs, double* charges,
                               pw_charges_cell_out* out) {
    return charges_cell_call(ctx, jobs, n_jobs, xyz, params, n_points, kvecs, n_kvecs, charges, out, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_charges_cell with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it) and, when times is not null, three floats: the count kernel, the rows
// kernels and the solver kernels in ms by HIP events
extern "C" int pw_internal_charges_cell(pw_context* ctx, const pw_charges_cell_job* jobs, int64_t n_jobs, const double* xyz,
                                        const double* params, int64_t n_points, const double* kvecs, int64_t n_kvecs,
                                        double* charges, pw_charges_cell_out* out, int64_t workspace_bytes, float* times) {
    return charges_cell_call(ctx, jobs, n_jobs, xyz, params, n_points, kvecs, n_kvecs, charges, out, workspace_bytes, times);
}

// pw_sincos element by element on the host (test instrumentation, not part of the header): what a restatement of the
// phase tables takes its sines and cosines from
extern "C" void pw_internal_sincos(const double* x, int64_t n, double* s, double* c) {
    for (int64_t i = 0; i < n; ++i) {
        const EwaldCS v = ewald_sincos(x[i]);
        s[i] = v.s;
        c[i] = v.c;
    }
}
