// pw_rigid_body.hip -- gfx950 kernels and the C ABI entry of the pose-averaged affinity of a cavity for a rigid guest given
// as a pose table (include/pywindow_amd.h: pw_rigid_body_affinity; definition of the result in pw_rigid_body.hpp).  The
// shape is pw_rigid.hip's, three kernels a launch group:
//   prefix   pw_affinity_dev.hpp, the one pw_affinity uses.
//   main     a work item is (job, chunk of 64 ranks), one wavefront an item, a lane a voxel.  The kernel is instantiated
//            on the number of sites (3, 4, 5, 7, and a guarded form that is unrolled to 8 and serves the rest) and on
//            `charged`, so that every per-site and per-pose value has a register of its own: nothing private is indexed
//            at run time.  A launch group runs every instance that one of its jobs needs; an instance passes over the
//            items of the other jobs.  The table of a job can be larger than LDS (1024 * 8 * 24 B), so the displacements
//            of RIGID_BODY_POSE_BLOCK poses are brought into LDS at a time, barriers around the copy; the atoms are
//            staged AFF_TILE at a time with their S rows of coefficients, once an item when n <= AFF_TILE and once per
//            pass of RB poses otherwise.  Per staged atom all S sites of RB poses are evaluated from one read of the
//            atom: RB * S independent accumulators.  The uncharged instances contain no square root.  The fold over
//            the poses is in o order in every lane; then the chunk tree of pw_affinity.hpp over the lanes with
//            __shfl_down, the minimum down the same tree with a strict <, the dead voxels by popcount of __ballot.
//            Lane 0 writes the chunk's partial (pw_rigid.hpp).
//   reduce   a wavefront a job, one lane a series of the partial.
// Every loop is bounded by n, M, the chunks, L or a constant; no workgroup waits for another; no floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_affinity_dev.hpp"
#include "pw_rigid_body.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_rigid_body(const pw_rigid_body_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                      const double* coef, const double* poses, const unsigned long long* words,
                                      const double* betas, double* maps, pw_affinity_level* levels, pw_rigid_out* out,
                                      int threads);                  // pw_hostpath.cpp

static_assert(PW_RIGID_MAX_SITES == RIGID_MAX_SITES && PW_RIGID_MAX_DIRS == RIGID_MAX_DIRS, "the header's constants and the kernel's");
static_assert(sizeof(pw_rigid_body_job) == 168 && sizeof(pw_rigid_out) == 56, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int BODY_CLASSES = 10;                     // (3, 4, 5, 7, guarded 8) x (uncharged, charged)
constexpr int BODY_RB_WIDE = 2, BODY_RB_NARROW = 1;  // poses held in registers at a time: S <= 5, and 7 or guarded 8
static_assert(RIGID_BODY_POSE_BLOCK % BODY_RB_WIDE == 0 && RIGID_BODY_POSE_BLOCK % BODY_RB_NARROW == 0, "a block is whole passes");

// a job as the kernels read it: firsts relative to the spans of the arrays that were uploaded
struct BodyJobDev {
    long atom_first, n, coef_first;
    long word_first;           // the job's ny * nz words in the uploaded span, or -1: every voxel
    long prefix_first;         // the job's rows + 1 integers in the workspace of its launch (an 8-byte word index), or -1
    long part_first;           // the job's [chunks][stride] partials in that workspace
    long map_first;            // the job's 2 V doubles in that workspace, or -1
    long item_first;           // the job's first chunk among the work items of its launch
    long chunks, V;
    long beta_first, pose_first;   // into the uploaded betas and pose rows
    long level_first;          // into the compact result of the call
    double o[3], h, core2, cutoff2;
    int nx, ny, nz, L, S, M, cls, map_level;
};

int body_class(int S, bool charged) {
    const int by_sites = S == 3 ? 0 : S == 4 ? 1 : S == 5 ? 2 : S == 7 ? 3 : 4;
    return by_sites * 2 + (charged ? 1 : 0);
}

// S_T sites unrolled; GUARD: the job has J.S <= S_T of them and every site is behind `s < S`; RB poses a pass
template <int S_T, bool GUARD, bool CHARGED, int RB>
__global__ void __launch_bounds__(AFF_CHUNK)
pw_rigid_body_kernel(const BodyJobDev* __restrict__ jobs, int n_jobs, long total, int cls, const double* __restrict__ xyz,
                     const double* __restrict__ coef, const double* __restrict__ poses, const u64* __restrict__ words,
                     const double* __restrict__ betas, u64* __restrict__ ws) {
    constexpr int NC = CHARGED ? 3 : 2;                              // columns of a staged row
    __shared__ double s_xyz[3 * AFF_TILE];
    __shared__ double s_coef[NC * S_T * AFF_TILE];                   // row (atom t, site s) at NC * (t * S_T + s)
    __shared__ double s_pose[3 * S_T * RIGID_BODY_POSE_BLOCK];       // row (pose q of the block, site s) at 3 * (q * S + s)
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += AFF_CHUNK) s_tab[t] = POW_EXP_TAB[t];
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
        const BodyJobDev& J = jobs[k];
        if (J.cls != cls) continue;                                  // (the same in every lane: another instance's item)
        const long chunk = item - J.item_first, rank = chunk * AFF_CHUNK + lane;
        const bool valid = rank < J.V;
        const int nx = J.nx, ny = J.ny, L = J.L, M = J.M, S = GUARD ? J.S : S_T;
        const long n = J.n;
        int i = 0, row = 0;
        if (valid) {
            const bool masked = J.word_first >= 0;
            const u64* w = masked ? words + J.word_first : nullptr;
            const int* prefix = masked ? (const int*)(ws + J.prefix_first) : nullptr;
            aff_voxel(rank, masked, nx, ny * J.nz, [&](int r) { return w[r]; }, [&](int r) { return prefix[r]; }, i, row);
        }
        const double x = cavity_coord(J.o[0], i, J.h), y = cavity_coord(J.o[1], row % ny, J.h),
                     z = cavity_coord(J.o[2], row / ny, J.h);
        const double core2 = J.core2, cutoff2 = J.cutoff2, inv_M = rigid_inv(M);
        const double* atoms = xyz + 3 * J.atom_first;
        const double* rows_abc = coef + 3 * J.coef_first;
        const double* table = poses + 3 * J.pose_first;
        // atoms [a0, a0 + len) and their S rows into LDS; the caller puts the barriers around it
        auto stage = [&](long a0, int len) {
            for (int t = lane; t < 3 * len; t += AFF_CHUNK) s_xyz[t] = atoms[3 * a0 + t];
            for (int q = lane; q < S * len; q += AFF_CHUNK) {
                const int s = q / len, t = q - s * len;
                const double* src = rows_abc + 3 * ((long)s * n + a0 + t);
                double* dst = s_coef + NC * (t * S_T + s);
                dst[0] = src[0];
                dst[1] = src[1];
                if constexpr (CHARGED) dst[2] = src[2];
            }
        };
        const bool once = n <= AFF_TILE;
        __syncthreads();                                             // (the item before is done with the LDS)
        if (once) stage(0, (int)n);                                  // (visible after the barriers of the first block)

        RigidFold fold[AFF_MAX_LEVELS];                              // (indexed by unrolled loops only: registers)
        double umin_v = aff_inf();
        int umin_o = -1, n_blocked = 0;
        bool any_live = false, clamped = false;
        for (int ob = 0; ob < M; ob += RIGID_BODY_POSE_BLOCK) {
            const int in_block = M - ob < RIGID_BODY_POSE_BLOCK ? M - ob : RIGID_BODY_POSE_BLOCK;
            __syncthreads();                                         // (the block before is done with)
            for (int t = lane; t < 3 * S * in_block; t += AFF_CHUNK) s_pose[t] = table[3 * (long)ob * S + t];
            __syncthreads();
            for (int q0 = 0; q0 < in_block; q0 += RB) {
                double px[RB][S_T], py[RB][S_T], pz[RB][S_T], U[RB][S_T];
                bool blocked[RB];
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int q = q0 + r < in_block ? q0 + r : in_block - 1;   // (past the end: the last one again, not used below)
                    blocked[r] = false;
#pragma unroll
                    for (int s = 0; s < S_T; ++s) {
                        U[r][s] = 0.0;
                        px[r][s] = py[r][s] = pz[r][s] = 0.0;
                        if (!GUARD || s < S) {
                            const double* p = s_pose + 3 * (q * S + s);
                            px[r][s] = rigid_body_site(x, p[0]);
                            py[r][s] = rigid_body_site(y, p[1]);
                            pz[r][s] = rigid_body_site(z, p[2]);
                        }
                    }
                }
                for (long a0 = 0; a0 < n; a0 += AFF_TILE) {
                    const int len = (int)(n - a0 < AFF_TILE ? n - a0 : AFF_TILE);
                    if (!once) {
                        __syncthreads();                             // (the atoms staged before are done with)
                        stage(a0, len);
                        __syncthreads();
                    }
                    for (int t = 0; t < len; ++t) {
                        const double X = s_xyz[3 * t], Y = s_xyz[3 * t + 1], Z = s_xyz[3 * t + 2];
#pragma unroll
                        for (int s = 0; s < S_T; ++s) {
                            if (GUARD && s >= S) continue;
                            const double* c = s_coef + NC * (t * S_T + s);
                            const double A = c[0], B = c[1], C = CHARGED ? c[NC - 1] : 0.0;
#pragma unroll
                            for (int r = 0; r < RB; ++r) {
                                const double r2 = aff_r2(px[r][s] - X, py[r][s] - Y, pz[r][s] - Z);
                                blocked[r] = blocked[r] || aff_blocked(r2, core2);
                                const double u = rigid_pair<CHARGED>(r2, A, B, C);
                                U[r][s] = aff_counts(r2, cutoff2) ? U[r][s] + u : U[r][s];
                            }
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    if (q0 + r >= in_block) continue;                // (the same in every lane)
                    double Ut = U[r][0];
#pragma unroll
                    for (int s = 1; s < S_T; ++s)
                        if (!GUARD || s < S) Ut = Ut + U[r][s];
                    const bool live = valid && !blocked[r];
                    n_blocked += valid && blocked[r];
                    any_live = any_live || live;
                    if (live && Ut < umin_v) {
                        umin_v = Ut;
                        umin_o = ob + q0 + r;
                    }
#pragma unroll
                    for (int b = 0; b < AFF_MAX_LEVELS; ++b) {
                        if (b >= L) continue;
                        bool over = false;
                        const double w = aff_weight(betas[J.beta_first + b], Ut, s_tab, over);
                        clamped = clamped || (live && over);
                        if (live) fold[b].add(w, Ut);
                    }
                }
            }
        }

        u64* part = ws + J.part_first + chunk * rigid_part_words(L);
        double zmap = 0.0;
#pragma unroll
        for (int b = 0; b < AFF_MAX_LEVELS; ++b) {
            if (b >= L) continue;
            double sz = fold[b].zbar(inv_M), se = fold[b].ebar(inv_M);   // (+0.0 in a lane without a voxel or a live pose)
            if (b == J.map_level) zmap = sz;
            for (int s = 1; s < AFF_CHUNK; s <<= 1) {
                sz = sz + __shfl_down(sz, s);
                se = se + __shfl_down(se, s);
            }
            if (lane == 0) {
                part[2 * b] = pw_d2bits(sz);
                part[2 * b + 1] = pw_d2bits(se);
            }
        }
        if (J.map_first >= 0 && valid) {
            ws[J.map_first + 2 * rank] = pw_d2bits(zmap);
            ws[J.map_first + 2 * rank + 1] = pw_d2bits(umin_v);
        }
        double m = umin_v;
        int m_lane = lane, m_o = umin_o;
        for (int s = 1; s < AFF_CHUNK; s <<= 1) {
            const double other = __shfl_down(m, s);
            const int other_lane = __shfl_down(m_lane, s), other_o = __shfl_down(m_o, s);
            n_blocked += __shfl_down(n_blocked, s);                  // (integers: lane 0 ends with the wave's total)
            if (other < m) {
                m = other;
                m_lane = other_lane;
                m_o = other_o;
            }
        }
        const u64 any_clamped = __ballot(clamped), dead = __ballot(valid && !any_live);
        if (lane == 0) {
            part[2 * L] = pw_d2bits(m);
            part[2 * L + 1] = (u64)(chunk * AFF_CHUNK + m_lane);
            part[2 * L + 2] = (u64)(long)m_o;
            part[2 * L + 3] = (u64)n_blocked;
            part[2 * L + 4] = (u64)cavity_popcount(dead);
            part[2 * L + 5] = any_clamped ? (u64)AFF_CLAMPED : 0ull;
        }
    }
}

// (pw_rigid_reduce_kernel's statements on this file's job record: the partial is pw_rigid.hpp's)
__global__ void __launch_bounds__(AFF_CHUNK)
pw_rigid_body_reduce_kernel(const BodyJobDev* __restrict__ jobs, const u64* __restrict__ words, const u64* __restrict__ ws,
                            pw_rigid_out* __restrict__ out, double* __restrict__ levels) {
    const BodyJobDev& J = jobs[blockIdx.x];
    const int t = threadIdx.x, L = J.L, stride = rigid_part_words(L);
    if (t >= stride || t == 2 * L + 1 || t == 2 * L + 2) return;     // (rank and pose go with the minimum)
    const u64* p = ws + J.part_first + t;
    pw_rigid_out& O = out[blockIdx.x];
    if (t < 2 * L) {
        double s = 0.0;
        for (long c = 0; c < J.chunks; ++c) s = s + pw_bits2d(p[c * stride]);
        levels[2 * J.level_first + t] = s;
    } else if (t == 2 * L) {
        double m = aff_inf();
        long rank = -1, pose = -1;
        for (long c = 0; c < J.chunks; ++c) {
            const double v = pw_bits2d(p[c * stride]);
            if (v < m) {
                m = v;
                rank = (long)p[c * stride + 1];
                pose = (long)p[c * stride + 2];
            }
        }
        int i = -1, row = -1;
        if (rank >= 0) {
            const bool masked = J.word_first >= 0;
            const u64* w = masked ? words + J.word_first : nullptr;
            const int* prefix = masked ? (const int*)(ws + J.prefix_first) : nullptr;
            aff_voxel(rank, masked, J.nx, J.ny * J.nz, [&](int r) { return w[r]; }, [&](int r) { return prefix[r]; }, i, row);
        }
        O.u_min = m;
        O.min_voxel[0] = i;
        O.min_voxel[1] = rank >= 0 ? row % J.ny : -1;
        O.min_voxel[2] = rank >= 0 ? row / J.ny : -1;
        O.min_dir = (int)pose;
    } else {
        unsigned long long s = 0;
        const bool flags = t == 2 * L + 5;
        for (long c = 0; c < J.chunks; ++c) s = flags ? s | p[c * stride] : s + p[c * stride];
        if (t == 2 * L + 3) {
            O.n_voxels = J.V;
            O.n_blocked_poses = (long)s;
        } else if (t == 2 * L + 4) {
            O.n_dead = (long)s;
        } else {
            O.flags = (int)s;
            O.reserved = 0;
        }
    }
}

// one instance over the items of a launch group
void body_launch(int cls, unsigned blocks, hipStream_t st, const BodyJobDev* jobs, int n_jobs, long total, const double* xyz,
                 const double* coef, const double* poses, const u64* words, const double* betas, u64* ws) {
#define BODY_GO(S_T, GUARD, CHARGED, RB)                                                                                  \
    hipLaunchKernelGGL((pw_rigid_body_kernel<S_T, GUARD, CHARGED, RB>), dim3(blocks), dim3(AFF_CHUNK), 0, st, jobs, n_jobs, \
                       total, cls, xyz, coef, poses, words, betas, ws)
    switch (cls) {
        case 0: BODY_GO(3, false, false, BODY_RB_WIDE); break;
        case 1: BODY_GO(3, false, true, BODY_RB_WIDE); break;
        case 2: BODY_GO(4, false, false, BODY_RB_WIDE); break;
        case 3: BODY_GO(4, false, true, BODY_RB_WIDE); break;
        case 4: BODY_GO(5, false, false, BODY_RB_WIDE); break;
        case 5: BODY_GO(5, false, true, BODY_RB_WIDE); break;
        case 6: BODY_GO(7, false, false, BODY_RB_NARROW); break;
        case 7: BODY_GO(7, false, true, BODY_RB_NARROW); break;
        case 8: BODY_GO(RIGID_MAX_SITES, true, false, BODY_RB_NARROW); break;
        default: BODY_GO(RIGID_MAX_SITES, true, true, BODY_RB_NARROW); break;
    }
#undef BODY_GO
}

const char* const ENTRY = "pw_rigid_body_affinity";
int body_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written.  V[k]: the voxels of job k's region
int body_check(const pw_rigid_body_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
               const double* poses, long n_pose_rows, const u64* words, long n_words, const double* betas, long n_betas,
               const double* maps, long n_maps, const pw_affinity_level* levels, long n_levels, long n_out,
               std::vector<long>& V) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_rigid_body_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        const long rows = (long)J.ny * J.nz, L = (long)J.n_betas, S = (long)J.n_sites, M = (long)J.n_dirs;
        if (J.n < 0) return body_bad(k, "a negative count");
        GRID_CHECK(grid_n_betas_check(ENTRY, k, L));
        if (S < 1 || S > RIGID_MAX_SITES) return body_bad(k, "n_sites outside 1 .. PW_RIGID_MAX_SITES (8)");
        if (M < 1 || M > RIGID_MAX_DIRS) return body_bad(k, "n_dirs outside 1 .. PW_RIGID_MAX_DIRS (1024)");
        if (J.charged != 0 && J.charged != 1) return body_bad(k, "charged is neither 0 nor 1");
        if (J.map_level < -1 || J.map_level >= L) return body_bad(k, "map_level outside -1 .. n_betas - 1");
        if (J.map_level >= 0 && J.map_first < 0) return body_bad(k, "map_level >= 0 with map_first < 0");
        if (span_outside(J.atom_first, J.n, n_points)) return body_bad(k, "atoms outside xyz");
        if (span_outside(J.coef_first, S * J.n, n_coef)) return body_bad(k, "coefficients outside coef");   // (n <= n_points: no overflow)
        if (span_outside(J.pose_first, M * S, n_pose_rows)) return body_bad(k, "poses outside their array");
        if (J.word_first < -1 || (J.word_first >= 0 && span_outside(J.word_first, rows, n_words)))
            return body_bad(k, "the words are outside their array");
        if (span_outside(J.beta_first, L, n_betas)) return body_bad(k, "betas outside the array");
        if (span_outside(J.level_first, L, n_levels)) return body_bad(k, "the rows are outside levels");
        if (span_outside(J.out, 1, n_out)) return body_bad(k, "the row is outside out");
        if ((J.n && (!xyz || !coef)) || (J.word_first >= 0 && !words) || !betas || !poses || !levels ||
            (J.map_level >= 0 && !maps))
            return body_bad(k, "null array");
        V[k] = grid_region_voxels(J.word_first >= 0 ? words + J.word_first : nullptr, J.nx, rows);
        if (J.map_level >= 0 && span_outside(J.map_first, 2 * V[k], n_maps)) return body_bad(k, "the maps are outside their array");
        GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
        GRID_CHECK(grid_core_check(ENTRY, k, J.core2, J.cutoff2));
        GRID_CHECK(grid_betas_check(ENTRY, k, betas, J.beta_first, L));
        for (long c = 0; c < 3 * M * S; ++c) {
            const double p = poses[3 * J.pose_first + c];
            if (!pw_finite(p) || pw_abs(p) > RIGID_MAX_OFFSET) return body_bad(k, "a pose component is not finite or beyond 16");
        }
        GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first, J.n));   // (every coordinate, then every row)
        GRID_CHECK(grid_coef_check(ENTRY, k, coef, J.coef_first, S * J.n, 3, J.charged != 0));
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of levels with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].level_first, (long)jobs[k].n_betas}; }));
    return shared_output(ENTRY, n_jobs, "shares maps with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].map_first, jobs[k].map_level >= 0 ? 2 * V[k] : 0}; });
}

// workspace_bytes: the budget of the prefixes, partials and maps of the jobs of one launch (0: RIGID_WORKSPACE_BYTES; at 1
// every job is a launch of its own); kernel_ms: when not null, the time of the device work of the call from the first
// launch to the last, the copies between them included, by HIP events on the context's stream
int body(pw_context* ctx, const pw_rigid_body_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points, const double* coef,
         int64_t n_coef, const double* poses, int64_t n_pose_rows, const uint64_t* words_, int64_t n_words, const double* betas,
         int64_t n_betas, double* maps, int64_t n_maps, pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out,
         int64_t n_out, int64_t workspace_bytes, float* kernel_ms) {
    const u64* words = (const u64*)words_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 ||
        n_pose_rows < 0 || n_words < 0 || n_betas < 0 || n_maps < 0 || n_levels < 0 || n_out < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    std::vector<long> V((size_t)N, 0);
    const int rc = body_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, poses, (long)n_pose_rows, words, (long)n_words,
                              betas, (long)n_betas, maps, (long)n_maps, levels, (long)n_levels, (long)n_out, V);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_rigid_body(jobs, N, V.data(), xyz, coef, poses, (const unsigned long long*)words, betas, maps, levels,
                                      out, pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // prefixes, partials and maps fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : RIGID_WORKSPACE_BYTES) / 8;
    Span atoms, rows_abq, region, beta_span, pose_span;
    for (long k = 0; k < N; ++k) {
        const pw_rigid_body_job& J = jobs[k];
        atoms.widen((long)J.atom_first, (long)J.n);
        rows_abq.widen((long)J.coef_first, (long)J.n_sites * (long)J.n);
        if (J.word_first >= 0) region.widen((long)J.word_first, (long)J.ny * J.nz);
        beta_span.widen((long)J.beta_first, (long)J.n_betas);
        pose_span.widen((long)J.pose_first, (long)J.n_dirs * (long)J.n_sites);
    }
    // betas and pose rows travel as one array (every job has some of each: the two spans have a lo)
    const long n_beta_span = beta_span.count(), n_pose_span = pose_span.count();
    std::vector<double> params((size_t)(n_beta_span + 3 * n_pose_span));
    memcpy(params.data(), betas + beta_span.lo, sizeof(double) * (size_t)n_beta_span);
    memcpy(params.data() + n_beta_span, poses + 3 * pose_span.lo, sizeof(double) * 3 * (size_t)n_pose_span);

    std::vector<BodyJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long n_level_rows = 0;
    for (long k = 0; k < N; ++k) {
        const pw_rigid_body_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, L = (long)J.n_betas;
        const long chunks = (V[k] + AFF_CHUNK - 1) / AFF_CHUNK;
        const bool masked = J.word_first >= 0;
        const long prefix_words = masked ? (rows + 2) / 2 : 0, part_words = chunks * rigid_part_words((int)L),
                   map_words = J.map_level >= 0 ? 2 * V[k] : 0, need = prefix_words + part_words + map_words;
        place(groups, cur, budget_words, need + 1);                  // (a word more a job: no job is free)
        BodyJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.coef_first = rows_abq.rel((long)J.coef_first, (long)J.n);
        D.word_first = masked ? (long)J.word_first - region.lo : -1;
        D.prefix_first = masked ? cur.words : -1;
        D.part_first = cur.words + prefix_words;
        D.map_first = J.map_level >= 0 ? cur.words + prefix_words + part_words : -1;
        D.item_first = cur.items;
        D.chunks = chunks;
        D.V = V[k];
        D.beta_first = (long)J.beta_first - beta_span.lo;
        D.pose_first = (long)J.pose_first - pose_span.lo;
        D.level_first = n_level_rows;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        D.h = J.spacing; D.core2 = J.core2; D.cutoff2 = J.cutoff2;
        D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.L = (int)L; D.S = (int)J.n_sites; D.M = (int)J.n_dirs;
        D.cls = body_class((int)J.n_sites, J.charged != 0);
        D.map_level = J.map_level;
        n_level_rows += L;
        cur.words += need + 1; cur.cost += need + 1; cur.items += chunks; cur.last += 1;
    }
    groups.push_back(cur);

    // the compact result of the call: the rows of out in job order, then the rows of levels
    const size_t out_bytes = sizeof(pw_rigid_out) * (size_t)N, levels_bytes = sizeof(pw_affinity_level) * (size_t)n_level_rows,
                 res_bytes = out_bytes + levels_bytes, ws_bytes = sizeof(u64) * (size_t)most_words(groups);
    std::vector<unsigned char> res(res_bytes);
    std::vector<std::vector<double>> got(groups.size());             // the maps of a launch, as its workspace has them

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        BodyJobDev* d_jobs;
        double *d_xyz, *d_coef, *d_params;
        u64 *d_words, *d_ws;
        unsigned char* d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(BodyJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(BodyJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_abq.upload(buf, &d_coef, coef, 3));
        STAT_TRY(region.upload(buf, &d_words, words, 1));
        STAT_TRY(buf.alloc(&d_params, sizeof(double) * params.size()));
        STAT_TRY(hipMemcpyAsync(d_params, params.data(), sizeof(double) * params.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        pw_rigid_out* d_out = (pw_rigid_out*)d_res;
        double* d_levels = (double*)(d_res + out_bytes);
        const double *d_betas = d_params, *d_poses = d_params + n_beta_span;
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over once the maps of this
        // one are on their way)
        for (size_t g = 0; g < groups.size(); ++g) {
            const LaunchGroup& G = groups[g];
            const unsigned n_group = (unsigned)(G.last - G.first);
            bool any_mask = false, needed[BODY_CLASSES] = {};
            Span maps_ws;                                            // the maps of the group in its workspace
            for (long k = G.first; k < G.last; ++k) {
                any_mask = any_mask || devs[k].prefix_first >= 0;
                if (devs[k].map_first >= 0) maps_ws.widen(devs[k].map_first, 2 * devs[k].V);
                if (devs[k].chunks) needed[devs[k].cls] = true;
            }
            if (any_mask) {
                hipLaunchKernelGGL(pw_region_prefix_kernel<BodyJobDev>, dim3(n_group), dim3(AFF_PREFIX_THREADS), 0, st,
                                   d_jobs + G.first, d_words, d_ws);
                STAT_TRY(hipGetLastError());
            }
            if (G.items) {
                for (int cls = 0; cls < BODY_CLASSES; ++cls) {
                    if (!needed[cls]) continue;
                    const long blocks = launch_blocks(G.items, 65536);   // (asked a launch: the test hook counts launches)
                    body_launch(cls, (unsigned)blocks, st, d_jobs + G.first, (int)n_group, G.items, d_xyz, d_coef, d_poses,
                                d_words, d_betas, d_ws);
                    STAT_TRY(hipGetLastError());
                }
            }
            hipLaunchKernelGGL(pw_rigid_body_reduce_kernel, dim3(n_group), dim3(AFF_CHUNK), 0, st, d_jobs + G.first, d_words,
                               d_ws, d_out + G.first, d_levels);
            STAT_TRY(hipGetLastError());
            if (maps_ws.lo >= 0) {
                got[g].resize((size_t)maps_ws.count());
                STAT_TRY(hipMemcpyAsync(got[g].data(), d_ws + maps_ws.lo, sizeof(double) * got[g].size(), hipMemcpyDeviceToHost, st));
                // (map_first of the group's jobs becomes relative to that copy)
                for (long k = G.first; k < G.last; ++k)
                    if (devs[k].map_first >= 0) devs[k].map_first -= maps_ws.lo;
            }
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's arrays, job by job
    const pw_rigid_out* r_out = (const pw_rigid_out*)res.data();
    const pw_affinity_level* r_levels = (const pw_affinity_level*)(res.data() + out_bytes);
    for (size_t g = 0; g < groups.size(); ++g)
        for (long k = groups[g].first; k < groups[g].last; ++k) {
            const pw_rigid_body_job& J = jobs[k];
            out[J.out] = r_out[k];
            memcpy(levels + J.level_first, r_levels + devs[k].level_first, sizeof(pw_affinity_level) * (size_t)J.n_betas);
            if (J.map_level >= 0 && V[k])
                memcpy(maps + J.map_first, got[g].data() + devs[k].map_first, sizeof(double) * 2 * (size_t)V[k]);
        }
    return PW_OK;
}

}  // namespace

extern "C" int pw_rigid_body_affinity(pw_context* ctx, const pw_rigid_body_job* jobs, int64_t n_jobs, const double* xyz,
                                      int64_t n_points, const double* coef, int64_t n_coef, const double* poses,
                                      int64_t n_pose_rows, const uint64_t* words, int64_t n_words, const double* betas,
                                      int64_t n_betas, double* maps, int64_t n_maps, pw_affinity_level* levels,
                                      int64_t n_levels, pw_rigid_out* out, int64_t n_out) {
    return body(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, poses, n_pose_rows, words, n_words, betas, n_betas, maps, n_maps,
                levels, n_levels, out, n_out, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_rigid_body_affinity with the budget of the workspace of a launch
// given (0: the default; the result may not depend on it) and, when kernel_ms is not null, the device work timed by HIP
// events
extern "C" int pw_internal_rigid_body_affinity(pw_context* ctx, const pw_rigid_body_job* jobs, int64_t n_jobs, const double* xyz,
                                               int64_t n_points, const double* coef, int64_t n_coef, const double* poses,
                                               int64_t n_pose_rows, const uint64_t* words, int64_t n_words, const double* betas,
                                               int64_t n_betas, double* maps, int64_t n_maps, pw_affinity_level* levels,
                                               int64_t n_levels, pw_rigid_out* out, int64_t n_out, int64_t workspace_bytes,
                                               float* kernel_ms) {
    return body(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, poses, n_pose_rows, words, n_words, betas, n_betas, maps, n_maps,
                levels, n_levels, out, n_out, workspace_bytes, kernel_ms);
}
