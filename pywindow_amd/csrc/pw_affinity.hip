// pw_affinity.hip -- gfx950 kernels and the C ABI entry of the Lennard-Jones energy map of a cavity and its Boltzmann
// sums (include/pywindow_amd.h: pw_affinity; definition of the result in pw_affinity.hpp).  Three kernels a launch group:
//   prefix   (pw_affinity_dev.hpp, shared with pw_rigid.hip) a workgroup a job that has a mask: the exclusive prefix of
//            the popcounts of its ny * nz words (bits at i >= nx dropped), rows + 1 integers in the workspace.  A thread
//            takes at most 16 consecutive rows.
//   main     a work item is (job, chunk of 64 ranks) and a wavefront takes one item after the other; the job of an item
//            is found by binary search in the prefix of work items, so one launch serves any mix of grids.  A lane is a
//            rank: to a row by binary search in the job's prefix (at most 12 steps), then to the bit inside the word
//            (six halvings); without a mask by one division.  The atoms go through LDS AFF_TILE at a time and are read
//            at one address per wave (a broadcast), so there is no capacity in n; pw_exp's 2 KB table is in LDS as
//            well.  The chunk tree of pw_affinity.hpp runs over the lanes with __shfl_down: at step k lane t takes lane
//            t + k, and the lanes that are multiples of 2k hold exactly the defined slots.  The minimum goes down the
//            same tree with a strict <, so the lower rank wins a tie.  Histogram counts are popcounts of __ballot.
//            Lane 0 writes the chunk's partial (pw_affinity.hpp) to the workspace.
//   reduce   a wavefront a job, one lane a series of the partial: the sums in chunk order from +0.0, the minimum with a
//            strict < in chunk order, the integers added, the flags OR-ed.
// Every loop is bounded by n, the chunks, L, E or a constant; no workgroup waits for another; no floating-point
// atomics.  Launches follow one another on the context's stream; memory is allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_affinity.hpp"
#include "pw_affinity_dev.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_affinity(const pw_affinity_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                    const double* coef, const unsigned long long* words, const double* betas,
                                    const double* edges, double* energies, pw_affinity_level* levels, long long* hist,
                                    pw_affinity_out* out, int threads);   // pw_hostpath.cpp

static_assert(PW_AFF_MAX_LEVELS == AFF_MAX_LEVELS && PW_AFF_MAX_EDGES == AFF_MAX_EDGES && PW_AFF_CLAMPED == AFF_CLAMPED,
              "the header's constants and the kernel's");
static_assert(sizeof(pw_affinity_job) == 160 && sizeof(pw_affinity_level) == 16 && sizeof(pw_affinity_out) == 40,
              "the layouts of the header");

namespace {

typedef cavity_word u64;

// a job as the kernels read it: firsts relative to the spans of the arrays that were uploaded
struct AffJobDev {
    long atom_first, n, coef_first;
    long word_first;           // the job's ny * nz words in the uploaded span, or -1: every voxel
    long prefix_first;         // the job's rows + 1 integers in the workspace of its launch (an 8-byte word index), or -1
    long part_first;           // the job's [chunks][stride] partials in that workspace
    long energy_first;         // the job's V energies in that workspace, or -1
    long item_first;           // the job's first chunk among the work items of its launch
    long chunks, V;
    long beta_first, edge_first;   // into the uploaded betas and edges (one array, the edges behind the betas)
    long level_first, hist_first;  // into the compact result of the call
    double o[3], h, core2, cutoff2;
    int nx, ny, nz, L, E, reserved;
};

__global__ void __launch_bounds__(AFF_CHUNK)
pw_affinity_kernel(const AffJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                   const double* __restrict__ coef, const u64* __restrict__ words, const double* __restrict__ params,
                   u64* __restrict__ ws) {
    __shared__ double s_xyz[3 * AFF_TILE];
    __shared__ double s_coef[2 * AFF_TILE];
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += AFF_CHUNK) s_tab[t] = POW_EXP_TAB[t];
    __syncthreads();
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
        const AffJobDev& J = jobs[k];
        const long chunk = item - J.item_first, rank = chunk * AFF_CHUNK + lane;
        const bool valid = rank < J.V;
        const int nx = J.nx, ny = J.ny, L = J.L, E = J.E;
        int i = 0, row = 0;
        if (valid) {
            const bool masked = J.word_first >= 0;
            const u64* w = masked ? words + J.word_first : nullptr;
            const int* prefix = masked ? (const int*)(ws + J.prefix_first) : nullptr;
            aff_voxel(rank, masked, nx, ny * J.nz, [&](int r) { return w[r]; }, [&](int r) { return prefix[r]; }, i, row);
        }
        const double x = cavity_coord(J.o[0], i, J.h), y = cavity_coord(J.o[1], row % ny, J.h),
                     z = cavity_coord(J.o[2], row / ny, J.h);
        const double core2 = J.core2, cutoff2 = J.cutoff2;
        const double* atoms = xyz + 3 * J.atom_first;
        const double* rows_ab = coef + 2 * J.coef_first;
        double U = 0.0;
        bool blocked = false;
        for (long a0 = 0; a0 < J.n; a0 += AFF_TILE) {
            const int len = (int)(J.n - a0 < AFF_TILE ? J.n - a0 : AFF_TILE);
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
        const bool live = valid && !blocked;
        if (J.energy_first >= 0 && valid) ws[J.energy_first + rank] = pw_d2bits(blocked ? aff_inf() : U);
        u64* part = ws + J.part_first + chunk * aff_part_words(L, E);
        bool clamped = false;
        for (int b = 0; b < L; ++b) {
            bool over = false;
            const double w = aff_weight(params[J.beta_first + b], U, s_tab, over);
            clamped = clamped || (live && over);
            double sz = live ? w : 0.0, se = live ? w * U : 0.0;
            for (int s = 1; s < AFF_CHUNK; s <<= 1) {
                sz = sz + __shfl_down(sz, s);
                se = se + __shfl_down(se, s);
            }
            if (lane == 0) {
                part[2 * b] = pw_d2bits(sz);
                part[2 * b + 1] = pw_d2bits(se);
            }
        }
        double m = live ? U : aff_inf();
        int m_lane = lane;
        for (int s = 1; s < AFF_CHUNK; s <<= 1) {
            const double other = __shfl_down(m, s);
            const int other_lane = __shfl_down(m_lane, s);
            if (other < m) {
                m = other;
                m_lane = other_lane;
            }
        }
        const u64 any_clamped = __ballot(clamped), all_blocked = __ballot(valid && blocked);
        if (lane == 0) {
            part[2 * L] = pw_d2bits(m);
            part[2 * L + 1] = (u64)(chunk * AFF_CHUNK + m_lane);
            part[2 * L + 2] = (u64)cavity_popcount(all_blocked);
            part[2 * L + 3] = any_clamped ? (u64)AFF_CLAMPED : 0ull;
        }
        for (int e = 0; e < E; ++e) {
            const u64 below = __ballot(live && U < params[J.edge_first + e]);
            if (lane == 0) part[2 * L + AFF_PART_FIXED + e] = (u64)cavity_popcount(below);
        }
    }
}

__global__ void __launch_bounds__(AFF_CHUNK)
pw_affinity_reduce_kernel(const AffJobDev* __restrict__ jobs, const u64* __restrict__ words, const u64* __restrict__ ws,
                          pw_affinity_out* __restrict__ out, double* __restrict__ levels, long long* __restrict__ hist) {
    const AffJobDev& J = jobs[blockIdx.x];
    const int t = threadIdx.x, L = J.L, E = J.E, stride = aff_part_words(L, E);
    if (t >= stride || t == 2 * L + 1) return;                       // (the rank of the minimum goes with the minimum)
    const u64* p = ws + J.part_first + t;
    pw_affinity_out& O = out[blockIdx.x];
    if (t < 2 * L) {
        double s = 0.0;
        for (long c = 0; c < J.chunks; ++c) s = s + pw_bits2d(p[c * stride]);
        levels[2 * J.level_first + t] = s;
    } else if (t == 2 * L) {
        double m = aff_inf();
        long rank = -1;
        for (long c = 0; c < J.chunks; ++c) {
            const double v = pw_bits2d(p[c * stride]);
            if (v < m) {
                m = v;
                rank = (long)p[c * stride + 1];
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
    } else {
        unsigned long long s = 0;
        const bool flags = t == 2 * L + 3;
        for (long c = 0; c < J.chunks; ++c) s = flags ? s | p[c * stride] : s + p[c * stride];
        if (t == 2 * L + 2) {
            O.n_voxels = J.V;
            O.n_blocked = (long)s;
        } else if (flags) {
            O.flags = (int)s;
        } else {
            hist[J.hist_first + (t - 2 * L - AFF_PART_FIXED)] = (long long)s;
        }
    }
}

const char* const ENTRY = "pw_affinity";
int aff_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written.  V[k]: the voxels of job k's region
int aff_check(const pw_affinity_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
              const u64* words, long n_words, const double* betas, long n_betas, const double* edges, long n_edges,
              const double* energies, long n_energies, const pw_affinity_level* levels, long n_levels, const int64_t* hist,
              long n_hist, long n_out, std::vector<long>& V) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_affinity_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        const long rows = (long)J.ny * J.nz, L = (long)J.n_betas, E = (long)J.n_edges;
        if (J.n < 0) return aff_bad(k, "a negative count");
        GRID_CHECK(grid_n_betas_check(ENTRY, k, L));
        if (E < 0 || E > AFF_MAX_EDGES) return aff_bad(k, "n_edges outside 0 .. PW_AFF_MAX_EDGES (16)");
        if (span_outside(J.atom_first, J.n, n_points)) return aff_bad(k, "atoms outside xyz");
        if (span_outside(J.coef_first, J.n, n_coef)) return aff_bad(k, "coefficients outside coef");
        if (J.word_first < -1 || (J.word_first >= 0 && span_outside(J.word_first, rows, n_words)))
            return aff_bad(k, "the words are outside their array");
        if (span_outside(J.beta_first, L, n_betas)) return aff_bad(k, "betas outside the array");
        if (span_outside(J.edge_first, E, n_edges)) return aff_bad(k, "edges outside the array");
        if (span_outside(J.level_first, L, n_levels)) return aff_bad(k, "the rows are outside levels");
        if (span_outside(J.hist_first, E, n_hist)) return aff_bad(k, "the counts are outside hist");
        if (span_outside(J.out, 1, n_out)) return aff_bad(k, "the row is outside out");
        if ((J.n && (!xyz || !coef)) || (J.word_first >= 0 && !words) || !betas || (E && (!edges || !hist)) || !levels ||
            (J.energy_first >= 0 && !energies))
            return aff_bad(k, "null array");
        V[k] = grid_region_voxels(J.word_first >= 0 ? words + J.word_first : nullptr, J.nx, rows);
        if (J.energy_first < -1 || (J.energy_first >= 0 && span_outside(J.energy_first, V[k], n_energies)))
            return aff_bad(k, "the energies are outside their array");
        GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
        GRID_CHECK(grid_core_check(ENTRY, k, J.core2, J.cutoff2));
        GRID_CHECK(grid_betas_check(ENTRY, k, betas, J.beta_first, L));
        for (long e = 0; e < E; ++e) {
            const double edge = edges[J.edge_first + e];
            if (!pw_finite(edge)) return aff_bad(k, "an edge is not finite");
            if (e && !(edge > edges[J.edge_first + e - 1])) return aff_bad(k, "the edges are not strictly ascending");
        }
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its row)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_coef_check(ENTRY, k, coef, J.coef_first + a, 1, 2, false));
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of levels with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].level_first, (long)jobs[k].n_betas}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares counts of hist with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].hist_first, (long)jobs[k].n_edges}; }));
    return shared_output(ENTRY, n_jobs, "shares energies with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].energy_first, jobs[k].energy_first >= 0 ? V[k] : 0}; });
}

// workspace_bytes: the budget of the prefixes, partials and energy maps of the jobs of one launch (0:
// AFF_WORKSPACE_BYTES; at 1 every job is a launch of its own); kernel_ms: when not null, the time of the device work of
// the call from the first launch to the last, the copies between them included, by HIP events on the context's stream
int affinity(pw_context* ctx, const pw_affinity_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
             const double* coef, int64_t n_coef, const uint64_t* words_, int64_t n_words, const double* betas,
             int64_t n_betas, const double* edges, int64_t n_edges, double* energies, int64_t n_energies,
             pw_affinity_level* levels, int64_t n_levels, int64_t* hist, int64_t n_hist, pw_affinity_out* out, int64_t n_out,
             int64_t workspace_bytes, float* kernel_ms) {
    const u64* words = (const u64*)words_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 ||
        n_words < 0 || n_betas < 0 || n_edges < 0 || n_energies < 0 || n_levels < 0 || n_hist < 0 || n_out < 0 ||
        workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    std::vector<long> V((size_t)N, 0);
    const int rc = aff_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, words, (long)n_words, betas, (long)n_betas,
                             edges, (long)n_edges, energies, (long)n_energies, levels, (long)n_levels, hist, (long)n_hist,
                             (long)n_out, V);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_affinity(jobs, N, V.data(), xyz, coef, (const unsigned long long*)words, betas, edges, energies,
                                    levels, (long long*)hist, out, pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // prefixes, partials and energy maps fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : AFF_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab, region, beta_span, edge_span;
    for (long k = 0; k < N; ++k) {
        const pw_affinity_job& J = jobs[k];
        atoms.widen((long)J.atom_first, (long)J.n);
        rows_ab.widen((long)J.coef_first, (long)J.n);
        if (J.word_first >= 0) region.widen((long)J.word_first, (long)J.ny * J.nz);
        beta_span.widen((long)J.beta_first, (long)J.n_betas);
        edge_span.widen((long)J.edge_first, (long)J.n_edges);
    }
    const long n_beta_span = beta_span.count(), n_edge_span = edge_span.count();
    std::vector<double> params((size_t)(n_beta_span + n_edge_span));
    memcpy(params.data(), betas + beta_span.lo_or_zero(), sizeof(double) * (size_t)n_beta_span);
    if (n_edge_span) memcpy(params.data() + n_beta_span, edges + edge_span.lo, sizeof(double) * (size_t)n_edge_span);

    std::vector<AffJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long n_level_rows = 0, n_counts = 0;
    for (long k = 0; k < N; ++k) {
        const pw_affinity_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, L = (long)J.n_betas, E = (long)J.n_edges;
        const long chunks = (V[k] + AFF_CHUNK - 1) / AFF_CHUNK;
        const bool masked = J.word_first >= 0;
        const long prefix_words = masked ? (rows + 2) / 2 : 0, part_words = chunks * aff_part_words((int)L, (int)E),
                   energy_words = J.energy_first >= 0 ? V[k] : 0, need = prefix_words + part_words + energy_words;
        place(groups, cur, budget_words, need + 1);                  // (a word more a job: no job is free)
        AffJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.coef_first = rows_ab.rel((long)J.coef_first, (long)J.n);
        D.word_first = masked ? (long)J.word_first - region.lo : -1;
        D.prefix_first = masked ? cur.words : -1;
        D.part_first = cur.words + prefix_words;
        D.energy_first = J.energy_first >= 0 ? cur.words + prefix_words + part_words : -1;
        D.item_first = cur.items;
        D.chunks = chunks;
        D.V = V[k];
        D.beta_first = beta_span.rel((long)J.beta_first, L);
        D.edge_first = n_beta_span + edge_span.rel((long)J.edge_first, E);
        D.level_first = n_level_rows;
        D.hist_first = n_counts;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        D.h = J.spacing; D.core2 = J.core2; D.cutoff2 = J.cutoff2;
        D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.L = (int)L; D.E = (int)E; D.reserved = 0;
        n_level_rows += L;
        n_counts += E;
        cur.words += need + 1; cur.cost += need + 1; cur.items += chunks; cur.last += 1;
    }
    groups.push_back(cur);

    // the compact result of the call: the rows of out in job order, then the rows of levels, then the counts
    const size_t out_bytes = sizeof(pw_affinity_out) * (size_t)N, levels_bytes = sizeof(pw_affinity_level) * (size_t)n_level_rows,
                 hist_bytes = sizeof(long long) * (size_t)n_counts, res_bytes = out_bytes + levels_bytes + hist_bytes,
                 ws_bytes = sizeof(u64) * (size_t)most_words(groups);
    std::vector<unsigned char> res(res_bytes);
    std::vector<std::vector<double>> maps(groups.size());            // the energy maps of a launch, as its workspace has them

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        AffJobDev* d_jobs;
        double *d_xyz, *d_coef, *d_params;
        u64 *d_words, *d_ws;
        unsigned char* d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(AffJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(AffJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, 2));
        STAT_TRY(region.upload(buf, &d_words, words, 1));
        STAT_TRY(buf.alloc(&d_params, sizeof(double) * params.size()));
        STAT_TRY(hipMemcpyAsync(d_params, params.data(), sizeof(double) * params.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        pw_affinity_out* d_out = (pw_affinity_out*)d_res;
        double* d_levels = (double*)(d_res + out_bytes);
        long long* d_hist = (long long*)(d_res + out_bytes + levels_bytes);
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over once the energy maps
        // of this one are on their way)
        for (size_t g = 0; g < groups.size(); ++g) {
            const LaunchGroup& G = groups[g];
            const unsigned n_group = (unsigned)(G.last - G.first);
            bool any_mask = false;
            Span maps_ws;                                            // the energy maps of the group in its workspace
            for (long k = G.first; k < G.last; ++k) {
                any_mask = any_mask || devs[k].prefix_first >= 0;
                if (devs[k].energy_first >= 0) maps_ws.widen(devs[k].energy_first, devs[k].V);
            }
            if (any_mask) {
                hipLaunchKernelGGL(pw_region_prefix_kernel<AffJobDev>, dim3(n_group), dim3(AFF_PREFIX_THREADS), 0, st, d_jobs + G.first,
                                   d_words, d_ws);
                STAT_TRY(hipGetLastError());
            }
            if (G.items) {
                const long blocks = launch_blocks(G.items, 65536);
                hipLaunchKernelGGL(pw_affinity_kernel, dim3((unsigned)blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                                   (int)n_group, G.items, d_xyz, d_coef, d_words, d_params, d_ws);
                STAT_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(pw_affinity_reduce_kernel, dim3(n_group), dim3(AFF_CHUNK), 0, st, d_jobs + G.first, d_words,
                               d_ws, d_out + G.first, d_levels, d_hist);
            STAT_TRY(hipGetLastError());
            if (maps_ws.lo >= 0) {
                maps[g].resize((size_t)maps_ws.count());
                STAT_TRY(hipMemcpyAsync(maps[g].data(), d_ws + maps_ws.lo, sizeof(double) * maps[g].size(), hipMemcpyDeviceToHost, st));
                // (energy_first of the group's jobs becomes relative to that copy)
                for (long k = G.first; k < G.last; ++k)
                    if (devs[k].energy_first >= 0) devs[k].energy_first -= maps_ws.lo;
            }
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's arrays, job by job
    const pw_affinity_out* r_out = (const pw_affinity_out*)res.data();
    const pw_affinity_level* r_levels = (const pw_affinity_level*)(res.data() + out_bytes);
    const long long* r_hist = (const long long*)(res.data() + out_bytes + levels_bytes);
    for (size_t g = 0; g < groups.size(); ++g)
        for (long k = groups[g].first; k < groups[g].last; ++k) {
            const pw_affinity_job& J = jobs[k];
            out[J.out] = r_out[k];
            memcpy(levels + J.level_first, r_levels + devs[k].level_first, sizeof(pw_affinity_level) * (size_t)J.n_betas);
            if (J.n_edges) memcpy(hist + J.hist_first, r_hist + devs[k].hist_first, sizeof(long long) * (size_t)J.n_edges);
            if (J.energy_first >= 0 && V[k])
                memcpy(energies + J.energy_first, maps[g].data() + devs[k].energy_first, sizeof(double) * (size_t)V[k]);
        }
    return PW_OK;
}

}  // namespace

extern "C" int pw_affinity(pw_context* ctx, const pw_affinity_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                           const double* coef, int64_t n_coef, const uint64_t* words, int64_t n_words, const double* betas,
                           int64_t n_betas, const double* edges, int64_t n_edges, double* energies, int64_t n_energies,
                           pw_affinity_level* levels, int64_t n_levels, int64_t* hist, int64_t n_hist, pw_affinity_out* out,
                           int64_t n_out) {
    return affinity(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, words, n_words, betas, n_betas, edges, n_edges, energies,
                    n_energies, levels, n_levels, hist, n_hist, out, n_out, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_affinity with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the device work timed by HIP events
extern "C" int pw_internal_affinity(pw_context* ctx, const pw_affinity_job* jobs, int64_t n_jobs, const double* xyz,
                                    int64_t n_points, const double* coef, int64_t n_coef, const uint64_t* words,
                                    int64_t n_words, const double* betas, int64_t n_betas, const double* edges,
                                    int64_t n_edges, double* energies, int64_t n_energies, pw_affinity_level* levels,
                                    int64_t n_levels, int64_t* hist, int64_t n_hist, pw_affinity_out* out, int64_t n_out,
                                    int64_t workspace_bytes, float* kernel_ms) {
    return affinity(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, words, n_words, betas, n_betas, edges, n_edges, energies,
                    n_energies, levels, n_levels, hist, n_hist, out, n_out, workspace_bytes, kernel_ms);
}
