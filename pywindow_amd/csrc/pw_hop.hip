// pw_hop.hip -- gfx950 kernels and the C ABI entry of the free-energy profile of a guest through a window of a cage
// (include/pywindow_amd.h: pw_hop; definition of the result and of the fill in pw_hop.hpp).  Two kernels a launch group:
//   field    pw_field_dev.hpp's body, the one pw_passage.hip runs: U of every voxel of the box of a job without a field
//            of its own, to the job's map in the workspace.  A caller's field is copied to the same place instead.
//   slab     ONE WAVEFRONT a (job, slab), found by stat_find in the prefix of the slabs of the launch.  The slab's whole
//            bit grid lives in registers: lane j owns row j as one 64-bit `open` word and one `fill` word, so the flood
//            fill needs no LDS and no workgroup barrier.  Rows j = 0 .. ny - 1: lane i loads U(i, j, l) (a coalesced
//            512 B), one __ballot of "not +inf and <= cap" is the row's word and lane j keeps it; then the planes as
//            cav_classify does, 64 at a time through lane reads (no capacity in m), one __ballot a row.  Lane sj sets bit
//            si if open.  A sweep spreads inside the row (hop_fill_word: six doubling shifts each way) after OR-ing in
//            the rows above and below, taken by __shfl_up / __shfl_down of the two halves; the sweeps stop when a
//            __ballot of "changed" is zero.  Counts are popcounts; ranks come from a wave prefix of the row popcounts:
//            lane t of chunk c finds its row in the 64-entry prefix by six lane reads and its bit with aff_select,
//            reloads U, weighs it with pw_exp's table in LDS and runs pw_affinity_kernel's shuffle tree; lane b keeps
//            the running total of beta b, the chunk sums added in order.  The minimum goes through a butterfly on (U,
//            position).  Lane 0 writes the slab's record, lanes b < L its sums, lanes j < ny its words.
// Loop bounds: the rows (ny), the planes (m, 64 at a time), the sweeps (nx * ny + 1), the scan and the search (six
// steps), the chunks (ceil(n / 64) <= 64), the betas (L <= 8), the trees (six steps).  No workgroup waits for another;
// no floating-point atomics; no inline assembly.  Launches follow one another on the context's stream; memory is
// allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_field_dev.hpp"
#include "pw_hop.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_hop(const pw_hop_job* jobs, long n_jobs, const double* xyz, const double* coef,
                               const double* planes, const double* field, const double* betas, pw_hop_slab* slabs,
                               pw_affinity_level* sums, pw_hop_out* out, unsigned long long* words, int threads);   // pw_hostpath.cpp

static_assert(PW_HOP_CLAMPED == HOP_CLAMPED, "the header's constants and the kernel's");
static_assert(sizeof(pw_hop_job) == 176 && sizeof(pw_hop_slab) == 32 && sizeof(pw_hop_out) == 16, "the layouts of the header");

namespace {

typedef cavity_word u64;

// a job as the kernels read it: firsts relative to the spans of the arrays that were uploaded
struct HopJobDev {
    long atom_first, n, coef_first, plane_first, m;
    long map_first;            // the job's V doubles in the workspace of its launch
    long item_first, chunks;   // the job's chunks among the work items of the field kernel (none: a caller's field)
    long slab_first;           // the job's first slab among the wavefronts of the slab kernel of its launch
    long V;
    long beta_first;
    long res_first;            // the job's nz records in the compact result of the call (an 8-byte word index)
    long resw_first;           // the job's ny * nz words in the compact result, or -1
    double o[3], h, core2, cutoff2, cap;
    int nx, ny, nz, L, si, sj;
};

__global__ void __launch_bounds__(AFF_CHUNK)
pw_hop_field_kernel(const HopJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                    const double* __restrict__ coef, u64* __restrict__ ws) {
    field_items(jobs, n_jobs, total, xyz, coef, ws);
}

// the word that lane `from` holds (a lane of its own for every lane)
__device__ inline u64 hop_word_of(u64 v, int from) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, from), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), from);
    return ((u64)hi << 32) | lo;
}

__global__ void __launch_bounds__(AFF_CHUNK)
pw_hop_kernel(const HopJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ planes,
              const double* __restrict__ betas, const u64* __restrict__ ws, u64* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += AFF_CHUNK) s_tab[t] = POW_EXP_TAB[t];
    __syncthreads();                                                 // (the only barrier: one wavefront, before any work)
    const int q = stat_find(n_jobs, (long)blockIdx.x, [&](int t) { return jobs[t].slab_first; });
    const HopJobDev& D = jobs[q];
    const int l = (int)((long)blockIdx.x - D.slab_first);
    const int nx = D.nx, ny = D.ny, L = D.L;
    const u64* map = ws + D.map_first + (long)l * ny * nx;
    const double h = D.h, cap = D.cap;
    const double x = cavity_coord(D.o[0], lane, h), z = cavity_coord(D.o[2], l, h);

    // the open words: the field, then the planes
    u64 open = 0;
    for (int j = 0; j < ny; ++j) {
        bool ok = false;
        if (lane < nx) ok = hop_admits(pw_bits2d(map[(long)j * nx + lane]), cap);
        const u64 word = __ballot(ok);
        if (lane == j) open = word;
    }
    const double* cuts = planes + 4 * D.plane_first;
    for (long base = 0; base < D.m; base += 64) {
        const long p = base + lane;
        double pa = 0.0, pb = 0.0, pc = 0.0, pd = 0.0;
        if (p < D.m) {
            pa = cuts[4 * p]; pb = cuts[4 * p + 1]; pc = cuts[4 * p + 2]; pd = cuts[4 * p + 3];
        }
        const int count = D.m - base < 64 ? (int)(D.m - base) : 64;
        for (int j = 0; j < ny; ++j) {
            const double y = cavity_coord(D.o[1], j, h);
            bool held = true;
            for (int b = 0; b < count; ++b)
                held = held && cavity_inside(cav_lane(pa, b), cav_lane(pb, b), cav_lane(pc, b), cav_lane(pd, b), x, y, z);
            const u64 word = __ballot(held);
            if (lane == j) open &= word;
        }
    }

    // the seed and the sweeps
    u64 fill = lane == D.sj ? open & (1ull << D.si) : 0ull;
    const int max_sweeps = nx * ny + 1;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        const int lo = (int)(unsigned)fill, hi = (int)(unsigned)(fill >> 32);
        u64 above = ((u64)(unsigned)__shfl_up(hi, 1) << 32) | (unsigned)__shfl_up(lo, 1);
        u64 below = ((u64)(unsigned)__shfl_down(hi, 1) << 32) | (unsigned)__shfl_down(lo, 1);
        if (lane == 0) above = 0;                                    // (a shuffle past the wave's end returns the lane's own)
        if (lane == 63) below = 0;
        const u64 g = hop_fill_word(fill | above | below, open);
        const bool changed = g != fill;
        fill = g;
        if (!__ballot(changed)) break;
    }

    // counts, and the exclusive prefix of the rows' voxels
    const int cnt = cavity_popcount(fill);
    int incl = cnt, face = hop_row_face(fill, nx, ny, lane);         // (a lane past ny holds no voxel)
    for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(incl, s);
        if (lane >= s) incl += t;
    }
    for (int s = 32; s >= 1; s >>= 1) face += __shfl_xor(face, s);
    const int excl = incl - cnt, n = __shfl(incl, 63);

    // the sums, chunk after chunk; lane b keeps the totals of beta b
    double z_total = 0.0, e_total = 0.0, best = aff_inf();
    int best_pos = 0x7fffffff;
    bool clamped = false;
    for (int c = 0; c * AFF_CHUNK < n; ++c) {
        const int rank = c * AFF_CHUNK + lane;
        const bool valid = rank < n;
        int row = 0;                                                 // the last row whose prefix is <= rank: it holds it
        for (int step = 32; step >= 1; step >>= 1) {
            const int cand = row + step;
            const int before = __shfl(excl, cand & 63);
            if (cand < 64 && before <= rank) row = cand;
        }
        const u64 word = hop_word_of(fill, row);
        const int first = __shfl(excl, row);
        double U = 0.0;
        int pos = 0x7fffffff;
        if (valid) {
            const int i = aff_select(word, rank - first);
            U = pw_bits2d(map[(long)row * nx + i]);
            pos = row * 64 + i;
        }
        if (valid && hop_before(U, pos, best, best_pos)) {
            best = U;
            best_pos = pos;
        }
        for (int b = 0; b < L; ++b) {
            bool over = false;
            const double w = aff_weight(betas[D.beta_first + b], U, s_tab, over);
            clamped = clamped || (valid && over);
            double sz = valid ? w : 0.0, se = valid ? w * U : 0.0;
            for (int s = 1; s < AFF_CHUNK; s <<= 1) {
                sz = sz + __shfl_down(sz, s);
                se = se + __shfl_down(se, s);
            }
            const double cz = cav_lane(sz, 0), ce = cav_lane(se, 0);
            if (lane == b) {
                z_total = z_total + cz;
                e_total = e_total + ce;
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double other = __shfl_xor(best, s);
        const int other_pos = __shfl_xor(best_pos, s);
        if (hop_before(other, other_pos, best, best_pos)) {
            best = other;
            best_pos = other_pos;
        }
    }
    const u64 any_clamped = __ballot(clamped);

    u64* R = res + D.res_first + (long)l * hop_record_words(L);
    if (lane == 0) {
        R[0] = (u64)n;
        R[1] = (u64)face;
        R[2] = pw_d2bits(best);
        R[3] = n ? (u64)(unsigned)(best_pos & 63) | ((u64)(unsigned)(best_pos >> 6) << 32) : ~0ull;
        R[4] = any_clamped ? (u64)HOP_CLAMPED : 0ull;
    }
    if (lane < L) {
        R[HOP_FIXED_WORDS + 2 * lane] = pw_d2bits(z_total);
        R[HOP_FIXED_WORDS + 2 * lane + 1] = pw_d2bits(e_total);
    }
    if (D.resw_first >= 0 && lane < ny) res[D.resw_first + (long)l * ny + lane] = fill;
}

const char* const ENTRY = "pw_hop";
int hop_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written
int hop_check(const pw_hop_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
              const double* planes, long n_planes, const double* field, long n_field, const double* betas, long n_betas,
              const pw_hop_slab* slabs, long n_slabs, const pw_affinity_level* sums, long n_sums, long n_out,
              const uint64_t* words, long n_words) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_hop_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        if (J.seed[0] < 0 || J.seed[0] >= J.nx || J.seed[1] < 0 || J.seed[1] >= J.ny)
            return hop_bad(k, "the seed column is outside the grid");
        const long rows = (long)J.ny * J.nz, V = rows * J.nx, L = (long)J.n_betas;
        const bool lj = J.field_first == -1;
        if (J.n < 0 || J.m < 0) return hop_bad(k, "a negative count");
        GRID_CHECK(grid_n_betas_check(ENTRY, k, L));
        if (lj && span_outside(J.atom_first, J.n, n_points)) return hop_bad(k, "atoms outside xyz");
        if (lj && span_outside(J.coef_first, J.n, n_coef)) return hop_bad(k, "coefficients outside coef");
        if (span_outside(J.plane_first, J.m, n_planes)) return hop_bad(k, "planes outside the array");
        if (J.field_first < -1 || (!lj && span_outside(J.field_first, V, n_field))) return hop_bad(k, "the field is outside its array");
        if (span_outside(J.beta_first, L, n_betas)) return hop_bad(k, "betas outside the array");
        if (span_outside(J.slab_first, J.nz, n_slabs)) return hop_bad(k, "the rows are outside slabs");
        if (span_outside(J.sum_first, J.nz * L, n_sums)) return hop_bad(k, "the pairs are outside sums");
        if (J.word_first < -1 || (J.word_first >= 0 && span_outside(J.word_first, rows, n_words)))
            return hop_bad(k, "the words are outside their array");
        if (span_outside(J.out, 1, n_out)) return hop_bad(k, "the row is outside out");
        if ((lj && J.n && (!xyz || !coef)) || (J.m && !planes) || (!lj && !field) || !betas || !slabs || !sums ||
            (J.word_first >= 0 && !words))
            return hop_bad(k, "null array");
        GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
        if (!pw_finite(J.cap)) return hop_bad(k, "the cap is not finite");
        GRID_CHECK(grid_betas_check(ENTRY, k, betas, J.beta_first, L));
        GRID_CHECK(grid_planes_check(ENTRY, k, planes, J.plane_first, J.m));
        if (!lj) {
            GRID_CHECK(grid_field_check(ENTRY, k, field, J.field_first, V));
            continue;
        }
        GRID_CHECK(grid_core_check(ENTRY, k, J.core2, J.cutoff2));
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its row)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_coef_check(ENTRY, k, coef, J.coef_first + a, 1, 2, false));
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of slabs with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].slab_first, (long)jobs[k].nz}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares pairs of sums with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].sum_first, (long)jobs[k].nz * (long)jobs[k].n_betas}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares a row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    return shared_output(ENTRY, n_jobs, "shares words with an earlier job", [&](long k) {
        const pw_hop_job& J = jobs[k];
        return OutSpan{(long)J.word_first, J.word_first >= 0 ? (long)J.ny * J.nz : 0};
    });
}

// the marks between the kernels of a call, for the measurement entry: mark() records an event, the times of the odd and
// of the even gaps are summed once the stream is synchronised.  off: nothing is made
struct Marks {
    bool on;
    std::vector<hipEvent_t> ev;
    explicit Marks(bool enabled) : on(enabled) {}
    ~Marks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipError_t mark(hipStream_t st) {
        if (!on) return hipSuccess;
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, st);
    }
    // marks come in threes a launch group: before the field kernel, after it, after the slab kernel
    hipError_t read(float* field_ms, float* slab_ms) {
        *field_ms = *slab_ms = 0.0f;
        for (size_t g = 0; on && 3 * g + 2 < ev.size(); ++g) {
            float a = 0.0f, b = 0.0f;
            hipError_t rc = hipEventElapsedTime(&a, ev[3 * g], ev[3 * g + 1]);
            if (rc == hipSuccess) rc = hipEventElapsedTime(&b, ev[3 * g + 1], ev[3 * g + 2]);
            if (rc != hipSuccess) return rc;
            *field_ms += a;
            *slab_ms += b;
        }
        return hipSuccess;
    }
};

// workspace_bytes: the budget of the maps of the jobs of one launch (0: HOP_WORKSPACE_BYTES; at 1 every job is a launch
// of its own); kernel_ms: when not null, three floats -- the time of the device work of the call from the first launch
// to the last, the copies between them included, then the field kernels' and the slab kernels' share of it, by HIP
// events on the context's stream
int hop(pw_context* ctx, const pw_hop_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points, const double* coef,
        int64_t n_coef, const double* planes, int64_t n_planes, const double* field, int64_t n_field, const double* betas,
        int64_t n_betas, pw_hop_slab* slabs, int64_t n_slabs, pw_affinity_level* sums, int64_t n_sums, pw_hop_out* out,
        int64_t n_out, uint64_t* words, int64_t n_words, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 ||
        n_planes < 0 || n_field < 0 || n_betas < 0 || n_slabs < 0 || n_sums < 0 || n_out < 0 || n_words < 0 ||
        workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = hop_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, planes, (long)n_planes, field, (long)n_field,
                             betas, (long)n_betas, slabs, (long)n_slabs, sums, (long)n_sums, (long)n_out, words, (long)n_words);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_hop(jobs, N, xyz, coef, planes, field, betas, slabs, sums, out, (unsigned long long*)words,
                               pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their maps
    // fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : HOP_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab, windows, beta_span;
    for (long k = 0; k < N; ++k) {
        const pw_hop_job& J = jobs[k];
        if (J.field_first == -1) {
            atoms.widen((long)J.atom_first, (long)J.n);
            rows_ab.widen((long)J.coef_first, (long)J.n);
        }
        windows.widen((long)J.plane_first, (long)J.m);
        beta_span.widen((long)J.beta_first, (long)J.n_betas);
    }
    std::vector<HopJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long res_words = 0;
    for (long k = 0; k < N; ++k) {
        const pw_hop_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, V = rows * J.nx;
        const bool lj = J.field_first == -1;
        place(groups, cur, budget_words, V);
        HopJobDev& D = devs[k];
        D.n = lj ? (long)J.n : 0;
        D.atom_first = atoms.rel((long)J.atom_first, D.n);
        D.coef_first = rows_ab.rel((long)J.coef_first, D.n);
        D.plane_first = windows.rel((long)J.plane_first, (long)J.m);
        D.m = (long)J.m;
        D.map_first = cur.words;
        D.item_first = cur.items;
        D.chunks = lj ? (V + AFF_CHUNK - 1) / AFF_CHUNK : 0;
        D.slab_first = cur.blocks;
        D.V = V;
        D.beta_first = (long)J.beta_first - beta_span.lo;
        D.res_first = res_words;
        res_words += (long)J.nz * hop_record_words((int)J.n_betas);
        D.resw_first = J.word_first >= 0 ? res_words : -1;
        if (J.word_first >= 0) res_words += rows;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        D.h = J.spacing; D.core2 = J.core2; D.cutoff2 = J.cutoff2; D.cap = J.cap;
        D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.L = (int)J.n_betas; D.si = J.seed[0]; D.sj = J.seed[1];
        cur.words += V; cur.cost += V; cur.items += D.chunks; cur.blocks += J.nz; cur.last += 1;
    }
    groups.push_back(cur);

    const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), res_bytes = sizeof(u64) * (size_t)res_words;
    std::vector<u64> res((size_t)res_words);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    Marks marks(kernel_ms != nullptr);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        HopJobDev* d_jobs;
        double *d_xyz, *d_coef, *d_planes, *d_betas;
        u64 *d_ws, *d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(HopJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(HopJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, 2));
        STAT_TRY(windows.upload(buf, &d_planes, planes, 4));
        STAT_TRY(beta_span.upload(buf, &d_betas, betas, 1));         // (every job has a beta: never empty)
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one takes the workspace over when this one is done)
        for (const LaunchGroup& G : groups) {
            const unsigned n_group = (unsigned)(G.last - G.first);
            for (long k = G.first; k < G.last; ++k)
                if (jobs[k].field_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].map_first, field + jobs[k].field_first, sizeof(double) * (size_t)devs[k].V,
                                            hipMemcpyHostToDevice, st));
            STAT_TRY(marks.mark(st));
            if (G.items) {
                const long blocks = launch_blocks(G.items, 65536);
                hipLaunchKernelGGL(pw_hop_field_kernel, dim3((unsigned)blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                                   (int)n_group, G.items, d_xyz, d_coef, d_ws);
                STAT_TRY(hipGetLastError());
            }
            STAT_TRY(marks.mark(st));
            hipLaunchKernelGGL(pw_hop_kernel, dim3((unsigned)G.blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first, (int)n_group,
                               d_planes, d_betas, d_ws, d_res);
            STAT_TRY(hipGetLastError());
            STAT_TRY(marks.mark(st));
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    if (kernel_ms) STAT_TRY(marks.read(kernel_ms + 1, kernel_ms + 2));
    // the caller's rows, job by job
    for (long k = 0; k < N; ++k) {
        const pw_hop_job& J = jobs[k];
        const int L = (int)J.n_betas, stride = hop_record_words(L);
        pw_hop_out o{0, 0, 0};
        for (long l = 0; l < J.nz; ++l) {
            const u64* R = res.data() + devs[k].res_first + l * stride;
            pw_hop_slab s;
            s.n = (int64_t)R[0];
            s.n_face = (int64_t)R[1];
            s.u_min = pw_bits2d(R[2]);
            s.min_i = (int32_t)(unsigned)R[3];
            s.min_j = (int32_t)(unsigned)(R[3] >> 32);
            slabs[J.slab_first + l] = s;
            o.n += s.n;
            o.flags |= (int32_t)R[4];
            for (int b = 0; b < L; ++b)
                sums[J.sum_first + l * L + b] = pw_affinity_level{pw_bits2d(R[HOP_FIXED_WORDS + 2 * b]), pw_bits2d(R[HOP_FIXED_WORDS + 2 * b + 1])};
        }
        out[J.out] = o;
        if (J.word_first >= 0)
            memcpy(words + J.word_first, res.data() + devs[k].resw_first, sizeof(u64) * (size_t)J.ny * (size_t)J.nz);
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_hop(pw_context* ctx, const pw_hop_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                      const double* coef, int64_t n_coef, const double* planes, int64_t n_planes, const double* field,
                      int64_t n_field, const double* betas, int64_t n_betas, pw_hop_slab* slabs, int64_t n_slabs,
                      pw_affinity_level* sums, int64_t n_sums, pw_hop_out* out, int64_t n_out, uint64_t* words,
                      int64_t n_words) {
    return hop(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, planes, n_planes, field, n_field, betas, n_betas, slabs,
               n_slabs, sums, n_sums, out, n_out, words, n_words, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_hop with the budget of the workspace of a launch given (0: the
// default; the result may not depend on it) and, when kernel_ms is not null, three floats: the device work of the call
// by HIP events, then the field kernels' and the slab kernels' share of it
extern "C" int pw_internal_hop(pw_context* ctx, const pw_hop_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                               const double* coef, int64_t n_coef, const double* planes, int64_t n_planes,
                               const double* field, int64_t n_field, const double* betas, int64_t n_betas,
                               pw_hop_slab* slabs, int64_t n_slabs, pw_affinity_level* sums, int64_t n_sums, pw_hop_out* out,
                               int64_t n_out, uint64_t* words, int64_t n_words, int64_t workspace_bytes, float* kernel_ms) {
    return hop(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, planes, n_planes, field, n_field, betas, n_betas, slabs,
               n_slabs, sums, n_sums, out, n_out, words, n_words, workspace_bytes, kernel_ms);
}
