// pw_passage.hip -- gfx950 kernels and the C ABI entry of the barrier a guest crosses at every window of a cage
// (include/pywindow_amd.h: pw_passage; definition of the result, the keys and why the bisection is exact in
// pw_passage.hpp; the seed and fill steps in pw_cavity_dev.hpp, shared with pw_cavity.hip and pw_pores.hip).  Two
// kernels a launch group:
//   field    for the jobs without a field of their own: a work item is (job, chunk of 64 ranks of the whole box) and a
//            wavefront takes one item after the other, the job of an item found by binary search in the prefix of work
//            items.  A lane is a rank, to its voxel by one division.  The atoms go through LDS PAS_FIELD_TILE at a time
//            and are read at one address per wave, so there is no capacity in n.  The pair terms are pw_affinity.hpp's in
//            pw_affinity_kernel's order; the lane writes U, +inf where blocked, to the job's map in the workspace.  A
//            caller's field is copied to the same place instead.
//   passage  a workgroup of CAV_THREADS a (job, row k), four bit grids of ny * nz words in dynamic LDS: `held` (the
//            planes but plane k, built once as cav_classify does its planes: a wave a row, lane i voxel i, the planes 64
//            at a time through lane reads), `open` (the level's allowed voxels), `fill` and `low`.  A LEVEL PASS reads
//            the map, a wave a row, sixteen rows' loads in flight: one __ballot of key <= mid is the row's open word, and
//            on the way every lane keeps the largest key <= mid and the smallest finite key > mid it saw, which two
//            shuffle trees and four LDS slots turn into the workgroup's.  The map is read where the answer is not known:
//            a level that passed leaves its open words in `held` (above it nothing is allowed again), one that failed
//            leaves them in `low` (allowed at every later level), and only the lanes of held voxels outside `low` load --
//            after a few steps a few voxels a row.  Then
//            cav_seed and cav_fill, and "a fill bit on a face" OR-ed by __syncthreads_or.  The first pass is at the
//            largest finite key: it gives the upper bound and NO_EXIT; the bisection follows (at most PAS_MAX_STEPS
//            steps, the bounds moved to voxel keys after every step); one fill at B with a pass over the filled voxels
//            for the count, the saddle (the lowest rank with key == B) and the well ((key, rank) pairs in order); one
//            fill at the key before B for the basin.  Thread 0 writes the row of the compact result.
// Every loop is bounded by n, m, the rows, the chunks, PAS_MAX_STEPS or cav_fill's nx * ny * nz + 1; no workgroup waits
// for another; no floating-point atomics.  Launches follow one another on the context's stream; memory is allocated
// and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_field_dev.hpp"
#include "pw_passage.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_passage(const pw_passage_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                   const double* planes, const double* field, pw_passage_out* out, int* fills,
                                   int threads);   // pw_hostpath.cpp

static_assert(PW_PAS_SEED_CLOSED == PAS_SEED_CLOSED && PW_PAS_NO_EXIT == PAS_NO_EXIT, "the header's constants and the kernel's");
static_assert(sizeof(pw_passage_job) == 128 && sizeof(pw_passage_out) == 72, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int PAS_WAVES = CAV_THREADS / 64;
constexpr int PAS_UNROLL = 16;                                   // rows of a wave whose loads are in flight together
constexpr int PAS_SCRATCH_WORDS = 4 * PAS_WAVES + 2;             // keys and ranks of the waves, a count
constexpr int PAS_GRIDS = 4;                                     // held, open, fill, low (3: without low, to measure it)
constexpr size_t pas_lds_bytes(long rows, int grids) { return 8 * ((size_t)grids * rows + PAS_SCRATCH_WORDS); }

// a job as the kernels read it: firsts relative to the spans of the arrays that were uploaded
struct PasJobDev {
    long atom_first, n, coef_first, plane_first, m;
    long map_first;            // the job's V doubles in the workspace of its launch
    long item_first, chunks;   // the job's chunks among the work items of the field kernel (none: a caller's field)
    long row_first;            // the job's first row among the workgroups of the passage kernel of its launch
    long V;
    double o[3], h, core2, cutoff2;
    int nx, ny, nz, seed[3];
};

__global__ void __launch_bounds__(AFF_CHUNK)
pw_passage_field_kernel(const PasJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                        const double* __restrict__ coef, u64* __restrict__ ws) {
    field_items(jobs, n_jobs, total, xyz, coef, ws);                 // (pw_field_dev.hpp, shared with pw_hop.hip)
}

// held: a wave takes rows (j, l), lane i is voxel i; every plane but `skip`, 64 at a time.  LOW: the kernel keeps s_low
template <bool LOW>
__device__ inline void pas_held(const double* __restrict__ cuts, long m, long skip, double ox, double oy, double oz,
                                double h, int nx, int ny, int rows, u64* s_held, u64* s_low) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = cavity_coord(ox, lane, h);
    for (int r = wave; r < rows; r += PAS_WAVES) {
        const double y = cavity_coord(oy, r % ny, h), z = cavity_coord(oz, r / ny, h);
        bool held = lane < nx;
        for (long base = 0; base < m; base += 64) {
            const long q = base + lane;
            double pa = 0.0, pb = 0.0, pc = 0.0, pd = 0.0;
            if (q < m) {
                pa = cuts[4 * q]; pb = cuts[4 * q + 1]; pc = cuts[4 * q + 2]; pd = cuts[4 * q + 3];
            }
            const int count = m - base < 64 ? (int)(m - base) : 64;
            for (int b = 0; b < count; ++b) {
                if (base + b == skip) continue;
                held = held && cavity_inside(cav_lane(pa, b), cav_lane(pb, b), cav_lane(pc, b), cav_lane(pd, b), x, y, z);
            }
        }
        const u64 word = __ballot(held);
        if (lane == 0) {
            s_held[r] = word;
            if (LOW) s_low[r] = 0;
        }
    }
}

// a level pass: s_open[r] = the held voxels of row r with key <= mid and s_fill[r] = 0.  s_held holds the CANDIDATES, the
// held voxels with key <= the upper bound, and s_low the voxels known to be at or below the lower bound (pas_narrow):
// only the candidates outside s_low are loaded, the voxels of s_low are allowed as they are.  below / above: the largest
// key <= mid and the smallest finite key > mid of a loaded voxel (0 / PAS_KEY_NONE without one), the same in every
// thread.  The workgroup passes two barriers here, the second one after the last read of s_red.  Without LOW there is no
// s_low: every candidate loads.
template <bool LOW>
__device__ inline void pas_level(const u64* __restrict__ map, int nx, int rows, u64 mid, const u64* s_held, const u64* s_low,
                                 u64* s_open, u64* s_fill, u64* s_red, u64& below, u64& above) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 lo_best = 0, hi_best = PAS_KEY_NONE;
    for (int r0 = wave; r0 < rows; r0 += PAS_WAVES * PAS_UNROLL) {
        u64 key[PAS_UNROLL], low[PAS_UNROLL];
#pragma unroll
        for (int u = 0; u < PAS_UNROLL; ++u) {
            const int r = r0 + PAS_WAVES * u;
            key[u] = PAS_KEY_NONE;
            low[u] = LOW && r < rows ? s_low[r] : 0;
            const u64 todo = r < rows ? s_held[r] & ~low[u] : 0;
            if ((todo >> lane) & 1ull) key[u] = pas_key(pw_bits2d(map[(long)r * nx + lane]));
        }
#pragma unroll
        for (int u = 0; u < PAS_UNROLL; ++u) {
            const int r = r0 + PAS_WAVES * u;
            if (r < rows) {                                          // (the same in every lane)
                const bool in = key[u] <= mid;
                const u64 word = __ballot(in) | low[u];         // (a lane that did not load holds PAS_KEY_NONE)
                if (lane == 0) {
                    s_open[r] = word;
                    s_fill[r] = 0;
                }
                if (in) lo_best = key[u] > lo_best ? key[u] : lo_best;
                else if (key[u] < PAS_KEY_INF) hi_best = key[u] < hi_best ? key[u] : hi_best;
            }
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 a = __shfl_xor(lo_best, s), b = __shfl_xor(hi_best, s);
        lo_best = a > lo_best ? a : lo_best;
        hi_best = b < hi_best ? b : hi_best;
    }
    if (lane == 0) {
        s_red[wave] = lo_best;
        s_red[PAS_WAVES + wave] = hi_best;
    }
    __syncthreads();
    below = 0;
    above = PAS_KEY_NONE;
    for (int w = 0; w < PAS_WAVES; ++w) {
        below = s_red[w] > below ? s_red[w] : below;
        above = s_red[PAS_WAVES + w] < above ? s_red[PAS_WAVES + w] : above;
    }
    __syncthreads();
}

// seed and fill the level that pas_level left; true iff the fill has a voxel on a face of the grid (every thread)
__device__ inline bool pas_fill(const int* seed, const u64* s_open, u64* s_fill, int nx, int ny, int nz) {
    cav_seed(seed, ny, s_open, s_fill);
    cav_fill(s_open, s_fill, nx, ny, nz);
    int hit = 0;
    for (int r = threadIdx.x; r < ny * nz; r += CAV_THREADS) {
        const u64 f = s_fill[r];
        if (f && cavity_row_face(f, nx, ny, nz, r % ny, r / ny)) hit = 1;
    }
    return __syncthreads_or(hit) != 0;
}

// after a level's fill: a level that passed is the new upper bound and its open words the candidates; one that failed
// the new lower bound and its open words, all of them allowed at every later level, go to s_low (with LOW).  One barrier
template <bool LOW>
__device__ inline void pas_narrow(bool passed, const u64* s_open, u64* s_held, u64* s_low, int rows) {
    if (!LOW && !passed) return;                                     // (the same in every thread)
    u64* to = passed ? s_held : s_low;
    for (int r = threadIdx.x; r < rows; r += CAV_THREADS) to[r] = s_open[r];
    __syncthreads();
}

// the voxels of the fill, the same in every thread; two barriers, the second after the last read of the count
__device__ inline long pas_count(const u64* s_fill, int rows, u64* s_red) {
    unsigned long long* total = (unsigned long long*)(s_red + 4 * PAS_WAVES);
    if (threadIdx.x == 0) *total = 0;
    __syncthreads();
    long mine = 0;
    for (int r = threadIdx.x; r < rows; r += CAV_THREADS) mine += cavity_popcount(s_fill[r]);
    if (mine) atomicAdd(total, (unsigned long long)mine);
    __syncthreads();
    const long n = (long)*total;
    __syncthreads();
    return n;
}

// over the voxels of the fill: the (key, rank) that is first in order -- the well -- and the lowest rank with key == B
// (-1: none), the same in every thread; two barriers
__device__ inline void pas_measure(const u64* __restrict__ map, int nx, int rows, u64 B, const u64* s_fill, u64* s_red,
                                   u64& well_key, long& well_rank, long& saddle_rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr long NO_RANK = 0x7fffffffffffffffl;
    u64 wk = PAS_KEY_NONE;
    long wr = NO_RANK, sr = NO_RANK;
    for (int r0 = wave; r0 < rows; r0 += PAS_WAVES * PAS_UNROLL) {
        u64 key[PAS_UNROLL];
#pragma unroll
        for (int u = 0; u < PAS_UNROLL; ++u) {
            const int r = r0 + PAS_WAVES * u;
            const u64 f = r < rows ? s_fill[r] : 0;
            key[u] = PAS_KEY_NONE;
            if ((f >> lane) & 1ull) key[u] = pas_key(pw_bits2d(map[(long)r * nx + lane]));
        }
#pragma unroll
        for (int u = 0; u < PAS_UNROLL; ++u) {
            const long rank = (long)(r0 + PAS_WAVES * u) * nx + lane;
            if (key[u] == PAS_KEY_NONE) continue;
            if (pas_before(key[u], rank, wk, wr)) {
                wk = key[u];
                wr = rank;
            }
            if (key[u] == B && rank < sr) sr = rank;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 ok = __shfl_xor(wk, s);
        const long orank = __shfl_xor(wr, s), os = __shfl_xor(sr, s);
        if (pas_before(ok, orank, wk, wr)) {
            wk = ok;
            wr = orank;
        }
        sr = os < sr ? os : sr;
    }
    if (lane == 0) {
        s_red[wave] = wk;
        s_red[PAS_WAVES + wave] = (u64)wr;
        s_red[2 * PAS_WAVES + wave] = (u64)sr;
    }
    __syncthreads();
    wk = PAS_KEY_NONE;
    wr = sr = NO_RANK;
    for (int w = 0; w < PAS_WAVES; ++w) {
        const u64 ok = s_red[w];
        const long orank = (long)s_red[PAS_WAVES + w], os = (long)s_red[2 * PAS_WAVES + w];
        if (pas_before(ok, orank, wk, wr)) {
            wk = ok;
            wr = orank;
        }
        sr = os < sr ? os : sr;
    }
    __syncthreads();
    well_key = wk;
    well_rank = wr == NO_RANK ? -1 : wr;
    saddle_rank = sr == NO_RANK ? -1 : sr;
}

// the row of the compact result; `reserved` carries the number of fills to the host, which clears it
template <bool LOW>
__global__ void __launch_bounds__(CAV_THREADS)
pw_passage_kernel(const PasJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ planes,
                  const u64* __restrict__ ws, pw_passage_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int q = stat_find(n_jobs, (long)blockIdx.x, [&](int t) { return jobs[t].row_first; });
    const PasJobDev& D = jobs[q];
    const long k = (long)blockIdx.x - D.row_first;
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz;
    u64* s_held = (u64*)lds;
    u64* s_open = s_held + rows;
    u64* s_fill = s_open + rows;
    u64* s_low = s_fill + rows;                                      // (with LOW; otherwise the scratch starts here)
    u64* s_red = LOW ? s_low + rows : s_low;
    const u64* map = ws + D.map_first;
    const int tid = threadIdx.x;
    pw_passage_out* O = out + blockIdx.x;

    pas_held<LOW>(planes + 4 * D.plane_first, D.m, k, D.o[0], D.o[1], D.o[2], D.h, nx, ny, rows, s_held, s_low);
    __syncthreads();
    const int seed_row = D.seed[2] * ny + D.seed[1];
    const long seed_rank = (long)seed_row * nx + D.seed[0];
    const u64 seed_bits = map[seed_rank], seed_key = pas_key(pw_bits2d(seed_bits));
    const bool seed_ok = ((s_held[seed_row] >> D.seed[0]) & 1ull) && seed_key != PAS_KEY_INF;
    if (!seed_ok) {                                                  // (the same in every thread)
        if (tid == 0) {
            O->barrier = O->well = aff_inf();
            O->u_seed = pw_bits2d(seed_bits);
            O->n_fill = O->n_basin = 0;
            for (int a = 0; a < 3; ++a) O->saddle[a] = O->well_voxel[a] = -1;
            O->flags = PAS_SEED_CLOSED;
            O->reserved = 0;
        }
        return;
    }

    // the largest finite level: the upper bound, and whether there is an exit at all
    int fills = 1, flags = 0;
    u64 below, above, B = PAS_KEY_NONE;
    pas_level<LOW>(map, nx, rows, PAS_KEY_INF - 1, s_held, s_low, s_open, s_fill, s_red, below, above);
    long n_fill, n_basin;
    const bool exit = pas_fill(D.seed, s_open, s_fill, nx, ny, nz);
    pas_narrow<LOW>(true, s_open, s_held, s_low, rows);                   // (the blocked voxels are no candidates)
    if (!exit) {
        flags = PAS_NO_EXIT;
        n_fill = n_basin = pas_count(s_fill, rows, s_red);
    } else {
        u64 lo = seed_key, hi = below;                               // P(hi), and not P(t) for every t < lo
        for (int step = 0; step < PAS_MAX_STEPS && lo < hi; ++step) {
            const u64 mid = lo + ((hi - lo) >> 1);
            pas_level<LOW>(map, nx, rows, mid, s_held, s_low, s_open, s_fill, s_red, below, above);
            ++fills;
            const bool passed = pas_fill(D.seed, s_open, s_fill, nx, ny, nz);
            if (!passed && above > hi) break;                        // (cannot be: P(hi) and not P(mid))
            pas_narrow<LOW>(passed, s_open, s_held, s_low, rows);
            if (passed) hi = below; else lo = above;
        }
        B = hi;
        n_basin = 0;
        if (seed_key < B) {
            pas_level<LOW>(map, nx, rows, B - 1, s_held, s_low, s_open, s_fill, s_red, below, above);
            pas_fill(D.seed, s_open, s_fill, nx, ny, nz);
            n_basin = pas_count(s_fill, rows, s_red);
            ++fills;
        }
        pas_level<LOW>(map, nx, rows, B, s_held, s_low, s_open, s_fill, s_red, below, above);
        pas_fill(D.seed, s_open, s_fill, nx, ny, nz);
        n_fill = pas_count(s_fill, rows, s_red);
        ++fills;
    }
    u64 well_key;
    long well_rank, saddle_rank;
    pas_measure(map, nx, rows, B, s_fill, s_red, well_key, well_rank, saddle_rank);
    if (tid == 0) {
        O->barrier = saddle_rank >= 0 ? pw_bits2d(map[saddle_rank]) : aff_inf();
        O->well = pw_bits2d(map[well_rank]);                         // (the seed voxel is in the fill: there is one)
        O->u_seed = pw_bits2d(seed_bits);
        O->n_fill = n_fill;
        O->n_basin = n_basin;
        const long ranks[2] = {saddle_rank, well_rank};
        for (int w = 0; w < 2; ++w) {
            int* v = w ? O->well_voxel : O->saddle;
            const long row = ranks[w] / nx;
            v[0] = ranks[w] >= 0 ? (int)(ranks[w] - row * nx) : -1;
            v[1] = ranks[w] >= 0 ? (int)(row % ny) : -1;
            v[2] = ranks[w] >= 0 ? (int)(row / ny) : -1;
        }
        O->flags = flags;
        O->reserved = fills;
    }
}

const char* const ENTRY = "pw_passage";
int pas_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written
int pas_check(const pw_passage_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
              const double* planes, long n_planes, const double* field, long n_field, long n_out) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_passage_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        if (J.seed[0] < 0 || J.seed[0] >= J.nx || J.seed[1] < 0 || J.seed[1] >= J.ny || J.seed[2] < 0 || J.seed[2] >= J.nz)
            return pas_bad(k, "the seed is outside the grid");
        const long V = (long)J.nx * J.ny * J.nz;
        const bool lj = J.field_first == -1;
        if (J.n < 0 || J.m < 0) return pas_bad(k, "a negative count");
        if (lj && span_outside(J.atom_first, J.n, n_points)) return pas_bad(k, "atoms outside xyz");
        if (lj && span_outside(J.coef_first, J.n, n_coef)) return pas_bad(k, "coefficients outside coef");
        if (span_outside(J.plane_first, J.m, n_planes)) return pas_bad(k, "planes outside the array");
        if (J.field_first < -1 || (!lj && span_outside(J.field_first, V, n_field))) return pas_bad(k, "the field is outside its array");
        if (span_outside(J.out_first, pas_rows_out((long)J.m), n_out)) return pas_bad(k, "the rows are outside out");
        if ((lj && J.n && (!xyz || !coef)) || (J.m && !planes) || (!lj && !field)) return pas_bad(k, "null array");
        GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
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
    return shared_output(ENTRY, n_jobs, "shares rows of out with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].out_first, (long)pas_rows_out((long)jobs[k].m)}; });
}

// workspace_bytes: the budget of the maps of the jobs of one launch (0: PAS_WORKSPACE_BYTES; at 1 every job is a launch
// of its own); kernel_ms: when not null, the time of the device work of the call from the first launch to the last, the
// copies between them included, by HIP events on the context's stream; fills: when not null, n_out integers of which a
// job's rows receive the number of flood fills the row took; grids: 4, or 3 for the kernel without s_low
int passage(pw_context* ctx, const pw_passage_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
            const double* coef, int64_t n_coef, const double* planes, int64_t n_planes, const double* field,
            int64_t n_field, pw_passage_out* out, int64_t n_out, int64_t workspace_bytes, float* kernel_ms, int32_t* fills,
            int grids) {
    if (grids != 3 && grids != PAS_GRIDS) return PW_E_BAD_ARG;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 ||
        n_planes < 0 || n_field < 0 || n_out < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = pas_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, planes, (long)n_planes, field, (long)n_field,
                             (long)n_out);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_passage(jobs, N, xyz, coef, planes, field, out, fills, pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their maps
    // fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : PAS_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab, windows;
    for (long k = 0; k < N; ++k) {
        const pw_passage_job& J = jobs[k];
        if (J.field_first == -1) {
            atoms.widen((long)J.atom_first, (long)J.n);
            rows_ab.widen((long)J.coef_first, (long)J.n);
        }
        windows.widen((long)J.plane_first, (long)J.m);
    }
    std::vector<PasJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    std::vector<long> res_first((size_t)N);
    LaunchGroup cur;
    long n_rows = 0;
    for (long k = 0; k < N; ++k) {
        const pw_passage_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, V = rows * J.nx, R = pas_rows_out((long)J.m);
        const bool lj = J.field_first == -1;
        place(groups, cur, budget_words, V);
        PasJobDev& D = devs[k];
        D.n = lj ? (long)J.n : 0;
        D.atom_first = atoms.rel((long)J.atom_first, D.n);
        D.coef_first = rows_ab.rel((long)J.coef_first, D.n);
        D.plane_first = windows.rel((long)J.plane_first, (long)J.m);
        D.m = (long)J.m;
        D.map_first = cur.words;
        D.item_first = cur.items;
        D.chunks = lj ? (V + AFF_CHUNK - 1) / AFF_CHUNK : 0;
        D.row_first = cur.blocks;
        D.V = V;
        for (int a = 0; a < 3; ++a) {
            D.o[a] = J.origin[a];
            D.seed[a] = J.seed[a];
        }
        D.h = J.spacing; D.core2 = J.core2; D.cutoff2 = J.cutoff2; D.nx = J.nx; D.ny = J.ny; D.nz = J.nz;
        res_first[k] = n_rows;
        n_rows += R;
        cur.words += V; cur.cost += V; cur.items += D.chunks; cur.blocks += R; cur.last += 1;
        cur.rows = rows > cur.rows ? rows : cur.rows;
    }
    groups.push_back(cur);

    const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), res_bytes = sizeof(pw_passage_out) * (size_t)n_rows;
    std::vector<pw_passage_out> res((size_t)n_rows);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    const auto kernel = grids == PAS_GRIDS ? pw_passage_kernel<true> : pw_passage_kernel<false>;
    STAT_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)pas_lds_bytes(CAVITY_MAX_G * CAVITY_MAX_G, grids)));
    {
        StreamBuffers buf(st);
        PasJobDev* d_jobs;
        double *d_xyz, *d_coef, *d_planes;
        u64* d_ws;
        pw_passage_out* d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(PasJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(PasJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, 2));
        STAT_TRY(windows.upload(buf, &d_planes, planes, 4));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one takes the workspace over when this one is done)
        long row0 = 0;
        for (const LaunchGroup& G : groups) {
            const unsigned n_group = (unsigned)(G.last - G.first);
            for (long k = G.first; k < G.last; ++k)
                if (jobs[k].field_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].map_first, field + jobs[k].field_first, sizeof(double) * (size_t)devs[k].V,
                                            hipMemcpyHostToDevice, st));
            if (G.items) {
                const long blocks = launch_blocks(G.items, 65536);
                hipLaunchKernelGGL(pw_passage_field_kernel, dim3((unsigned)blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                                   (int)n_group, G.items, d_xyz, d_coef, d_ws);
                STAT_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(kernel, dim3((unsigned)G.blocks), dim3(CAV_THREADS), pas_lds_bytes(G.rows, grids), st,
                               d_jobs + G.first, (int)n_group, d_planes, d_ws, d_res + row0);
            STAT_TRY(hipGetLastError());
            row0 += G.blocks;
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's rows, job by job
    for (long k = 0; k < N; ++k) {
        const long R = pas_rows_out((long)jobs[k].m);
        for (long r = 0; r < R; ++r) {
            pw_passage_out o = res[(size_t)(res_first[k] + r)];
            if (fills) fills[jobs[k].out_first + r] = o.reserved;
            o.reserved = 0;
            out[jobs[k].out_first + r] = o;
        }
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_passage(pw_context* ctx, const pw_passage_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                          const double* coef, int64_t n_coef, const double* planes, int64_t n_planes, const double* field,
                          int64_t n_field, pw_passage_out* out, int64_t n_out) {
    return passage(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, planes, n_planes, field, n_field, out, n_out, 0, nullptr,
                   nullptr, PAS_GRIDS);
}

// measurement and test hook (not part of the header): pw_passage with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it), the device work timed by HIP events when kernel_ms is not null, and
// the number of flood fills of every row in fills[0 .. n_out) when that is not null; grids (0 or 4: as pw_passage; 3: the
// passage kernel without its fourth bit grid, every candidate voxel loaded at every level -- what the grid buys is
// measured against this in one run, profiles/passage_times.py; the result may not depend on it)
extern "C" int pw_internal_passage(pw_context* ctx, const pw_passage_job* jobs, int64_t n_jobs, const double* xyz,
                                   int64_t n_points, const double* coef, int64_t n_coef, const double* planes,
                                   int64_t n_planes, const double* field, int64_t n_field, pw_passage_out* out,
                                   int64_t n_out, int64_t workspace_bytes, float* kernel_ms, int32_t* fills, int grids) {
    return passage(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, planes, n_planes, field, n_field, out, n_out,
                   workspace_bytes, kernel_ms, fills, grids ? grids : PAS_GRIDS);
}
