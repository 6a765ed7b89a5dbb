// pw_percolate.hip -- gfx950 kernels and the C ABI entry of the energy levels at which the voids of a periodic cell
// connect (include/pywindow_amd.h: pw_percolation; definition of the result, the proofs, the cull and the search in
// pw_percolate.hpp).  Two kernels a launch group:
//   field    for the jobs without a field of their own: field_items_cell (pw_field_cell_dev.hpp), pw_field_dev.hpp's
//            field_items on the skewed grid.  A work item is (job, chunk of 64 ranks), a wavefront takes one item after
//            the other, the atoms go through LDS PAS_FIELD_TILE at a time; no atom is skipped.  A caller's field is
//            copied to the job's map in the workspace instead.
//   levels   a workgroup of four waves a job, four bit grids of ny * nz words in dynamic LDS -- `allowed`, `todo` (the
//            face candidates not yet in a component), `p0` and `p1` (the parities of a fill) -- and 64 words of scratch
//            (128.5 KiB at 64 x 64 rows); the map stays in the workspace.  One scan of the map gives n_blocked, u_min and
//            the two ends of the keys.  AN EVALUATION of a level (perc_evaluate): a wave a row ballots key <= level into
//            the row's word, keeping the nearest keys on both sides; todo = perc_candidates; then pw_channels_kernel's
//            component loop by the same functions (pw_channels_dev.hpp) -- chan_first, the first bit of todo; chan_walk,
//            the component, its n_voxels and winding bits -- and the component leaves todo.  It stops
//            as soon as every criterion it was asked about is met.  The search of pw_percolate.hpp lives in LDS, stepped
//            by thread 0 between barriers; then one evaluation that goes through every candidate at each distinct B_c
//            writes the rows: of the components that meet a criterion, the one with the lowest first voxel, measured
//            (saddle, well) when it takes the lead.
// Every branch that leads to a barrier depends on values read from LDS after a barrier or reduced over the workgroup,
// the same in every thread.  Loops are bounded by n, the rows, the chunks, PERC_MAX_STEPS, the voxels (a turn of the
// component loop strikes a candidate off) and chan_fill's 2 * nx * ny * nz + 1; nothing spins, no workgroup waits for
// another, no floating-point atomics.  Launches follow one another on the context's stream; memory is allocated and
// released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_channels_dev.hpp"
#include "pw_field_cell_dev.hpp"
#include "pw_percolate.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_percolation(const pw_percolation_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                       const double* field, double* map, pw_percolation_level* levels, pw_percolation_out* out,
                                       int* n_evaluations, int* n_fills, int threads);   // pw_hostpath.cpp

static_assert(PW_PERC_NEVER == PERC_NEVER && PW_PERC_CRITERIA == PERC_CRITERIA, "the header's constants and the kernel's");
static_assert(sizeof(pw_percolation_job) == 160 && sizeof(pw_percolation_level) == 80 && sizeof(pw_percolation_out) == 32,
              "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int PERC_WAVES = CAV_THREADS / 64;
constexpr int PERC_UNROLL = 8;                                   // rows of a wave whose loads are in flight together
constexpr unsigned PERC_NONE = 0xFFFFFFFFu;                      // no set bit
constexpr long PERC_NO_RANK = 0x7fffffffffffffffl;
constexpr int PERC_SCRATCH_WORDS = 64;
constexpr size_t perc_lds_bytes(long rows) { return 8 * (4 * (size_t)rows + PERC_SCRATCH_WORDS); }

// a job as the kernels read it: firsts relative to the spans of the arrays that were uploaded
struct PercJobDev {
    long atom_first, n, coef_first;
    long map_first;            // the job's V doubles in the workspace of its launch
    long item_first, chunks;   // the job's chunks among the work items of the field kernel (none: a caller's field)
    long V;
    double o[3], s[6], core2, cutoff2;
    int nx, ny, nz, reserved;
};

// the scratch of the levels kernel behind the four grids
struct PercShared {
    u64 red[4 * PERC_WAVES];                 // reductions: a slot a wave, four values
    unsigned long long sum[5];               // n_voxels, n_cross[3] of a component; n_allowed of a level
    u64 lo[PERC_CRITERIA], hi[PERC_CRITERIA];
    long best[PERC_CRITERIA];                // the first voxel of the component a criterion's row holds
    u64 mid;
    int needed, go;
    unsigned first, comp_first;
};
static_assert(sizeof(PercShared) <= 8 * PERC_SCRATCH_WORDS, "the scratch behind the grids");

__global__ void __launch_bounds__(AFF_CHUNK)
pw_percolation_field_kernel(const PercJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                            const double* __restrict__ coef, u64* __restrict__ ws) {
    field_items_cell(jobs, n_jobs, total, xyz, coef, ws);            // (pw_field_cell_dev.hpp)
}

// (key, rank) pairs: the wave's first in order by a shuffle tree
__device__ inline void perc_wave_first(u64& key, long& rank) {
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 ok = __shfl_xor(key, s);
        const long orank = __shfl_xor(rank, s);
        if (pas_before(ok, orank, key, rank)) {
            key = ok;
            rank = orank;
        }
    }
}

// one scan of the map: the first (key, rank) in order, the largest finite key (0: none) and the voxels at +inf, the same
// in every thread; two barriers, the second after the last read of the scratch
__device__ inline void perc_scan(const u64* __restrict__ map, long V, PercShared* S, u64& min_key, long& min_rank, u64& max_key,
                                 long& n_blocked) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 wk = PAS_KEY_NONE, top = 0;
    long wr = PERC_NO_RANK, blocked = 0;
    for (long v = threadIdx.x; v < V; v += CAV_THREADS) {                // (the voxels)
        const u64 key = pas_key(pw_bits2d(map[v]));
        if (key == PAS_KEY_INF) {
            ++blocked;
            continue;
        }
        if (pas_before(key, v, wk, wr)) {
            wk = key;
            wr = v;
        }
        top = key > top ? key : top;
    }
    perc_wave_first(wk, wr);
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 a = __shfl_xor(top, s);
        top = a > top ? a : top;
        blocked += __shfl_xor(blocked, s);
    }
    if (lane == 0) {
        S->red[wave] = wk;
        S->red[PERC_WAVES + wave] = (u64)wr;
        S->red[2 * PERC_WAVES + wave] = top;
        S->red[3 * PERC_WAVES + wave] = (u64)blocked;
    }
    __syncthreads();
    min_key = PAS_KEY_NONE;
    min_rank = PERC_NO_RANK;
    max_key = 0;
    n_blocked = 0;
    for (int w = 0; w < PERC_WAVES; ++w) {
        if (pas_before(S->red[w], (long)S->red[PERC_WAVES + w], min_key, min_rank)) {
            min_key = S->red[w];
            min_rank = (long)S->red[PERC_WAVES + w];
        }
        max_key = S->red[2 * PERC_WAVES + w] > max_key ? S->red[2 * PERC_WAVES + w] : max_key;
        n_blocked += (long)S->red[3 * PERC_WAVES + w];
    }
    __syncthreads();
}

// a level pass: s_allowed[r] = the voxels of row r with key <= level (level < PAS_KEY_INF: no blocked voxel passes);
// below / above: the largest key <= level and the smallest finite key > level (0 / PAS_KEY_NONE without one), the same
// in every thread; two barriers, the second after the last read of the scratch
__device__ inline void perc_level(const u64* __restrict__ map, int nx, int rows, u64 level, u64* s_allowed, PercShared* S,
                                  u64& below, u64& above) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 lo_best = 0, hi_best = PAS_KEY_NONE;
    for (int r0 = wave; r0 < rows; r0 += PERC_WAVES * PERC_UNROLL) {    // (the rows of the wave, PERC_UNROLL loads in flight)
        u64 key[PERC_UNROLL];
#pragma unroll
        for (int u = 0; u < PERC_UNROLL; ++u) {
            const int r = r0 + PERC_WAVES * u;
            key[u] = r < rows && lane < nx ? pas_key(pw_bits2d(map[(long)r * nx + lane])) : PAS_KEY_NONE;
        }
#pragma unroll
        for (int u = 0; u < PERC_UNROLL; ++u) {
            const int r = r0 + PERC_WAVES * u;
            if (r >= rows) continue;                                 // (the same in every lane)
            const bool in = key[u] <= level;
            const u64 word = __ballot(in);
            if (lane == 0) s_allowed[r] = word;
            if (in) lo_best = key[u] > lo_best ? key[u] : lo_best;
            else if (key[u] < PAS_KEY_INF) hi_best = key[u] < hi_best ? key[u] : hi_best;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 a = __shfl_xor(lo_best, s), b = __shfl_xor(hi_best, s);
        lo_best = a > lo_best ? a : lo_best;
        hi_best = b < hi_best ? b : hi_best;
    }
    if (lane == 0) {
        S->red[wave] = lo_best;
        S->red[PERC_WAVES + wave] = hi_best;
    }
    __syncthreads();
    below = 0;
    above = PAS_KEY_NONE;
    for (int w = 0; w < PERC_WAVES; ++w) {
        below = S->red[w] > below ? S->red[w] : below;
        above = S->red[PERC_WAVES + w] < above ? S->red[PERC_WAVES + w] : above;
    }
    __syncthreads();
}

// over the voxels of the component p0 | p1: the (key, rank) that is first in order -- the well -- and the lowest rank with
// key == B (-1: none), the same in every thread; two barriers
__device__ inline void perc_measure(const u64* __restrict__ map, int nx, int rows, u64 B, const u64* s_p0, const u64* s_p1,
                                    PercShared* S, long& well_rank, long& saddle_rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 wk = PAS_KEY_NONE;
    long wr = PERC_NO_RANK, sr = PERC_NO_RANK;
    for (int r = wave; r < rows; r += PERC_WAVES) {                      // (the rows of the wave)
        const u64 f = s_p0[r] | s_p1[r];
        if (!((f >> lane) & 1ull)) continue;
        const long rank = (long)r * nx + lane;
        const u64 key = pas_key(pw_bits2d(map[rank]));
        if (pas_before(key, rank, wk, wr)) {
            wk = key;
            wr = rank;
        }
        if (key == B && rank < sr) sr = rank;
    }
    perc_wave_first(wk, wr);
    for (int s = 32; s >= 1; s >>= 1) {
        const long os = __shfl_xor(sr, s);
        sr = os < sr ? os : sr;
    }
    if (lane == 0) {
        S->red[wave] = wk;
        S->red[PERC_WAVES + wave] = (u64)wr;
        S->red[2 * PERC_WAVES + wave] = (u64)sr;
    }
    __syncthreads();
    wk = PAS_KEY_NONE;
    wr = sr = PERC_NO_RANK;
    for (int w = 0; w < PERC_WAVES; ++w) {
        const long os = (long)S->red[2 * PERC_WAVES + w];
        if (pas_before(S->red[w], (long)S->red[PERC_WAVES + w], wk, wr)) {
            wk = S->red[w];
            wr = (long)S->red[PERC_WAVES + w];
        }
        sr = os < sr ? os : sr;
    }
    __syncthreads();
    well_rank = wr == PERC_NO_RANK ? -1 : wr;
    saddle_rank = sr == PERC_NO_RANK ? -1 : sr;
}

// AN EVALUATION of the level `key` (the head of the file): the criteria met by the components found, bit c for criterion
// c.  `asked`: with rows == nullptr the criteria after all of which the evaluation stops (complete = false then); with
// rows the criteria whose rows are written at this level, and every candidate is gone through.  The same in every thread;
// the workgroup leaves through a barrier.
__device__ inline int perc_evaluate(const u64* __restrict__ map, int nx, int ny, int nz, u64 key, int asked,
                                    pw_percolation_level* rows_out, u64* s_allowed, u64* s_todo, u64* s_p0, u64* s_p1,
                                    PercShared* S, bool& complete, u64& below, u64& above, int& fills) {
    const int tid = threadIdx.x, rows = ny * nz;
    const bool final = rows_out != nullptr;
    if (tid == 0) S->sum[4] = 0;
    perc_level(map, nx, rows, key, s_allowed, S, below, above);
    {
        long mine = 0;
        for (int r = tid; r < rows; r += CAV_THREADS) {                  // (the rows of the thread)
            const u64 a = s_allowed[r];
            const int j = r % ny, l = r / ny;
            s_todo[r] = a ? perc_candidates(a, s_allowed[l * ny], s_allowed[j], nx, ny, nz, j, l) : 0;
            mine += cavity_popcount(a);
        }
        if (final && mine) atomicAdd(S->sum + 4, (unsigned long long)mine);
    }
    int met = 0;
    complete = true;
    const long n_voxels_grid = (long)nx * rows;
    int cursor = tid;                                                // (chan_first's, pw_channels_dev.hpp)
    for (long turn = 0; turn <= n_voxels_grid; ++turn) {             // (a turn takes a candidate or more out of todo, or ends)
        const unsigned first = chan_first(s_todo, rows, cursor, &S->first);
        if (first == CHAN_NONE) break;
        const ChannelsWalk W = chan_walk(s_allowed, s_p0, s_p1, S->sum, (int)(first >> 6), 1ull << (first & 63u), nx, ny, nz);
        const long n_voxels = W.n_voxels;
        const int wraps = W.wraps;
        fills += W.fills;
        const int crit = perc_criteria(wraps);
        met |= crit;

        // the component's candidates leave todo; p0 | p1 is still the component, and nobody stores to it before the
        // next barrier
        for (int r = tid; r < rows; r += CAV_THREADS) {
            const u64 f = s_p0[r] | s_p1[r];
            if (f) s_todo[r] &= ~f;
        }
        if (!final) {
            if ((met & asked) == asked) {                            // (the same in every thread)
                complete = false;
                break;
            }
            continue;
        }
        if (!(crit & asked)) continue;
        // the component's first voxel, and the rows it takes the lead of
        if (tid == 0) S->comp_first = PERC_NONE;
        __syncthreads();
        for (int r = tid; r < rows; r += CAV_THREADS) {
            const u64 f = s_p0[r] | s_p1[r];
            if (f) atomicMin(&S->comp_first, (unsigned)r * 64u + (unsigned)(__ffsll((long long)f) - 1));
        }
        __syncthreads();
        const long comp_first = (long)(S->comp_first >> 6) * nx + (long)(S->comp_first & 63u);
        int lead = 0;
#pragma unroll
        for (int c = 0; c < PERC_CRITERIA; ++c)
            if (((crit & asked) >> c) & 1) lead |= (comp_first < S->best[c]) << c;
        if (!lead) continue;                                         // (read after a barrier: the same in every thread)
        long well_rank, saddle_rank;
        perc_measure(map, nx, rows, key, s_p0, s_p1, S, well_rank, saddle_rank);
        if (tid == 0) {
            for (int c = 0; c < PERC_CRITERIA; ++c) {
                if (!((lead >> c) & 1)) continue;
                S->best[c] = comp_first;
                pw_percolation_level& R = rows_out[c];
                R.level = saddle_rank >= 0 ? pw_bits2d(map[saddle_rank]) : aff_inf();   // (there is one: pw_percolate.hpp)
                R.well = pw_bits2d(map[well_rank]);
                R.first = comp_first;
                R.n_voxels = n_voxels;
                grid_voxel(saddle_rank, nx, ny, R.saddle);
                grid_voxel(well_rank, nx, ny, R.well_voxel);
                R.wraps = wraps;
                R.rank = channels_rank(wraps);
                R.flags = 0;
                R.reserved = 0;
            }
        }
        __syncthreads();                                             // (best is read again in the next turn)
    }
    __syncthreads();
    if (final && tid == 0)
        for (int c = 0; c < PERC_CRITERIA; ++c)
            if ((asked >> c) & 1) rows_out[c].n_allowed = (long)S->sum[4];
    __syncthreads();
    return met;
}

// diag: n_evaluations and n_fills of the job (diagnostic: not part of the defined result)
__global__ void __launch_bounds__(CAV_THREADS)
pw_percolation_kernel(const PercJobDev* __restrict__ jobs, const u64* __restrict__ ws, pw_percolation_level* __restrict__ levels,
                      pw_percolation_out* __restrict__ out, int* __restrict__ diag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const PercJobDev& D = jobs[blockIdx.x];
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz, tid = threadIdx.x;
    u64* s_allowed = (u64*)lds;
    u64* s_todo = s_allowed + rows;
    u64* s_p0 = s_todo + rows;
    u64* s_p1 = s_p0 + rows;
    PercShared* S = (PercShared*)(s_p1 + rows);
    const u64* map = ws + D.map_first;
    pw_percolation_level* R = levels + (long)PERC_CRITERIA * blockIdx.x;

    u64 kmin, kmax;
    long min_rank, n_blocked;
    perc_scan(map, D.V, S, kmin, min_rank, kmax, n_blocked);
    const bool some = min_rank != PERC_NO_RANK;
    int evaluations = 0, fills = 0, met = 0;
    bool complete;
    u64 below, above;
    if (some) {                                                      // (the same in every thread)
        // the largest finite level: which criteria hold at all
        met = perc_evaluate(map, nx, ny, nz, kmax, 63, nullptr, s_allowed, s_todo, s_p0, s_p1, S, complete, below, above, fills);
        ++evaluations;
    }
    if (tid == 0) {
        pw_percolation_out& O = out[blockIdx.x];
        O.n_blocked = n_blocked;
        O.u_min = some ? pw_bits2d(map[min_rank]) : aff_inf();
        grid_voxel(some ? min_rank : -1, nx, ny, O.u_min_voxel);
        O.flags = (met & 1) ? 0 : PERC_NEVER;
        for (int c = 0; c < PERC_CRITERIA; ++c) {                    // (the rows of the criteria that never hold stay so)
            pw_percolation_level& N = R[c];
            N.level = N.well = aff_inf();
            N.first = -1;
            N.n_voxels = N.n_allowed = 0;
            for (int a = 0; a < 3; ++a) N.saddle[a] = N.well_voxel[a] = -1;
            N.wraps = N.rank = 0;
            N.flags = PERC_NEVER;
            N.reserved = 0;
            S->best[c] = PERC_NO_RANK;
        }
        perc_search_begin(S->lo, S->hi, kmin, kmax, met);
    }
    if (some) {
        for (int step = 0; step < PERC_MAX_STEPS; ++step) {              // (the search: pw_percolate.hpp)
            __syncthreads();
            if (tid == 0) {
                u64 mid = 0;
                int needed = 0;
                S->go = perc_search_next(S->lo, S->hi, mid, needed);
                S->mid = mid;
                S->needed = needed;
            }
            __syncthreads();
            if (!S->go) break;
            const u64 mid = S->mid;
            const int needed = S->needed;
            met = perc_evaluate(map, nx, ny, nz, mid, needed, nullptr, s_allowed, s_todo, s_p0, s_p1, S, complete, below, above, fills);
            ++evaluations;
            if (tid == 0) perc_search_learn(S->lo, S->hi, met, complete, below, above);
        }
        __syncthreads();
        // the rows: one evaluation that goes through every candidate at each distinct B_c
        for (int c = 0; c < PERC_CRITERIA; ++c) {
            const u64 B = S->hi[c];
            int asked = 0;
            bool seen = false;
            for (int d = 0; d < PERC_CRITERIA; ++d) {
                if (S->hi[d] != B) continue;
                asked |= 1 << d;
                seen = seen || d < c;
            }
            if (B == PAS_KEY_INF || seen) continue;                  // (read after a barrier: the same in every thread)
            perc_evaluate(map, nx, ny, nz, B, asked, R, s_allowed, s_todo, s_p0, s_p1, S, complete, below, above, fills);
            ++evaluations;
        }
    }
    if (tid == 0) {
        diag[2 * blockIdx.x] = evaluations;
        diag[2 * blockIdx.x + 1] = fills;
    }
}

const char* const ENTRY = "pw_percolation";
int perc_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

inline long perc_voxels(const pw_percolation_job& J) { return (long)J.nx * J.ny * J.nz; }

// Everything is checked before anything is launched or written
int perc_check(const pw_percolation_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
               const double* field, long n_field, const double* map, long n_map, const pw_percolation_level* levels,
               long n_levels, long n_out) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_percolation_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        const long V = perc_voxels(J);
        const bool lj = J.field_first == -1;
        if (J.n < 0) return perc_bad(k, "a negative count");
        if (lj && span_outside(J.atom_first, J.n, n_points)) return perc_bad(k, "atoms outside xyz");
        if (lj && span_outside(J.coef_first, J.n, n_coef)) return perc_bad(k, "coefficients outside coef");
        if (J.field_first < -1 || (!lj && span_outside(J.field_first, V, n_field))) return perc_bad(k, "the field is outside its array");
        if (J.map_first < -1 || (J.map_first >= 0 && span_outside(J.map_first, V, n_map))) return perc_bad(k, "the map is outside its array");
        if (span_outside(J.level_first, PERC_CRITERIA, n_levels)) return perc_bad(k, "the rows are outside levels");
        if (span_outside(J.out, 1, n_out)) return perc_bad(k, "the row is outside out");
        if ((lj && J.n && (!xyz || !coef)) || (!lj && !field) || (J.map_first >= 0 && !map) || !levels) return perc_bad(k, "null array");
        bool finite = true;
        for (int a = 0; a < 3; ++a) finite = finite && pw_finite(J.origin[a]);
        for (int a = 0; a < 6; ++a) finite = finite && pw_finite(J.step[a]);
        if (!finite) return perc_bad(k, "the origin or a step is not finite");
        if (!(J.step[0] > 0.0 && J.step[2] > 0.0 && J.step[5] > 0.0)) return perc_bad(k, "ax, by or cz <= 0");
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
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of levels with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].level_first, (long)PERC_CRITERIA}; }));
    return shared_output(ENTRY, n_jobs, "shares entries of map with an earlier job", [&](long k) {
        return OutSpan{(long)jobs[k].map_first, jobs[k].map_first >= 0 ? perc_voxels(jobs[k]) : 0};
    });
}

// workspace_bytes: the budget of the maps of the jobs of one launch (0: PERC_WORKSPACE_BYTES; at 1 every job is a launch
// of its own); kernel_ms: when not null, the time of the device work of the call from the first launch to the last, the
// copies between them included, by HIP events on the context's stream; n_evaluations, n_fills: when not null, n_jobs
// integers, job k's evaluations of a level and parity fills (diagnostic: they differ between the paths)
int percolation(pw_context* ctx, const pw_percolation_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                const double* coef, int64_t n_coef, const double* field, int64_t n_field, double* map, int64_t n_map,
                pw_percolation_level* levels, int64_t n_levels, pw_percolation_out* out, int64_t n_out, int64_t workspace_bytes,
                float* kernel_ms, int32_t* n_evaluations, int32_t* n_fills) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 || n_field < 0 ||
        n_map < 0 || n_levels < 0 || n_out < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = perc_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, field, (long)n_field, map, (long)n_map, levels,
                              (long)n_levels, (long)n_out);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_percolation(jobs, N, xyz, coef, field, map, levels, out, n_evaluations, n_fills,
                                       pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their maps
    // fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : PERC_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab;
    for (long k = 0; k < N; ++k) {
        if (jobs[k].field_first != -1) continue;
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        rows_ab.widen((long)jobs[k].coef_first, (long)jobs[k].n);
    }
    std::vector<PercJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    for (long k = 0; k < N; ++k) {
        const pw_percolation_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, V = rows * J.nx;
        const bool lj = J.field_first == -1;
        place(groups, cur, budget_words, V);
        PercJobDev& D = devs[k];
        D.n = lj ? (long)J.n : 0;
        D.atom_first = atoms.rel((long)J.atom_first, D.n);
        D.coef_first = rows_ab.rel((long)J.coef_first, D.n);
        D.map_first = cur.words;
        D.item_first = cur.items;
        D.chunks = lj ? (V + AFF_CHUNK - 1) / AFF_CHUNK : 0;
        D.V = V;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        for (int a = 0; a < 6; ++a) D.s[a] = J.step[a];
        D.core2 = J.core2; D.cutoff2 = J.cutoff2; D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.reserved = 0;
        cur.words += V; cur.cost += V; cur.items += D.chunks; cur.blocks += 1; cur.last += 1;
        cur.rows = rows > cur.rows ? rows : cur.rows;
    }
    groups.push_back(cur);

    const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), level_bytes = sizeof(pw_percolation_level) * PERC_CRITERIA * (size_t)N,
                 out_bytes = sizeof(pw_percolation_out) * (size_t)N, diag_bytes = sizeof(int) * 2 * (size_t)N;
    std::vector<pw_percolation_level> res_levels((size_t)N * PERC_CRITERIA);
    std::vector<pw_percolation_out> res_out((size_t)N);
    std::vector<int> res_diag(2 * (size_t)N);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    STAT_TRY(hipFuncSetAttribute((const void*)pw_percolation_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)perc_lds_bytes(CAVITY_MAX_G * CAVITY_MAX_G)));
    {
        StreamBuffers buf(st);
        PercJobDev* d_jobs;
        double *d_xyz, *d_coef;
        u64* d_ws;
        pw_percolation_level* d_levels;
        pw_percolation_out* d_out;
        int* d_diag;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(PercJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(PercJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, 2));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_levels, level_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        STAT_TRY(buf.alloc(&d_diag, diag_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_levels, level_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(poison_scratch(poison, d_diag, diag_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one takes the workspace over when this one is done
        // and its maps are on their way)
        for (const LaunchGroup& G : groups) {
            const unsigned n_group = (unsigned)(G.last - G.first);
            for (long k = G.first; k < G.last; ++k)
                if (jobs[k].field_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].map_first, field + jobs[k].field_first, sizeof(double) * (size_t)devs[k].V,
                                            hipMemcpyHostToDevice, st));
            if (G.items) {
                const long blocks = launch_blocks(G.items, 65536);
                hipLaunchKernelGGL(pw_percolation_field_kernel, dim3((unsigned)blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                                   (int)n_group, G.items, d_xyz, d_coef, d_ws);
                STAT_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(pw_percolation_kernel, dim3(n_group), dim3(CAV_THREADS), perc_lds_bytes(G.rows), st, d_jobs + G.first,
                               d_ws, d_levels + PERC_CRITERIA * G.first, d_out + G.first, d_diag + 2 * G.first);
            STAT_TRY(hipGetLastError());
            for (long k = G.first; k < G.last; ++k)
                if (jobs[k].map_first >= 0)
                    STAT_TRY(hipMemcpyAsync(map + jobs[k].map_first, d_ws + devs[k].map_first, sizeof(double) * (size_t)devs[k].V,
                                            hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res_levels.data(), d_levels, level_bytes, hipMemcpyDeviceToHost, st));
        STAT_TRY(hipMemcpyAsync(res_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st));
        STAT_TRY(hipMemcpyAsync(res_diag.data(), d_diag, diag_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's rows, job by job
    for (long k = 0; k < N; ++k) {
        out[jobs[k].out] = res_out[(size_t)k];
        for (int c = 0; c < PERC_CRITERIA; ++c) levels[jobs[k].level_first + c] = res_levels[(size_t)k * PERC_CRITERIA + c];
        if (n_evaluations) n_evaluations[k] = res_diag[2 * (size_t)k];
        if (n_fills) n_fills[k] = res_diag[2 * (size_t)k + 1];
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_percolation(pw_context* ctx, const pw_percolation_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                              const double* coef, int64_t n_coef, const double* field, int64_t n_field, double* map, int64_t n_map,
                              pw_percolation_level* levels, int64_t n_levels, pw_percolation_out* out, int64_t n_out) {
    return percolation(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, field, n_field, map, n_map, levels, n_levels, out, n_out, 0,
                       nullptr, nullptr, nullptr);
}

// measurement and test hook (not part of the header): pw_percolation with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it), the device work timed by HIP events when kernel_ms is not null, and
// per job the evaluations of a level and the parity fills it took in n_evaluations[0 .. n_jobs) and n_fills[0 .. n_jobs)
// when those are not null -- diagnostic, not part of the defined bytes
extern "C" int pw_internal_percolation(pw_context* ctx, const pw_percolation_job* jobs, int64_t n_jobs, const double* xyz,
                                       int64_t n_points, const double* coef, int64_t n_coef, const double* field, int64_t n_field,
                                       double* map, int64_t n_map, pw_percolation_level* levels, int64_t n_levels,
                                       pw_percolation_out* out, int64_t n_out, int64_t workspace_bytes, float* kernel_ms,
                                       int32_t* n_evaluations, int32_t* n_fills) {
    return percolation(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, field, n_field, map, n_map, levels, n_levels, out, n_out,
                       workspace_bytes, kernel_ms, n_evaluations, n_fills);
}
