// pw_trans.hip -- gfx950 kernels and the C ABI entry of the lagged state-transition counts of a series
// (include/pywindow_amd.h: pw_trans_counts; definition of the result in pw_trans.hpp).  Two kernels per launch.
//
// pw_trans_pack_kernel classifies every entry once: a wave takes 64 entries, every lane finds the state of its own
// (trans_state) and one ballot a state gives two 32-bit words of that state's mask.  The masks of a job lie in the
// workspace as [word][P], P the padded state count (2, 4, 8, 16), so that the P words of one time step are one vector
// load; gaps and entries past n are in no mask and at least one word of zeros follows the last word that holds entries.
//
// pw_trans_count_kernel, the hot path: a workgroup takes one (chunk of TRANS_CHUNK origins, tile of TRANS_TILE lags,
// block of BI origin states) and every lane owns one lag k.  Per word w of 32 origins a lane loads the P partner words
// at w + k / 32 + 1 (the words at w + k / 32 it has from the step before), funnel-shifts each pair by k % 32
// (v_alignbit_b32) and adds popcount(origin_i & partner_j) to its BI x P accumulators (v_and_b32, v_bcnt_u32_b32), all
// registers with compile-time indices: no atomics and no branch in the loop.  The origin words are the same for every
// lane (an LDS broadcast); the partner words of a tile lie in a window of chunk + tile * lag_step entries that is staged
// in LDS while it fits TRANS_WINDOW and read through L2 otherwise.  At the end of the work item a lane adds its
// non-zero accumulators to its row with 64-bit integer atomics -- sums of integers do not depend on the order --: at
// most BI * P of them against 256 steps of 2 * BI * P + 2 * P instructions, under one in five hundred.
// Everything is queued on the context's stream, memory included.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_trans.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_trans(const pw_trans_job* jobs, long n_jobs, const double* series, const double* edges,
                                 long n_states, long* counts, int threads);   // pw_hostpath.cpp

static_assert(PW_TRANS_MAX_STATES == TRANS_MAX_STATES, "the header's bound and the kernels'");

namespace {

typedef unsigned long long u64;

constexpr int CW = TRANS_CHUNK / 32;     // origin words of a work item
constexpr int WINW = TRANS_WINDOW / 32;  // words a state of the partner window in LDS
static_assert(WINW >= CW + 2, "a window holds the chunk, the word after it and one more lag word at the least");

// one job with rows: its masks are [words][P] 32-bit words in the workspace of its launch
struct TransSlabDev {
    long a_first, n;           // into the uploaded span of series
    long e_first;              // the job's first edge in the uploaded span of edges
    long lag_first, lag_step, n_lags;
    long row_first;            // the job's n_lags rows in the compact result of the call
    long m_first;              // first word of the job's masks
    long nw;                   // words that hold entries, (n + 31) / 32; the words nw .. 2 * waves - 1 are zeros
    long wave_first;           // first of the job's nw / 2 + 1 pack waves in its launch
    long item_first;           // first of the job's (chunk, tile, block of origin states) items in its launch
    long tiles;
    int n_edges;
};

template <int P>
__global__ void __launch_bounds__(256)
pw_trans_pack_kernel(const TransSlabDev* __restrict__ slabs, int n_slabs, long total, const double* __restrict__ series,
                     const double* __restrict__ edges, unsigned* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long it = (long)blockIdx.x * 4 + wave; it < total; it += (long)gridDim.x * 4) {
        const int q = stat_find(n_slabs, it, [&](int i) { return slabs[i].wave_first; });
        const long lw = it - slabs[q].wave_first, t = lw * 64 + lane;
        int s = TRANS_GAP;
        if (t < slabs[q].n) s = trans_state(series[slabs[q].a_first + t], edges + slabs[q].e_first, slabs[q].n_edges);
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const u64 b = __ballot(s == j);
            mine = lane == j ? b : mine;
        }
        if (lane < P) {
            unsigned* m = ws + slabs[q].m_first + 2 * lw * P + lane;
            m[0] = (unsigned)mine;
            m[P] = (unsigned)(mine >> 32);
        }
    }
}

// P consecutive words from a 16-byte aligned (P == 2: 8-byte aligned) address, LDS or global
template <int P, class Ptr>
__device__ inline void trans_load(Ptr p, unsigned (&v)[P]) {
    if constexpr (P == 2) {
        const uint2 x = *(const uint2*)p;
        v[0] = x.x; v[1] = x.y;
    } else {
#pragma unroll
        for (int g = 0; g < P / 4; ++g) {
            const uint4 x = ((const uint4*)p)[g];
            v[4 * g] = x.x; v[4 * g + 1] = x.y; v[4 * g + 2] = x.z; v[4 * g + 3] = x.w;
        }
    }
}

// a copy in a register of its own: the 64-bit operand of the atomic is a register pair, and without the copy every
// accumulator is kept in a pair with a zero beside it for the length of the kernel
__device__ inline unsigned trans_copy(unsigned v) {
    unsigned c;
    asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "v"(v));
    return c;
}

// S: the call's n_states; a lane's row is [S][S].  BI origin states a work item, so that a lane holds BI * P sums.
template <int P, int BI>
__global__ void __launch_bounds__(TRANS_TILE)
pw_trans_count_kernel(const TransSlabDev* __restrict__ slabs, int n_slabs, long total, const unsigned* __restrict__ ws,
                      long* counts, int S) {
    __shared__ __attribute__((aligned(16))) unsigned s_org[CW * BI];
    __shared__ __attribute__((aligned(16))) unsigned s_win[WINW * P];
    const int tid = threadIdx.x;
    const int nob = (S + BI - 1) / BI;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int q = stat_find(n_slabs, item, [&](int i) { return slabs[i].item_first; });
        const TransSlabDev D = slabs[q];
        const long local = item - D.item_first;
        const int i0 = (int)(local % nob) * BI;                      // (origin blocks fastest, then tiles: neighbours
        const long rest = local / nob;                               //  share the chunk)
        const long tile = rest % D.tiles, ch = rest / D.tiles;
        const long w0 = ch * CW;
        const int wn = (int)(D.nw - w0 < CW ? D.nw - w0 : CW);
        const long q0 = tile * TRANS_TILE;
        const int lanes = (int)(D.n_lags - q0 < TRANS_TILE ? D.n_lags - q0 : TRANS_TILE);
        const long k_lo = D.lag_first + q0 * D.lag_step;
        if (k_lo >= D.n) continue;                                   // (the whole tile: rows of zeros, already there)
        long k_hi = D.lag_first + (q0 + lanes - 1) * D.lag_step;     // (a lag of n or more counts nothing: n stands
        k_hi = k_hi < D.n ? k_hi : D.n;                              //  for all of them)
        const long base = w0 + (k_lo >> 5);                          // the window's first word
        const long len = wn + (k_hi >> 5) - (k_lo >> 5) + 1;         // its words: every lane reads off + 0 .. off + wn
        const bool in_lds = len <= WINW;
        const bool active = tid < lanes;
        long k = D.lag_first + (q0 + tid) * D.lag_step;
        k = active && k < k_hi ? k : k_hi;                           // (idle lanes repeat the last lag and write nothing)
        const int off = (int)((k >> 5) - (k_lo >> 5));
        const unsigned r = (unsigned)(k & 31);
        const unsigned* M = ws + D.m_first;
        __syncthreads();                                             // (the previous item's words are done with)
#pragma clang loop vectorize(disable) unroll(disable)
        for (int x = tid; x < wn * BI; x += TRANS_TILE) s_org[x] = M[(w0 + x / BI) * P + i0 + x % BI];
        if (in_lds)
#pragma clang loop vectorize(disable) unroll(disable)
            for (int x = tid; x < (int)len * P; x += TRANS_TILE) {
                const long g = base + x / P;                         // (words past nw: word nw, zeros)
                s_win[x] = M[(g < D.nw ? g : D.nw) * P + x % P];
            }
        __syncthreads();
        unsigned acc[BI][P];
#pragma unroll
        for (int i = 0; i < BI; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) acc[i][j] = 0;
        // (four words a round, the two sets of partner words changing places: no copies; written out by hand)
        auto walk = [&](auto&& fetch) {
            unsigned pv[P], nx[P];
            auto step = [&](int w, const unsigned (&lo)[P], const unsigned (&hi)[P]) {
                unsigned o[BI];
                trans_load<BI>(s_org + w * BI, o);
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const unsigned partner = trans_funnel(hi[j], lo[j], r);
#pragma unroll
                    for (int i = 0; i < BI; ++i) trans_count(acc[i][j], o[i] & partner);
                }
            };
            fetch(0, pv);
            int w = 0;
#pragma clang loop vectorize(disable) unroll(disable)
            for (; w + 4 <= wn; w += 4) {
                fetch(w + 1, nx); step(w, pv, nx);
                fetch(w + 2, pv); step(w + 1, nx, pv);
                fetch(w + 3, nx); step(w + 2, pv, nx);
                fetch(w + 4, pv); step(w + 3, nx, pv);
            }
#pragma clang loop vectorize(disable) unroll(disable)
            for (; w < wn; ++w) {
                fetch(w + 1, nx); step(w, pv, nx);
#pragma unroll
                for (int j = 0; j < P; ++j) pv[j] = nx[j];
            }
        };
        if (in_lds) {
            const unsigned* win = s_win + off * P;
            walk([&](int x, unsigned (&v)[P]) { trans_load<P>(win + x * P, v); });
        } else {
            const long first = base + off;
            walk([&](int x, unsigned (&v)[P]) {
                const long g = first + x;
                trans_load<P>(M + (g < D.nw ? g : D.nw) * P, v);
            });
        }
        if (active) {
            u64* row = (u64*)counts + (D.row_first + q0 + tid) * S * S;
#pragma unroll
            for (int i = 0; i < BI; ++i)
#pragma unroll
                for (int j = 0; j < P; ++j)
                    if (acc[i][j] && i0 + i < S && j < S) atomicAdd(row + (i0 + i) * S + j, (u64)trans_copy(acc[i][j]));
        }
    }
}

// slabs [first, last) share one launch (two kernels) and one workspace of `words` mask words
struct TransLaunch {
    long first, last, waves, items, words;
};

// rows [dev, dev + rows) of the compact result are rows [host, host + rows) of the caller's array
struct TransCopy {
    long host, dev, rows;
};

// The plan of a call.  The masks of a job are P * 2 * (nw / 2 + 1) words, about P * n / 8 bytes; jobs are gathered
// into launches while their masks fit the budget, and a job whose masks alone exceed it goes alone.  Nothing of the
// result depends on the cut: a job's rows are its own.
void trans_plan(const pw_trans_job* jobs, long n_jobs, long s_lo, long e_lo, long budget, int P, int nob,
                std::vector<TransSlabDev>& slabs, std::vector<TransLaunch>& launches, std::vector<TransCopy>& copies) {
    long rows = 0;
    TransLaunch cur{0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_trans_job& J = jobs[k];
        const long n = (long)J.n, nl = (long)J.n_lags;
        if (n == 0 || nl == 0) continue;
        if (!copies.empty() && copies.back().host + copies.back().rows == (long)J.out_first)
            copies.back().rows += nl;
        else
            copies.push_back(TransCopy{(long)J.out_first, rows, nl});
        TransSlabDev D{};
        D.n = n; D.a_first = (long)J.a_first - s_lo;
        D.e_first = J.n_edges ? (long)J.e_first - e_lo : 0;
        D.n_edges = (int)J.n_edges;
        D.lag_first = (long)J.lag_first; D.lag_step = (long)J.lag_step; D.n_lags = nl;
        D.nw = (n + 31) / 32;
        D.tiles = (nl + TRANS_TILE - 1) / TRANS_TILE;
        const long waves = D.nw / 2 + 1, words = (long)P * 2 * waves;
        if (cur.last > cur.first && cur.words + words > budget) {
            launches.push_back(cur);
            cur = TransLaunch{cur.last, cur.last, 0, 0, 0};
        }
        D.m_first = cur.words; D.wave_first = cur.waves; D.item_first = cur.items;
        D.row_first = rows;
        cur.words += words;
        cur.waves += waves;
        cur.items += (D.nw + CW - 1) / CW * D.tiles * nob;
        rows += nl;
        cur.last += 1;
        slabs.push_back(D);
    }
    if (cur.last > cur.first) launches.push_back(cur);
}

template <int P, int BI>
hipError_t trans_launch(const TransLaunch& L, const TransSlabDev* d_slabs, const double* d_x, const double* d_e, unsigned* d_ws,
                        long* d_counts, int S, hipStream_t st) {
    const int count = (int)(L.last - L.first);
    hipLaunchKernelGGL((pw_trans_pack_kernel<P>), dim3((unsigned)launch_blocks((L.waves + 3) / 4, 1l << 20)), dim3(256), 0, st, d_slabs + L.first, count,
                       L.waves, d_x, d_e, d_ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pw_trans_count_kernel<P, BI>), dim3((unsigned)launch_blocks(L.items, 1l << 20)), dim3(TRANS_TILE), 0, st, d_slabs + L.first,
                       count, L.items, d_ws, d_counts, S);
    return hipGetLastError();
}

constexpr int trans_block(int P) { return P == 16 ? 4 : P; }     // BI of the instantiation for P

// workspace_bytes: the budget of masks (0: TRANS_WORKSPACE_BYTES); kernel_ms: when not null, the time of all kernels
// of the call (the zeroing of the result included) by HIP events on the context's stream
int trans_counts(pw_context* ctx, const pw_trans_job* jobs, int64_t n_jobs, const double* series, const double* edges,
                 int64_t n_states, int64_t* counts, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0, e_lo = -1, e_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_trans_job& J = jobs[k];
        if (J.n < 0 || J.n_edges < 0 || J.n_lags < 0 || J.a_first < 0 || J.e_first < 0 || J.lag_first < 0 || J.out_first < 0)
            return stat_bad("pw_trans_counts", k, "negative range");
        if (J.lag_step < 1) return stat_bad("pw_trans_counts", k, "lag_step < 1");
        if (n_states < 1 || n_states > TRANS_MAX_STATES) return stat_bad("pw_trans_counts", k, "n_states outside 1 .. 16");
        if (J.n_edges >= n_states) return stat_bad("pw_trans_counts", k, "n_edges >= n_states");
        if (J.n > TRANS_MAX) return stat_bad("pw_trans_counts", k, "too long (n > 2^31)");
        if (J.n == 0 || J.n_lags == 0) continue;
        long reach;
        if (__builtin_mul_overflow((long)J.n_lags - 1, (long)J.lag_step, &reach) ||
            __builtin_add_overflow(reach, (long)J.lag_first, &reach) || reach >= TRANS_MAX_LAG)
            return stat_bad("pw_trans_counts", k, "the largest lag exceeds 2^62");
        if (!series || !counts || (J.n_edges && !edges)) return stat_bad("pw_trans_counts", k, "null array");
        for (long i = 0; i < (long)J.n; ++i) {
            const double v = series[J.a_first + i];
            if (!pw_finite(v) && !pw_isnan_bits(v)) return stat_bad("pw_trans_counts", k, "the series holds an infinity");
        }
        for (long i = 0; i < (long)J.n_edges; ++i) {
            if (!pw_finite(edges[J.e_first + i])) return stat_bad("pw_trans_counts", k, "an edge is a NaN or an infinity");
            if (i && !(edges[J.e_first + i - 1] < edges[J.e_first + i]))
                return stat_bad("pw_trans_counts", k, "the edges do not increase strictly");
        }
        const long lo = (long)J.a_first, hi = lo + (long)J.n;
        if (s_lo < 0 || lo < s_lo) s_lo = lo;
        if (hi > s_hi) s_hi = hi;
        if (J.n_edges) {
            const long el = (long)J.e_first, eh = el + (long)J.n_edges;
            if (e_lo < 0 || el < e_lo) e_lo = el;
            if (eh > e_hi) e_hi = eh;
        }
    }
    if (s_lo < 0) return PW_OK;                                  // no job has a row
    if (e_lo < 0) e_lo = e_hi = 0;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_trans(jobs, (long)n_jobs, series, edges, (long)n_states, (long*)counts,
                                 pw_context_host_threads(ctx, 0));

    const int S = (int)n_states, P = trans_padded(S), BI = trans_block(P), nob = (S + BI - 1) / BI;
    std::vector<TransSlabDev> slabs;
    std::vector<TransLaunch> launches;
    std::vector<TransCopy> copies;
    trans_plan(jobs, (long)n_jobs, s_lo, e_lo, (long)(workspace_bytes ? workspace_bytes : TRANS_WORKSPACE_BYTES) / 4, P, nob,
               slabs, launches, copies);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_trans_counts", (long)n_jobs - 1, "too large");
    long words = 0;
    for (const TransLaunch& L : launches) words = L.words > words ? L.words : words;
    const long rows = slabs.back().row_first + slabs.back().n_lags;
    const size_t row_bytes = sizeof(long) * (size_t)S * (size_t)S;
    const size_t count_bytes = row_bytes * (size_t)rows;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        TransSlabDev* d_slabs;
        double *d_x, *d_e;
        unsigned* d_ws;
        long* d_counts;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(TransSlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_e, sizeof(double) * (size_t)(e_hi - e_lo)));
        STAT_TRY(buf.alloc(&d_ws, sizeof(unsigned) * (size_t)words));
        STAT_TRY(buf.alloc(&d_counts, count_bytes));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp; the result is zeroed below)
        STAT_TRY(poison_scratch(poison, d_ws, sizeof(unsigned) * (size_t)words, st));
        STAT_TRY(poison_scratch(poison, d_counts, count_bytes, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(TransSlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_x, series + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        if (e_hi > e_lo)
            STAT_TRY(hipMemcpyAsync(d_e, edges + e_lo, sizeof(double) * (size_t)(e_hi - e_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        STAT_TRY(hipMemsetAsync(d_counts, 0, count_bytes, st));
        // (launches follow one another on the stream, so the next one may take the workspace over; both kernels
        // stride over their work -- tests/test_gpu_launch_cap.py sends them round again -- and a launch has a job with
        // a term and a lag, so neither count is zero)
        for (const TransLaunch& L : launches) {
            hipError_t e = P == 2   ? trans_launch<2, trans_block(2)>(L, d_slabs, d_x, d_e, d_ws, d_counts, S, st)
                           : P == 4 ? trans_launch<4, trans_block(4)>(L, d_slabs, d_x, d_e, d_ws, d_counts, S, st)
                           : P == 8 ? trans_launch<8, trans_block(8)>(L, d_slabs, d_x, d_e, d_ws, d_counts, S, st)
                                    : trans_launch<16, trans_block(16)>(L, d_slabs, d_x, d_e, d_ws, d_counts, S, st);
            STAT_TRY(e);
        }
        STAT_TRY(ev.stop(st));
        // (the compact result is in job order: neighbours in the caller's array come back in one copy)
        for (const TransCopy& c : copies)
            STAT_TRY(hipMemcpyAsync((char*)counts + (size_t)c.host * row_bytes, (char*)d_counts + (size_t)c.dev * row_bytes,
                                     (size_t)c.rows * row_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_trans_counts(pw_context* ctx, const pw_trans_job* jobs, int64_t n_jobs, const double* series,
                               const double* edges, int64_t n_states, int64_t* counts) {
    return trans_counts(ctx, jobs, n_jobs, series, edges, n_states, counts, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_trans_counts with the budget of masks given (0: the default;
// the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_trans_counts(pw_context* ctx, const pw_trans_job* jobs, int64_t n_jobs, const double* series,
                                        const double* edges, int64_t n_states, int64_t* counts, int64_t workspace_bytes,
                                        float* kernel_ms) {
    return trans_counts(ctx, jobs, n_jobs, series, edges, n_states, counts, workspace_bytes, kernel_ms);
}
