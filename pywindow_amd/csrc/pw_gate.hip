// pw_gate.hip -- gfx950 kernels and the C ABI entry of the gating statistics of a series against many thresholds
// (include/pywindow_amd.h: pw_gate_counts; definition of the result in pw_gate.hpp).  Two kernels per launch.
//
// pw_gate_chunk_kernel, the hot path: a workgroup stages one chunk of GATE_CHUNK entries of a series in LDS and
// every lane owns one of GATE_TILE thresholds.  A lane walks the chunk -- all lanes read the same LDS word, a
// broadcast -- with its run and its twelve counts in registers (32-bit: nothing within a chunk exceeds its
// length), tallies the runs strictly inside the chunk, stores the chunk's summary (one 32-bit word) in the
// workspace and adds what it counted to the threshold's row with integer atomics: sums and maxima of integers do
// not depend on the order.  pw_gate_merge_kernel: one lane per (job, threshold) takes that threshold's summaries
// in chunk order (lanes consecutive: coalesced) and tallies the runs that touch or cross chunk boundaries.  No
// floating-point arithmetic beyond the comparison with the threshold.  Everything is queued on the context's
// stream, memory included.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_gate.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_gate(const pw_gate_job* jobs, long n_jobs, const double* series, const double* thresholds,
                                long n_bins, long* counts, long* hist, int threads);   // pw_hostpath.cpp

static_assert(PW_GATE_FIELDS == GATE_FIELDS, "the header's row and the tally");

namespace {

typedef unsigned long long u64;

// a slab: thresholds [first, first + m) of one job; the workspace is an array of 32-bit summaries
struct GateSlabDev {
    long a_first, n;           // into the uploaded span of series
    long d_first;              // the slab's first threshold in the uploaded span of thresholds
    long m;
    long row_first;            // the slab's m rows in the compact result of the call
    long ws_first;             // the slab's [chunks][m] summaries in the workspace of its launch
    long item_first;           // first (chunk, tile of thresholds) pair of the slab in its launch
    long lane_first;           // first of the slab's m thresholds among those of its launch
    int tiles, chunks;
};

// one more complete run of `len` entries in row `row`, s = 0 open, 1 closed; the last bin takes every length >= B
struct GateHistAtomic {
    u64* hist;                 // the row's [2][B], or anything when B == 0
    long B;
    __device__ void operator()(int s, long len) const {
        if (B > 0) atomicAdd(hist + s * B + (len < B ? len : B) - 1, 1ull);
    }
};
struct GateHistPlain {
    long* hist;
    long B;
    __device__ void operator()(int s, long len) const {
        if (B > 0) hist[s * B + (len < B ? len : B) - 1] += 1;
    }
};

__device__ inline void gate_atomic_add(u64* p, unsigned v) { if (v) atomicAdd(p, (u64)v); }
__device__ inline void gate_atomic_max(u64* p, unsigned v) { if (v) atomicMax(p, (u64)v); }

__global__ void __launch_bounds__(GATE_TILE)
pw_gate_chunk_kernel(const GateSlabDev* __restrict__ slabs, int n_slabs, long total, const double* __restrict__ series,
                     const double* __restrict__ thresholds, unsigned* __restrict__ ws, long* counts, long* hist, long n_bins) {
    __shared__ double s_a[GATE_CHUNK];
    const int tid = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int q = stat_find(n_slabs, item, [&](int i) { return slabs[i].item_first; });
        const GateSlabDev S = slabs[q];
        const long local = item - S.item_first;
        const long ch = local / S.tiles;                             // (tiles fastest: neighbours share the chunk)
        const long f = (local - ch * S.tiles) * GATE_TILE + tid;     // the lane's threshold within the slab
        const long t0 = ch * GATE_CHUNK;
        const int len = (int)(S.n - t0 < GATE_CHUNK ? S.n - t0 : GATE_CHUNK);
        __syncthreads();                                             // (the previous item's chunk is done with)
        for (int i = tid; i < len; i += GATE_TILE) s_a[i] = series[S.a_first + t0 + i];
        __syncthreads();
        if (f < S.m) {
            const long row = S.row_first + f;
            GateTally<unsigned> T;
            const unsigned summary = gate_chunk(s_a, len, thresholds[S.d_first + f], T,
                                                GateHistAtomic{(u64*)hist + row * 2 * n_bins, n_bins});
            ws[S.ws_first + ch * S.m + f] = summary;
            u64* c = (u64*)counts + row * GATE_FIELDS;
            gate_atomic_add(c + 0, T.n_open);
            gate_atomic_add(c + 1, T.n_closed);
            gate_atomic_add(c + 2, T.open_runs);
            gate_atomic_add(c + 3, T.closed_runs);
            gate_atomic_max(c + 4, T.longest_open);
            gate_atomic_max(c + 5, T.longest_closed);
            gate_atomic_add(c + 6, T.openings);
            gate_atomic_add(c + 7, T.closings);
            gate_atomic_add(c + 8, T.complete_open_runs);
            gate_atomic_add(c + 9, T.complete_closed_runs);
            gate_atomic_add(c + 10, T.complete_open_frames);
            gate_atomic_add(c + 11, T.complete_closed_frames);
        }
    }
}

// the runs that touch a chunk's edge, for every threshold of the slabs of one launch.  Runs after the chunk kernel
// of the same launch on the same stream, and a row belongs to one lane: plain additions.
__global__ void __launch_bounds__(256)
pw_gate_merge_kernel(const GateSlabDev* __restrict__ slabs, int n_slabs, long total, const unsigned* __restrict__ ws,
                     long* counts, long* hist, long n_bins) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int q = stat_find(n_slabs, t, [&](int i) { return slabs[i].lane_first; });
        const long f = t - slabs[q].lane_first, m = slabs[q].m;
        const int chunks = slabs[q].chunks;
        const long row = slabs[q].row_first + f;
        const unsigned* p = ws + slabs[q].ws_first + f;
        const GateHistPlain h{hist + row * 2 * n_bins, n_bins};
        GateWalk W;
        GateTally<long> T;
        for (int ch = 0; ch < chunks; ++ch) gate_merge(W, p[(long)ch * m], T, h);
        gate_finish(W, T, h);
        long* c = counts + row * GATE_FIELDS;
        c[0] += T.n_open;
        c[1] += T.n_closed;
        c[2] += T.open_runs;
        c[3] += T.closed_runs;
        c[4] = c[4] > T.longest_open ? c[4] : T.longest_open;
        c[5] = c[5] > T.longest_closed ? c[5] : T.longest_closed;
        c[6] += T.openings;
        c[7] += T.closings;
        c[8] += T.complete_open_runs;
        c[9] += T.complete_closed_runs;
        c[10] += T.complete_open_frames;
        c[11] += T.complete_closed_frames;
    }
}

// slabs [first, last) share one launch (two kernels) and one workspace of `ws` summaries
struct GateLaunch {
    long first, last, items, lanes, ws;
};

// rows [dev, dev + rows) of the compact result are rows [host, host + rows) of the caller's arrays
struct GateCopy {
    long host, dev, rows;
};

// The plan of a call.  A threshold costs one summary of 4 bytes a chunk, so the thresholds of a job are cut into
// slabs of whole tiles that fit the budget, and slabs are gathered into launches while they fit.  The workspace of
// a call is the largest launch's: at most `budget` summaries, or one tile's share of the longest job where that
// alone is more.  Nothing of the result depends on the cut: a threshold's row is its own.
void gate_plan(const pw_gate_job* jobs, long n_jobs, long s_lo, long d_lo, long budget, std::vector<GateSlabDev>& slabs,
               std::vector<GateLaunch>& launches, std::vector<GateCopy>& copies) {
    long rows = 0;
    GateLaunch cur{0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_gate_job& J = jobs[k];
        const long n = (long)J.n, nt = (long)J.n_thr;
        if (n == 0 || nt == 0) continue;
        if (!copies.empty() && copies.back().host + copies.back().rows == (long)J.out_first)
            copies.back().rows += nt;
        else
            copies.push_back(GateCopy{(long)J.out_first, rows, nt});
        const long chunks = (n + GATE_CHUNK - 1) / GATE_CHUNK;
        long slab = nt;
        if (chunks > budget / nt) {
            slab = budget / chunks / GATE_TILE * GATE_TILE;
            if (slab < GATE_TILE) slab = GATE_TILE;
        }
        for (long q0 = 0; q0 < nt; q0 += slab) {
            GateSlabDev D{};
            D.n = n; D.a_first = (long)J.a_first - s_lo;
            D.d_first = (long)J.d_first + q0 - d_lo;
            D.m = nt - q0 < slab ? nt - q0 : slab;
            D.tiles = (int)((D.m + GATE_TILE - 1) / GATE_TILE);
            D.chunks = (int)chunks;
            if (cur.last > cur.first && cur.ws + chunks * D.m > budget) {
                launches.push_back(cur);
                cur = GateLaunch{cur.last, cur.last, 0, 0, 0};
            }
            D.ws_first = cur.ws; D.item_first = cur.items; D.lane_first = cur.lanes;
            D.row_first = rows;
            cur.ws += chunks * D.m;
            cur.items += (long)D.tiles * chunks;
            cur.lanes += D.m;
            rows += D.m;
            cur.last += 1;
            slabs.push_back(D);
        }
    }
    if (cur.last > cur.first) launches.push_back(cur);
}

// workspace_bytes: the budget of summaries (0: GATE_WORKSPACE_BYTES); kernel_ms: when not null, the time of all
// kernels of the call (the zeroing of the result included) by HIP events on the context's stream
int gate_counts(pw_context* ctx, const pw_gate_job* jobs, int64_t n_jobs, const double* series, const double* thresholds,
                int64_t n_bins, int64_t* counts, int64_t* hist, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0, d_lo = -1, d_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_gate_job& J = jobs[k];
        if (J.n < 0 || J.n_thr < 0 || J.a_first < 0 || J.d_first < 0 || J.out_first < 0)
            return stat_bad("pw_gate_counts", k, "negative range");
        if (J.n > GATE_MAX) return stat_bad("pw_gate_counts", k, "too long (n > 2^31)");
        if (n_bins < 0) return stat_bad("pw_gate_counts", k, "n_bins is negative");
        if (J.n == 0 || J.n_thr == 0) continue;
        if (!series || !thresholds || !counts) return stat_bad("pw_gate_counts", k, "null array");
        if (n_bins > 0 && !hist) return stat_bad("pw_gate_counts", k, "hist is null with n_bins > 0");
        for (long i = 0; i < (long)J.n; ++i) {
            const double v = series[J.a_first + i];
            if (!pw_finite(v) && !pw_isnan_bits(v)) return stat_bad("pw_gate_counts", k, "the series holds an infinity");
        }
        for (long i = 0; i < (long)J.n_thr; ++i)
            if (!pw_finite(thresholds[J.d_first + i]))
                return stat_bad("pw_gate_counts", k, "a threshold is a NaN or an infinity");
        const long lo = (long)J.a_first, hi = lo + (long)J.n, dl = (long)J.d_first, dh = dl + (long)J.n_thr;
        if (s_lo < 0 || lo < s_lo) s_lo = lo;
        if (hi > s_hi) s_hi = hi;
        if (d_lo < 0 || dl < d_lo) d_lo = dl;
        if (dh > d_hi) d_hi = dh;
    }
    if (s_lo < 0) return PW_OK;                                  // no job has a row
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_gate(jobs, (long)n_jobs, series, thresholds, (long)n_bins, (long*)counts, (long*)hist,
                                pw_context_host_threads(ctx, 0));

    std::vector<GateSlabDev> slabs;
    std::vector<GateLaunch> launches;
    std::vector<GateCopy> copies;
    gate_plan(jobs, (long)n_jobs, s_lo, d_lo, (long)(workspace_bytes ? workspace_bytes : GATE_WORKSPACE_BYTES) / 4, slabs,
              launches, copies);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_gate_counts", (long)n_jobs - 1, "too large");
    long words = 0;
    for (const GateLaunch& L : launches) words = L.ws > words ? L.ws : words;
    const long rows = slabs.back().row_first + slabs.back().m;
    const size_t count_bytes = sizeof(long) * (size_t)rows * GATE_FIELDS;
    const size_t hist_bytes = sizeof(long) * (size_t)rows * 2 * (size_t)n_bins;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        GateSlabDev* d_slabs;
        double *d_x, *d_thr;
        unsigned* d_ws;
        long *d_counts, *d_hist;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(GateSlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_thr, sizeof(double) * (size_t)(d_hi - d_lo)));
        STAT_TRY(buf.alloc(&d_ws, sizeof(unsigned) * (size_t)words));
        STAT_TRY(buf.alloc(&d_counts, count_bytes));
        STAT_TRY(buf.alloc(&d_hist, hist_bytes));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp; the result is zeroed below)
        STAT_TRY(poison_scratch(poison, d_ws, sizeof(unsigned) * (size_t)words, st));
        STAT_TRY(poison_scratch(poison, d_counts, count_bytes, st));
        STAT_TRY(poison_scratch(poison, d_hist, hist_bytes, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(GateSlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_x, series + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_thr, thresholds + d_lo, sizeof(double) * (size_t)(d_hi - d_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        STAT_TRY(hipMemsetAsync(d_counts, 0, count_bytes, st));
        if (hist_bytes) STAT_TRY(hipMemsetAsync(d_hist, 0, hist_bytes, st));
        // (launches follow one another on the stream, so the next one may take the workspace over; both kernels
        // stride over their work -- tests/test_gpu_launch_cap.py sends them round again -- and a launch has a slab, so
        // neither count is zero)
        for (const GateLaunch& L : launches) {
            const int count = (int)(L.last - L.first);
            hipLaunchKernelGGL(pw_gate_chunk_kernel, dim3((unsigned)launch_blocks(L.items, 1l << 20)), dim3(GATE_TILE), 0, st, d_slabs + L.first, count,
                               L.items, d_x, d_thr, d_ws, d_counts, d_hist, (long)n_bins);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_gate_merge_kernel, dim3((unsigned)launch_blocks((L.lanes + 255) / 256, 1l << 20)), dim3(256), 0, st, d_slabs + L.first,
                               count, L.lanes, d_ws, d_counts, d_hist, (long)n_bins);
            STAT_TRY(hipGetLastError());
        }
        STAT_TRY(ev.stop(st));
        // (the compact result is in job order: neighbours in the caller's arrays come back in one copy)
        for (const GateCopy& c : copies) {
            STAT_TRY(hipMemcpyAsync(counts + c.host * GATE_FIELDS, d_counts + c.dev * GATE_FIELDS,
                                    sizeof(long) * (size_t)c.rows * GATE_FIELDS, hipMemcpyDeviceToHost, st));
            if (hist_bytes)
                STAT_TRY(hipMemcpyAsync(hist + c.host * 2 * n_bins, d_hist + c.dev * 2 * n_bins,
                                        sizeof(long) * (size_t)c.rows * 2 * (size_t)n_bins, hipMemcpyDeviceToHost, st));
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_gate_counts(pw_context* ctx, const pw_gate_job* jobs, int64_t n_jobs, const double* series,
                              const double* thresholds, int64_t n_bins, int64_t* counts, int64_t* hist) {
    return gate_counts(ctx, jobs, n_jobs, series, thresholds, n_bins, counts, hist, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_gate_counts with the budget of summaries given (0: the
// default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_gate_counts(pw_context* ctx, const pw_gate_job* jobs, int64_t n_jobs, const double* series,
                                       const double* thresholds, int64_t n_bins, int64_t* counts, int64_t* hist,
                                       int64_t workspace_bytes, float* kernel_ms) {
    return gate_counts(ctx, jobs, n_jobs, series, thresholds, n_bins, counts, hist, workspace_bytes, kernel_ms);
}
