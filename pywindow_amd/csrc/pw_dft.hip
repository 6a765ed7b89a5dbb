// pw_dft.hip -- gfx950 kernels and the C ABI entry of the raw sums of a spectrum at rational frequencies
// (include/pywindow_amd.h: pw_dft_sums; definition of the result in pw_dft.hpp).  Three kernels per launch:
// the 512 twiddles of every frequency of the launch's slabs (the only transcendental work in proportion to the
// number of frequencies), the partial sums of every (frequency, chunk) -- the hot path, a real x complex matrix
// product without a sine or cosine in it -- and the rotation and sum of a frequency's partials in chunk order.
//
// A term is TWO FP64 FMAs that share the series' value, so an operand fetched per term would leave the kernel
// waiting on memory.  The partial kernel works on a register tile: a lane owns DFT_LANE_FREQS = 2 frequencies x
// DFT_WAVE_CHUNKS = 8 chunks (32 accumulators); per time step within the chunks it reads its two twiddles from LDS
// (two 16-byte reads, lanes consecutive: no bank conflict) and the eight chunks' a[t] from wave-uniform addresses of
// read-only memory (scalar loads into SGPRs, as pw_kdew.hip takes its weights), and issues 32 FMAs.  The four
// wavefronts of a workgroup share the frequencies and take consecutive groups of chunks, so a twiddle fetched from
// global memory into LDS once feeds 64 FMAs.  Every accumulator runs strictly in r order.  Everything is queued on
// the context's stream, memory included.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_dft.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_dft(const pw_dft_job* jobs, long n_jobs, const double* series, double* re, double* im,
                               int threads);       // pw_hostpath.cpp
extern "C" void pw_hostpath_dft_twiddles(long j, long M, const long* k, long n, double* c, double* s);

namespace {

constexpr int F = DFT_LANE_FREQS;
constexpr int C = DFT_WAVE_CHUNKS;
constexpr int DFT_THREADS = DFT_WAVE * DFT_GROUP_WAVES;
constexpr int DFT_RB = 8;                                  // time steps of one staged block of twiddles
constexpr int DFT_BLOCKS = DFT_CHUNK / DFT_RB;
constexpr int DFT_STAGE = DFT_RB * DFT_TILE / DFT_THREADS; // twiddles a thread moves per block
constexpr int DFT_RED_FREQS = 16;                          // frequencies of one block of the reduce kernel ...
constexpr int DFT_RED_CHUNKS = 16;                         // ... and chunks it rotates side by side
static_assert(DFT_CHUNK % DFT_RB == 0 && (DFT_RB * DFT_TILE) % DFT_THREADS == 0, "whole blocks, whole shares");
static_assert(DFT_RED_FREQS * DFT_RED_CHUNKS == 256, "the reduce kernel's block");

// a slab: frequencies [first, first + m) of one job; the workspace is an array of (cosine, sine) / (pc, ps) pairs
struct DftSlabDev {
    long a_first, n;           // into the uploaded span of series
    long M, j0, j_step;        // frequency f of the slab: j = j0 + f * j_step
    long m;
    long tw_first;             // the slab's [512][m] twiddles in the workspace of its launch
    long part_first;           // the slab's [chunks][m] partial sums there
    long out_first;            // the slab's m sums in the compact result of the call
    long tw_item_first;        // first of the slab's 512 m twiddles among those of ITS launch
    long item_first;           // first (group of chunks, tile of frequencies) pair of the slab in its launch
    long red_first;            // first block of DFT_RED_FREQS frequencies of the slab in its launch
    int tiles, groups, chunks;
};

// (cA, sA) of every (frequency, r < 512) of the slabs of one launch: pw_sincos once per pair
__global__ void __launch_bounds__(256)
pw_dft_twiddle_kernel(const DftSlabDev* __restrict__ slabs, int n_slabs, long total, double2* __restrict__ ws) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int q = stat_find(n_slabs, t, [&](int i) { return slabs[i].tw_item_first; });
        const long local = t - slabs[q].tw_item_first;     // r * m + f
        const long r = local / slabs[q].m, f = local - r * slabs[q].m;
        double c, s;
        dft_phase(slabs[q].j0 + f * slabs[q].j_step, r, slabs[q].M, &c, &s);
        ws[slabs[q].tw_first + local] = make_double2(c, s);
    }
}

// One staged block of DFT_RB time steps for one wavefront: s_tw[rr * DFT_TILE + f] the twiddles, a the series at
// the first time of the wave's first chunk + the block's first step (wave-uniform), acc[f][c] = (pc, ps).
// EDGE: some chunk of the wave is cut short or does not exist; chunk c has len[c] terms and sees exactly those.
template <bool EDGE>
__device__ inline void dft_block(const double2* s_tw, int lane, const double* __restrict__ a, int t0, const int (&len)[C],
                                 double2 (&acc)[F][C]) {
#pragma unroll
    for (int rr = 0; rr < DFT_RB; ++rr) {
        double2 tw[F];
#pragma unroll
        for (int i = 0; i < F; ++i) tw[i] = s_tw[rr * DFT_TILE + i * DFT_WAVE + lane];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (!EDGE || t0 + rr < len[c]) {
                const double av = a[c * DFT_CHUNK + rr];
#pragma unroll
                for (int i = 0; i < F; ++i) {
                    acc[i][c].x = pw_fma(av, tw[i].x, acc[i][c].x);
                    acc[i][c].y = pw_fma(av, tw[i].y, acc[i][c].y);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(DFT_THREADS)
pw_dft_partial_kernel(const DftSlabDev* __restrict__ slabs, int n_slabs, long total, const double* __restrict__ series,
                      double2* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) double2 s_tw[2][DFT_RB * DFT_TILE];
    const int tid = threadIdx.x, lane = tid & (DFT_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / DFT_WAVE);
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int q = stat_find(n_slabs, item, [&](int i) { return slabs[i].item_first; });
        const DftSlabDev job = slabs[q];
        const long local = item - job.item_first;
        const long group = local / job.tiles;
        const long f0 = (local - group * job.tiles) * DFT_TILE;      // the tile's first frequency within the slab
        const long ch0 = group * DFT_GROUP_CHUNKS + (long)wave * C;  // the wave's first chunk
        int len[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long left = job.n - (ch0 + c) * DFT_CHUNK;
            len[c] = (int)(left < 0 ? 0 : left < DFT_CHUNK ? left : DFT_CHUNK);
        }
        const bool whole = len[C - 1] == DFT_CHUNK;                  // (then every chunk of the wave is)
        const double* a = series + job.a_first + ch0 * DFT_CHUNK;
        double2 acc[F][C];
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[i][c] = make_double2(0.0, 0.0);
        // a thread's share of a block of twiddles: elements tid + DFT_THREADS * i of [DFT_RB][DFT_TILE]
        const double2* tw = ws + job.tw_first + f0;
        double2 stage[DFT_STAGE];
        auto fetch = [&](int rb) {
#pragma unroll
            for (int i = 0; i < DFT_STAGE; ++i) {
                const int e = tid + DFT_THREADS * i, rr = e / DFT_TILE, ff = e % DFT_TILE;
                stage[i] = f0 + ff < job.m ? tw[(long)(rb * DFT_RB + rr) * job.m + ff] : make_double2(0.0, 0.0);
            }
        };
        auto put = [&](int buf) {
#pragma unroll
            for (int i = 0; i < DFT_STAGE; ++i) s_tw[buf][tid + DFT_THREADS * i] = stage[i];
        };
        fetch(0);
        __syncthreads();                                             // (the previous item's images are done with)
        put(0);
        __syncthreads();
        for (int rb = 0; rb < DFT_BLOCKS; ++rb) {
            if (rb + 1 < DFT_BLOCKS) fetch(rb + 1);
            if (whole)
                dft_block<false>(s_tw[rb & 1], lane, a + rb * DFT_RB, rb * DFT_RB, len, acc);
            else if (len[0] > rb * DFT_RB)
                dft_block<true>(s_tw[rb & 1], lane, a + rb * DFT_RB, rb * DFT_RB, len, acc);
            if (rb + 1 < DFT_BLOCKS) put((rb + 1) & 1);              // (last read one barrier ago)
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (len[c] > 0) {
#pragma unroll
                for (int i = 0; i < F; ++i) {
                    const long f = f0 + i * DFT_WAVE + lane;
                    if (f < job.m) ws[job.part_first + (ch0 + c) * job.m + f] = acc[i][c];
                }
            }
        }
    }
}

// the sums of the slabs of one launch.  A block takes DFT_RED_FREQS frequencies; the rotations of DFT_RED_CHUNKS
// chunks are computed side by side (they are independent), then one thread per frequency adds them in chunk order.
__global__ void __launch_bounds__(256)
pw_dft_reduce_kernel(const DftSlabDev* __restrict__ slabs, int n_slabs, long total, long outs,
                     const double2* __restrict__ ws, double* __restrict__ out) {
    __shared__ double2 s_rot[DFT_RED_CHUNKS][DFT_RED_FREQS];
    const int fl = threadIdx.x % DFT_RED_FREQS, cl = threadIdx.x / DFT_RED_FREQS;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int q = stat_find(n_slabs, item, [&](int i) { return slabs[i].red_first; });
        const long f = (item - slabs[q].red_first) * DFT_RED_FREQS + fl;
        const long m = slabs[q].m, M = slabs[q].M;
        const int chunks = slabs[q].chunks;
        const bool live = f < m;
        const long j = slabs[q].j0 + f * slabs[q].j_step;
        const double2* p = ws + slabs[q].part_first + f;
        double re = 0.0, im = 0.0;
        for (int base = 0; base < chunks; base += DFT_RED_CHUNKS) {
            const int ch = base + cl;
            if (live && ch < chunks) {
                const double2 v = p[(long)ch * m];
                double cB, sB, x, y;
                dft_phase(j, (long)ch * DFT_CHUNK, M, &cB, &sB);
                dft_rotate(cB, sB, v.x, v.y, &x, &y);
                s_rot[cl][fl] = make_double2(x, y);
            }
            __syncthreads();
            if (live && cl == 0) {
                const int count = chunks - base < DFT_RED_CHUNKS ? chunks - base : DFT_RED_CHUNKS;
                for (int c = 0; c < count; ++c) {
                    re = re + s_rot[c][fl].x;
                    im = im + s_rot[c][fl].y;
                }
            }
            __syncthreads();
        }
        if (live && cl == 0) {
            out[slabs[q].out_first + f] = re;
            out[outs + slabs[q].out_first + f] = im;
        }
    }
}

// the phases of arbitrary k (test hook)
__global__ void __launch_bounds__(256)
pw_dft_phase_kernel(long j, long M, const long* __restrict__ k, long n, double* __restrict__ c, double* __restrict__ s) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
        dft_phase(j, k[t], M, &c[t], &s[t]);
}

// slabs [first, last) share one launch (three kernels) and one workspace of `ws` pairs of doubles
struct DftLaunch {
    long first, last, tw_items, items, red_items, ws;
};

// The plan of a call.  A frequency costs 512 twiddles and `chunks` partial sums of 16 bytes each, so the
// frequencies of a job are cut into slabs of whole tiles that fit the budget, and slabs are gathered into launches
// while they fit.  The workspace of a call is the largest launch's: at most `budget` pairs, or one tile's share
// of the longest job where that alone is more.  Nothing of the result depends on the cut: a frequency's sum is
// its own.
void dft_plan(const pw_dft_job* jobs, long n_jobs, long s_lo, long budget, std::vector<DftSlabDev>& slabs,
              std::vector<DftLaunch>& launches) {
    long outs = 0;
    DftLaunch cur{0, 0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_dft_job& J = jobs[k];
        const long n = (long)J.n, nf = (long)J.n_freq;
        if (n == 0 || nf == 0) continue;
        const long chunks = (n + DFT_CHUNK - 1) / DFT_CHUNK;
        const long each = DFT_CHUNK + chunks;                        // pairs of one frequency
        long slab = nf;
        if (each > budget / nf) {
            slab = budget / each / DFT_TILE * DFT_TILE;
            if (slab < DFT_TILE) slab = DFT_TILE;
        }
        for (long q0 = 0; q0 < nf; q0 += slab) {
            DftSlabDev D{};
            D.n = n; D.a_first = (long)J.a_first - s_lo;
            D.M = (long)J.period; D.j_step = (long)J.j_step; D.j0 = (long)J.j_first + q0 * (long)J.j_step;
            D.m = nf - q0 < slab ? nf - q0 : slab;
            D.tiles = (int)((D.m + DFT_TILE - 1) / DFT_TILE);
            D.chunks = (int)chunks;
            D.groups = (int)((chunks + DFT_GROUP_CHUNKS - 1) / DFT_GROUP_CHUNKS);
            if (cur.last > cur.first && cur.ws + each * D.m > budget) {
                launches.push_back(cur);
                cur = DftLaunch{cur.last, cur.last, 0, 0, 0, 0};
            }
            D.tw_first = cur.ws; D.part_first = cur.ws + DFT_CHUNK * D.m;
            D.tw_item_first = cur.tw_items; D.item_first = cur.items; D.red_first = cur.red_items;
            D.out_first = outs;
            cur.ws += each * D.m;
            cur.tw_items += DFT_CHUNK * D.m;
            cur.items += (long)D.tiles * D.groups;
            cur.red_items += (D.m + DFT_RED_FREQS - 1) / DFT_RED_FREQS;
            outs += D.m;
            cur.last += 1;
            slabs.push_back(D);
        }
    }
    if (cur.last > cur.first) launches.push_back(cur);
}

// workspace_bytes: the budget of twiddles and partial sums (0: DFT_WORKSPACE_BYTES); kernel_ms: when not null, the
// time of all kernels of the call by HIP events on the context's stream
int dft_sums(pw_context* ctx, const pw_dft_job* jobs, int64_t n_jobs, const double* series, double* re, double* im,
             int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_dft_job& J = jobs[k];
        if (J.n < 0 || J.n_freq < 0 || J.a_first < 0 || J.out_first < 0) return stat_bad("pw_dft_sums", k, "negative range");
        if (J.n > DFT_MAX) return stat_bad("pw_dft_sums", k, "too long (n > 2^31)");
        if (J.period < 2 || J.period > DFT_MAX) return stat_bad("pw_dft_sums", k, "period outside 2 .. 2^31");
        if (J.j_step < 1) return stat_bad("pw_dft_sums", k, "j_step < 1");
        if (J.j_first < 0 || J.j_first >= J.period)
            return stat_bad("pw_dft_sums", k, "a frequency outside 0 .. period - 1 (j_first)");
        if (J.n_freq > 0 && (J.n_freq - 1 > (J.period - 1 - J.j_first) / J.j_step))
            return stat_bad("pw_dft_sums", k, "a frequency outside 0 .. period - 1 (j_first + (n_freq - 1) j_step >= period)");
        if (J.n == 0 || J.n_freq == 0) continue;
        if (!series || !re || !im) return stat_bad("pw_dft_sums", k, "null array");
        for (long i = 0; i < (long)J.n; ++i)
            if (!pw_finite(series[J.a_first + i])) return stat_bad("pw_dft_sums", k, "the series holds a NaN or an infinity");
        const long lo = (long)J.a_first, hi = lo + (long)J.n;
        if (s_lo < 0 || lo < s_lo) s_lo = lo;
        if (hi > s_hi) s_hi = hi;
    }
    if (s_lo < 0) return PW_OK;                                  // no job has a term
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_dft(jobs, (long)n_jobs, series, re, im, pw_context_host_threads(ctx, 0));

    std::vector<DftSlabDev> slabs;
    std::vector<DftLaunch> launches;
    dft_plan(jobs, (long)n_jobs, s_lo, (long)(workspace_bytes ? workspace_bytes : DFT_WORKSPACE_BYTES) / 16, slabs, launches);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_dft_sums", (long)n_jobs - 1, "too large");
    long pairs = 0;
    for (const DftLaunch& L : launches) pairs = L.ws > pairs ? L.ws : pairs;
    const long outs = slabs.back().out_first + slabs.back().m;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<double> host_out((size_t)outs * 2);
    {
        StreamBuffers buf(st);
        DftSlabDev* d_slabs;
        double *d_x, *d_out;
        double2* d_ws;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(DftSlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_ws, sizeof(double2) * (size_t)pairs));
        STAT_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs * 2));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, sizeof(double2) * (size_t)pairs, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(double) * (size_t)outs * 2, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(DftSlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_x, series + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over; all three kernels
        // stride over their work -- tests/test_gpu_launch_cap.py sends them round again -- and a launch has a slab, so
        // none of the three counts is zero)
        for (const DftLaunch& L : launches) {
            const int count = (int)(L.last - L.first);
            hipLaunchKernelGGL(pw_dft_twiddle_kernel, dim3((unsigned)launch_blocks((L.tw_items + 255) / 256, 1l << 20)), dim3(256), 0, st,
                               d_slabs + L.first, count, L.tw_items, d_ws);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_dft_partial_kernel, dim3((unsigned)launch_blocks(L.items, 1l << 20)), dim3(DFT_THREADS), 0, st, d_slabs + L.first,
                               count, L.items, d_x, d_ws);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_dft_reduce_kernel, dim3((unsigned)launch_blocks(L.red_items, 1l << 20)), dim3(256), 0, st, d_slabs + L.first, count,
                               L.red_items, outs, d_ws, d_out);
            STAT_TRY(hipGetLastError());
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(host_out.data(), d_out, sizeof(double) * (size_t)outs * 2, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    long at = 0;                                                 // (the compact result is in job order)
    for (long k = 0; k < (long)n_jobs; ++k)
        if (jobs[k].n && jobs[k].n_freq)
            for (long q = 0; q < (long)jobs[k].n_freq; ++q, ++at) {
                re[jobs[k].out_first + q] = host_out[(size_t)at];
                im[jobs[k].out_first + q] = host_out[(size_t)(outs + at)];
            }
    return PW_OK;
}

}  // namespace

extern "C" int pw_dft_sums(pw_context* ctx, const pw_dft_job* jobs, int64_t n_jobs, const double* series, double* re,
                           double* im) {
    return dft_sums(ctx, jobs, n_jobs, series, re, im, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_dft_sums with the budget of twiddles and partial sums given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_dft_sums(pw_context* ctx, const pw_dft_job* jobs, int64_t n_jobs, const double* series,
                                    double* re, double* im, int64_t workspace_bytes, float* kernel_ms) {
    return dft_sums(ctx, jobs, n_jobs, series, re, im, workspace_bytes, kernel_ms);
}

// test hook (not part of the header): c[i], s[i] = the phase of (j, k[i]) as pw_dft.hpp defines it, computed on the
// context's device or, for a device == -1 context, on the host.  0 <= j < M, 2 <= M <= 2^31, 0 <= k[i] <= 2^32.
extern "C" int pw_internal_dft_twiddles(pw_context* ctx, int64_t j, int64_t M, const int64_t* k, int64_t n, double* c,
                                        double* s) {
    if (!ctx || n < 0 || M < 2 || M > DFT_MAX || j < 0 || j >= M || (n && (!k || !c || !s))) return PW_E_BAD_ARG;
    for (long i = 0; i < (long)n; ++i)
        if (k[i] < 0 || k[i] > (1ll << 32)) return PW_E_BAD_ARG;
    if (n == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    if (pw_context_device(ctx) < 0) {
        pw_hostpath_dft_twiddles((long)j, (long)M, (const long*)k, (long)n, c, s);
        return PW_OK;
    }
    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    {
        StreamBuffers buf(st);
        long* d_k;
        double* d_cs;
        STAT_TRY(buf.alloc(&d_k, sizeof(long) * (size_t)n));
        STAT_TRY(buf.alloc(&d_cs, sizeof(double) * (size_t)n * 2));
        STAT_TRY(hipMemcpyAsync(d_k, k, sizeof(long) * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(pw_dft_phase_kernel, dim3((unsigned)launch_blocks((n + 255) / 256, 1l << 20)), dim3(256), 0, st, (long)j, (long)M, d_k,
                           (long)n, d_cs, d_cs + n);
        STAT_TRY(hipGetLastError());
        STAT_TRY(hipMemcpyAsync(c, d_cs, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
        STAT_TRY(hipMemcpyAsync(s, d_cs + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    return PW_OK;
}
