// pw_corr.hip -- gfx950 kernels and the C ABI entry of the lagged sums of a time correlation
// (include/pywindow_amd.h: pw_corr_sums; definition of the result in pw_corr.hpp).  Two kernels per launch pair,
// as for the KDE sums: the partial sums of every (slab of lags, chunk of times, tile of CORR_TILE lags) -- one
// wavefront each -- then the sum of a lag's partials in chunk order.
//
// A term is ONE FP64 FMA, so an operand fetched per term would leave the kernel waiting on LDS.  The partial
// kernel therefore works on a register tile of the Toeplitz product: a lane owns R = CORR_LANE_LAGS CONSECUTIVE
// lags k0 .. k0 + R - 1 and walks R consecutive times per step, so the 2R - 1 values b[t + k0 ..] it holds in
// registers and R wave-uniform values of a feed R x R FMAs; every lag's accumulator still runs strictly in t
// order.  Per step a lane reads R new values of b (R / 2 16-byte LDS reads; the image is padded by two doubles
// per R so that the lanes' 64-byte stride does not fall on the same banks) and the wave reads R values of a at
// one address (a broadcast).  Everything is queued on the context's stream, memory included.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_corr.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_corr(const pw_corr_job* jobs, long n_jobs, const double* series, double* sums,
                                int threads);      // pw_hostpath.cpp

namespace {

constexpr int R = CORR_LANE_LAGS;
constexpr int CORR_STEPS = CORR_CHUNK / R;                 // steps of R times in a chunk
constexpr int CORR_B_GROUPS = CORR_WAVE + CORR_STEPS;      // groups of R values of b a tile reads
constexpr int CORR_B_PITCH = R + 2;                        // doubles from one group to the next in LDS
static_assert(R == 8 && CORR_CHUNK % R == 0, "the register tile is written for eight lags a lane");

// a slab: lags [lag_first, lag_first + m) of one job
struct CorrSlabDev {
    long a_first, b_first, n;  // into the uploaded span of series
    long lag_first, m;
    long item_first;           // first (chunk, tile) pair of the slab in ITS launch
    long part_first;           // the slab's [chunks][m] partial sums in the workspace of its launch
    long out_first;            // the slab's m sums in the compact result of the call
    int tiles, chunks;         // chunks: those that have a term for the slab's first lag
};

// R doubles at a 16-byte aligned LDS address, as R / 2 16-byte reads
__device__ inline void corr_read(const double* p, double (&v)[R]) {
#pragma unroll
    for (int q = 0; q < R; q += 2) {
        const double2 d = *(const double2*)(p + q);
        v[q] = d.x; v[q + 1] = d.y;
    }
}

// One step: R times from `t` on against the lane's R lags.  lo, hi: b at those times + the lane's first lag and the
// R after them; lag r takes b[i + r] at time i, each accumulator in time order.
__device__ inline void corr_step(const double* s_a, int t, const double (&lo)[R], const double (&hi)[R], double (&acc)[R]) {
    double a[R];
    corr_read(s_a + t, a);
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = pw_fma(a[i], i + r < R ? lo[i + r] : hi[i + r - R], acc[r]);
    }
}

// The chunk's steps for one lane.  s_a: the chunk's a; s_bl: the lane's first group of b in the padded image.
// Three groups of b rotate through the roles (low half of the window, high half, being read for the step after),
// so the window slides without a register being moved; CORR_STEPS = 3 * 21 + 1.
// EDGE: the chunk is cut short for some lag of the tile.  Lag r of the lane has `count - r` terms (or all of the
// chunk where that is more), so a lane takes part in the steps that are whole for all its lags -- they come first
// in time -- and adds the few terms after them one by one at the end, each lag still in time order.
template <bool EDGE>
__device__ inline void corr_tile_chunk(const double* s_a, const double* s_bl, int count, double (&acc)[R]) {
    static_assert(CORR_STEPS % 3 == 1, "the rotation below ends on its first phase");
    double g0[R], g1[R], g2[R];
    corr_read(s_bl, g0);
    corr_read(s_bl + CORR_B_PITCH, g1);
    const double* next = s_bl + 2 * CORR_B_PITCH;
    const int whole = EDGE ? count - (2 * R - 1) : CORR_CHUNK;   // a step from t on is whole when t <= whole
    int t = 0;
    for (int s = 0; s < CORR_STEPS / 3; ++s, next += 3 * CORR_B_PITCH, t += 3 * R) {
        corr_read(next, g2);
        if (!EDGE || t <= whole) corr_step(s_a, t, g0, g1, acc);
        corr_read(next + CORR_B_PITCH, g0);
        if (!EDGE || t + R <= whole) corr_step(s_a, t + R, g1, g2, acc);
        corr_read(next + 2 * CORR_B_PITCH, g1);
        if (!EDGE || t + 2 * R <= whole) corr_step(s_a, t + 2 * R, g2, g0, acc);
    }
    if (!EDGE || t <= whole) corr_step(s_a, t, g0, g1, acc);
    if (EDGE) {
        const int end = count < CORR_CHUNK ? count : CORR_CHUNK;
        for (int u = whole < 0 ? 0 : (whole / R + 1) * R; u < end; ++u) {
            const double a = s_a[u];
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (u < count - r) acc[r] = pw_fma(a, s_bl[((u + r) / R) * CORR_B_PITCH + (u + r) % R], acc[r]);
        }
    }
}

__global__ void __launch_bounds__(CORR_WAVE)
pw_corr_partial_kernel(const CorrSlabDev* __restrict__ slabs, int n_slabs, long total, const double* __restrict__ series,
                       double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double s_a[CORR_CHUNK];
    __shared__ __attribute__((aligned(16))) double s_b[CORR_B_GROUPS * CORR_B_PITCH];
    const int lane = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int q = stat_find(n_slabs, item, [&](int j) { return slabs[j].item_first; });
        const CorrSlabDev job = slabs[q];
        const long local = item - job.item_first;
        const long chunk = local / job.tiles;
        const long tile = local - chunk * job.tiles;
        const long t0 = chunk * CORR_CHUNK;
        const long lag0 = job.lag_first + tile * CORR_TILE;      // the tile's first lag
        if (t0 >= job.n - lag0) continue;                        // no lag of the tile has a term in this chunk
        __syncthreads();                                         // (the previous item's images are done with)
        const double* a = series + job.a_first;
        const double* b = series + job.b_first;
        for (int i = lane; i < CORR_CHUNK; i += CORR_WAVE) s_a[i] = t0 + i < job.n ? a[t0 + i] : 0.0;
        for (int i = lane; i < CORR_B_GROUPS * R; i += CORR_WAVE) {
            const long at = t0 + lag0 + i;
            s_b[(i / R) * CORR_B_PITCH + (i % R)] = at < job.n ? b[at] : 0.0;
        }
        __syncthreads();
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        const long k0 = lag0 + (long)lane * R;                   // the lane's first lag
        const long left = job.n - k0 - t0;                       // terms of the lane's first lag from t0 on
        const int count = (int)(left < CORR_CHUNK + R ? (left < 0 ? 0 : left) : CORR_CHUNK + R);   // lag r: count - r of them
        const double* s_bl = s_b + lane * CORR_B_PITCH;
        if (t0 + CORR_CHUNK + lag0 + CORR_TILE - 1 <= job.n)     // the tile's last lag has the whole chunk
            corr_tile_chunk<false>(s_a, s_bl, count, acc);
        else
            corr_tile_chunk<true>(s_a, s_bl, count, acc);
        const long j0 = k0 - job.lag_first;                      // the lane's first lag within the slab
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (j0 + r < job.m && r < count) part[job.part_first + chunk * job.m + j0 + r] = acc[r];
    }
}

// the sums of the slabs of one launch: out[out_lo + t], t < count
__global__ void __launch_bounds__(256)
pw_corr_reduce_kernel(const CorrSlabDev* __restrict__ slabs, int n_slabs, long out_lo, long count,
                      const double* __restrict__ part, double* __restrict__ out) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x) {
        const int q = stat_find(n_slabs, t, [&](int j) { return slabs[j].out_first - out_lo; });
        const long m = slabs[q].m, j = out_lo + t - slabs[q].out_first;
        const long terms = slabs[q].n - (slabs[q].lag_first + j);            // >= 1: n_lags <= n
        const long chunks = (terms + CORR_CHUNK - 1) / CORR_CHUNK;
        const double* p = part + slabs[q].part_first + j;
        double s = p[0];
        for (long c = 1; c < chunks; ++c) s = s + p[c * m];
        out[out_lo + t] = s;
    }
}

// slabs [first, last) share one launch pair and one workspace of `parts` doubles
struct CorrLaunch {
    long first, last, items, parts, out_lo, out_hi;
};

// The plan of a call.  A job's [chunks][n_lags] partial sums may not fit the budget (1 000 000 x 32 768 lags:
// 512 MB), so its lags are cut into slabs of whole tiles whose partials do, and slabs are gathered into launches
// while they fit.  The workspace of a call is the largest launch's: at most `budget` doubles, or one tile's
// partials of the longest job where that alone is more.  Nothing of the result depends on the cut: a lag's sum
// is its own.
void corr_plan(const pw_corr_job* jobs, long n_jobs, long s_lo, long budget, std::vector<CorrSlabDev>& slabs,
               std::vector<CorrLaunch>& launches) {
    long outs = 0;
    CorrLaunch cur{0, 0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_corr_job& J = jobs[k];
        const long n = (long)J.n, lags = (long)J.n_lags;
        if (n == 0) continue;
        const long chunks_all = (n + CORR_CHUNK - 1) / CORR_CHUNK;
        long slab = lags;
        if (chunks_all > budget / lags) {
            slab = budget / chunks_all / CORR_TILE * CORR_TILE;
            if (slab < CORR_TILE) slab = CORR_TILE;
        }
        for (long l0 = 0; l0 < lags; l0 += slab) {
            CorrSlabDev D{};
            D.n = n; D.lag_first = l0; D.m = lags - l0 < slab ? lags - l0 : slab;
            D.a_first = (long)J.a_first - s_lo; D.b_first = (long)J.b_first - s_lo;
            const long chunks = (n - l0 + CORR_CHUNK - 1) / CORR_CHUNK;
            D.tiles = (int)((D.m + CORR_TILE - 1) / CORR_TILE); D.chunks = (int)chunks;
            if (cur.last > cur.first && cur.parts + chunks * D.m > budget) {
                launches.push_back(cur);
                cur = CorrLaunch{cur.last, cur.last, 0, 0, outs, outs};
            }
            D.item_first = cur.items; D.part_first = cur.parts; D.out_first = outs;
            cur.items += (long)D.tiles * chunks; cur.parts += chunks * D.m;
            outs += D.m;
            cur.last += 1; cur.out_hi = outs;
            slabs.push_back(D);
        }
    }
    if (cur.last > cur.first) launches.push_back(cur);
}

// workspace_bytes: the budget of the partial sums (0: CORR_WORKSPACE_BYTES); kernel_ms: when not null, the time
// of all kernels of the call by HIP events on the context's stream
int corr_sums(pw_context* ctx, const pw_corr_job* jobs, int64_t n_jobs, const double* series, double* sums,
              int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_corr_job& J = jobs[k];
        if (J.n < 0 || J.a_first < 0 || J.b_first < 0 || J.out_first < 0) return stat_bad("pw_corr_sums", k, "negative range");
        if (J.n_lags > J.n) return stat_bad("pw_corr_sums", k, "more lags than entries (n_lags > n)");
        if (J.n == 0) continue;
        if (J.n_lags < 1) return stat_bad("pw_corr_sums", k, "no lag (n_lags < 1)");
        if (!series || !sums) return stat_bad("pw_corr_sums", k, "null array");
        if ((J.n + CORR_CHUNK - 1) / CORR_CHUNK > 0x7fffffff) return stat_bad("pw_corr_sums", k, "too large");
        for (long i = 0; i < (long)J.n; ++i)
            if (!pw_finite(series[J.a_first + i]) || !pw_finite(series[J.b_first + i]))
                return stat_bad("pw_corr_sums", k, "a series holds a NaN or an infinity");
        const long lo = (long)(J.a_first < J.b_first ? J.a_first : J.b_first);
        const long hi = (long)(J.a_first > J.b_first ? J.a_first : J.b_first) + (long)J.n;
        if (s_lo < 0 || lo < s_lo) s_lo = lo;
        if (hi > s_hi) s_hi = hi;
    }
    if (s_lo < 0) return PW_OK;                                  // no job has an entry
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_corr(jobs, (long)n_jobs, series, sums, pw_context_host_threads(ctx, 0));

    std::vector<CorrSlabDev> slabs;
    std::vector<CorrLaunch> launches;
    corr_plan(jobs, (long)n_jobs, s_lo, (long)(workspace_bytes ? workspace_bytes : CORR_WORKSPACE_BYTES) / 8, slabs, launches);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_corr_sums", (long)n_jobs - 1, "too large");
    long parts = 0;
    for (const CorrLaunch& L : launches) parts = L.parts > parts ? L.parts : parts;
    const long outs = launches.back().out_hi;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<double> host_out((size_t)outs);
    {
        StreamBuffers buf(st);
        CorrSlabDev* d_slabs;
        double *d_x, *d_part, *d_out;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(CorrSlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_part, sizeof(double) * (size_t)parts));
        STAT_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_part, sizeof(double) * (size_t)parts, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(double) * (size_t)outs, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(CorrSlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_x, series + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over; both kernels
        // stride over their work, so the launch geometry is free)
        for (const CorrLaunch& L : launches) {
            const int count = (int)(L.last - L.first);
            const long grid1 = launch_blocks(L.items, 1l << 20);
            hipLaunchKernelGGL(pw_corr_partial_kernel, dim3((unsigned)grid1), dim3(CORR_WAVE), 0, st, d_slabs + L.first, count,
                               L.items, d_x, d_part);
            STAT_TRY(hipGetLastError());
            const long blocks2 = (L.out_hi - L.out_lo + 255) / 256;
            hipLaunchKernelGGL(pw_corr_reduce_kernel, dim3((unsigned)launch_blocks(blocks2, 65536)), dim3(256), 0, st,
                               d_slabs + L.first, count, L.out_lo, L.out_hi - L.out_lo, d_part, d_out);
            STAT_TRY(hipGetLastError());
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(host_out.data(), d_out, sizeof(double) * (size_t)outs, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    long at = 0;                                                 // (the compact result is in job order)
    for (long k = 0; k < (long)n_jobs; ++k)
        if (jobs[k].n)
            for (long j = 0; j < (long)jobs[k].n_lags; ++j) sums[jobs[k].out_first + j] = host_out[(size_t)at++];
    return PW_OK;
}

}  // namespace

extern "C" int pw_corr_sums(pw_context* ctx, const pw_corr_job* jobs, int64_t n_jobs, const double* series, double* sums) {
    return corr_sums(ctx, jobs, n_jobs, series, sums, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_corr_sums with the budget of the partial sums given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_corr_sums(pw_context* ctx, const pw_corr_job* jobs, int64_t n_jobs, const double* series,
                                     double* sums, int64_t workspace_bytes, float* kernel_ms) {
    return corr_sums(ctx, jobs, n_jobs, series, sums, workspace_bytes, kernel_ms);
}
