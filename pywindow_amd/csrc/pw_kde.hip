// pw_kde.hip -- gfx950 kernels and the C ABI entry of the Gaussian KDE sums (include/pywindow_amd.h:
// pw_kde_sums; definition of the result in pw_kde.hpp).  Two kernels per call: the partial sums of
// every (job, chunk of samples, tile of grid points) -- one wavefront each, a lane owning
// KDE_LANE_POINTS grid points in registers, the chunk's samples staged in LDS and read at one address
// per wave (a broadcast), pw_exp's 2 KB table in LDS as well -- then the sum of the partials in chunk
// order.  Everything is queued on the context's stream, memory included (stream-ordered allocation:
// nothing here waits for other work of the device).
// pw_kde2_sums, the two-dimensional entry, follows the same plan with kernels of its own (pw_kde2_*): the
// job shape is the opposite one -- few samples, a mesh of many points -- so the points of a call go through
// in slabs whose partial sums stay within KDE2_WORKSPACE_BYTES, one launch pair per slab group.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_stat_host.hpp"
#include "pw_kde.hpp"

using namespace pw;

extern "C" int pw_hostpath_kde(const pw_kde_job* jobs, long n_jobs, const double* samples, const double* points,
                               double* sums, int threads);   // pw_hostpath.cpp
extern "C" void pw_hostpath_exp(const double* x, long n, double* y);
extern "C" int pw_hostpath_kde2(const pw_kde2_job* jobs, long n_jobs, const double* samples, const double* points,
                                double* sums, int threads);

namespace {

struct KdeJobDev {
    long sample_first, n;      // into the uploaded span of samples
    long point_first, m;       // into the uploaded span of points
    double r;
    long item_first;           // first (chunk, tile) pair of the job in the launch; entry n_jobs: the total
    long part_first;           // the job's [chunks][m] partial sums
    long out_first;            // the job's m sums in the compact result; entry n_jobs: the total
    int tiles, chunks;
};

__global__ void __launch_bounds__(KDE_WAVE)
pw_kde_partial_kernel(const KdeJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ samples,
                      const double* __restrict__ points, double* __restrict__ part) {
    __shared__ double s_x[KDE_CHUNK];
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += KDE_WAVE) s_tab[t] = POW_EXP_TAB[t];
    const long total = jobs[n_jobs].item_first;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
        const KdeJobDev job = jobs[k];
        const long local = item - job.item_first;
        const long chunk = local / job.tiles;
        const long tile = local - chunk * job.tiles;
        const long i0 = chunk * KDE_CHUNK;
        const int len = (int)(job.n - i0 < KDE_CHUNK ? job.n - i0 : KDE_CHUNK);
        __syncthreads();                                   // (the previous item's samples are done with)
        for (int t = lane; t < len; t += KDE_WAVE) s_x[t] = samples[job.sample_first + i0 + t];
        __syncthreads();
        double g[KDE_LANE_POINTS], acc[KDE_LANE_POINTS];
        long j[KDE_LANE_POINTS];
#pragma unroll
        for (int p = 0; p < KDE_LANE_POINTS; ++p) {
            j[p] = tile * KDE_TILE + p * KDE_WAVE + lane;
            g[p] = j[p] < job.m ? points[job.point_first + j[p]] : 0.0;
            acc[p] = 0.0;
        }
        // kde_chunk_sum for KDE_LANE_POINTS points side by side: the same additions in the same order
        for (int i = 0; i < len; ++i) {
            const double x = s_x[i];
#pragma unroll
            for (int p = 0; p < KDE_LANE_POINTS; ++p) acc[p] = acc[p] + kde_term(g[p], x, job.r, s_tab);
        }
#pragma unroll
        for (int p = 0; p < KDE_LANE_POINTS; ++p)
            if (j[p] < job.m) part[job.part_first + chunk * job.m + j[p]] = acc[p];
    }
}

__global__ void __launch_bounds__(256)
pw_kde_reduce_kernel(const KdeJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ part,
                     double* __restrict__ out) {
    const long total = jobs[n_jobs].out_first;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int k = stat_find(n_jobs, t, [&](int q) { return jobs[q].out_first; });
        const long m = jobs[k].m, j = t - jobs[k].out_first;
        const double* p = part + jobs[k].part_first + j;
        double s = 0.0;
        for (int c = 0; c < jobs[k].chunks; ++c) s = c == 0 ? p[0] : s + p[(long)c * m];
        out[t] = s;
    }
}

// ---- two dimensions ----------------------------------------------------------------------------------

// a slab: points [point_first, point_first + m) of one job, all of the job's samples
struct Kde2SlabDev {
    long sample_first, n;      // pairs, into the uploaded span of samples
    long point_first, m;       // pairs, into the uploaded span of points
    double w00, w10, w11;
    long item_first;           // first (chunk, tile) pair of the slab in ITS launch
    long part_first;           // the slab's [chunks][m] partial sums in the workspace of its launch
    long out_first;            // the slab's m sums in the compact result of the call
    int tiles, chunks;
};

// One wavefront per (slab, chunk, tile of KDE2_TILE points).  A lane keeps KDE2_LANE_POINTS points -- both
// coordinates and the accumulator -- in registers; the chunk's sample pairs go through LDS KDE2_STAGE at a
// time, in order, and a pair is one 16-byte read at one address per wave (a broadcast), as the table read is.
__global__ void __launch_bounds__(KDE_WAVE)
pw_kde2_partial_kernel(const Kde2SlabDev* __restrict__ slabs, int n_slabs, long total, const double2* __restrict__ samples,
                       const double2* __restrict__ points, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double2 s_xy[KDE2_STAGE];
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += KDE_WAVE) s_tab[t] = POW_EXP_TAB[t];
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = stat_find(n_slabs, item, [&](int q) { return slabs[q].item_first; });
        const Kde2SlabDev job = slabs[k];
        const long local = item - job.item_first;
        const long chunk = local / job.tiles;
        const long tile = local - chunk * job.tiles;
        const long i0 = chunk * KDE_CHUNK;
        const int len = (int)(job.n - i0 < KDE_CHUNK ? job.n - i0 : KDE_CHUNK);
        double g0[KDE2_LANE_POINTS], g1[KDE2_LANE_POINTS], acc[KDE2_LANE_POINTS];
        long j[KDE2_LANE_POINTS];
#pragma unroll
        for (int p = 0; p < KDE2_LANE_POINTS; ++p) {
            j[p] = tile * KDE2_TILE + p * KDE_WAVE + lane;
            const double2 g = j[p] < job.m ? points[job.point_first + j[p]] : double2{0.0, 0.0};
            g0[p] = g.x; g1[p] = g.y;
            acc[p] = 0.0;
        }
        for (int s0 = 0; s0 < len; s0 += KDE2_STAGE) {
            const int slen = len - s0 < KDE2_STAGE ? len - s0 : KDE2_STAGE;
            __syncthreads();                               // (the pairs staged before are done with)
            for (int t = lane; t < slen; t += KDE_WAVE) s_xy[t] = samples[job.sample_first + i0 + s0 + t];
            __syncthreads();
            // kde2_chunk_sum for KDE2_LANE_POINTS points side by side: the same additions in the same order
#pragma unroll 2
            for (int i = 0; i < slen; ++i) {
                const double2 x = s_xy[i];
#pragma unroll
                for (int p = 0; p < KDE2_LANE_POINTS; ++p)
                    acc[p] = acc[p] + kde2_term(g0[p], g1[p], x.x, x.y, job.w00, job.w10, job.w11, s_tab);
            }
        }
#pragma unroll
        for (int p = 0; p < KDE2_LANE_POINTS; ++p)
            if (j[p] < job.m) part[job.part_first + chunk * job.m + j[p]] = acc[p];
    }
}

// the sums of the slabs of one launch: out[out_lo + t], t < count
__global__ void __launch_bounds__(256)
pw_kde2_reduce_kernel(const Kde2SlabDev* __restrict__ slabs, int n_slabs, long out_lo, long count,
                      const double* __restrict__ part, double* __restrict__ out) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x) {
        const int k = stat_find(n_slabs, t, [&](int q) { return slabs[q].out_first - out_lo; });
        const long m = slabs[k].m, j = out_lo + t - slabs[k].out_first;
        const double* p = part + slabs[k].part_first + j;
        double s = 0.0;
        for (int c = 0; c < slabs[k].chunks; ++c) s = c == 0 ? p[0] : s + p[(long)c * m];
        out[out_lo + t] = s;
    }
}

// pw_exp itself, element by element, with the table where the KDE kernel keeps it (test instrumentation)
__global__ void __launch_bounds__(256)
pw_exp_kernel(long n, const double* __restrict__ x, double* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    s_tab[threadIdx.x] = POW_EXP_TAB[threadIdx.x];
    __syncthreads();
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        y[i] = pw_exp_tab(x[i], s_tab);
}

// kernel_ms: when not null, the time of the two kernels by HIP events on the context's stream
int kde_sums(pw_context* ctx, const pw_kde_job* jobs, int64_t n_jobs, const double* samples, const double* points,
             double* sums, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs)) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0, p_lo = -1, p_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_kde_job& J = jobs[k];
        if (J.n_samples < 0 || J.n_points < 0 || J.sample_first < 0 || J.point_first < 0)
            return stat_bad("pw_kde_sums", k, "negative range");
        if ((J.n_samples && !samples) || (J.n_points && (!points || !sums))) return stat_bad("pw_kde_sums", k, "null array");
        if (!pw_finite(J.inv_bandwidth) || !(J.inv_bandwidth > 0.0))
            return stat_bad("pw_kde_sums", k, "bandwidth not positive and finite");
        for (long i = 0; i < (long)J.n_samples; ++i)
            if (!pw_finite(samples[J.sample_first + i])) return stat_bad("pw_kde_sums", k, "a sample is NaN or infinite");
        for (long i = 0; i < (long)J.n_points; ++i)
            if (!pw_finite(points[J.point_first + i])) return stat_bad("pw_kde_sums", k, "a point is NaN or infinite");
        if (J.n_samples) {
            if (s_lo < 0 || J.sample_first < s_lo) s_lo = (long)J.sample_first;
            if (J.sample_first + J.n_samples > s_hi) s_hi = (long)(J.sample_first + J.n_samples);
        }
        if (J.n_points) {
            if (p_lo < 0 || J.point_first < p_lo) p_lo = (long)J.point_first;
            if (J.point_first + J.n_points > p_hi) p_hi = (long)(J.point_first + J.n_points);
        }
    }
    if (p_lo < 0) return PW_OK;                                  // no job has a point
    if (s_lo < 0) s_lo = s_hi = 0;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_kde(jobs, (long)n_jobs, samples, points, sums, pw_context_host_threads(ctx, 0));

    std::vector<KdeJobDev> dev((size_t)n_jobs + 1);
    long items = 0, parts = 0, outs = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_kde_job& J = jobs[k];
        KdeJobDev& D = dev[k];
        D.n = (long)J.n_samples; D.m = (long)J.n_points;
        D.sample_first = D.n ? (long)J.sample_first - s_lo : 0;
        D.point_first = D.m ? (long)J.point_first - p_lo : 0;
        D.r = J.inv_bandwidth;
        const long tiles = (D.m + KDE_TILE - 1) / KDE_TILE, chunks = D.m ? (D.n + KDE_CHUNK - 1) / KDE_CHUNK : 0;
        if (tiles > 0x7fffffff || chunks > 0x7fffffff) return stat_bad("pw_kde_sums", k, "too large");
        D.tiles = (int)tiles; D.chunks = (int)chunks;
        D.item_first = items; D.part_first = parts; D.out_first = outs;
        items += tiles * chunks; parts += chunks * D.m; outs += D.m;
    }
    KdeJobDev& E = dev[n_jobs];
    E = KdeJobDev{};
    E.item_first = items; E.part_first = parts; E.out_first = outs;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<double> host_out((size_t)outs);
    {
        StreamBuffers buf(st);
        KdeJobDev* d_jobs;
        double *d_x, *d_g, *d_part, *d_out;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(KdeJobDev) * dev.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_g, sizeof(double) * (size_t)(p_hi - p_lo)));
        STAT_TRY(buf.alloc(&d_part, sizeof(double) * (size_t)parts));
        STAT_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_part, sizeof(double) * (size_t)parts, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(double) * (size_t)outs, st));
        STAT_TRY(hipMemcpyAsync(d_jobs, dev.data(), sizeof(KdeJobDev) * dev.size(), hipMemcpyHostToDevice, st));
        if (s_hi > s_lo)
            STAT_TRY(hipMemcpyAsync(d_x, samples + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_g, points + p_lo, sizeof(double) * (size_t)(p_hi - p_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (a job without samples has no pair and its sums are the reduce kernel's zeros; the launch geometry is
        // free: both kernels stride over their work)
        const long grid1 = items < 1 ? 1 : launch_blocks(items, 1l << 20);
        hipLaunchKernelGGL(pw_kde_partial_kernel, dim3((unsigned)grid1), dim3(KDE_WAVE), 0, st, d_jobs, (int)n_jobs, d_x, d_g,
                           d_part);
        STAT_TRY(hipGetLastError());
        const long blocks2 = (outs + 255) / 256;
        hipLaunchKernelGGL(pw_kde_reduce_kernel, dim3((unsigned)launch_blocks(blocks2, 65536)), dim3(256), 0, st, d_jobs,
                           (int)n_jobs, d_part, d_out);
        STAT_TRY(hipGetLastError());
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(host_out.data(), d_out, sizeof(double) * (size_t)outs, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    for (long k = 0; k < (long)n_jobs; ++k)
        for (long j = 0; j < dev[k].m; ++j) sums[jobs[k].point_first + j] = host_out[(size_t)(dev[k].out_first + j)];
    return PW_OK;
}

// slabs [first, last) share one launch pair and one workspace of `parts` doubles
struct Kde2Launch {
    long first, last, items, parts, out_lo, out_hi;
};

// The plan of a call.  A job's [chunks][m] partial sums may not fit the budget (400 000 samples x 65 536 points:
// 410 MB), so its points are cut into slabs of whole tiles whose partials do, and slabs are gathered into
// launches while they fit.  The workspace of a call is the largest launch's: at most `budget` doubles, or one
// tile's partials of the longest job where that alone is more (n > 33e6 at the default).  Nothing of the result
// depends on the cut: a point's sum is its own.
void kde2_plan(const pw_kde2_job* jobs, long n_jobs, long s_lo, long p_lo, long budget, std::vector<Kde2SlabDev>& slabs,
               std::vector<Kde2Launch>& launches) {
    long outs = 0;
    Kde2Launch cur{0, 0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_kde2_job& J = jobs[k];
        const long n = (long)J.n_samples, m = (long)J.n_points;
        if (m == 0) continue;
        const long chunks = (n + KDE_CHUNK - 1) / KDE_CHUNK;
        long slab = m;
        if (chunks && chunks > budget / m) {
            slab = budget / chunks / KDE2_TILE * KDE2_TILE;
            if (slab < KDE2_TILE) slab = KDE2_TILE;
        }
        for (long p0 = 0; p0 < m; p0 += slab) {
            Kde2SlabDev D{};
            D.n = n; D.m = m - p0 < slab ? m - p0 : slab;
            D.sample_first = n ? (long)J.sample_first - s_lo : 0;
            D.point_first = (long)J.point_first - p_lo + p0;
            D.w00 = J.w00; D.w10 = J.w10; D.w11 = J.w11;
            D.tiles = (int)((D.m + KDE2_TILE - 1) / KDE2_TILE); D.chunks = (int)chunks;
            if (cur.last > cur.first && cur.parts + chunks * D.m > budget) {
                launches.push_back(cur);
                cur = Kde2Launch{cur.last, cur.last, 0, 0, outs, outs};
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

// workspace_bytes: the budget of the partial sums (0: KDE2_WORKSPACE_BYTES); kernel_ms: when not null, the time
// of all kernels of the call by HIP events on the context's stream
int kde2_sums(pw_context* ctx, const pw_kde2_job* jobs, int64_t n_jobs, const double* samples, const double* points,
              double* sums, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0, p_lo = -1, p_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_kde2_job& J = jobs[k];
        if (J.n_samples < 0 || J.n_points < 0 || J.sample_first < 0 || J.point_first < 0)
            return stat_bad("pw_kde2_sums", k, "negative range");
        if ((J.n_samples && !samples) || (J.n_points && (!points || !sums))) return stat_bad("pw_kde2_sums", k, "null array");
        if (!pw_finite(J.w00) || !pw_finite(J.w10) || !pw_finite(J.w11) || !(J.w00 > 0.0) || !(J.w11 > 0.0))
            return stat_bad("pw_kde2_sums", k, "factors not finite with a positive diagonal");
        if ((J.n_samples + KDE_CHUNK - 1) / KDE_CHUNK > 0x7fffffff) return stat_bad("pw_kde2_sums", k, "too large");
        for (long i = 0; i < 2 * (long)J.n_samples; ++i)
            if (!pw_finite(samples[2 * J.sample_first + i])) return stat_bad("pw_kde2_sums", k, "a sample is NaN or infinite");
        for (long i = 0; i < 2 * (long)J.n_points; ++i)
            if (!pw_finite(points[2 * J.point_first + i])) return stat_bad("pw_kde2_sums", k, "a point is NaN or infinite");
        if (J.n_samples) {
            if (s_lo < 0 || J.sample_first < s_lo) s_lo = (long)J.sample_first;
            if (J.sample_first + J.n_samples > s_hi) s_hi = (long)(J.sample_first + J.n_samples);
        }
        if (J.n_points) {
            if (p_lo < 0 || J.point_first < p_lo) p_lo = (long)J.point_first;
            if (J.point_first + J.n_points > p_hi) p_hi = (long)(J.point_first + J.n_points);
        }
    }
    if (p_lo < 0) return PW_OK;                                  // no job has a point
    if (s_lo < 0) s_lo = s_hi = 0;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_kde2(jobs, (long)n_jobs, samples, points, sums, pw_context_host_threads(ctx, 0));

    std::vector<Kde2SlabDev> slabs;
    std::vector<Kde2Launch> launches;
    kde2_plan(jobs, (long)n_jobs, s_lo, p_lo, (long)(workspace_bytes ? workspace_bytes : KDE2_WORKSPACE_BYTES) / 8, slabs, launches);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_kde2_sums", (long)n_jobs - 1, "too large");
    long parts = 0;
    for (const Kde2Launch& L : launches) parts = L.parts > parts ? L.parts : parts;
    const long outs = launches.back().out_hi;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<double> host_out((size_t)outs);
    {
        StreamBuffers buf(st);
        Kde2SlabDev* d_slabs;
        double2 *d_x, *d_g;
        double *d_part, *d_out;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(Kde2SlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double2) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_g, sizeof(double2) * (size_t)(p_hi - p_lo)));
        STAT_TRY(buf.alloc(&d_part, sizeof(double) * (size_t)parts));
        STAT_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_part, sizeof(double) * (size_t)parts, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(double) * (size_t)outs, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(Kde2SlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        if (s_hi > s_lo)
            STAT_TRY(hipMemcpyAsync(d_x, samples + 2 * s_lo, sizeof(double2) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_g, points + 2 * p_lo, sizeof(double2) * (size_t)(p_hi - p_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over; a slab without
        // samples has no item and its sums are the reduce kernel's zeros; both kernels stride over their work)
        for (const Kde2Launch& L : launches) {
            const int count = (int)(L.last - L.first);
            if (L.items) {
                const long grid1 = launch_blocks(L.items, 1l << 20);
                hipLaunchKernelGGL(pw_kde2_partial_kernel, dim3((unsigned)grid1), dim3(KDE_WAVE), 0, st, d_slabs + L.first, count,
                                   L.items, d_x, d_g, d_part);
                STAT_TRY(hipGetLastError());
            }
            const long blocks2 = (L.out_hi - L.out_lo + 255) / 256;
            hipLaunchKernelGGL(pw_kde2_reduce_kernel, dim3((unsigned)launch_blocks(blocks2, 65536)), dim3(256), 0, st,
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
        for (long j = 0; j < (long)jobs[k].n_points; ++j) sums[jobs[k].point_first + j] = host_out[(size_t)at++];
    return PW_OK;
}

}  // namespace

extern "C" int pw_kde_sums(pw_context* ctx, const pw_kde_job* jobs, int64_t n_jobs, const double* samples,
                           const double* points, double* sums) {
    return kde_sums(ctx, jobs, n_jobs, samples, points, sums, nullptr);
}

// measurement hook (not part of the header): pw_kde_sums with the two kernels timed by HIP events
extern "C" int pw_internal_kde_sums_timed(pw_context* ctx, const pw_kde_job* jobs, int64_t n_jobs, const double* samples,
                                          const double* points, double* sums, float* kernel_ms) {
    return kde_sums(ctx, jobs, n_jobs, samples, points, sums, kernel_ms);
}

extern "C" int pw_kde2_sums(pw_context* ctx, const pw_kde2_job* jobs, int64_t n_jobs, const double* samples,
                            const double* points, double* sums) {
    return kde2_sums(ctx, jobs, n_jobs, samples, points, sums, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_kde2_sums with the budget of the partial sums given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_kde2_sums(pw_context* ctx, const pw_kde2_job* jobs, int64_t n_jobs, const double* samples,
                                     const double* points, double* sums, int64_t workspace_bytes, float* kernel_ms) {
    return kde2_sums(ctx, jobs, n_jobs, samples, points, sums, workspace_bytes, kernel_ms);
}

// test hook (not part of the header): on != 0 makes every statistical entry of the library -- the two here and those
// of pw_kdew.hip, pw_corr.hip, pw_dft.hip and pw_gate.hip -- fill its device workspace and its compact device result
// with bytes 0xFF before its first kernel (pw_stat_host.hpp: poison_scratch).  Process-wide, off at start; no kernel and
// no result changes, unless a kernel reads what the call never wrote.
extern "C" void pw_internal_poison_scratch(int on) { g_poison_scratch.store(on != 0, std::memory_order_relaxed); }

// test hook (not part of the header): while blocks > 0, every capped launch of the library -- the kernels whose
// workgroups stride over their work items; pw_stat_host.hpp: launch_blocks -- gets min(items, blocks) workgroups, so
// that a small batch sends every workgroup round its item loop again; 0 gives every launch site its own cap back.
// Process-wide, off at start; no kernel reads it and the host path never does.  Returns how many launches were given
// fewer workgroups than items since the hook was last called, and clears that count.
extern "C" long pw_internal_launch_cap(int blocks) { return launch_cap_hook(blocks); }

// test instrumentation (not part of the header): y[i] = pw_exp(x[i]) on the context's device, or on the host
// for a device == -1 context -- the two must agree to the bit (tests/test_gpu_kde.py)
extern "C" int pw_internal_exp(pw_context* ctx, const double* x, int64_t n, double* y) {
    if (!ctx || n < 0 || (n && (!x || !y))) return PW_E_BAD_ARG;
    if (n == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    if (pw_context_device(ctx) < 0) {
        pw_hostpath_exp(x, (long)n, y);
        return PW_OK;
    }
    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    {
        StreamBuffers buf(st);
        double *d_x, *d_y;
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)n));
        STAT_TRY(buf.alloc(&d_y, sizeof(double) * (size_t)n));
        STAT_TRY(hipMemcpyAsync(d_x, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        const long blocks = ((long)n + 255) / 256;
        hipLaunchKernelGGL(pw_exp_kernel, dim3((unsigned)launch_blocks(blocks, 65536)), dim3(256), 0, st, (long)n, d_x, d_y);
        STAT_TRY(hipGetLastError());
        STAT_TRY(hipMemcpyAsync(y, d_y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    return PW_OK;
}
