// pw_kde.hip -- gfx950 kernels and the C ABI entry of the Gaussian KDE sums (include/pywindow_amd.h:
// pw_kde_sums; definition of the result in pw_kde.hpp).  Two kernels per call: the partial sums of
// every (job, chunk of samples, tile of grid points) -- one wavefront each, a lane owning
// KDE_LANE_POINTS grid points in registers, the chunk's samples staged in LDS and read at one address
// per wave (a broadcast), pw_exp's 2 KB table in LDS as well -- then the sum of the partials in chunk
// order.  Everything is queued on the context's stream, memory included (stream-ordered allocation:
// nothing here waits for other work of the device).
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_host.hpp"
#include "pw_kde.hpp"

using namespace pw;

extern "C" char* pw_internal_error_buffer(void);   // pw_kernels.hip
extern "C" int pw_context_device(pw_context* ctx);
extern "C" int pw_hostpath_kde(const pw_kde_job* jobs, long n_jobs, const double* samples, const double* points,
                               double* sums, int threads);   // pw_hostpath.cpp
extern "C" void pw_hostpath_exp(const double* x, long n, double* y);

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

// the last entry k with key(k) <= v; keys ascending, key(0) == 0 <= v < key(n)
template <class Key>
__device__ inline int kde_find(int n, long v, Key key) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(KDE_WAVE)
pw_kde_partial_kernel(const KdeJobDev* __restrict__ jobs, int n_jobs, const double* __restrict__ samples,
                      const double* __restrict__ points, double* __restrict__ part) {
    __shared__ double s_x[KDE_CHUNK];
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += KDE_WAVE) s_tab[t] = POW_EXP_TAB[t];
    const long total = jobs[n_jobs].item_first;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = kde_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
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
        const int k = kde_find(n_jobs, t, [&](int q) { return jobs[q].out_first; });
        const long m = jobs[k].m, j = t - jobs[k].out_first;
        const double* p = part + jobs[k].part_first + j;
        double s = 0.0;
        for (int c = 0; c < jobs[k].chunks; ++c) s = c == 0 ? p[0] : s + p[(long)c * m];
        out[t] = s;
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

// device memory of one call, allocated and released in stream order
struct StreamBuffers {
    static constexpr int CAP = 8;
    hipStream_t st;
    void* p[CAP];
    int n = 0;
    explicit StreamBuffers(hipStream_t s) : st(s) {}
    ~StreamBuffers() { for (int i = 0; i < n; ++i) if (p[i]) (void)hipFreeAsync(p[i], st); }
    template <class X> hipError_t alloc(X** out, size_t bytes) {
        if (n >= CAP) return hipErrorOutOfMemory;
        hipError_t e = hipMallocAsync((void**)out, bytes ? bytes : 8, st);
        if (e == hipSuccess) p[n++] = *out;
        return e;
    }
};

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

#define KDE_TRY(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            snprintf(pw_internal_error_buffer(), 512, "%s: %s", #call, hipGetErrorString(e_)); \
            return PW_E_HIP;                                                               \
        }                                                                                  \
    } while (0)

int kde_bad(const char* what, long k) {
    snprintf(pw_internal_error_buffer(), 512, "pw_kde_sums: job %ld: %s", k, what);
    return PW_E_BAD_ARG;
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
        if (J.n_samples < 0 || J.n_points < 0 || J.sample_first < 0 || J.point_first < 0) return kde_bad("negative range", k);
        if ((J.n_samples && !samples) || (J.n_points && (!points || !sums))) return kde_bad("null array", k);
        if (!kde_finite(J.inv_bandwidth) || !(J.inv_bandwidth > 0.0)) return kde_bad("bandwidth not positive and finite", k);
        for (long i = 0; i < (long)J.n_samples; ++i)
            if (!kde_finite(samples[J.sample_first + i])) return kde_bad("a sample is NaN or infinite", k);
        for (long i = 0; i < (long)J.n_points; ++i)
            if (!kde_finite(points[J.point_first + i])) return kde_bad("a point is NaN or infinite", k);
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
        if (tiles > 0x7fffffff || chunks > 0x7fffffff) return kde_bad("too large", k);
        D.tiles = (int)tiles; D.chunks = (int)chunks;
        D.item_first = items; D.part_first = parts; D.out_first = outs;
        items += tiles * chunks; parts += chunks * D.m; outs += D.m;
    }
    KdeJobDev& E = dev[n_jobs];
    E = KdeJobDev{};
    E.item_first = items; E.part_first = parts; E.out_first = outs;

    DeviceScope dev_scope_;
    KDE_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev;
    if (kernel_ms) {
        KDE_TRY(hipEventCreate(&ev.a));
        KDE_TRY(hipEventCreate(&ev.b));
    }
    std::vector<double> host_out((size_t)outs);
    {
        StreamBuffers buf(st);
        KdeJobDev* d_jobs;
        double *d_x, *d_g, *d_part, *d_out;
        KDE_TRY(buf.alloc(&d_jobs, sizeof(KdeJobDev) * dev.size()));
        KDE_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        KDE_TRY(buf.alloc(&d_g, sizeof(double) * (size_t)(p_hi - p_lo)));
        KDE_TRY(buf.alloc(&d_part, sizeof(double) * (size_t)parts));
        KDE_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs));
        KDE_TRY(hipMemcpyAsync(d_jobs, dev.data(), sizeof(KdeJobDev) * dev.size(), hipMemcpyHostToDevice, st));
        if (s_hi > s_lo)
            KDE_TRY(hipMemcpyAsync(d_x, samples + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
        KDE_TRY(hipMemcpyAsync(d_g, points + p_lo, sizeof(double) * (size_t)(p_hi - p_lo), hipMemcpyHostToDevice, st));
        if (kernel_ms) KDE_TRY(hipEventRecord(ev.a, st));
        // (a job without samples has no pair and its sums are the reduce kernel's zeros; the launch geometry is
        // free: both kernels stride over their work)
        const long grid1 = items < 1 ? 1 : (items < (1l << 20) ? items : (1l << 20));
        hipLaunchKernelGGL(pw_kde_partial_kernel, dim3((unsigned)grid1), dim3(KDE_WAVE), 0, st, d_jobs, (int)n_jobs, d_x, d_g,
                           d_part);
        KDE_TRY(hipGetLastError());
        const long blocks2 = (outs + 255) / 256;
        hipLaunchKernelGGL(pw_kde_reduce_kernel, dim3((unsigned)(blocks2 < 65536 ? blocks2 : 65536)), dim3(256), 0, st, d_jobs,
                           (int)n_jobs, d_part, d_out);
        KDE_TRY(hipGetLastError());
        if (kernel_ms) KDE_TRY(hipEventRecord(ev.b, st));
        KDE_TRY(hipMemcpyAsync(host_out.data(), d_out, sizeof(double) * (size_t)outs, hipMemcpyDeviceToHost, st));
    }
    KDE_TRY(hipStreamSynchronize(st));
    if (kernel_ms) KDE_TRY(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
    for (long k = 0; k < (long)n_jobs; ++k)
        for (long j = 0; j < dev[k].m; ++j) sums[jobs[k].point_first + j] = host_out[(size_t)(dev[k].out_first + j)];
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
    KDE_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    {
        StreamBuffers buf(st);
        double *d_x, *d_y;
        KDE_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)n));
        KDE_TRY(buf.alloc(&d_y, sizeof(double) * (size_t)n));
        KDE_TRY(hipMemcpyAsync(d_x, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
        const long blocks = ((long)n + 255) / 256;
        hipLaunchKernelGGL(pw_exp_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, (long)n, d_x, d_y);
        KDE_TRY(hipGetLastError());
        KDE_TRY(hipMemcpyAsync(y, d_y, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    KDE_TRY(hipStreamSynchronize(st));
    return PW_OK;
}
