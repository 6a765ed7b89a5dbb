// pw_kdew.hip -- gfx950 kernels and the C ABI entry of the Gaussian KDE sums under many weight vectors
// (include/pywindow_amd.h: pw_kde_wsums; definition of the result in pw_kde.hpp).  The plan is pw_kde2_sums':
// the partial sums of every work item -- one wavefront each -- then the sum of the partials in chunk order, the
// partials bounded by a workspace, everything queued on the context's stream, memory included.
//
// A work item is (slab, chunk of samples, tile of KDEW_TILE points, tile of KDEW_REPLICAS replicas).  A lane owns
// KDEW_LANE_POINTS points x KDEW_REPLICAS replicas of accumulators in registers: it computes a term ONCE per
// (sample, point) -- pw_kde_sums' 19 FP64 instructions -- and feeds it to KDEW_REPLICAS fused multiply-adds.  A
// sample's weights are the same for every lane: they are read at a wave-uniform address of read-only memory, which
// the compiler turns into scalar loads (s_load_dwordx*) into SGPRs, so the FMAs take their weight operand from
// a scalar register and neither LDS nor the vector memory path sees them.  The chunk's samples and pw_exp's
// table sit in LDS as in pw_kde_partial_kernel.  The exponential is recomputed once per replica tile (DESIGN.md
// 7b, "Weights and bootstrap bands", says why the terms are not shared through LDS instead).
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_stat_host.hpp"
#include "pw_kde.hpp"

using namespace pw;

extern "C" int pw_hostpath_kdew(const pw_kdew_job* jobs, long n_jobs, const double* samples, const double* points,
                                const double* weights, double* sums, int threads);   // pw_hostpath.cpp

namespace {

constexpr int P = KDEW_LANE_POINTS;
constexpr int RT = KDEW_REPLICAS;
static_assert(RT % KDEW_GROUP == 0, "a cut-short replica tile goes through in whole groups");

// a slab: points [point_first, +m) x replicas [b0, b0 + nb) of one job, all of the job's samples
struct KdewSlabDev {
    long sample_first, n;      // into the uploaded span of samples
    long point_first, m;       // into the uploaded span of points
    long weight_first, stride; // weight of sample 0 under the slab's first replica, in the uploaded span; doubles a sample
    long nb;                   // replicas of the slab
    double r;
    long item_first;           // first work item of the slab in ITS launch
    long part_first;           // the slab's [chunks][nb][m] partial sums in the workspace of its launch
    long out_first;            // the slab's [nb][m] sums in the compact result of the call
    int ptiles, rtiles, chunks;
};

// kdew_chunk_sums for P points x the replicas of a tile side by side: the same operations in the same order for
// every (point, replica).  w: the chunk's first sample's weights from the tile's first replica on (wave-uniform).
// WHOLE: the tile has all RT replicas; otherwise nb < RT of them, taken in groups of KDEW_GROUP (a group's surplus
// replicas read the tile's last weight -- nothing outside the array -- and their sums are never stored).
template <bool WHOLE>
__device__ inline void kdew_tile_chunk(const double* s_x, const uint64_t* s_tab, const double* __restrict__ w, long stride,
                                       int len, int nb, double r, const double (&g)[P], double (&acc)[P][RT]) {
    for (int i = 0; i < len; ++i, w += stride) {
        const double x = s_x[i];
        double e[P];
#pragma unroll
        for (int p = 0; p < P; ++p) e[p] = kde_term(g[p], x, r, s_tab);
        if (WHOLE) {
#pragma unroll
            for (int b = 0; b < RT; ++b) {
                const double wv = w[b];
#pragma unroll
                for (int p = 0; p < P; ++p) acc[p][b] = pw_fma(wv, e[p], acc[p][b]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < RT; q += KDEW_GROUP) {
                if (q < nb) {
#pragma unroll
                    for (int u = 0; u < KDEW_GROUP; ++u) {
                        const double wv = w[q + u < nb ? q + u : nb - 1];
#pragma unroll
                        for (int p = 0; p < P; ++p) acc[p][q + u] = pw_fma(wv, e[p], acc[p][q + u]);
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(KDE_WAVE)
pw_kdew_partial_kernel(const KdewSlabDev* __restrict__ slabs, int n_slabs, long total, const double* __restrict__ samples,
                       const double* __restrict__ points, const double* __restrict__ weights, double* __restrict__ part) {
    __shared__ double s_x[KDE_CHUNK];
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const int lane = threadIdx.x;
    for (int t = lane; t < 256; t += KDE_WAVE) s_tab[t] = POW_EXP_TAB[t];
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = stat_find(n_slabs, item, [&](int q) { return slabs[q].item_first; });
        const KdewSlabDev job = slabs[k];
        const long local = item - job.item_first;
        const long per_chunk = (long)job.ptiles * job.rtiles;
        const long chunk = local / per_chunk;
        const long rest = local - chunk * per_chunk;
        const long rtile = rest / job.ptiles;
        const long ptile = rest - rtile * job.ptiles;
        const long i0 = chunk * KDE_CHUNK;
        const int len = (int)(job.n - i0 < KDE_CHUNK ? job.n - i0 : KDE_CHUNK);
        const long b0 = rtile * RT;
        const int nb = (int)(job.nb - b0 < RT ? job.nb - b0 : RT);
        __syncthreads();                                   // (the previous item's samples are done with)
        for (int t = lane; t < len; t += KDE_WAVE) s_x[t] = samples[job.sample_first + i0 + t];
        __syncthreads();
        double g[P], acc[P][RT];
        long j[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            j[p] = ptile * KDEW_TILE + p * KDE_WAVE + lane;
            g[p] = j[p] < job.m ? points[job.point_first + j[p]] : 0.0;
#pragma unroll
            for (int b = 0; b < RT; ++b) acc[p][b] = 0.0;
        }
        const double* w = weights + job.weight_first + i0 * job.stride + b0;
        if (nb == RT)
            kdew_tile_chunk<true>(s_x, s_tab, w, job.stride, len, nb, job.r, g, acc);
        else
            kdew_tile_chunk<false>(s_x, s_tab, w, job.stride, len, nb, job.r, g, acc);
        double* out = part + job.part_first + (chunk * job.nb + b0) * job.m;
#pragma unroll
        for (int b = 0; b < RT; ++b) {
            if (b < nb) {
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (j[p] < job.m) out[(long)b * job.m + j[p]] = acc[p][b];
            }
        }
    }
}

// the sums of the slabs of one launch: out[out_lo + t], t < count
__global__ void __launch_bounds__(256)
pw_kdew_reduce_kernel(const KdewSlabDev* __restrict__ slabs, int n_slabs, long out_lo, long count,
                      const double* __restrict__ part, double* __restrict__ out) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x) {
        const int k = stat_find(n_slabs, t, [&](int q) { return slabs[q].out_first - out_lo; });
        const long at = out_lo + t - slabs[k].out_first;         // b * m + j within the slab
        const long pitch = slabs[k].nb * slabs[k].m;             // from one chunk's partials to the next
        const double* p = part + slabs[k].part_first + at;
        double s = 0.0;
        for (int c = 0; c < slabs[k].chunks; ++c) s = c == 0 ? p[0] : s + p[(long)c * pitch];
        out[out_lo + t] = s;
    }
}

// slabs [first, last) share one launch pair and one workspace of `parts` doubles
struct KdewLaunch {
    long first, last, items, parts, out_lo, out_hi;
};

// where a slab's sums go in the caller's array: job, first point, first replica
struct KdewPlace {
    long job, p0, b0;
};

constexpr long KDEW_LIMIT = 1l << 40;      // samples, points, replicas and points x replicas of a job

// The plan of a call.  A job's [chunks][R][m] partial sums may not fit the budget (400 000 x 1000 x 64: 400 MB),
// so the job is cut into slabs whose partials do: whole replica tiles over all points while a tile of replicas
// fits, whole point tiles of one replica tile otherwise; slabs are gathered into launches while they fit.  The
// workspace of a call is the largest launch's: at most `budget` doubles, or one (point tile, replica tile)'s
// partials of the longest job where that alone is more.  Nothing of the result depends on the cut: the sum of a
// (replica, point) is its own.
void kdew_plan(const pw_kdew_job* jobs, long n_jobs, long s_lo, long p_lo, long w_lo, long budget,
               std::vector<KdewSlabDev>& slabs, std::vector<KdewPlace>& places, std::vector<KdewLaunch>& launches) {
    long outs = 0;
    KdewLaunch cur{0, 0, 0, 0, 0, 0};
    for (long k = 0; k < n_jobs; ++k) {
        const pw_kdew_job& J = jobs[k];
        const long n = (long)J.n_samples, m = (long)J.n_points, R = (long)J.n_replicas;
        if (m == 0) continue;
        const long chunks = (n + KDE_CHUNK - 1) / KDE_CHUNK;
        long pm = m, br = R;
        if (chunks && chunks > budget / m / R) {
            br = budget / chunks / m / RT * RT;
            if (br < RT) {
                br = RT;
                pm = budget / chunks / RT / KDEW_TILE * KDEW_TILE;
                if (pm < KDEW_TILE) pm = KDEW_TILE;
            }
        }
        for (long b0 = 0; b0 < R; b0 += br) {
            for (long p0 = 0; p0 < m; p0 += pm) {
                KdewSlabDev D{};
                D.n = n; D.m = m - p0 < pm ? m - p0 : pm; D.nb = R - b0 < br ? R - b0 : br;
                D.sample_first = n ? (long)J.sample_first - s_lo : 0;
                D.point_first = (long)J.point_first - p_lo + p0;
                D.weight_first = n ? (long)J.weight_first - w_lo + b0 : 0;
                D.stride = R;
                D.r = J.inv_bandwidth;
                D.ptiles = (int)((D.m + KDEW_TILE - 1) / KDEW_TILE); D.rtiles = (int)((D.nb + RT - 1) / RT);
                D.chunks = (int)chunks;
                const long parts = chunks * D.nb * D.m;
                if (cur.last > cur.first && cur.parts + parts > budget) {
                    launches.push_back(cur);
                    cur = KdewLaunch{cur.last, cur.last, 0, 0, outs, outs};
                }
                D.item_first = cur.items; D.part_first = cur.parts; D.out_first = outs;
                cur.items += (long)D.ptiles * D.rtiles * chunks; cur.parts += parts;
                outs += D.nb * D.m;
                cur.last += 1; cur.out_hi = outs;
                slabs.push_back(D);
                places.push_back(KdewPlace{k, p0, b0});
            }
        }
    }
    if (cur.last > cur.first) launches.push_back(cur);
}

// workspace_bytes: the budget of the partial sums (0: KDEW_WORKSPACE_BYTES); kernel_ms: when not null, the time
// of all kernels of the call by HIP events on the context's stream
int kdew_sums(pw_context* ctx, const pw_kdew_job* jobs, int64_t n_jobs, const double* samples, const double* points,
              const double* weights, double* sums, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || workspace_bytes < 0) return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    long s_lo = -1, s_hi = 0, p_lo = -1, p_hi = 0, w_lo = -1, w_hi = 0;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_kdew_job& J = jobs[k];
        if (J.n_samples < 0 || J.n_points < 0 || J.sample_first < 0 || J.point_first < 0 || J.weight_first < 0 || J.out_first < 0)
            return stat_bad("pw_kde_wsums", k, "negative range");
        if (J.n_replicas < 1) return stat_bad("pw_kde_wsums", k, "no replica (n_replicas < 1)");
        if (J.n_samples > KDEW_LIMIT || J.n_points > KDEW_LIMIT || J.n_replicas > KDEW_LIMIT ||
            (J.n_points && J.n_replicas > KDEW_LIMIT / J.n_points) || (J.n_samples && J.n_replicas > KDEW_LIMIT / J.n_samples))
            return stat_bad("pw_kde_wsums", k, "too large");
        if ((J.n_samples && (!samples || !weights)) || (J.n_points && (!points || !sums)))
            return stat_bad("pw_kde_wsums", k, "null array");
        if (!pw_finite(J.inv_bandwidth) || !(J.inv_bandwidth > 0.0))
            return stat_bad("pw_kde_wsums", k, "bandwidth not positive and finite");
        for (long i = 0; i < (long)J.n_samples; ++i)
            if (!pw_finite(samples[J.sample_first + i])) return stat_bad("pw_kde_wsums", k, "a sample is NaN or infinite");
        for (long i = 0; i < (long)J.n_points; ++i)
            if (!pw_finite(points[J.point_first + i])) return stat_bad("pw_kde_wsums", k, "a point is NaN or infinite");
        for (long i = 0; i < (long)(J.n_samples * J.n_replicas); ++i) {
            const double w = weights[J.weight_first + i];
            if (!pw_finite(w) || !(w >= 0.0)) return stat_bad("pw_kde_wsums", k, "a weight is negative, NaN or infinite");
        }
        if (J.n_points == 0) continue;
        if (J.n_samples) {
            const long wn = (long)(J.n_samples * J.n_replicas);
            if (s_lo < 0 || J.sample_first < s_lo) s_lo = (long)J.sample_first;
            if (J.sample_first + J.n_samples > s_hi) s_hi = (long)(J.sample_first + J.n_samples);
            if (w_lo < 0 || J.weight_first < w_lo) w_lo = (long)J.weight_first;
            if (J.weight_first + wn > w_hi) w_hi = (long)J.weight_first + wn;
        }
        if (p_lo < 0 || J.point_first < p_lo) p_lo = (long)J.point_first;
        if (J.point_first + J.n_points > p_hi) p_hi = (long)(J.point_first + J.n_points);
    }
    if (p_lo < 0) return PW_OK;                                  // no job has a point
    if (s_lo < 0) s_lo = s_hi = w_lo = w_hi = 0;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_kdew(jobs, (long)n_jobs, samples, points, weights, sums, pw_context_host_threads(ctx, 0));

    std::vector<KdewSlabDev> slabs;
    std::vector<KdewPlace> places;
    std::vector<KdewLaunch> launches;
    kdew_plan(jobs, (long)n_jobs, s_lo, p_lo, w_lo, (long)(workspace_bytes ? workspace_bytes : KDEW_WORKSPACE_BYTES) / 8, slabs,
              places, launches);
    if (slabs.size() > 0x7ffffff0) return stat_bad("pw_kde_wsums", (long)n_jobs - 1, "too large");
    long parts = 0;
    for (const KdewLaunch& L : launches) parts = L.parts > parts ? L.parts : parts;
    const long outs = launches.back().out_hi;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<double> host_out((size_t)outs);
    {
        StreamBuffers buf(st);
        KdewSlabDev* d_slabs;
        double *d_x, *d_g, *d_w, *d_part, *d_out;
        STAT_TRY(buf.alloc(&d_slabs, sizeof(KdewSlabDev) * slabs.size()));
        STAT_TRY(buf.alloc(&d_x, sizeof(double) * (size_t)(s_hi - s_lo)));
        STAT_TRY(buf.alloc(&d_g, sizeof(double) * (size_t)(p_hi - p_lo)));
        STAT_TRY(buf.alloc(&d_w, sizeof(double) * (size_t)(w_hi - w_lo)));
        STAT_TRY(buf.alloc(&d_part, sizeof(double) * (size_t)parts));
        STAT_TRY(buf.alloc(&d_out, sizeof(double) * (size_t)outs));
        const bool poison = scratch_poisoned();                  // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_part, sizeof(double) * (size_t)parts, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(double) * (size_t)outs, st));
        STAT_TRY(hipMemcpyAsync(d_slabs, slabs.data(), sizeof(KdewSlabDev) * slabs.size(), hipMemcpyHostToDevice, st));
        if (s_hi > s_lo) {
            STAT_TRY(hipMemcpyAsync(d_x, samples + s_lo, sizeof(double) * (size_t)(s_hi - s_lo), hipMemcpyHostToDevice, st));
            STAT_TRY(hipMemcpyAsync(d_w, weights + w_lo, sizeof(double) * (size_t)(w_hi - w_lo), hipMemcpyHostToDevice, st));
        }
        STAT_TRY(hipMemcpyAsync(d_g, points + p_lo, sizeof(double) * (size_t)(p_hi - p_lo), hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over; a slab without
        // samples has no item and its sums are the reduce kernel's zeros; both kernels stride over their work)
        for (const KdewLaunch& L : launches) {
            const int count = (int)(L.last - L.first);
            if (L.items) {
                const long grid1 = launch_blocks(L.items, 1l << 20);
                hipLaunchKernelGGL(pw_kdew_partial_kernel, dim3((unsigned)grid1), dim3(KDE_WAVE), 0, st, d_slabs + L.first, count,
                                   L.items, d_x, d_g, d_w, d_part);
                STAT_TRY(hipGetLastError());
            }
            const long blocks2 = (L.out_hi - L.out_lo + 255) / 256;
            hipLaunchKernelGGL(pw_kdew_reduce_kernel, dim3((unsigned)launch_blocks(blocks2, 65536)), dim3(256), 0, st,
                               d_slabs + L.first, count, L.out_lo, L.out_hi - L.out_lo, d_part, d_out);
            STAT_TRY(hipGetLastError());
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(host_out.data(), d_out, sizeof(double) * (size_t)outs, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    for (size_t q = 0; q < slabs.size(); ++q) {                   // a slab's [nb][m] block into the job's [R][n_points]
        const KdewSlabDev& D = slabs[q];
        const pw_kdew_job& J = jobs[places[q].job];
        for (long b = 0; b < D.nb; ++b) {
            const double* src = host_out.data() + D.out_first + b * D.m;
            double* dst = sums + J.out_first + (places[q].b0 + b) * (long)J.n_points + places[q].p0;
            for (long j = 0; j < D.m; ++j) dst[j] = src[j];
        }
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_kde_wsums(pw_context* ctx, const pw_kdew_job* jobs, int64_t n_jobs, const double* samples,
                            const double* points, const double* weights, double* sums) {
    return kdew_sums(ctx, jobs, n_jobs, samples, points, weights, sums, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_kde_wsums with the budget of the partial sums given
// (0: the default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events
extern "C" int pw_internal_kde_wsums(pw_context* ctx, const pw_kdew_job* jobs, int64_t n_jobs, const double* samples,
                                     const double* points, const double* weights, double* sums, int64_t workspace_bytes,
                                     float* kernel_ms) {
    return kdew_sums(ctx, jobs, n_jobs, samples, points, weights, sums, workspace_bytes, kernel_ms);
}
