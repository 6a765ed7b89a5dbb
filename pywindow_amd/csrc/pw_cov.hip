// pw_cov.hip -- gfx950 kernels and the C ABI entries of the column mean, the scatter matrix and the projections of
// superposed frames (include/pywindow_amd.h: pw_covariance, pw_project; definition of the result in pw_cov.hpp).
//
// The mean takes two small kernels: the column sums of every chunk of a range of chunks (a lane a column, sequential
// in t), then a lane a column adding them in chunk order onto the running total.
//
// pw_cov_partial_kernel is the contraction, shaped as pw_corr_partial_kernel: a workgroup of 256 lanes takes ONE
// COV_TILE x COV_TILE tile of S on or above the diagonal and ONE chunk of rows.  It stages the transformed and centred
// values z of COV_STAGE rows at a time in LDS -- lane `tid` owns one of the tile's 2 x 128 columns for the whole chunk,
// so its mean, its point and its row of the rotation are found once -- and every lane keeps an 8 x 8 square of
// accumulators in registers: per row 8 + 8 operands (eight 16-byte LDS reads) feed 64 FMAs, each accumulator strictly
// in t order.  A lane's columns are the pairs 32 q + 2 l, 32 q + 2 l + 1 (q = 0 .. 3), so that the 16 lanes that differ
// in l read 256 contiguous bytes.  pw_cov_reduce_kernel adds a range of chunk partials in order onto S and writes both
// triangles.  A job's tiles go through in slabs and its chunks in ranges that keep the partials within the workspace;
// a later range continues the sum where the one before left it, so the order of summation is the definition's
// whatever the cut.  Everything is queued on the context's stream, memory included.  No atomics of any kind.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cov.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_covariance(const pw_cov_job* jobs, long n_jobs, const double* data, const double* transforms,
                                      double* mean, double* scatter, int threads);   // pw_hostpath.cpp
extern "C" int pw_hostpath_project(const pw_project_job* jobs, long n_jobs, const double* data, const double* transforms,
                                   const double* mean, const double* vectors, double* proj, int threads);

static_assert(sizeof(pw_superpose_out) == 8 * COV_TRANSFORM_DOUBLES, "a transform row as doubles");
static_assert(sizeof(pw_cov_job) == 48 && sizeof(pw_project_job) == 64, "six and eight int64");
static_assert(COV_CHUNK == PW_COV_CHUNK && COV_MAX_D == PW_COV_MAX_D, "the header's constants");

namespace {

constexpr int COV_LANES = 256;                       // lanes of a workgroup of every kernel here
constexpr int COV_R = 8;                             // a lane's square of accumulators is COV_R x COV_R
constexpr int COV_STAGE = 16;                        // rows staged in LDS at a time
constexpr long COV_TILE_DOUBLES = (long)COV_TILE * COV_TILE;
constexpr int COV_PROJ_WAVES = 4;                    // waves of a workgroup of the projection kernel
constexpr int COV_PROJ_VECTORS = 8;                  // vectors a wave takes in one pass over a row
static_assert(COV_TILE == 16 * COV_R && COV_LANES == 2 * COV_TILE && COV_CHUNK % COV_STAGE == 0, "the lane layout");

// ws[q * D + a]: the sum of column a over chunk c0 + q
__global__ void __launch_bounds__(COV_LANES)
pw_cov_colsum_kernel(const double* __restrict__ x, const double* __restrict__ tr, long T, int D, long c0, long chunks,
                     double* __restrict__ ws) {
    const int blocks = (D + COV_LANES - 1) / COV_LANES;
    for (long item = blockIdx.x; item < chunks * blocks; item += gridDim.x) {
        const long q = item / blocks;
        const int a = (int)(item - q * blocks) * COV_LANES + (int)threadIdx.x;
        if (a >= D) continue;
        const long t0 = (c0 + q) * COV_CHUNK, t1 = t0 + COV_CHUNK < T ? t0 + COV_CHUNK : T;
        double s = 0.0;
#pragma unroll 4
        for (long t = t0; t < t1; ++t) s = s + cov_y(x + t * D, tr ? tr + t * COV_TRANSFORM_DOUBLES : nullptr, a);
        ws[q * D + a] = s;
    }
}

// total[a] takes the chunk sums c0 .. c0 + chunks - 1 in order; after the last range mean = total / T
__global__ void __launch_bounds__(COV_LANES)
pw_cov_mean_kernel(const double* __restrict__ ws, long T, int D, long c0, long chunks, int last, double* __restrict__ total,
                   double* __restrict__ mean) {
    for (long a = (long)blockIdx.x * COV_LANES + threadIdx.x; a < D; a += (long)gridDim.x * COV_LANES) {
        double s = c0 == 0 ? ws[a] : total[a] + ws[a];
#pragma unroll 8
        for (long q = 1; q < chunks; ++q) s = s + ws[q * D + a];
        total[a] = s;
        if (last) mean[a] = s / (double)T;
    }
}

// eight doubles as four 16-byte LDS reads, 32 doubles apart
__device__ inline void cov_read(const double* p, double (&v)[COV_R]) {
#pragma unroll
    for (int q = 0; q < COV_R / 2; ++q) {
        const double2 d = *(const double2*)(p + 32 * q);
        v[2 * q] = d.x; v[2 * q + 1] = d.y;
    }
}

__device__ inline void cov_row(const double* row, int ly, int lx, double (&acc)[COV_R][COV_R]) {
    double a[COV_R], b[COV_R];
    cov_read(row + 2 * ly, a);
    cov_read(row + COV_TILE + 2 * lx, b);
#pragma unroll
    for (int i = 0; i < COV_R; ++i)
#pragma unroll
        for (int j = 0; j < COV_R; ++j) acc[i][j] = pw_fma(a[i], b[j], acc[i][j]);
}

// part[(q * tiles + w) * COV_TILE_DOUBLES + i * COV_TILE + j]: the partial of chunk c0 + q of entry (i, j) of tile
// tile0 + w (row-major over the tiles on or above the diagonal)
__global__ void __launch_bounds__(COV_LANES)
pw_cov_partial_kernel(const double* __restrict__ x, const double* __restrict__ tr, const double* __restrict__ mean, long T,
                      int D, long tile0, long tiles, long c0, long chunks, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double s_z[COV_STAGE][2 * COV_TILE];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int nt = (D + COV_TILE - 1) / COV_TILE;
    for (long item = blockIdx.x; item < chunks * tiles; item += gridDim.x) {
        const long q = item / tiles, w = item - q * tiles;
        int ta, tb;
        cov_tile_of(tile0 + w, nt, ta, tb);
        // the column this lane stages: lanes 0 .. 127 those of the tile's rows, 128 .. 255 those of its columns
        const int g = tid < COV_TILE ? ta * COV_TILE + tid : tb * COV_TILE + tid - COV_TILE;
        const bool live = g < D;
        const double m = live ? mean[g] : 0.0;
        const long t0 = (c0 + q) * COV_CHUNK, t1 = t0 + COV_CHUNK < T ? t0 + COV_CHUNK : T;
        double acc[COV_R][COV_R];
#pragma unroll
        for (int i = 0; i < COV_R; ++i)
#pragma unroll
            for (int j = 0; j < COV_R; ++j) acc[i][j] = 0.0;
        for (long t = t0; t < t1; t += COV_STAGE) {
            const int rows = (int)(t1 - t < COV_STAGE ? t1 - t : COV_STAGE);
            __syncthreads();                                     // (the rows staged before are done with)
            // a column past D is staged as 0.0 only so that LDS is defined: what is computed from it is never stored
#pragma unroll 4
            for (int f = 0; f < rows; ++f)
                s_z[f][tid] = live ? cov_y(x + (t + f) * D, tr ? tr + (t + f) * COV_TRANSFORM_DOUBLES : nullptr, g) - m : 0.0;
            __syncthreads();
#pragma unroll 1
            for (int f = 0; f < rows; ++f) cov_row(s_z[f], ly, lx, acc);   // (rows < COV_STAGE: the short end of the last chunk)
        }
        double* p = part + (q * tiles + w) * COV_TILE_DOUBLES;
#pragma unroll
        for (int i = 0; i < COV_R; ++i) {
            const int ti = 32 * (i >> 1) + 2 * ly + (i & 1);
            if (ta * COV_TILE + ti >= D) continue;
#pragma unroll
            for (int j = 0; j < COV_R; j += 2) {
                const int tj = 32 * (j >> 1) + 2 * lx;
                if (tb * COV_TILE + tj < D) p[ti * COV_TILE + tj] = acc[i][j];
                if (tb * COV_TILE + tj + 1 < D) p[ti * COV_TILE + tj + 1] = acc[i][j + 1];
            }
        }
    }
}

// S takes the partials of the chunks c0 .. c0 + chunks - 1 of the tiles tile0 .. tile0 + tiles - 1 in order, both
// triangles; of a tile on the diagonal only the entries on or above it are used
__global__ void __launch_bounds__(COV_LANES)
pw_cov_reduce_kernel(const double* __restrict__ part, int D, long tile0, long tiles, long c0, long chunks,
                     double* __restrict__ S) {
    const int nt = (D + COV_TILE - 1) / COV_TILE;
    for (long e = (long)blockIdx.x * COV_LANES + threadIdx.x; e < tiles * COV_TILE_DOUBLES; e += (long)gridDim.x * COV_LANES) {
        const long w = e / COV_TILE_DOUBLES, r = e - w * COV_TILE_DOUBLES;
        int ta, tb;
        cov_tile_of(tile0 + w, nt, ta, tb);
        const long ga = (long)ta * COV_TILE + r / COV_TILE, gb = (long)tb * COV_TILE + r % COV_TILE;
        if (ga >= D || gb >= D || ga > gb) continue;
        const double* p = part + e;
        double s = c0 == 0 ? p[0] : S[ga * D + gb] + p[0];
#pragma unroll 8
        for (long q = 1; q < chunks; ++q) s = s + p[q * tiles * COV_TILE_DOUBLES];
        S[ga * D + gb] = s;
        S[gb * D + ga] = s;
    }
}

// acc[l] + acc[l ^ S] in every lane: the fold of pw_superpose.hpp across the lanes of a wave
template <int S>
__device__ inline double cov_partner(double v) {
    if constexpr (S == 32) {
        return __shfl_xor(v, 32, 64);
    } else {
        union { double d; int i[2]; } a, b;
        a.d = v;
        constexpr int pattern = 0x1f | (S << 10);          // bit mode: and 0x1f, or 0, xor S
        b.i[0] = __builtin_amdgcn_ds_swizzle(a.i[0], pattern);
        b.i[1] = __builtin_amdgcn_ds_swizzle(a.i[1], pattern);
        return b.d;
    }
}

__device__ inline double cov_wave_fold(double v) {
    v = v + cov_partner<32>(v);
    v = v + cov_partner<16>(v);
    v = v + cov_partner<8>(v);
    v = v + cov_partner<4>(v);
    v = v + cov_partner<2>(v);
    v = v + cov_partner<1>(v);
    return v;
}

// a wave a row: lane l is accumulator l of every projection of the row
__global__ void __launch_bounds__(64 * COV_PROJ_WAVES)
pw_cov_project_kernel(const double* __restrict__ x, const double* __restrict__ tr, const double* __restrict__ mean,
                      const double* __restrict__ V, long T, int D, int k, double* __restrict__ P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long t = (long)blockIdx.x * COV_PROJ_WAVES + wave; t < T; t += (long)gridDim.x * COV_PROJ_WAVES) {
        const double* xrow = x + t * D;
        const double* trow = tr ? tr + t * COV_TRANSFORM_DOUBLES : nullptr;
        for (int j0 = 0; j0 < k; j0 += COV_PROJ_VECTORS) {
            double acc[COV_PROJ_VECTORS];
#pragma unroll
            for (int r = 0; r < COV_PROJ_VECTORS; ++r) acc[r] = 0.0;
            for (int a = lane; a < D; a += COV_PROJ_ACC) {
                const double z = cov_y(xrow, trow, a) - mean[a];
#pragma unroll
                for (int r = 0; r < COV_PROJ_VECTORS; ++r)
                    if (j0 + r < k) acc[r] = pw_fma(z, V[(long)(j0 + r) * D + a], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < COV_PROJ_VECTORS; ++r) {
                const double s = cov_wave_fold(acc[r]);
                if (lane == 0 && j0 + r < k) P[t * k + j0 + r] = s;
            }
        }
    }
}

// ---- the checks both entries share -----------------------------------------------------------------------------
struct CovSpan {
    long first, last, job;
};

// the first job that shares an output entry with an earlier span, or -1
long cov_shared(std::vector<CovSpan>& spans) {
    std::sort(spans.begin(), spans.end(), [](const CovSpan& a, const CovSpan& b) {
        return a.first != b.first ? a.first < b.first : a.job < b.job;
    });
    long reach = -1, bad = -1;
    for (const CovSpan& s : spans) {
        if (s.first < reach && (bad < 0 || s.job < bad)) bad = s.job;
        reach = s.last > reach ? s.last : reach;
    }
    return bad;
}

inline bool cov_inside(long first, long count, long limit) { return first >= 0 && count >= 0 && first <= limit && count <= limit - first; }

inline bool cov_all_finite(const double* p, long n) {
    for (long i = 0; i < n; ++i)
        if (!pw_finite(p[i])) return false;
    return true;
}

// the input side of a job of either entry; null: fine, otherwise the reason
const char* cov_input_fault(long x_first, long T, long D, long transform_first, const double* data, long n_data,
                            const pw_superpose_out* transforms, long n_transforms) {
    if (T < 1) return "T < 1";
    if (D < 1) return "D < 1";
    if (D > PW_COV_MAX_D) return "D > PW_COV_MAX_D";
    if (transform_first < -1) return "a negative row of the transforms";
    if (transform_first >= 0 && D % 3 != 0) return "D is not a multiple of 3 with transforms";
    if (x_first < 0 || x_first > n_data || T > (n_data - x_first) / D) return "a matrix outside data";
    if (!data) return "null array";
    if (transform_first >= 0 && (!transforms || !cov_inside(transform_first, T, n_transforms))) return "rows outside the transforms";
    if (!cov_all_finite(data + x_first, T * D)) return "a value of the matrix is not finite";
    if (transform_first >= 0)
        for (long t = 0; t < T; ++t) {
            const pw_superpose_out& o = transforms[transform_first + t];
            if (!cov_all_finite(&o.rotation[0][0], 9) || !cov_all_finite(o.centre_mobile, 3) || !cov_all_finite(o.centre_target, 3))
                return "a transform is not finite";
        }
    return nullptr;
}

// the device memory a job's input takes and its upload
struct CovInput {
    double *x = nullptr, *tr = nullptr;
};
hipError_t cov_upload(StreamBuffers& buf, hipStream_t st, const double* data, const pw_superpose_out* transforms, long x_first,
                      long T, long D, long transform_first, CovInput& in) {
    hipError_t e = buf.alloc(&in.x, sizeof(double) * (size_t)(T * D));
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(in.x, data + x_first, sizeof(double) * (size_t)(T * D), hipMemcpyHostToDevice, st);
    if (e != hipSuccess || transform_first < 0) return e;
    e = buf.alloc(&in.tr, sizeof(pw_superpose_out) * (size_t)T);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(in.tr, transforms + transform_first, sizeof(pw_superpose_out) * (size_t)T, hipMemcpyHostToDevice, st);
}

// workspace_bytes: the budget of the chunk sums and the partials of a launch (0: COV_WORKSPACE_BYTES); kernel_ms:
// when not null, the time of all kernels of the call by HIP events on the context's stream
int covariance(pw_context* ctx, const pw_cov_job* jobs, int64_t n_jobs, const double* data, int64_t n_data,
               const pw_superpose_out* transforms, int64_t n_transforms, double* mean, int64_t n_mean, double* scatter,
               int64_t n_scatter, int64_t workspace_bytes, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || n_data < 0 || n_transforms < 0 || n_mean < 0 ||
        n_scatter < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written
    std::vector<CovSpan> means, scatters;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_cov_job& J = jobs[k];
        const char* fault = cov_input_fault((long)J.x_first, (long)J.T, (long)J.D, (long)J.transform_first, data, (long)n_data,
                                            transforms, (long)n_transforms);
        if (fault) return stat_bad("pw_covariance", k, fault);
        if (!mean || !cov_inside((long)J.mean_first, (long)J.D, (long)n_mean)) return stat_bad("pw_covariance", k, "a mean outside the array");
        if (J.s_first < -1 || (J.s_first >= 0 && (!scatter || !cov_inside((long)J.s_first, (long)(J.D * J.D), (long)n_scatter))))
            return stat_bad("pw_covariance", k, "a scatter matrix outside the array");
        means.push_back(CovSpan{(long)J.mean_first, (long)(J.mean_first + J.D), k});
        if (J.s_first >= 0) scatters.push_back(CovSpan{(long)J.s_first, (long)(J.s_first + J.D * J.D), k});
    }
    long shared = cov_shared(means);
    if (shared >= 0) return stat_bad("pw_covariance", shared, "shares entries of the mean with another job");
    shared = cov_shared(scatters);
    if (shared >= 0) return stat_bad("pw_covariance", shared, "shares entries of the scatter matrix with another job");
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_covariance(jobs, (long)n_jobs, data, (const double*)transforms, mean, scatter,
                                      pw_context_host_threads(ctx, 0));

    const long budget = std::max(1l, (long)(workspace_bytes ? workspace_bytes : COV_WORKSPACE_BYTES) / 8);   // doubles
    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_cov_job& J = jobs[k];
        const long T = (long)J.T, D = (long)J.D;
        const long chunks_all = (T + COV_CHUNK - 1) / COV_CHUNK;
        const long nt = (D + COV_TILE - 1) / COV_TILE, tiles_all = J.s_first < 0 ? 0 : nt * (nt + 1) / 2;
        // the cut: chunk sums in ranges of `mean_range` chunks; partials in slabs of `slab` tiles and ranges of
        // `part_range` chunks.  The workspace is the budget, or one chunk's sums or one partial tile where that is more.
        const long mean_range = std::min(chunks_all, std::max(1l, budget / D));
        const long slab = tiles_all ? std::min(tiles_all, std::max(1l, budget / COV_TILE_DOUBLES / chunks_all)) : 0;
        const long part_range = tiles_all ? std::min(chunks_all, std::max(1l, budget / COV_TILE_DOUBLES / slab)) : 0;
        const size_t ws_bytes = sizeof(double) * (size_t)std::max(mean_range * D, slab * part_range * COV_TILE_DOUBLES);
        const size_t s_bytes = sizeof(double) * (size_t)(tiles_all ? D * D : 0);
        float ms = 0.0f;
        Events ev(kernel_ms ? &ms : nullptr);
        STAT_TRY(ev.create());
        {
            StreamBuffers buf(st);
            CovInput in;
            double *d_ws, *d_total, *d_mean, *d_S;
            STAT_TRY(cov_upload(buf, st, data, transforms, (long)J.x_first, T, D, (long)J.transform_first, in));
            STAT_TRY(buf.alloc(&d_ws, ws_bytes));
            STAT_TRY(buf.alloc(&d_total, sizeof(double) * (size_t)D));
            STAT_TRY(buf.alloc(&d_mean, sizeof(double) * (size_t)D));
            STAT_TRY(buf.alloc(&d_S, s_bytes));
            STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
            STAT_TRY(poison_scratch(poison, d_total, sizeof(double) * (size_t)D, st));
            STAT_TRY(poison_scratch(poison, d_mean, sizeof(double) * (size_t)D, st));
            STAT_TRY(poison_scratch(poison, d_S, s_bytes, st));
            STAT_TRY(ev.start(st));
            // (launches follow one another on the stream, so the next one may take the workspace over; every kernel
            // strides over its work -- tests/test_gpu_launch_cap.py sends them round again -- and T, D >= 1 and a range
            // has a chunk and a tile, so no count is zero)
            const long col_blocks = (D + COV_LANES - 1) / COV_LANES;
            for (long c0 = 0; c0 < chunks_all; c0 += mean_range) {
                const long chunks = std::min(mean_range, chunks_all - c0);
                hipLaunchKernelGGL(pw_cov_colsum_kernel, dim3((unsigned)launch_blocks(chunks * col_blocks, 1l << 16)), dim3(COV_LANES), 0, st, in.x, in.tr,
                                   T, (int)D, c0, chunks, d_ws);
                STAT_TRY(hipGetLastError());
                hipLaunchKernelGGL(pw_cov_mean_kernel, dim3((unsigned)launch_blocks(col_blocks, 1l << 16)), dim3(COV_LANES), 0, st, d_ws, T, (int)D, c0,
                                   chunks, c0 + chunks == chunks_all ? 1 : 0, d_total, d_mean);
                STAT_TRY(hipGetLastError());
            }
            for (long tile0 = 0; tile0 < tiles_all; tile0 += slab) {
                const long tiles = std::min(slab, tiles_all - tile0);
                for (long c0 = 0; c0 < chunks_all; c0 += part_range) {
                    const long chunks = std::min(part_range, chunks_all - c0);
                    hipLaunchKernelGGL(pw_cov_partial_kernel, dim3((unsigned)launch_blocks(chunks * tiles, 1l << 16)), dim3(COV_LANES), 0, st, in.x, in.tr,
                                       d_mean, T, (int)D, tile0, tiles, c0, chunks, d_ws);
                    STAT_TRY(hipGetLastError());
                    hipLaunchKernelGGL(pw_cov_reduce_kernel, dim3((unsigned)launch_blocks(tiles * COV_TILE_DOUBLES / COV_LANES, 1l << 16)),
                                       dim3(COV_LANES), 0, st, d_ws, (int)D, tile0, tiles, c0, chunks, d_S);
                    STAT_TRY(hipGetLastError());
                }
            }
            STAT_TRY(ev.stop(st));
            STAT_TRY(hipMemcpyAsync(mean + J.mean_first, d_mean, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, st));
            if (tiles_all) STAT_TRY(hipMemcpyAsync(scatter + J.s_first, d_S, s_bytes, hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(hipStreamSynchronize(st));
        STAT_TRY(ev.read());
        if (kernel_ms) *kernel_ms += ms;
    }
    return PW_OK;
}

int project(pw_context* ctx, const pw_project_job* jobs, int64_t n_jobs, const double* data, int64_t n_data,
            const pw_superpose_out* transforms, int64_t n_transforms, const double* mean, int64_t n_mean,
            const double* vectors, int64_t n_vectors, double* proj, int64_t n_proj, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || n_data < 0 || n_transforms < 0 || n_mean < 0 ||
        n_vectors < 0 || n_proj < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    std::vector<CovSpan> outs;
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_project_job& J = jobs[k];
        const char* fault = cov_input_fault((long)J.x_first, (long)J.T, (long)J.D, (long)J.transform_first, data, (long)n_data,
                                            transforms, (long)n_transforms);
        if (fault) return stat_bad("pw_project", k, fault);
        if (J.k < 1) return stat_bad("pw_project", k, "k < 1");
        if (!mean || !cov_inside((long)J.mean_first, (long)J.D, (long)n_mean)) return stat_bad("pw_project", k, "a mean outside the array");
        if (!vectors || J.v_first < 0 || J.v_first > n_vectors || J.k > (n_vectors - J.v_first) / J.D)
            return stat_bad("pw_project", k, "vectors outside the array");
        if (!proj || J.p_first < 0 || J.p_first > n_proj || J.k > (n_proj - J.p_first) / J.T)
            return stat_bad("pw_project", k, "projections outside the array");
        if (J.k > 0x7fffffff) return stat_bad("pw_project", k, "too large");
        if (!cov_all_finite(mean + J.mean_first, (long)J.D)) return stat_bad("pw_project", k, "a value of the mean is not finite");
        if (!cov_all_finite(vectors + J.v_first, (long)(J.k * J.D))) return stat_bad("pw_project", k, "a value of the vectors is not finite");
        outs.push_back(CovSpan{(long)J.p_first, (long)(J.p_first + J.T * J.k), k});
    }
    const long shared = cov_shared(outs);
    if (shared >= 0) return stat_bad("pw_project", shared, "shares entries of the projections with another job");
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_project(jobs, (long)n_jobs, data, (const double*)transforms, mean, vectors, proj,
                                   pw_context_host_threads(ctx, 0));

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    const bool poison = scratch_poisoned();
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_project_job& J = jobs[k];
        const long T = (long)J.T, D = (long)J.D, K = (long)J.k;
        float ms = 0.0f;
        Events ev(kernel_ms ? &ms : nullptr);
        STAT_TRY(ev.create());
        {
            StreamBuffers buf(st);
            CovInput in;
            double *d_mean, *d_V, *d_P;
            STAT_TRY(cov_upload(buf, st, data, transforms, (long)J.x_first, T, D, (long)J.transform_first, in));
            STAT_TRY(buf.alloc(&d_mean, sizeof(double) * (size_t)D));
            STAT_TRY(buf.alloc(&d_V, sizeof(double) * (size_t)(K * D)));
            STAT_TRY(buf.alloc(&d_P, sizeof(double) * (size_t)(T * K)));
            STAT_TRY(poison_scratch(poison, d_P, sizeof(double) * (size_t)(T * K), st));
            STAT_TRY(hipMemcpyAsync(d_mean, mean + J.mean_first, sizeof(double) * (size_t)D, hipMemcpyHostToDevice, st));
            STAT_TRY(hipMemcpyAsync(d_V, vectors + J.v_first, sizeof(double) * (size_t)(K * D), hipMemcpyHostToDevice, st));
            STAT_TRY(ev.start(st));
            hipLaunchKernelGGL(pw_cov_project_kernel, dim3((unsigned)launch_blocks((T + COV_PROJ_WAVES - 1) / COV_PROJ_WAVES, 1l << 16)),
                               dim3(64 * COV_PROJ_WAVES), 0, st, in.x, in.tr, d_mean, d_V, T, (int)D, (int)K, d_P);
            STAT_TRY(hipGetLastError());
            STAT_TRY(ev.stop(st));
            STAT_TRY(hipMemcpyAsync(proj + J.p_first, d_P, sizeof(double) * (size_t)(T * K), hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(hipStreamSynchronize(st));
        STAT_TRY(ev.read());
        if (kernel_ms) *kernel_ms += ms;
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_covariance(pw_context* ctx, const pw_cov_job* jobs, int64_t n_jobs, const double* data, int64_t n_data,
                             const pw_superpose_out* transforms, int64_t n_transforms, double* mean, int64_t n_mean,
                             double* scatter, int64_t n_scatter) {
    return covariance(ctx, jobs, n_jobs, data, n_data, transforms, n_transforms, mean, n_mean, scatter, n_scatter, 0, nullptr);
}

extern "C" int pw_project(pw_context* ctx, const pw_project_job* jobs, int64_t n_jobs, const double* data, int64_t n_data,
                          const pw_superpose_out* transforms, int64_t n_transforms, const double* mean, int64_t n_mean,
                          const double* vectors, int64_t n_vectors, double* proj, int64_t n_proj) {
    return project(ctx, jobs, n_jobs, data, n_data, transforms, n_transforms, mean, n_mean, vectors, n_vectors, proj, n_proj,
                   nullptr);
}

// measurement and test hooks (not part of the header): pw_covariance with the budget of the workspace given (0: the
// default; the result may not depend on it) and, when kernel_ms is not null, the kernels timed by HIP events;
// pw_project with its kernel timed
extern "C" int pw_internal_covariance(pw_context* ctx, const pw_cov_job* jobs, int64_t n_jobs, const double* data,
                                      int64_t n_data, const pw_superpose_out* transforms, int64_t n_transforms, double* mean,
                                      int64_t n_mean, double* scatter, int64_t n_scatter, int64_t workspace_bytes,
                                      float* kernel_ms) {
    return covariance(ctx, jobs, n_jobs, data, n_data, transforms, n_transforms, mean, n_mean, scatter, n_scatter,
                      workspace_bytes, kernel_ms);
}

extern "C" int pw_internal_project(pw_context* ctx, const pw_project_job* jobs, int64_t n_jobs, const double* data,
                                   int64_t n_data, const pw_superpose_out* transforms, int64_t n_transforms, const double* mean,
                                   int64_t n_mean, const double* vectors, int64_t n_vectors, double* proj, int64_t n_proj,
                                   float* kernel_ms) {
    return project(ctx, jobs, n_jobs, data, n_data, transforms, n_transforms, mean, n_mean, vectors, n_vectors, proj, n_proj,
                   kernel_ms);
}
