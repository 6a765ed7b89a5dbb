// pw_cluster.hip -- gfx950 kernels and the C ABI entry of the gromos clustering of frames (include/pywindow_amd.h:
// pw_cluster_gromos; definition of the result and the layout of the bit matrix in pw_cluster.hpp).
//
// pw_cluster_pack_kernel thresholds the matrix once.  The matrix comes to the device in slabs of whole rows; a wave
// takes 64 consecutive columns of a row, reads the distance only where row < col < n and one ballot gives the word of
// the bit matrix.  Every job of the launch group that shares the matrix is packed from the same slab (blockIdx.y).
// pw_cluster_mirror_kernel fills the lower triangle from the BITS -- its rows may have been in another slab --: a wave
// takes the 64 x 64 tile (I, J), I <= J, lane l holding the word of row 64 I + l; 64 ballots, lane c keeping ballot c,
// are the transposed tile, stored as tile (J, I); a diagonal tile is OR-ed with its own transpose.
// pw_cluster_count_kernel, the hot path: a wave takes an active row, its lanes stride over the row in 16-byte loads,
// AND it with the active words and count the bits; the wave's sum makes the key of pw_cluster.hpp, the keys are reduced
// over the workgroup in LDS and ONE 64-bit integer atomicMax a workgroup goes to the job's slot.
// pw_cluster_pick_kernel, a workgroup a job: a key of 0 means that no frame is active and sets the job's done flag;
// otherwise it decodes the centre, writes centre and size, labels the set bits of bits[c] & active, clears them from
// active, bumps the number of clusters and zeroes the slot.
// Count and pick alternate as ordered launches on the context's stream, `rounds_per_check` pairs queued without a host
// synchronisation, both returning at once for a job that is done; then one small copy brings the done flags back.  No
// workgroup waits for another inside a kernel: stream order is the only synchronisation.  Memory is allocated and
// released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cluster.hpp"
#include "pw_stat_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_cluster(const pw_cluster_job* jobs, long n_jobs, const double* dist, int* labels, int* centres,
                                   int* sizes, long* n_clusters, int threads);   // pw_hostpath.cpp

static_assert(PW_CLUSTER_MAX_N == CLUSTER_MAX_N, "the header's bound and the kernels'");

namespace {

typedef cluster_word u64;

// one job with frames; the jobs of a launch group lie one after the other
struct ClusterJobDev {
    long n, S;                 // frames; words of a row of the bit matrix (even)
    long bits_first;           // first word of the job's bit matrix in the workspace of its launch group
    long active_first;         // first of the job's S active words (an even number: 16-byte loads)
    long out_first;            // the job's n entries in the compact labels / centres / sizes of the call
    long slot;                 // the job's key, cluster count and done flag
    long matrix;               // which of the call's distinct matrices the job reads
    double cutoff;
};

// active = every frame, no cluster yet, centres -1 and sizes 0; a workgroup a job
__global__ void __launch_bounds__(256)
pw_cluster_init_kernel(const ClusterJobDev* __restrict__ jobs, u64* __restrict__ active, u64* __restrict__ keys,
                       long* __restrict__ ncl, int* __restrict__ done, int* __restrict__ centres, int* __restrict__ sizes) {
    const ClusterJobDev D = jobs[blockIdx.x];
    for (long w = threadIdx.x; w < D.S; w += blockDim.x) active[D.active_first + w] = cluster_tail_mask(D.n, w);
    for (long j = threadIdx.x; j < D.n; j += blockDim.x) {
        centres[D.out_first + j] = -1;
        sizes[D.out_first + j] = 0;
    }
    if (threadIdx.x == 0) {
        keys[D.slot] = 0;
        ncl[D.slot] = 0;
        done[D.slot] = 0;
    }
}

// rows [r0, r0 + rows) of matrix `matrix`, row-major in `slab`; all S words of those rows are written (the words under
// the diagonal as zeros: the mirror kernel stores over them)
__global__ void __launch_bounds__(256)
pw_cluster_pack_kernel(const ClusterJobDev* __restrict__ jobs, long matrix, const double* __restrict__ slab, long r0,
                       long rows, u64* __restrict__ ws) {
    const ClusterJobDev D = jobs[blockIdx.y];
    if (D.matrix != matrix) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* B = ws + D.bits_first;
    const long total = rows * D.S;
    for (long it = (long)blockIdx.x * 4 + wave; it < total; it += (long)gridDim.x * 4) {
        const long lr = it / D.S, w = it % D.S;
        const long row = r0 + lr, col = 64 * w + lane;
        double d = 0.0;
        if (col > row && col < D.n) d = slab[lr * D.n + col];
        const u64 word = __ballot(cluster_pack_bit(row, col, D.n, d, D.cutoff));
        if (lane == 0) B[row * D.S + w] = word;
    }
}

__global__ void __launch_bounds__(256)
pw_cluster_mirror_kernel(const ClusterJobDev* __restrict__ jobs, u64* __restrict__ ws) {
    const ClusterJobDev D = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long T = cluster_words(D.n);
    u64* B = ws + D.bits_first;
    for (long it = (long)blockIdx.x * 4 + wave; it < T * T; it += (long)gridDim.x * 4) {
        const long I = it / T, J = it % T;
        if (I > J) continue;                                         // (the whole wave: I and J are the wave's)
        const long row = 64 * I + lane;
        const u64 word = row < D.n ? B[row * D.S + J] : 0;
        u64 mine = 0;
#pragma unroll
        for (int c = 0; c < 64; ++c) {
            const u64 b = __ballot((word >> c) & 1);
            mine = lane == c ? b : mine;
        }
        const long orow = 64 * J + lane;                             // (I == J: orow == row, `word` is this row's)
        if (orow < D.n) B[orow * D.S + I] = I == J ? (word | mine) : mine;
    }
}

__global__ void __launch_bounds__(256)
pw_cluster_count_kernel(const ClusterJobDev* __restrict__ jobs, const u64* __restrict__ ws, const u64* __restrict__ active,
                        u64* __restrict__ keys, const int* __restrict__ done) {
    __shared__ u64 s_key[4];
    const ClusterJobDev D = jobs[blockIdx.y];
    if (done[D.slot]) return;                                        // (the whole workgroup)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* A = active + D.active_first;
    const ulonglong2* A2 = (const ulonglong2*)A;
    const int pairs = (int)(D.S / 2);
    u64 best = 0;
    for (long i = (long)blockIdx.x * 4 + wave; i < D.n; i += (long)gridDim.x * 4) {
        if (!((A[i >> 6] >> (i & 63)) & 1)) continue;                // (the whole wave: i is the wave's)
        const ulonglong2* R2 = (const ulonglong2*)(ws + D.bits_first + i * D.S);
        int count = 0;
        for (int p = lane; p < pairs; p += 64) {
            const ulonglong2 x = R2[p], y = A2[p];
            count += cluster_popcount(x.x & y.x) + cluster_popcount(x.y & y.y);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) count += __shfl_xor(count, o);
        const u64 key = cluster_key((unsigned)count, (unsigned)i);
        best = key > best ? key : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) best = s_key[k] > best ? s_key[k] : best;
        if (best) atomicMax(keys + D.slot, best);
    }
}

__global__ void __launch_bounds__(256)
pw_cluster_pick_kernel(const ClusterJobDev* __restrict__ jobs, const u64* __restrict__ ws, u64* __restrict__ active,
                       u64* __restrict__ keys, long* __restrict__ ncl, int* __restrict__ done, int* __restrict__ labels,
                       int* __restrict__ centres, int* __restrict__ sizes) {
    const ClusterJobDev D = jobs[blockIdx.x];
    if (done[D.slot]) return;                                        // (the whole workgroup)
    const u64 key = keys[D.slot];
    const long k = ncl[D.slot];
    __syncthreads();                                                 // (every thread has read the key and the count)
    const long c = (long)cluster_key_row(key);
    if (key == 0 || k >= D.n || c >= D.n) {                          // no frame is active (the other two cannot be)
        if (threadIdx.x == 0) done[D.slot] = 1;
        return;
    }
    if (threadIdx.x == 0) {
        keys[D.slot] = 0;
        ncl[D.slot] = k + 1;
        centres[D.out_first + k] = (int)c;
        sizes[D.out_first + k] = (int)cluster_key_count(key);
    }
    u64* A = active + D.active_first;
    const u64* R = ws + D.bits_first + c * D.S;
    const long W = cluster_words(D.n);
    for (long w = threadIdx.x; w < W; w += blockDim.x) {
        const u64 a = A[w];
        u64 m = R[w] & a;                                            // (bits at columns >= n are in neither)
        if (!m) continue;
        A[w] = a & ~m;
        while (m) {
            const int b = __ffsll((long long)m) - 1;
            labels[D.out_first + 64 * w + b] = (int)k;
            m &= m - 1;
        }
    }
}

struct ClusterMatrix {
    long d_first, n;
};

// jobs [first, last) of the live jobs share the launches of their rounds and one workspace of `words` words
struct ClusterGroup {
    long first, last, words, n_max;
};

// entries [dev, dev + count) of the compact result are entries [host, host + count) of the caller's arrays
struct ClusterCopy {
    long host, dev, count;
};

// workspace_bytes: the budget of a slab of the matrix, and a quarter of the budget of the bit matrices of a launch
// group (0: CLUSTER_SLAB_BYTES and CLUSTER_BITS_BYTES; at 1 every slab is one row and every job a group of its own);
// rounds_per_check: count + pick pairs between two looks at the done flags (0: CLUSTER_ROUNDS); kernel_ms: when not
// null, the time of the device work of the call from the first initialisation to the last pick, the uploads of the
// slabs and the copies of the flags included, by HIP events on the context's stream
int cluster_gromos(pw_context* ctx, const pw_cluster_job* jobs, int64_t n_jobs, const double* dist, int64_t n_dist,
                   int32_t* labels, int32_t* centres, int32_t* sizes, int64_t* n_clusters, int64_t workspace_bytes,
                   int64_t rounds_per_check, float* kernel_ms) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !n_clusters)) || n_dist < 0 || workspace_bytes < 0 ||
        rounds_per_check < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    // everything is checked before anything is launched or written; a matrix that several jobs share is read once
    std::vector<ClusterMatrix> mats;
    std::vector<long> mat_of((size_t)n_jobs, -1);
    for (long k = 0; k < (long)n_jobs; ++k) {
        const pw_cluster_job& J = jobs[k];
        if (J.d_first < 0 || J.n < 0 || J.out_first < 0) return stat_bad("pw_cluster_gromos", k, "negative field");
        if (J.n > CLUSTER_MAX_N) return stat_bad("pw_cluster_gromos", k, "n above PW_CLUSTER_MAX_N (32768)");
        if (pw_isnan_bits(J.cutoff)) return stat_bad("pw_cluster_gromos", k, "the cutoff is a NaN");
        const long n = (long)J.n;
        if ((long)J.d_first > (long)n_dist || n * n > (long)n_dist - (long)J.d_first)
            return stat_bad("pw_cluster_gromos", k, "the matrix reaches outside dist");
        if (n == 0) continue;
        if (!dist || !labels || !centres || !sizes) return stat_bad("pw_cluster_gromos", k, "null array");
        for (size_t m = 0; m < mats.size(); ++m)
            if (mats[m].d_first == (long)J.d_first && mats[m].n == n) mat_of[k] = (long)m;
        if (mat_of[k] >= 0) continue;
        const double* d = dist + J.d_first;
        for (long i = 0; i + 1 < n; ++i)
            for (long j = i + 1; j < n; ++j)
                if (pw_isnan_bits(d[i * n + j]))
                    return stat_bad("pw_cluster_gromos", k, "a NaN in the strict upper triangle of the matrix");
        mat_of[k] = (long)mats.size();
        mats.push_back(ClusterMatrix{(long)J.d_first, n});
    }
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_cluster(jobs, (long)n_jobs, dist, labels, centres, sizes, (long*)n_clusters,
                                   pw_context_host_threads(ctx, 0));
    if (mats.empty()) {                                              // no job has a frame
        for (long k = 0; k < (long)n_jobs; ++k) n_clusters[k] = 0;
        return PW_OK;
    }

    // the plan: live jobs in job order, gathered into launch groups while their bit matrices fit the budget
    const long slab_bytes = workspace_bytes ? (long)workspace_bytes : CLUSTER_SLAB_BYTES;
    const long bits_words = (workspace_bytes ? 4 * (long)workspace_bytes : CLUSTER_BITS_BYTES) / 8;
    const int rounds = rounds_per_check ? (int)(rounds_per_check < 4096 ? rounds_per_check : 4096) : CLUSTER_ROUNDS;
    std::vector<ClusterJobDev> devs;
    std::vector<long> job_of;                                        // the caller's index of a live job
    std::vector<ClusterGroup> groups;
    std::vector<ClusterCopy> copies;
    long total = 0, active_words = 0, slab_doubles = 0, max_words = 0;
    ClusterGroup cur{0, 0, 0, 0};
    for (long k = 0; k < (long)n_jobs; ++k) {
        const long n = (long)jobs[k].n;
        if (n == 0) continue;
        ClusterJobDev D{};
        D.n = n; D.S = cluster_stride(n); D.cutoff = jobs[k].cutoff; D.matrix = mat_of[k];
        const long words = n * D.S;
        if (cur.last > cur.first && cur.words + words > bits_words) {
            groups.push_back(cur);
            cur = ClusterGroup{cur.last, cur.last, 0, 0};
        }
        D.bits_first = cur.words; D.active_first = active_words; D.out_first = total; D.slot = (long)devs.size();
        cur.words += words; cur.last += 1; cur.n_max = n > cur.n_max ? n : cur.n_max;
        max_words = cur.words > max_words ? cur.words : max_words;
        if (!copies.empty() && copies.back().host + copies.back().count == (long)jobs[k].out_first)
            copies.back().count += n;
        else
            copies.push_back(ClusterCopy{(long)jobs[k].out_first, total, n});
        const long slab_rows = slab_bytes / (8 * n) < 1 ? 1 : slab_bytes / (8 * n) < n ? slab_bytes / (8 * n) : n;
        slab_doubles = slab_rows * n > slab_doubles ? slab_rows * n : slab_doubles;
        active_words += D.S; total += n;
        devs.push_back(D);
        job_of.push_back(k);
    }
    groups.push_back(cur);
    const long live = (long)devs.size();

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    std::vector<long> ncl_host((size_t)live, 0);
    std::vector<int> done_host((size_t)live, 0);
    {
        StreamBuffers buf(st);
        ClusterJobDev* d_jobs;
        double* d_slab;
        u64 *d_bits, *d_active, *d_state;                            // d_state: keys [live], then cluster counts [live]
        int *d_done, *d_out;                                         // d_out: labels, centres, sizes [total] each
        STAT_TRY(buf.alloc(&d_jobs, sizeof(ClusterJobDev) * (size_t)live));
        STAT_TRY(buf.alloc(&d_slab, sizeof(double) * (size_t)slab_doubles));
        STAT_TRY(buf.alloc(&d_bits, sizeof(u64) * (size_t)max_words));
        STAT_TRY(buf.alloc(&d_active, sizeof(u64) * (size_t)active_words));
        STAT_TRY(buf.alloc(&d_state, sizeof(u64) * 2 * (size_t)live));
        STAT_TRY(buf.alloc(&d_done, sizeof(int) * (size_t)live));
        STAT_TRY(buf.alloc(&d_out, sizeof(int) * 3 * (size_t)total));
        u64* d_keys = d_state;
        long* d_ncl = (long*)(d_state + live);
        int *d_labels = d_out, *d_centres = d_out + total, *d_sizes = d_out + 2 * total;
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_bits, sizeof(u64) * (size_t)max_words, st));
        STAT_TRY(poison_scratch(poison, d_active, sizeof(u64) * (size_t)active_words, st));
        STAT_TRY(poison_scratch(poison, d_state, sizeof(u64) * 2 * (size_t)live, st));
        STAT_TRY(poison_scratch(poison, d_done, sizeof(int) * (size_t)live, st));
        STAT_TRY(poison_scratch(poison, d_out, sizeof(int) * 3 * (size_t)total, st));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(ClusterJobDev) * (size_t)live, hipMemcpyHostToDevice, st));
        STAT_TRY(ev.start(st));
        hipLaunchKernelGGL(pw_cluster_init_kernel, dim3((unsigned)live), dim3(256), 0, st, d_jobs, d_active, d_keys, d_ncl,
                           d_done, d_centres, d_sizes);
        STAT_TRY(hipGetLastError());
        // (groups follow one another on the stream, so the next one may take the workspace and the slab over; every
        // kernel strides over its work along x -- tests/test_gpu_launch_cap.py sends them round again -- and a group
        // has a job with a frame, so no count is zero; y is the job)
        for (const ClusterGroup& G : groups) {
            const unsigned count = (unsigned)(G.last - G.first);
            const ClusterJobDev* gj = d_jobs + G.first;
            std::vector<long> seen;
            for (long q = G.first; q < G.last; ++q) {
                const long m = devs[q].matrix;
                bool had = false;
                for (long s : seen) had = had || s == m;
                if (had) continue;
                seen.push_back(m);
                const long n = mats[m].n, S = cluster_stride(n);
                const long slab_rows = slab_bytes / (8 * n) < 1 ? 1 : slab_bytes / (8 * n) < n ? slab_bytes / (8 * n) : n;
                for (long r0 = 0; r0 < n; r0 += slab_rows) {
                    const long rows = n - r0 < slab_rows ? n - r0 : slab_rows;
                    STAT_TRY(hipMemcpyAsync(d_slab, dist + mats[m].d_first + r0 * n, sizeof(double) * (size_t)(rows * n),
                                               hipMemcpyHostToDevice, st));
                    hipLaunchKernelGGL(pw_cluster_pack_kernel, dim3((unsigned)launch_blocks((rows * S + 3) / 4, 1l << 16), count), dim3(256),
                                       0, st, gj, m, d_slab, r0, rows, d_bits);
                    STAT_TRY(hipGetLastError());
                }
            }
            const long T = cluster_words(G.n_max);
            hipLaunchKernelGGL(pw_cluster_mirror_kernel, dim3((unsigned)launch_blocks((T * T + 3) / 4, 1l << 16), count), dim3(256), 0, st,
                               gj, d_bits);
            STAT_TRY(hipGetLastError());
            // a job takes one round a cluster and one more to find no frame active
            for (long queued = 0;;) {
                for (int r = 0; r < rounds; ++r) {
                    hipLaunchKernelGGL(pw_cluster_count_kernel, dim3((unsigned)launch_blocks((G.n_max + 3) / 4, 2048), count), dim3(256), 0,
                                       st, gj, d_bits, d_active, d_keys, d_done);
                    STAT_TRY(hipGetLastError());
                    hipLaunchKernelGGL(pw_cluster_pick_kernel, dim3(count), dim3(256), 0, st, gj, d_bits, d_active, d_keys, d_ncl,
                                       d_done, d_labels, d_centres, d_sizes);
                    STAT_TRY(hipGetLastError());
                }
                queued += rounds;
                STAT_TRY(hipMemcpyAsync(done_host.data() + G.first, d_done + G.first, sizeof(int) * count,
                                           hipMemcpyDeviceToHost, st));
                STAT_TRY(hipStreamSynchronize(st));
                bool all = true;
                for (long q = G.first; q < G.last; ++q) all = all && done_host[q] != 0;
                if (all) break;
                if (queued > G.n_max + 1) {                          // (cannot be: a round takes at least one frame)
                    snprintf(pw_internal_error_buffer(), 512, "pw_cluster_gromos: the rounds did not end");
                    return PW_E_HIP;
                }
            }
        }
        STAT_TRY(ev.stop(st));
        // (the compact result is in job order: neighbours in the caller's arrays come back in one copy an array)
        for (const ClusterCopy& c : copies) {
            const size_t bytes = sizeof(int) * (size_t)c.count;
            STAT_TRY(hipMemcpyAsync(labels + c.host, d_labels + c.dev, bytes, hipMemcpyDeviceToHost, st));
            STAT_TRY(hipMemcpyAsync(centres + c.host, d_centres + c.dev, bytes, hipMemcpyDeviceToHost, st));
            STAT_TRY(hipMemcpyAsync(sizes + c.host, d_sizes + c.dev, bytes, hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(hipMemcpyAsync(ncl_host.data(), d_ncl, sizeof(long) * (size_t)live, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    for (long k = 0; k < (long)n_jobs; ++k)
        if (jobs[k].n == 0) n_clusters[k] = 0;
    for (long q = 0; q < live; ++q) n_clusters[job_of[q]] = ncl_host[q];
    return PW_OK;
}

}  // namespace

extern "C" int pw_cluster_gromos(pw_context* ctx, const pw_cluster_job* jobs, int64_t n_jobs, const double* dist,
                                 int64_t n_dist, int32_t* labels, int32_t* centres, int32_t* sizes, int64_t* n_clusters) {
    return cluster_gromos(ctx, jobs, n_jobs, dist, n_dist, labels, centres, sizes, n_clusters, 0, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_cluster_gromos with the budget of a slab given (0: the
// default), the rounds between two looks at the done flags (0: the default) -- the result may depend on neither -- and,
// when kernel_ms is not null, the device work timed by HIP events
extern "C" int pw_internal_cluster_gromos(pw_context* ctx, const pw_cluster_job* jobs, int64_t n_jobs, const double* dist,
                                          int64_t n_dist, int32_t* labels, int32_t* centres, int32_t* sizes,
                                          int64_t* n_clusters, int64_t workspace_bytes, int64_t rounds_per_check,
                                          float* kernel_ms) {
    return cluster_gromos(ctx, jobs, n_jobs, dist, n_dist, labels, centres, sizes, n_clusters, workspace_bytes,
                          rounds_per_check, kernel_ms);
}
