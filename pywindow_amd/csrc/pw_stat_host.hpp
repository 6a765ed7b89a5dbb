// pw_stat_host.hpp -- what the translation units of the statistical entries (pw_kde.hip, pw_kdew.hip, pw_corr.hip,
// pw_dft.hip, pw_gate.hip, pw_trans.hip, pw_superpose.hip, pw_cluster.hip, pw_cov.hip) and, through pw_grid_host.hpp,
// those of the grid entries (listed there) share on the host side of a call: device
// memory and events of one call, the two ways an entry reports a failure, the search of a work item's slab, the
// poison switch and, for every launch whose workgroups stride over its work items (pw_kernels.hip's math probe among
// them), the grid of a capped launch with its test hook.  Not for pw_hostpath.cpp: this is HIP.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_host.hpp"

extern "C" char* pw_internal_error_buffer(void);   // pw_kernels.hip (512 bytes, thread local)
extern "C" int pw_context_device(pw_context* ctx);

namespace pw {

// Test hook (pw_kde.hip: pw_internal_poison_scratch): while the flag is set, the statistical entries (pw_kde_sums,
// pw_kde2_sums, pw_kde_wsums, pw_corr_sums, pw_dft_sums, pw_gate_counts, pw_trans_counts, pw_superpose, pw_cluster_gromos, pw_covariance, pw_project, pw_cavity, pw_sasa, pw_pore_sizes, pw_affinity, pw_rigid_affinity, pw_rigid_cell, pw_rigid_cell_ewald, pw_passage, pw_hop, pw_charges, pw_channels) fill their workspace and their
// compact device result with bytes 0xFF -- a NaN as a double, garbage as a gate summary or a bit mask -- before their first kernel,
// so that a read of device memory the call never wrote shows in the result.  The periodic pre-processing (pw_rebuild.hip) does
// the same with its team slabs and its device outputs.  Off at start; an entry reads the flag
// once a call, and the host path (device -1) never does.  Its companion is the launch-cap hook below (pw_kde.hip:
// pw_internal_launch_cap), which makes the workgroups of a small batch take a second work item: the tests set both.
inline std::atomic<int> g_poison_scratch{0};
inline bool scratch_poisoned() { return g_poison_scratch.load(std::memory_order_relaxed) != 0; }
inline hipError_t poison_scratch(bool on, void* p, size_t bytes, hipStream_t st) {
    return on && bytes ? hipMemsetAsync(p, 0xFF, bytes, st) : hipSuccess;
}

// The grid of a capped launch: the kernels whose workgroups walk their work items with
// `for (item = blockIdx.x; item < total; item += gridDim.x)` -- or by wave or by thread, `items` then being the
// workgroups that would take one turn each -- are launched with min(items, cap) workgroups, `cap` being the launch
// site's own; the guard for zero items stays with the site.  The caps: 65536 at every site of the grid and crystal
// entries, at the reduce kernels of pw_kde.hip, pw_kdew.hip and pw_corr.hip, at the probes, at the three kernels of
// pw_superpose.hip, the five of pw_cov.hip and the pack and mirror kernels of pw_cluster.hip (x; y is the job); 2^20 at
// the partial kernels of pw_kde.hip, pw_kdew.hip and pw_corr.hip and at every kernel of pw_dft.hip (its phase probe
// included), pw_gate.hip and pw_trans.hip; 2048 at pw_cluster_count_kernel; 4096 at pw_shape_kernel.  Not through here:
// the launches of one workgroup a job (pw_cluster_init_kernel, pw_cluster_pick_kernel) and pw_circumcircle_kernel, which
// do not stride.  Plain C++.  Test hook (pw_kde.hip: pw_internal_launch_cap(blocks)): while blocks > 0
// every site gets min(items, blocks) instead, so that a batch of a few dozen items sends every workgroup round its loop
// again -- the second item of a workgroup is otherwise met only beyond the cap -- and 0 gives every site its own cap
// back.  Off at start; read on the host at the launch site only, never by a kernel or by the host path (device -1).
// g_launch_cut counts the calls that returned fewer workgroups than items; the hook returns and clears it, which is how
// a test knows that the launches it meant to cut were cut.
inline std::atomic<long> g_launch_cap{0};
inline std::atomic<long> g_launch_cut{0};
inline long launch_blocks(long items, long cap) {
    const long hook = g_launch_cap.load(std::memory_order_relaxed);
    const long blocks = hook > 0 ? (items < hook ? items : hook) : (items < cap ? items : cap);
    if (blocks < items) g_launch_cut.fetch_add(1, std::memory_order_relaxed);
    return blocks;
}
inline long launch_cap_hook(long blocks) {
    g_launch_cap.store(blocks > 0 ? blocks : 0, std::memory_order_relaxed);
    return g_launch_cut.exchange(0, std::memory_order_relaxed);
}

// (what follows has internal linkage, as when every file had a copy of its own: it adds nothing to the library's symbols)
namespace {

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

// the time of a call's kernels by HIP events on its stream, for the measurement hooks; ms null (every entry of the
// header): no event is made and every step is hipSuccess
struct Events {
    float* ms;
    hipEvent_t a = nullptr, b = nullptr;
    explicit Events(float* kernel_ms) : ms(kernel_ms) {}
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t create() {
        if (!ms) return hipSuccess;
        const hipError_t e = hipEventCreate(&a);
        return e != hipSuccess ? e : hipEventCreate(&b);
    }
    hipError_t start(hipStream_t st) { return ms ? hipEventRecord(a, st) : hipSuccess; }
    hipError_t stop(hipStream_t st) { return ms ? hipEventRecord(b, st) : hipSuccess; }
    hipError_t read() { return ms ? hipEventElapsedTime(ms, a, b) : hipSuccess; }   // (after the stream is synchronised)
};

// a job the entry `entry` (its name in the header) refuses
inline int stat_bad(const char* entry, long k, const char* what) {
    snprintf(pw_internal_error_buffer(), 512, "%s: job %ld: %s", entry, k, what);
    return PW_E_BAD_ARG;
}

// of spans (first, length, job) that must not overlap: the earliest job that shares an entry with a job before it, or -1
inline long stat_shared(std::vector<std::array<long, 3>>& spans) {
    std::sort(spans.begin(), spans.end());
    long bad = -1, end = -1, owner = -1;                             // the furthest end so far and the job it belongs to
    for (const auto& s : spans) {
        if (s[0] < end) {
            const long later = s[2] > owner ? s[2] : owner;
            if (bad < 0 || later < bad) bad = later;
        }
        if (s[0] + s[1] > end) {
            end = s[0] + s[1];
            owner = s[2];
        }
    }
    return bad;
}

#if defined(__HIPCC__)
// the last entry k with key(k) <= v; keys ascending, key(0) == 0 <= v < key(n)
template <class Key>
__device__ inline int stat_find(int n, long v, Key key) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}
#endif

}  // namespace

}  // namespace pw

#define STAT_TRY(call)                                                                     \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            snprintf(pw_internal_error_buffer(), 512, "%s: %s", #call, hipGetErrorString(e_)); \
            return PW_E_HIP;                                                               \
        }                                                                                  \
    } while (0)
