// pw_host.hpp -- host-side helpers shared by the translation units of libpywindow_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace pw {

// Every C-ABI entry point works on its context's device and hands the calling thread back the
// device it came with: the HIP runtime (and its per-thread current device) is shared with the
// application -- with PyTorch in a one-process-per-GPU job -- and a library call must not move it.
struct DeviceScope {
    int prev = -1;
    bool moved = false;
    hipError_t enter(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == device) return hipSuccess;
        hipError_t e = hipSetDevice(device);
        moved = (e == hipSuccess);
        return e;
    }
    ~DeviceScope() {
        if (moved && prev >= 0) (void)hipSetDevice(prev);
    }
};

// Test hook (pw_kde.hip: pw_internal_poison_scratch): while the flag is set, the statistical entries (pw_kde_sums,
// pw_kde2_sums, pw_kde_wsums, pw_corr_sums, pw_dft_sums, pw_gate_counts, pw_trans_counts, pw_superpose, pw_cluster_gromos) fill their workspace and their
// compact device result with bytes 0xFF -- a NaN as a double, garbage as a gate summary or a bit mask -- before their first kernel,
// so that a read of device memory the call never wrote shows in the result.  Off at start; an entry reads the flag
// once a call, and the host path (device -1) never does.
inline std::atomic<int> g_poison_scratch{0};
inline bool scratch_poisoned() { return g_poison_scratch.load(std::memory_order_relaxed) != 0; }
inline hipError_t poison_scratch(bool on, void* p, size_t bytes, hipStream_t st) {
    return on && bytes ? hipMemsetAsync(p, 0xFF, bytes, st) : hipSuccess;
}

}  // namespace pw

// Threads (include/pywindow_amd.h, "Threads"): every entry point that takes a context holds the context's
// mutex for the duration of the call, so calls from several threads on ONE context are serialised and
// contexts never share mutable state.  Recursive: entry points are built from each other
// (pw_analysis_batch = upload + launch + download).
struct pw_context;
extern "C" void pw_internal_lock(pw_context* ctx);
extern "C" void pw_internal_unlock(pw_context* ctx);
struct PwContextLock {
    pw_context* c;
    explicit PwContextLock(pw_context* c_) : c(c_) { if (c) pw_internal_lock(c); }
    ~PwContextLock() { if (c) pw_internal_unlock(c); }
    PwContextLock(const PwContextLock&) = delete;
    PwContextLock& operator=(const PwContextLock&) = delete;
};
#define PW_LOCK_CONTEXT(c) PwContextLock ctx_lock_(c)
