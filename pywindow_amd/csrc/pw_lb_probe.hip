// pw_lb_probe.hip -- test instrumentation (not part of the header): pw_internal_lb_probe runs a batch of cases of
// pw_lb_probe.hpp on the host path of a device == -1 context; pw_internal_lb_fields exports the field table.  A
// translation unit of its own: the analysis kernels and their out-of-line optimiser routines (pw_kernels.hip) are
// compiled exactly as without it.
//
// There is no device side yet.  The dispatcher (lb_probe_run) is written for any team, and a kernel that ran it --
// one workgroup per case, the LbMem<N> in LDS, the object in a local variable -- was built, but its first launch
// ended in a memory aperture violation whose cause was not found (docs/HISTORY.md), so it is not part of the
// library: a device context is refused, nothing is launched and nothing falls back to the host.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/pywindow_amd.h"
#include "pw_host.hpp"
#include "pw_lb_probe.hpp"

using namespace pw;

extern "C" char* pw_internal_error_buffer(void);   // pw_kernels.hip
extern "C" int pw_context_device(pw_context* ctx);
extern "C" int pw_hostpath_lb_probe(int n, void* cases, long n_cases);     // pw_hostpath.cpp

namespace {

template <int N>
int run(pw_context* ctx, void* cases, long n_cases) {
    const LbProbeCase<N>* cs = (const LbProbeCase<N>*)cases;
    for (long u = 0; u < n_cases; ++u)
        if (!lb_probe_safe<N>(cs[u])) {
            snprintf(pw_internal_error_buffer(), 512, "pw_internal_lb_probe: case %ld is not safe to run", u);
            return PW_E_BAD_ARG;       // nothing has run
        }
    if (pw_context_device(ctx) >= 0) {
        snprintf(pw_internal_error_buffer(), 512, "pw_internal_lb_probe: host path only (a device == -1 context)");
        return PW_E_NO_DEVICE;
    }
    return pw_hostpath_lb_probe(N, cases, n_cases);
}

}  // namespace

// cases: n_cases x LbProbeCase<n>, read and written in place; case_bytes: what the caller believes one case takes
extern "C" int pw_internal_lb_probe(pw_context* ctx, int n, void* cases, int64_t n_cases, size_t case_bytes) {
    if (!ctx || (n != 1 && n != 3) || n_cases < 0 || (n_cases && !cases)) return PW_E_BAD_ARG;
    if (case_bytes != (n == 3 ? sizeof(LbProbeCase<3>) : sizeof(LbProbeCase<1>))) return PW_E_BAD_ARG;
    if (n_cases == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    return n == 3 ? run<3>(ctx, cases, (long)n_cases) : run<1>(ctx, cases, (long)n_cases);
}

// the field table of LbProbeCase<n>: returns the number of fields (out receives the first cap of them)
extern "C" int pw_internal_lb_fields(int n, LbProbeField* out, int cap, size_t* case_bytes) {
    if (n != 1 && n != 3) return PW_E_BAD_ARG;
    if (case_bytes) *case_bytes = n == 3 ? sizeof(LbProbeCase<3>) : sizeof(LbProbeCase<1>);
    return n == 3 ? lb_probe_fields<3>(out, out ? cap : 0) : lb_probe_fields<1>(out, out ? cap : 0);
}
