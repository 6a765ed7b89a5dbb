// pw_grid_host.hpp -- what the translation units of the grid entries (pw_cavity.hip, pw_sasa.hip, pw_pores.hip,
// pw_affinity.hip, pw_rigid.hip, pw_rigid_cell.hip, pw_passage.hip, pw_hop.hip), pw_charges.hip, pw_channels.hip, pw_percolate.hip and pw_basins.hip share on the host side of a call beyond pw_stat_host.hpp:
// the one range predicate, the span of an array that the jobs of a call read, the launch groups of a plan and the
// refusals that several entries word alike.  The checks that are an entry's own, the plan loop that fills its job
// records, its launches and its copy-back stay in its file.  Everything but Span::upload is plain C++ (tests/tools/
// grid_plan_check builds it for the CPU).  Not for pw_hostpath.cpp: pw_stat_host.hpp is HIP.
#pragma once
#include "pw_passage.hpp"   // pas_value_ok; with it pw_affinity.hpp (AFF_*) and pw_cavity.hpp (CAVITY_MAX_G, the words)
#include "pw_stat_host.hpp"

namespace pw {

// (internal linkage, as in pw_stat_host.hpp)
namespace {

// [first, first + count) is not inside [0, limit); count >= 0, limit >= 0
inline bool span_outside(long first, long count, long limit) { return first < 0 || count > limit || first > limit - count; }

// the part [lo, hi) of a caller's array that the jobs of a call read: only that is uploaded, and a job's first becomes
// relative to lo.  Without a member that has entries the span is (0, 0)
struct Span {
    long lo = -1, hi = 0;
    void widen(long first, long count) {
        if (count == 0) return;
        if (lo < 0 || first < lo) lo = first;
        if (first + count > hi) hi = first + count;
    }
    long lo_or_zero() const { return lo < 0 ? 0 : lo; }
    long count() const { return hi - lo_or_zero(); }
    // a member's first in the uploaded span; a member without entries reads nothing and gets 0
    long rel(long first, long n) const { return n ? first - lo : 0; }
#if defined(__HIPCC__)
    // device memory for the span's count() * width elements and, when there are any, their copy from host + width * lo
    template <class X>
    hipError_t upload(StreamBuffers& buf, X** dev, const X* host, long width) const {
        const size_t bytes = sizeof(X) * (size_t)width * (size_t)count();
        const hipError_t e = buf.alloc(dev, bytes);
        return e != hipSuccess || !bytes ? e : hipMemcpyAsync(*dev, host + width * lo, bytes, hipMemcpyHostToDevice, buf.st);
    }
#endif
};

// jobs [first, last) go in one launch and share one workspace of `words` 8-byte words; `cost` is what they take of the
// budget; `items` and `blocks` are the work items and workgroups of their kernels and the largest of them has `rows`
// rows of the grid.  An entry leaves at 0 what it does not use
struct LaunchGroup {
    long first = 0, last = 0, words = 0, cost = 0, items = 0, blocks = 0, rows = 0;
};

// before job cur.last joins: the group is closed and the next one opened iff it has a job and this one's cost would take
// it past the budget, so a job larger than the budget is a launch of its own.  The caller then adds the job to cur
inline void place(std::vector<LaunchGroup>& groups, LaunchGroup& cur, long budget_words, long cost_of_job) {
    if (cur.last > cur.first && cur.cost + cost_of_job > budget_words) {
        groups.push_back(cur);
        cur = LaunchGroup{cur.last, cur.last};
    }
}

// the workspace that serves every group in turn
inline long most_words(const std::vector<LaunchGroup>& groups) {
    long most = 0;
    for (const LaunchGroup& G : groups) most = G.words > most ? G.words : most;
    return most;
}

// ---- refusals that several entries share: PW_OK, or the entry's stat_bad.  An entry calls them in its own order
#define GRID_CHECK(call)                \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != PW_OK) return rc_;   \
    } while (0)

inline int grid_dims_check(const char* entry, long k, int nx, int ny, int nz) {
    if (nx < 1 || nx > CAVITY_MAX_G || ny < 1 || ny > CAVITY_MAX_G || nz < 1 || nz > CAVITY_MAX_G)
        return stat_bad(entry, k, "a dimension outside 1 .. PW_CAVITY_MAX_G (64)");
    return PW_OK;
}

inline int grid_frame_check(const char* entry, long k, const double* origin, double spacing) {
    if (!pw_finite(origin[0]) || !pw_finite(origin[1]) || !pw_finite(origin[2]) || !pw_finite(spacing))
        return stat_bad(entry, k, "the origin or the spacing is not finite");
    if (!(spacing > 0.0)) return stat_bad(entry, k, "spacing <= 0");
    return PW_OK;
}

inline int grid_core_check(const char* entry, long k, double core2, double cutoff2) {
    if (!pw_finite(core2) || !(core2 >= AFF_MIN_CORE2)) return stat_bad(entry, k, "core2 below 1e-6 or not finite");
    if (!pw_finite(cutoff2) || !(cutoff2 == 0.0 || cutoff2 > core2))
        return stat_bad(entry, k, "cutoff2 is neither 0 nor above core2");
    return PW_OK;
}

inline int grid_n_betas_check(const char* entry, long k, long L) {
    return L < 1 || L > AFF_MAX_LEVELS ? stat_bad(entry, k, "n_betas outside 1 .. PW_AFF_MAX_LEVELS (8)") : PW_OK;
}

// (the array checks read the members [first, first + n) of the caller's array, which may be null when n is 0)
inline int grid_betas_check(const char* entry, long k, const double* betas, long first, long L) {
    for (long b = first; b < first + L; ++b)
        if (!pw_finite(betas[b]) || betas[b] < 0.0) return stat_bad(entry, k, "a beta is negative or not finite");
    return PW_OK;
}

inline int grid_planes_check(const char* entry, long k, const double* planes, long first, long m) {
    for (long q = 4 * first; q < 4 * (first + m); ++q)
        if (!pw_finite(planes[q])) return stat_bad(entry, k, "a plane is not finite");
    return PW_OK;
}

inline int grid_field_check(const char* entry, long k, const double* field, long first, long V) {
    for (long v = first; v < first + V; ++v)
        if (!pas_value_ok(field[v])) return stat_bad(entry, k, "a field value is -inf or not a number");
    return PW_OK;
}

// n atoms (an entry that checks something else of an atom in between passes them one at a time)
inline int grid_xyz_check(const char* entry, long k, const double* xyz, long first, long n) {
    for (long c = 3 * first; c < 3 * (first + n); ++c)
        if (!pw_finite(xyz[c])) return stat_bad(entry, k, "a coordinate is not finite");
    return PW_OK;
}

inline int grid_radii_check(const char* entry, long k, const double* radii, long first, long n) {
    for (long a = first; a < first + n; ++a) {
        if (!pw_finite(radii[a])) return stat_bad(entry, k, "a radius is not finite");
        if (radii[a] < 0.0) return stat_bad(entry, k, "a negative radius");
    }
    return PW_OK;
}

// n rows of `width` doubles: (A, B) and, with width 3, a charge term that counts when `charged`
inline int grid_coef_check(const char* entry, long k, const double* coef, long first, long n, int width, bool charged) {
    for (long r = first; r < first + n; ++r) {
        const double* c = coef + width * r;
        if (!pw_finite(c[0]) || !pw_finite(c[1])) return stat_bad(entry, k, "a coefficient is not finite");
        if (c[0] < 0.0 || c[1] < 0.0 || c[0] > AFF_MAX_COEF || c[1] > AFF_MAX_COEF)
            return stat_bad(entry, k, "a coefficient outside 0 .. 1e100");
        if (charged && (!pw_finite(c[2]) || pw_abs(c[2]) > AFF_MAX_COEF))
            return stat_bad(entry, k, "a charge term is not finite or beyond 1e100");
    }
    return PW_OK;
}

// the voxels of a region: of the `rows` words of a mask (bits at i >= nx dropped), or of the whole grid (words null)
inline long grid_region_voxels(const cavity_word* words, int nx, long rows) {
    if (!words) return (long)nx * rows;
    long count = 0;
    for (long r = 0; r < rows; ++r) count += cavity_popcount(words[r] & cavity_row_mask(nx));
    return count;
}

// outputs of two jobs: span_of_job(k) is {first, count} of what job k writes (count 0: nothing, the job takes no part);
// the later of two jobs that share an entry is named
typedef std::array<long, 2> OutSpan;
template <class SpanOfJob>
inline int shared_output(const char* entry, long n_jobs, const char* what, SpanOfJob span_of_job) {
    std::vector<std::array<long, 3>> spans;
    for (long k = 0; k < n_jobs; ++k) {
        const OutSpan s = span_of_job(k);
        if (s[1]) spans.push_back({s[0], s[1], k});
    }
    const long bad = stat_shared(spans);
    return bad >= 0 ? stat_bad(entry, bad, what) : PW_OK;
}

}  // namespace

}  // namespace pw
