// pw_pores.hip -- gfx950 kernel and the C ABI entry of the probe-swept cavity for a ladder of probes (include/
// pywindow_amd.h: pw_pore_sizes; definition of the result and of the sweep in pw_pores.hpp, of a level's reach in
// pw_cavity.hpp).
//
// pw_pores_kernel, a workgroup of four waves a job, everything of the job in LDS: four bit grids of ny * nz words --
// `open` and `fill` of the level at hand, `domain` (the reach of level 0) and `assigned` (the voxels of the domain that a
// level above the one at hand has swept) -- and a few integers, as dynamic LDS sized by the largest job of the launch.
//   seeds     lane l of wave 0 tests the seed voxel at level l (the voxel test itself, against every atom and plane,
//             or the seed's bit of the level's ready-made words); one __ballot is the set of levels that have a reach.
//             A level outside it is empty by definition: its row is zeros and PW_CAV_SEED_CLOSED, nothing is computed.
//   levels    level 0 first -- its reach is the domain --, then from the last one down to level 1.  A level classifies
//             and fills exactly as pw_cavity_kernel does (pw_cavity_dev.hpp); then thread t takes rows t, t + 256, ...:
//             the row's popcount and face voxels, its swept word (pores_dilate_row over the `fill` grid, integer
//             arithmetic, at most ny * nz source rows; a row without a domain voxel is skipped), AND domain for
//             n_swept and the mask, AND ~assigned for n_largest, OR-ed into assigned.  The counts of a thread are
//             summed in registers and combined by 64-bit integer LDS atomics.  Level 0 is not swept: a ball holds
//             its centre, so swept_0 & domain is the domain, and what no level above has taken is its n_largest.
// No floating-point atomics, no loop without a bound derived from n, m, L or the grid, no workgroup waits for another.
// Launches follow one another on the context's stream; memory is allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_pores.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_pore_sizes(const pw_pores_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                      const double* planes, const double* probes, pw_pores_level* levels,
                                      pw_pores_out* out, unsigned long long* mask, const unsigned long long* open_words,
                                      const long* open_first, int threads);   // pw_hostpath.cpp

static_assert(PW_PORES_MAX_LEVELS == PORES_MAX_LEVELS && PW_PORES_MAX_K2 == PORES_MAX_K2, "the header's constants and the kernel's");
static_assert(sizeof(pw_pores_job) == 136 && sizeof(pw_pores_level) == 40 && sizeof(pw_pores_out) == 24, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int PORES_SUMS = 4;                                    // n_reach, n_face, n_swept, n_largest
constexpr size_t pores_lds_bytes(long rows) { return 32 * (size_t)rows + 8 * (PORES_SUMS + 1) + 8; }   // (a multiple of 16)

// a job as the kernel reads it: firsts relative to the spans of the arrays that were uploaded
struct PoresJobDev {
    long atom_first, n, radius_first, plane_first, m;
    long open_first;           // the job's L * ny * nz ready-made open words in the workspace of its launch, or -1: classify
    long mask_first;           // where the job's L * ny * nz swept words go in that workspace, or -1
    long level_first;          // the job's first entry of the plan and of the compact level rows
    double o[3], h;
    int nx, ny, nz, seed[3], levels, reserved;
};
// a level of a job: its probe and its K (pores_k2, on the host)
struct PoresLevelDev {
    double probe;
    int k2, reserved;
};

__global__ void __launch_bounds__(CAV_THREADS)
pw_pores_kernel(const PoresJobDev* __restrict__ jobs, const double* __restrict__ xyz, const double* __restrict__ radii,
                const double* __restrict__ planes, const PoresLevelDev* __restrict__ plan, u64* __restrict__ ws,
                pw_pores_level* __restrict__ levels, pw_pores_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const PoresJobDev& D = jobs[blockIdx.x];
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz, L = D.levels;
    u64* s_open = (u64*)lds;
    u64* s_fill = s_open + rows;
    u64* s_domain = s_fill + rows;
    u64* s_assigned = s_domain + rows;
    unsigned long long* s_sum = s_assigned + rows;              // [PORES_SUMS], then the levels whose seed is open
    const int tid = threadIdx.x;
    const u64 xmask = cavity_row_mask(nx);
    const double* atoms = xyz + 3 * D.atom_first;
    const double* reach = radii + D.radius_first;
    const double* cuts = planes + 4 * D.plane_first;
    const PoresLevelDev* P = plan + D.level_first;
    pw_pores_level* LV = levels + D.level_first;
    const int seed_row = D.seed[2] * ny + D.seed[1];

    // ---- seeds: which levels have a reach at all
    if (tid < 64) {
        bool ok = false;
        if (tid < L) {
            if (D.open_first >= 0) {
                ok = ((ws[D.open_first + (long)tid * rows + seed_row] & xmask) >> D.seed[0]) & 1;
            } else {
                const double x = cavity_coord(D.o[0], D.seed[0], D.h), y = cavity_coord(D.o[1], D.seed[1], D.h),
                             z = cavity_coord(D.o[2], D.seed[2], D.h), probe = P[tid].probe;
                ok = true;
                for (long a = 0; a < D.n && ok; ++a)
                    ok = cavity_free(x - atoms[3 * a], y - atoms[3 * a + 1], z - atoms[3 * a + 2], cavity_reach2(reach[a], probe));
                for (long q = 0; q < D.m && ok; ++q) ok = cavity_inside(cuts + 4 * q, x, y, z);
            }
        }
        const u64 live = __ballot(ok);
        if (tid == 0) s_sum[PORES_SUMS] = live;
    }
    if (tid < PORES_SUMS) s_sum[tid] = 0;
    __syncthreads();
    const u64 live = s_sum[PORES_SUMS];

    // ---- levels: 0, then L - 1 down to 1
    for (int step = 0; step < L; ++step) {
        const int lv = step == 0 ? 0 : L - step;
        const bool first = step == 0;
        const int k2 = P[lv].k2;
        if (!((live >> lv) & 1)) {                                   // (the same in every thread)
            if (tid == 0) LV[lv] = pw_pores_level{0, 0, 0, 0, k2, CAVITY_SEED_CLOSED};
            for (int r = tid; r < rows; r += CAV_THREADS) {
                if (first) s_domain[r] = s_assigned[r] = 0;
                if (D.mask_first >= 0) ws[D.mask_first + (long)lv * rows + r] = 0;
            }
            continue;
        }
        if (D.open_first >= 0)
            cav_load_open(ws + D.open_first + (long)lv * rows, nx, rows, s_open, s_fill);
        else
            cav_classify(atoms, reach, D.n, cuts, D.m, D.o[0], D.o[1], D.o[2], D.h, P[lv].probe, nx, ny, rows, s_open, s_fill);
        __syncthreads();
        const bool seed_open = cav_seed(D.seed, ny, s_open, s_fill); // (thread 0's, for the flags)
        cav_fill(s_open, s_fill, nx, ny, nz);

        long n_reach = 0, n_face = 0, n_swept = 0, n_largest = 0;
        for (int r = tid; r < rows; r += CAV_THREADS) {              // (a thread's rows are its own in every level)
            const u64 f = s_fill[r];
            const int j = r % ny, l = r / ny;
            n_reach += cavity_popcount(f);
            n_face += cavity_row_face(f, nx, ny, nz, j, l);
            u64 swept = f;
            if (first) {
                s_domain[r] = f;
                s_assigned[r] = 0;
            } else {
                const u64 dom = s_domain[r];
                swept = dom ? pores_dilate_row([&](int s) { return s_fill[s]; }, j, l, ny, nz, k2, xmask) & dom : 0;
                const u64 taken = s_assigned[r], mine = swept & ~taken;
                s_assigned[r] = taken | mine;
                n_largest += cavity_popcount(mine);
            }
            n_swept += cavity_popcount(swept);
            if (D.mask_first >= 0) ws[D.mask_first + (long)lv * rows + r] = swept;
        }
        if (n_reach) atomicAdd(s_sum + 0, (unsigned long long)n_reach);
        if (n_face) atomicAdd(s_sum + 1, (unsigned long long)n_face);
        if (n_swept) atomicAdd(s_sum + 2, (unsigned long long)n_swept);
        if (n_largest) atomicAdd(s_sum + 3, (unsigned long long)n_largest);
        __syncthreads();
        if (tid == 0) {                                              // (level 0's n_largest comes last)
            LV[lv] = pw_pores_level{(long)s_sum[0], (long)s_sum[1], (long)s_sum[2], (long)s_sum[3], k2,
                                    seed_open ? 0 : CAVITY_SEED_CLOSED};
            for (int a = 0; a < PORES_SUMS; ++a) s_sum[a] = 0;       // (the next additions are behind a barrier)
        }
    }

    // ---- level 0 takes what no level above it has; nothing of the domain is left without a cover
    __syncthreads();
    long n_domain = 0, n_rest = 0;
    for (int r = tid; r < rows; r += CAV_THREADS) {
        const u64 dom = s_domain[r];
        n_domain += cavity_popcount(dom);
        n_rest += cavity_popcount(dom & ~s_assigned[r]);
    }
    if (n_domain) atomicAdd(s_sum + 0, (unsigned long long)n_domain);
    if (n_rest) atomicAdd(s_sum + 3, (unsigned long long)n_rest);
    __syncthreads();
    if (tid == 0) {
        LV[0].n_largest = (long)s_sum[3];
        out[blockIdx.x] = pw_pores_out{(long)s_sum[0], 0, L};
    }
}

const char* const ENTRY = "pw_pore_sizes";
int pores_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written.  open_first (may be null; an entry -1: classify) names
// the ready-made open words of a job, level after level, in open_words[0 .. n_open_words).
int pores_check(const pw_pores_job* jobs, long n_jobs, const double* xyz, long n_points, const double* radii, long n_radii,
                const double* planes, long n_planes, const double* probes, long n_probes, const pw_pores_level* levels,
                long n_levels, long n_out, const u64* mask, long n_mask, const u64* open_words, const long* open_first,
                long n_open_words) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_pores_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        if (J.seed[0] < 0 || J.seed[0] >= J.nx || J.seed[1] < 0 || J.seed[1] >= J.ny || J.seed[2] < 0 || J.seed[2] >= J.nz)
            return pores_bad(k, "the seed is outside the grid");
        if (J.n_levels < 1 || J.n_levels > PORES_MAX_LEVELS) return pores_bad(k, "n_levels outside 1 .. PW_PORES_MAX_LEVELS (64)");
        const long L = (long)J.n_levels, words = L * J.ny * J.nz;
        if (J.n < 0 || J.m < 0) return pores_bad(k, "a negative count");
        if (span_outside(J.atom_first, J.n, n_points)) return pores_bad(k, "atoms outside xyz");
        if (span_outside(J.radius_first, J.n, n_radii)) return pores_bad(k, "radii outside the array");
        if (span_outside(J.plane_first, J.m, n_planes)) return pores_bad(k, "planes outside the array");
        if (span_outside(J.probe_first, L, n_probes)) return pores_bad(k, "probes outside the array");
        if (span_outside(J.level_first, L, n_levels)) return pores_bad(k, "the rows are outside levels");
        if (span_outside(J.out, 1, n_out)) return pores_bad(k, "the row is outside out");
        if (J.mask_first < -1 || (J.mask_first >= 0 && span_outside(J.mask_first, words, n_mask)))
            return pores_bad(k, "the words are outside mask");
        if ((J.n && (!xyz || !radii)) || (J.m && !planes) || !probes || !levels || (J.mask_first >= 0 && !mask))
            return pores_bad(k, "null array");
        if (open_first && open_first[k] != -1 && (!open_words || span_outside(open_first[k], words, n_open_words)))
            return pores_bad(k, "the open words are outside their array");
        GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
        for (long l = 0; l < L; ++l) {
            const double p = probes[J.probe_first + l];
            if (!pw_finite(p)) return pores_bad(k, "a probe is not finite");
            if (p < 0.0) return pores_bad(k, "a negative probe");
            if (l && !(p > probes[J.probe_first + l - 1])) return pores_bad(k, "the probes are not strictly ascending");
        }
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its radius)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_radii_check(ENTRY, k, radii, J.radius_first + a, 1));
        }
        GRID_CHECK(grid_planes_check(ENTRY, k, planes, J.plane_first, J.m));
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of levels with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].level_first, (long)jobs[k].n_levels}; }));
    return shared_output(ENTRY, n_jobs, "shares words of mask with an earlier job", [&](long k) {
        const pw_pores_job& J = jobs[k];
        return OutSpan{(long)J.mask_first, J.mask_first >= 0 ? (long)J.n_levels * J.ny * J.nz : 0};
    });
}

// workspace_bytes: the budget of the open words and the masks of the jobs of one launch (0: PORES_WORKSPACE_BYTES; at
// 1 every job is a launch of its own); kernel_ms: when not null, the time of the device work of the call from the first
// launch to the last, the copies between them included, by HIP events on the context's stream
int pore_sizes(pw_context* ctx, const pw_pores_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
               const double* radii, int64_t n_radii, const double* planes, int64_t n_planes, const double* probes,
               int64_t n_probes, pw_pores_level* levels, int64_t n_levels, pw_pores_out* out, int64_t n_out, uint64_t* mask_,
               int64_t n_mask, const uint64_t* open_words_, const int64_t* open_first_, int64_t n_open_words,
               int64_t workspace_bytes, float* kernel_ms) {
    u64* mask = (u64*)mask_;
    const u64* open_words = (const u64*)open_words_;
    const long* open_first = (const long*)open_first_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_radii < 0 ||
        n_planes < 0 || n_probes < 0 || n_levels < 0 || n_out < 0 || n_mask < 0 || n_open_words < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = pores_check(jobs, N, xyz, (long)n_points, radii, (long)n_radii, planes, (long)n_planes, probes,
                               (long)n_probes, levels, (long)n_levels, (long)n_out, mask, (long)n_mask, open_words,
                               open_first, (long)n_open_words);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_pore_sizes(jobs, N, xyz, radii, planes, probes, levels, out, mask, open_words, open_first,
                                      pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, the levels of all jobs one after the other (probe and K), and the
    // plan: jobs in order, gathered into launches while their open words and masks fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : PORES_WORKSPACE_BYTES) / 8;
    Span atoms, atom_radii, windows;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        atom_radii.widen((long)jobs[k].radius_first, (long)jobs[k].n);
        windows.widen((long)jobs[k].plane_first, (long)jobs[k].m);
    }
    std::vector<PoresJobDev> devs((size_t)N);
    std::vector<PoresLevelDev> plan;
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    for (long k = 0; k < N; ++k) {
        const pw_pores_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, L = (long)J.n_levels;
        const bool given = open_first && open_first[k] >= 0;
        const long words = (given ? L * rows : 0) + (J.mask_first >= 0 ? L * rows : 0);
        place(groups, cur, budget_words, words + 1);                 // (a word more a job than it uses: no job is free)
        PoresJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.radius_first = atom_radii.rel((long)J.radius_first, (long)J.n);
        D.plane_first = windows.rel((long)J.plane_first, (long)J.m);
        D.m = (long)J.m;
        D.mask_first = J.mask_first >= 0 ? cur.words : -1;           // (masks of neighbours side by side: one copy)
        D.open_first = given ? cur.words + (J.mask_first >= 0 ? L * rows : 0) : -1;
        D.level_first = (long)plan.size();
        for (int a = 0; a < 3; ++a) {
            D.o[a] = J.origin[a];
            D.seed[a] = J.seed[a];
        }
        D.h = J.spacing; D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.levels = (int)L; D.reserved = 0;
        for (long l = 0; l < L; ++l) {
            const double p = probes[J.probe_first + l];
            plan.push_back(PoresLevelDev{p, pores_k2(p, J.spacing), 0});
        }
        cur.words += words; cur.cost += words + 1; cur.last += 1; cur.rows = rows > cur.rows ? rows : cur.rows;
    }
    groups.push_back(cur);
    const long n_plan = (long)plan.size();

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    STAT_TRY(hipFuncSetAttribute((const void*)pw_pores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)pores_lds_bytes(CAVITY_MAX_G * CAVITY_MAX_G)));
    {
        StreamBuffers buf(st);
        PoresJobDev* d_jobs;
        PoresLevelDev* d_plan;
        double *d_xyz, *d_radii, *d_planes;
        u64* d_ws;
        pw_pores_level* d_levels;
        pw_pores_out* d_out;
        const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), levels_bytes = sizeof(pw_pores_level) * (size_t)n_plan,
                     out_bytes = sizeof(pw_pores_out) * (size_t)N;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(PoresJobDev) * (size_t)N));
        STAT_TRY(buf.alloc(&d_plan, sizeof(PoresLevelDev) * (size_t)n_plan));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(PoresJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_plan, plan.data(), sizeof(PoresLevelDev) * (size_t)n_plan, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(atom_radii.upload(buf, &d_radii, radii, 1));
        STAT_TRY(windows.upload(buf, &d_planes, planes, 4));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_levels, levels_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_levels, levels_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over once the masks of
        // this one are on their way; neighbours in the workspace and in the caller's array travel in one copy)
        auto job_words = [&](long k) { return (long)jobs[k].n_levels * jobs[k].ny * jobs[k].nz; };
        for (const LaunchGroup& G : groups) {
            for (long k = G.first; k < G.last; ++k)
                if (devs[k].open_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].open_first, open_words + open_first[k], sizeof(u64) * (size_t)job_words(k),
                                            hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(pw_pores_kernel, dim3((unsigned)(G.last - G.first)), dim3(CAV_THREADS), pores_lds_bytes(G.rows), st,
                               d_jobs + G.first, d_xyz, d_radii, d_planes, d_plan, d_ws, d_levels, d_out + G.first);
            STAT_TRY(hipGetLastError());
            for (long k = G.first; k < G.last;) {
                if (devs[k].mask_first < 0) {
                    ++k;
                    continue;
                }
                long e = k, words = 0;
                for (;;) {
                    words += job_words(e);
                    if (e + 1 >= G.last || devs[e + 1].mask_first != devs[k].mask_first + words ||
                        (long)jobs[e + 1].mask_first != (long)jobs[k].mask_first + words)
                        break;
                    ++e;
                }
                STAT_TRY(hipMemcpyAsync(mask + jobs[k].mask_first, d_ws + devs[k].mask_first, sizeof(u64) * (size_t)words,
                                        hipMemcpyDeviceToHost, st));
                k = e + 1;
            }
        }
        STAT_TRY(ev.stop(st));
        // (the compact results are in job order: neighbours in the caller's arrays come back in one copy)
        for (long k = 0; k < N;) {
            long e = k + 1;
            while (e < N && jobs[e].out == jobs[e - 1].out + 1) ++e;
            STAT_TRY(hipMemcpyAsync(out + jobs[k].out, d_out + k, sizeof(pw_pores_out) * (size_t)(e - k), hipMemcpyDeviceToHost, st));
            k = e;
        }
        for (long k = 0; k < N;) {
            long e = k + 1, count = (long)jobs[k].n_levels;
            while (e < N && jobs[e].level_first == jobs[e - 1].level_first + jobs[e - 1].n_levels) count += (long)jobs[e++].n_levels;
            STAT_TRY(hipMemcpyAsync(levels + jobs[k].level_first, d_levels + devs[k].level_first, sizeof(pw_pores_level) * (size_t)count,
                                    hipMemcpyDeviceToHost, st));
            k = e;
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_pore_sizes(pw_context* ctx, const pw_pores_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                             const double* radii, int64_t n_radii, const double* planes, int64_t n_planes,
                             const double* probes, int64_t n_probes, pw_pores_level* levels, int64_t n_levels,
                             pw_pores_out* out, int64_t n_out, uint64_t* mask, int64_t n_mask) {
    return pore_sizes(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, planes, n_planes, probes, n_probes, levels, n_levels,
                      out, n_out, mask, n_mask, nullptr, nullptr, 0, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_pore_sizes with ready-made open words for the jobs k whose
// open_first[k] >= 0 -- open_words[open_first[k] .. + n_levels * ny * nz), level after level, one word a row, bits at
// i >= nx ignored -- in place of the classification of the atoms and planes (open_first null or -1: classify); the fill
// still runs from the seed, K still comes from the probes, and the levels need not be nested: each one is computed.
// With the budget of the workspace of a launch given (0: the default; the result may not depend on it); and, when
// kernel_ms is not null, the device work timed by HIP events
extern "C" int pw_internal_pore_sizes(pw_context* ctx, const pw_pores_job* jobs, int64_t n_jobs, const double* xyz,
                                      int64_t n_points, const double* radii, int64_t n_radii, const double* planes,
                                      int64_t n_planes, const double* probes, int64_t n_probes, pw_pores_level* levels,
                                      int64_t n_levels, pw_pores_out* out, int64_t n_out, uint64_t* mask, int64_t n_mask,
                                      const uint64_t* open_words, const int64_t* open_first, int64_t n_open_words,
                                      int64_t workspace_bytes, float* kernel_ms) {
    return pore_sizes(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, planes, n_planes, probes, n_probes, levels, n_levels,
                      out, n_out, mask, n_mask, open_words, open_first, n_open_words, workspace_bytes, kernel_ms);
}
