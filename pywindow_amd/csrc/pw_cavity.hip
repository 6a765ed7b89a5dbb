// pw_cavity.hip -- gfx950 kernel and the C ABI entry of the cavity of a cage (include/pywindow_amd.h: pw_cavity;
// definition of the result, the bit layout and why the culling is exact in pw_cavity.hpp; the classify and fill steps
// themselves in pw_cavity_dev.hpp, which pw_pores.hip shares).
//
// pw_cavity_kernel, a workgroup of four waves a job, everything of the job in LDS: two bit grids of ny * nz words,
// `open` and `fill`, and a few integers of reduction scratch, as dynamic LDS sized by the largest job of the launch
// (at 64 x 64 rows 2 x 32 KiB, which with the scratch is past what a static array may hold).
//   classify  a wave takes rows (j, l), lane i is voxel i.  The atoms come 64 at a time, lane a loading atom base + a
//             (coalesced, whatever n is: nothing is staged and nothing has a capacity) and testing whether the whole
//             row is clear of it (cavity_row_clear, exact); one __ballot of that is the list of atoms the row has to
//             look at -- a few of a cage's 168 -- and each of those is read from its lane by every lane (v_readlane)
//             for the voxel test.  Planes likewise, without a row test.  One __ballot of the lanes' answers is the
//             row's word.  (A job with ready-made open words -- the test hook -- loads and masks them instead.)
//   fill      thread t owns rows t, t + 256, ...; a sweep is fill |= spread(open, fill | neighbour rows) with the x
//             direction run to its fixed point inside the word (cavity_fill_word); neighbours are read while their
//             owners may be storing them (relaxed atomics: either value is a subset of the component), and the sweeps
//             repeat while __syncthreads_or(changed), at most nx * ny * nz + 1 times.  The barrier's answer is the
//             workgroup's, so every thread reaches every barrier the same number of times.
//   reduce    popcounts and integer sums of bit positions a row (cavity_row_sums), combined by integer LDS atomics --
//             the order cannot show -- and one thread writes the job's row of the compact result.
// No floating-point atomics, no loop without a bound derived from the grid, no workgroup waits for another.
// Launches follow one another on the context's stream; memory is allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_cavity(const pw_cavity_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                  const double* planes, pw_cavity_out* out, unsigned long long* mask,
                                  const unsigned long long* open_words, const long* open_first, int threads);   // pw_hostpath.cpp

static_assert(PW_CAVITY_MAX_G == CAVITY_MAX_G && PW_CAV_SEED_CLOSED == CAVITY_SEED_CLOSED, "the header's constants and the kernel's");
static_assert(sizeof(pw_cavity_job) == 120 && sizeof(pw_cavity_out) == 136, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int CAV_SUMS = 14;                                     // n_voxels, n_open, n_surface, n_face, first, second
constexpr size_t CAV_SCRATCH_BYTES = 8 * (CAV_SUMS + 1) + 4 * 4 + 8;   // the sums, the OR of the words, j / l min / max
constexpr size_t cav_lds_bytes(long rows) { return 16 * (size_t)rows + ((CAV_SCRATCH_BYTES + 15) & ~(size_t)15); }

// a job as the kernel reads it: firsts relative to the spans of the arrays that were uploaded
struct CavJobDev {
    long atom_first, n, radius_first, plane_first, m;
    long open_first;           // the job's ready-made open words in the workspace of its launch, or -1: classify
    long mask_first;           // where the job's cavity words go in that workspace, or -1
    double o[3], h, probe;
    int nx, ny, nz, seed[3];
};

__global__ void __launch_bounds__(CAV_THREADS)
pw_cavity_kernel(const CavJobDev* __restrict__ jobs, const double* __restrict__ xyz, const double* __restrict__ radii,
                 const double* __restrict__ planes, u64* __restrict__ ws, pw_cavity_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const CavJobDev& D = jobs[blockIdx.x];
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz;
    u64* s_open = (u64*)lds;
    u64* s_fill = s_open + rows;
    unsigned long long* s_sum = s_fill + rows;                  // [CAV_SUMS], then the OR of the cavity's words
    int* s_box = (int*)(s_sum + CAV_SUMS + 1);                  // j_min, j_max, l_min, l_max
    const int tid = threadIdx.x;

    // ---- classify
    if (D.open_first >= 0)
        cav_load_open(ws + D.open_first, nx, rows, s_open, s_fill);
    else
        cav_classify(xyz + 3 * D.atom_first, radii + D.radius_first, D.n, planes + 4 * D.plane_first, D.m, D.o[0], D.o[1],
                     D.o[2], D.h, D.probe, nx, ny, rows, s_open, s_fill);
    if (tid <= CAV_SUMS) s_sum[tid] = 0;
    if (tid < 4) s_box[tid] = (tid & 1) ? -1 : CAVITY_MAX_G;
    __syncthreads();
    const bool seed_open = cav_seed(D.seed, ny, s_open, s_fill);     // (thread 0's, for the flags)

    // ---- fill
    cav_fill(s_open, s_fill, nx, ny, nz);

    // ---- reduce
    for (int r = tid; r < rows; r += CAV_THREADS) {
        const long n_open = cavity_popcount(s_open[r]);
        if (n_open) atomicAdd(s_sum + 1, (unsigned long long)n_open);
        const u64 f = s_fill[r];
        if (D.mask_first >= 0) ws[D.mask_first + r] = f;
        if (!f) continue;
        const int j = r % ny, l = r / ny;
        CavityRow R;
        cavity_row_sums(f, j > 0 ? s_fill[r - 1] : 0, j + 1 < ny ? s_fill[r + 1] : 0, l > 0 ? s_fill[r - ny] : 0,
                        l + 1 < nz ? s_fill[r + ny] : 0, nx, ny, nz, j, l, R);
        atomicAdd(s_sum + 0, (unsigned long long)R.n);
        atomicAdd(s_sum + 2, (unsigned long long)R.surface);
        if (R.face) atomicAdd(s_sum + 3, (unsigned long long)R.face);
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd(s_sum + 4 + a, (unsigned long long)R.first[a]);
#pragma unroll
        for (int a = 0; a < 6; ++a) atomicAdd(s_sum + 7 + a, (unsigned long long)R.second[a]);
        atomicOr(s_sum + CAV_SUMS, f);
        atomicMin(s_box + 0, j);
        atomicMax(s_box + 1, j);
        atomicMin(s_box + 2, l);
        atomicMax(s_box + 3, l);
    }
    __syncthreads();
    if (tid == 0) {
        pw_cavity_out* o = out + blockIdx.x;
        const u64 any = s_sum[CAV_SUMS];
        o->n_voxels = (long)s_sum[0];
        o->n_open = (long)s_sum[1];
        o->n_surface = (long)s_sum[2];
        o->n_face = (long)s_sum[3];
        for (int a = 0; a < 3; ++a) o->first[a] = (long)s_sum[4 + a];
        for (int a = 0; a < 6; ++a) o->second[a] = (long)s_sum[7 + a];
        o->box[0] = any ? __ffsll((long long)any) - 1 : -1;
        o->box[1] = any ? 63 - __clzll((long long)any) : -1;
        for (int a = 0; a < 4; ++a) o->box[2 + a] = any ? s_box[a] : -1;
        o->flags = seed_open ? 0 : CAVITY_SEED_CLOSED;
        o->reserved = 0;
    }
}

const char* const ENTRY = "pw_cavity";
int cav_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written.  open_first (may be null; an entry -1: classify) names
// ready-made open words of a job in open_words[0 .. n_open_words).
int cav_check(const pw_cavity_job* jobs, long n_jobs, const double* xyz, long n_points, const double* radii, long n_radii,
              const double* planes, long n_planes, long n_out, const u64* mask, long n_mask, const u64* open_words,
              const long* open_first, long n_open_words) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_cavity_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        if (J.seed[0] < 0 || J.seed[0] >= J.nx || J.seed[1] < 0 || J.seed[1] >= J.ny || J.seed[2] < 0 || J.seed[2] >= J.nz)
            return cav_bad(k, "the seed is outside the grid");
        const long rows = (long)J.ny * J.nz;
        if (J.n < 0 || J.m < 0) return cav_bad(k, "a negative count");
        if (span_outside(J.atom_first, J.n, n_points)) return cav_bad(k, "atoms outside xyz");
        if (span_outside(J.radius_first, J.n, n_radii)) return cav_bad(k, "radii outside the array");
        if (span_outside(J.plane_first, J.m, n_planes)) return cav_bad(k, "planes outside the array");
        if (span_outside(J.out, 1, n_out)) return cav_bad(k, "the row is outside out");
        if (J.mask_first < -1 || (J.mask_first >= 0 && span_outside(J.mask_first, rows, n_mask)))
            return cav_bad(k, "the words are outside mask");
        if ((J.n && (!xyz || !radii)) || (J.m && !planes) || (J.mask_first >= 0 && !mask)) return cav_bad(k, "null array");
        if (open_first && open_first[k] != -1 && (!open_words || span_outside(open_first[k], rows, n_open_words)))
            return cav_bad(k, "the open words are outside their array");
        if (!pw_finite(J.origin[0]) || !pw_finite(J.origin[1]) || !pw_finite(J.origin[2]) || !pw_finite(J.spacing) ||
            !pw_finite(J.probe))
            return cav_bad(k, "the origin, the spacing or the probe is not finite");
        if (!(J.spacing > 0.0)) return cav_bad(k, "spacing <= 0");
        if (J.probe < 0.0) return cav_bad(k, "a negative probe");
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its radius)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_radii_check(ENTRY, k, radii, J.radius_first + a, 1));
        }
        GRID_CHECK(grid_planes_check(ENTRY, k, planes, J.plane_first, J.m));
    }
    // outputs of two jobs: the later of the two is named.  (Of rows, all of length 1, stat_shared names the second
    // lowest job of a row that is shared, as the sweep over equal neighbours did.  The words of mask keep their sweep,
    // which orders spans of one first by job where stat_shared orders them by length.)
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    long bad = -1;
    std::vector<std::pair<long, long>> spans;
    for (long k = 0; k < n_jobs; ++k)
        if (jobs[k].mask_first >= 0) spans.push_back({(long)jobs[k].mask_first, k});
    std::sort(spans.begin(), spans.end());
    long end = -1, owner = -1;                                       // the furthest end so far and the job it belongs to
    for (const auto& s : spans) {
        const long k = s.second, stop = s.first + (long)jobs[k].ny * jobs[k].nz;
        if (s.first < end) {
            const long later = k > owner ? k : owner;
            if (bad < 0 || later < bad) bad = later;
        }
        if (stop > end) {
            end = stop;
            owner = k;
        }
    }
    if (bad >= 0) return cav_bad(bad, "shares words of mask with an earlier job");
    return PW_OK;
}

// workspace_bytes: the budget of the open words and the masks of the jobs of one launch (0: CAVITY_WORKSPACE_BYTES; at
// 1 every job is a launch of its own); kernel_ms: when not null, the time of the device work of the call from the first
// launch to the last, the copies between them included, by HIP events on the context's stream
int cavity(pw_context* ctx, const pw_cavity_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
           const double* radii, int64_t n_radii, const double* planes, int64_t n_planes, pw_cavity_out* out, int64_t n_out,
           uint64_t* mask_, int64_t n_mask, const uint64_t* open_words_, const int64_t* open_first_, int64_t n_open_words,
           int64_t workspace_bytes, float* kernel_ms) {
    u64* mask = (u64*)mask_;
    const u64* open_words = (const u64*)open_words_;
    const long* open_first = (const long*)open_first_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_radii < 0 ||
        n_planes < 0 || n_out < 0 || n_mask < 0 || n_open_words < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = cav_check(jobs, N, xyz, (long)n_points, radii, (long)n_radii, planes, (long)n_planes, (long)n_out, mask,
                             (long)n_mask, open_words, open_first, (long)n_open_words);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_cavity(jobs, N, xyz, radii, planes, out, mask, open_words, open_first,
                                  pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // open words and masks fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : CAVITY_WORKSPACE_BYTES) / 8;
    Span atoms, atom_radii, windows;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        atom_radii.widen((long)jobs[k].radius_first, (long)jobs[k].n);
        windows.widen((long)jobs[k].plane_first, (long)jobs[k].m);
    }
    std::vector<CavJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    for (long k = 0; k < N; ++k) {
        const pw_cavity_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz;
        const bool given = open_first && open_first[k] >= 0;
        const long words = (given ? rows : 0) + (J.mask_first >= 0 ? rows : 0);
        place(groups, cur, budget_words, words + 1);                 // (a word more a job than it uses: no job is free)
        CavJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.radius_first = atom_radii.rel((long)J.radius_first, (long)J.n);
        D.plane_first = windows.rel((long)J.plane_first, (long)J.m);
        D.m = (long)J.m;
        D.mask_first = J.mask_first >= 0 ? cur.words : -1;           // (masks of neighbours side by side: one copy)
        D.open_first = given ? cur.words + (J.mask_first >= 0 ? rows : 0) : -1;
        for (int a = 0; a < 3; ++a) {
            D.o[a] = J.origin[a];
            D.seed[a] = J.seed[a];
        }
        D.h = J.spacing; D.probe = J.probe; D.nx = J.nx; D.ny = J.ny; D.nz = J.nz;
        cur.words += words; cur.cost += words + 1; cur.last += 1; cur.rows = rows > cur.rows ? rows : cur.rows;
    }
    groups.push_back(cur);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    STAT_TRY(hipFuncSetAttribute((const void*)pw_cavity_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)cav_lds_bytes(CAVITY_MAX_G * CAVITY_MAX_G)));
    {
        StreamBuffers buf(st);
        CavJobDev* d_jobs;
        double *d_xyz, *d_radii, *d_planes;
        u64* d_ws;
        pw_cavity_out* d_out;
        const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), out_bytes = sizeof(pw_cavity_out) * (size_t)N;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(CavJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(CavJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(atom_radii.upload(buf, &d_radii, radii, 1));
        STAT_TRY(windows.upload(buf, &d_planes, planes, 4));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over once the masks of
        // this one are on their way; neighbours in the workspace and in the caller's array travel in one copy)
        for (const LaunchGroup& G : groups) {
            for (long k = G.first; k < G.last; ++k)
                if (devs[k].open_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].open_first, open_words + open_first[k],
                                            sizeof(u64) * (size_t)((long)jobs[k].ny * jobs[k].nz), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(pw_cavity_kernel, dim3((unsigned)(G.last - G.first)), dim3(CAV_THREADS), cav_lds_bytes(G.rows), st,
                               d_jobs + G.first, d_xyz, d_radii, d_planes, d_ws, d_out + G.first);
            STAT_TRY(hipGetLastError());
            for (long k = G.first; k < G.last;) {
                if (devs[k].mask_first < 0) {
                    ++k;
                    continue;
                }
                long e = k, words = 0;
                for (;;) {
                    words += (long)jobs[e].ny * jobs[e].nz;
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
        // (the compact result is in job order: neighbours in the caller's array come back in one copy)
        for (long k = 0; k < N;) {
            long e = k + 1;
            while (e < N && jobs[e].out == jobs[e - 1].out + 1) ++e;
            STAT_TRY(hipMemcpyAsync(out + jobs[k].out, d_out + k, sizeof(pw_cavity_out) * (size_t)(e - k), hipMemcpyDeviceToHost, st));
            k = e;
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_cavity(pw_context* ctx, const pw_cavity_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                         const double* radii, int64_t n_radii, const double* planes, int64_t n_planes, pw_cavity_out* out,
                         int64_t n_out, uint64_t* mask, int64_t n_mask) {
    return cavity(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, planes, n_planes, out, n_out, mask, n_mask, nullptr,
                  nullptr, 0, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_cavity with ready-made open words for the jobs k whose
// open_first[k] >= 0 -- open_words[open_first[k] .. + ny * nz), one word a row, bits at i >= nx ignored -- in place of
// the classification of the atoms and planes (open_first null or -1: classify); with the budget of the workspace of a
// launch given (0: the default; the result may not depend on it); and, when kernel_ms is not null, the device work
// timed by HIP events
extern "C" int pw_internal_cavity(pw_context* ctx, const pw_cavity_job* jobs, int64_t n_jobs, const double* xyz,
                                  int64_t n_points, const double* radii, int64_t n_radii, const double* planes,
                                  int64_t n_planes, pw_cavity_out* out, int64_t n_out, uint64_t* mask, int64_t n_mask,
                                  const uint64_t* open_words, const int64_t* open_first, int64_t n_open_words,
                                  int64_t workspace_bytes, float* kernel_ms) {
    return cavity(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, planes, n_planes, out, n_out, mask, n_mask, open_words,
                  open_first, n_open_words, workspace_bytes, kernel_ms);
}
