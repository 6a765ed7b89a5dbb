// pw_channels.hip -- gfx950 kernel and the C ABI entry of the pore network of a periodic cell (include/pywindow_amd.h:
// pw_channels; definition of the result, the fill, its bounds and the proofs of the fills that are not run in
// pw_channels.hpp).
//
// pw_channels_kernel, a workgroup of four waves a job, everything of the job in LDS: four bit grids of ny * nz words --
// `todo` (the open voxels not yet given to a component), `p0` and `p1` (the two parities of a fill) and `acc` (the
// accessible words) -- and a few integers, as dynamic LDS sized by the largest job of the launch (128 KiB at 64 x 64 rows).
//   classify  the wave-a-row scheme of cav_classify (pw_cavity_dev.hpp) on the skewed centres, with its row cull.
//   loop      the first set bit of todo in rank order (chan_first); its component as p0 | p1, the component's n_voxels,
//             n_cross and winding bits (chan_walk, which runs chan_fill) -- all three in pw_channels_dev.hpp, shared with
//             pw_percolate.hip --; then, here, the row of the table, the labels, acc and the totals; the component leaves
//             todo.  Until todo is empty: at most n_open turns.
// Every branch that leads to a barrier depends on values read from LDS after a barrier, the same in every thread.  No
// floating-point atomics, no loop without a bound derived from the grid, no workgroup waits for another.
// Launches follow one another on the context's stream; memory is allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_cavity_dev.hpp"
#include "pw_channels.hpp"
#include "pw_channels_dev.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_channels(const pw_channels_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                    pw_channels_out* out, pw_channels_comp* comps, unsigned long long* mask,
                                    unsigned char* labels, const unsigned long long* open_words, const long* open_first,
                                    int threads);   // pw_hostpath.cpp

static_assert(PW_CHAN_MAX_COMPONENTS == CHAN_MAX_COMPONENTS && PW_CHAN_TRUNCATED == CHAN_TRUNCATED, "the header's constants and the kernel's");
static_assert(sizeof(pw_channels_job) == 152 && sizeof(pw_channels_comp) == 48 && sizeof(pw_channels_out) == 96, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr size_t CHAN_SCRATCH_BYTES = 64;                        // n_voxels, n_cross[3], n_open; the first voxel
constexpr size_t chan_lds_bytes(long rows) { return 32 * (size_t)rows + CHAN_SCRATCH_BYTES; }

// a job as the kernel reads it: firsts relative to the spans of the arrays that were uploaded
struct ChanJobDev {
    long atom_first, n, radius_first;
    long open_first;           // the job's ready-made open words in the workspace of its launch, or -1: classify
    long mask_first;           // where the job's accessible words go in that workspace, or -1
    long label_first;          // the WORD of that workspace at which the job's label bytes start, or -1
    long comp_first;           // the job's first row of the compact table
    double o[3], s[6], probe;
    int nx, ny, nz, c_max;
};

// classify: a wave takes rows (j, l), lane i is voxel i; s_todo[r] gets the row's word
__device__ inline void chan_classify(const double* __restrict__ atoms, const double* __restrict__ reach, long n,
                                     const ChanJobDev& D, int rows, u64* s_todo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nx = D.nx, ny = D.ny;
    for (int r = wave; r < rows; r += CAV_THREADS / 64) {
        const int j = r % ny, l = r / ny;
        const double x = channels_x(D.o[0], lane, D.s[0], j, D.s[1], l, D.s[3]);
        const double y = channels_y(D.o[1], j, D.s[2], l, D.s[4]), z = channels_z(D.o[2], l, D.s[5]);
        bool open = lane < nx;
        for (long base = 0; base < n; base += 64) {
            if (!__ballot(open)) break;                          // (no voxel of the row is open any more)
            const long a = base + lane;
            double X = 0.0, Y = 0.0, Z = 0.0, r2 = 0.0;
            bool near = false;
            if (a < n) {
                X = atoms[3 * a]; Y = atoms[3 * a + 1]; Z = atoms[3 * a + 2];
                r2 = cavity_reach2(reach[a], D.probe);
                near = !cavity_row_clear(y - Y, z - Z, r2);
            }
            for (u64 todo = __ballot(near); todo; todo &= todo - 1) {   // (at most 64 bits, one fewer a turn)
                const int b = __ffsll((long long)todo) - 1;
                open = open && cavity_free(x - cav_lane(X, b), y - cav_lane(Y, b), z - cav_lane(Z, b), cav_lane(r2, b));
            }
        }
        const u64 word = __ballot(open);
        if (lane == 0) s_todo[r] = word;
    }
}

__global__ void __launch_bounds__(CAV_THREADS)
pw_channels_kernel(const ChanJobDev* __restrict__ jobs, const double* __restrict__ xyz, const double* __restrict__ radii,
                   u64* __restrict__ ws, pw_channels_comp* __restrict__ comps, pw_channels_out* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const ChanJobDev& D = jobs[blockIdx.x];
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz, c_max = D.c_max;
    u64* s_todo = (u64*)lds;
    u64* s_p0 = s_todo + rows;
    u64* s_p1 = s_p0 + rows;
    u64* s_acc = s_p1 + rows;
    unsigned long long* s_sum = s_acc + rows;                   // n_voxels, n_cross[3] of a component; n_open
    unsigned* s_first = (unsigned*)(s_sum + 5);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* label = D.label_first >= 0 ? (unsigned char*)(ws + D.label_first) : nullptr;
    pw_channels_comp* table = comps + D.comp_first;

    // ---- classify
    if (D.open_first >= 0) {
        const u64 xmask = cavity_row_mask(nx);
        for (int r = tid; r < rows; r += CAV_THREADS) s_todo[r] = ws[D.open_first + r] & xmask;
    } else {
        chan_classify(xyz + 3 * D.atom_first, radii + D.radius_first, D.n, D, rows, s_todo);
    }
    if (tid < 5) s_sum[tid] = 0;
    __syncthreads();
    {
        long mine = 0;
        for (int r = tid; r < rows; r += CAV_THREADS) {
            s_acc[r] = 0;
            mine += cavity_popcount(s_todo[r]);
        }
        if (mine) atomicAdd(s_sum + 4, (unsigned long long)mine);
        if (label)
            for (int r = wave; r < rows; r += CAV_THREADS / 64)
                if (lane < nx && !((s_todo[r] >> lane) & 1ull)) label[(long)r * nx + lane] = (unsigned char)CHAN_LABEL_CLOSED;
    }

    // ---- the components, in the order of their first voxels
    long voxels_by_rank[4] = {0, 0, 0, 0}, comps_by_rank[4] = {0, 0, 0, 0}, count = 0;
    const long n_voxels_grid = (long)nx * rows;
    int cursor = tid;                                                // (chan_first's, pw_channels_dev.hpp)
    for (long turn = 0; turn <= n_voxels_grid; ++turn) {             // (a turn takes a voxel or more out of todo, or ends)
        const unsigned first = chan_first(s_todo, rows, cursor, s_first);
        if (first == CHAN_NONE) break;
        const int seed_row = (int)(first >> 6);
        const ChannelsWalk W = chan_walk(s_todo, s_p0, s_p1, s_sum, seed_row, 1ull << (first & 63u), nx, ny, nz);
        const long n_voxels = W.n_voxels;
        const int wraps = W.wraps, rank = channels_rank(wraps);

        // the component leaves todo; p0 | p1 is still the component, and nobody stores to it before the next barrier
        for (int r = tid; r < rows; r += CAV_THREADS) {
            const u64 f = s_p0[r] | s_p1[r];
            if (!f) continue;
            s_todo[r] &= ~f;
            if (rank >= 1) s_acc[r] |= f;
        }
        if (label) {
            const unsigned char name = (unsigned char)(count < c_max ? count : CHAN_LABEL_BEYOND);
            for (int r = wave; r < rows; r += CAV_THREADS / 64)
                if (lane < nx && (((s_p0[r] | s_p1[r]) >> lane) & 1ull)) label[(long)r * nx + lane] = name;
        }
        if (tid == 0 && count < c_max) {
            pw_channels_comp& C = table[count];
            C.first = (long)seed_row * nx + (long)(first & 63u);
            C.n_voxels = n_voxels;
            for (int k = 0; k < 3; ++k) C.n_cross[k] = W.n_cross[k];
            C.wraps = wraps;
            C.rank = rank;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            voxels_by_rank[q] += q == rank ? n_voxels : 0;
            comps_by_rank[q] += q == rank ? 1 : 0;
        }
        ++count;
    }

    // ---- the job's row, the rest of its rows of the table, the accessible words
    __syncthreads();
    if (D.mask_first >= 0)
        for (int r = tid; r < rows; r += CAV_THREADS) ws[D.mask_first + r] = s_acc[r];
    for (long c = count + tid; c < c_max; c += CAV_THREADS) {
        pw_channels_comp& C = table[c];
        C.first = -1;
        C.n_voxels = 0;
        for (int k = 0; k < 3; ++k) C.n_cross[k] = 0;
        C.wraps = 0;
        C.rank = 0;
    }
    if (tid == 0) {
        pw_channels_out* o = out + blockIdx.x;
        o->n_open = (long)s_sum[4];
        o->n_components = count;
        o->n_recorded = count < c_max ? count : c_max;
        for (int q = 0; q < 4; ++q) {
            o->n_voxels_by_rank[q] = voxels_by_rank[q];
            o->n_components_by_rank[q] = comps_by_rank[q];
        }
        o->flags = count > c_max ? CHAN_TRUNCATED : 0;
        o->reserved = 0;
    }
}

const char* const ENTRY = "pw_channels";
int chan_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

inline long chan_voxels(const pw_channels_job& J) { return (long)J.nx * J.ny * J.nz; }

// Everything is checked before anything is launched or written.  open_first (may be null; an entry -1: classify) names
// ready-made open words of a job in open_words[0 .. n_open_words).
int chan_check(const pw_channels_job* jobs, long n_jobs, const double* xyz, long n_points, const double* radii, long n_radii,
               long n_out, const pw_channels_comp* comps, long n_comps, const u64* mask, long n_mask,
               const unsigned char* labels, long n_labels, const u64* open_words, const long* open_first, long n_open_words) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_channels_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        if (J.c_max < 0 || J.c_max > CHAN_MAX_COMPONENTS) return chan_bad(k, "c_max outside 0 .. PW_CHAN_MAX_COMPONENTS (254)");
        const long rows = (long)J.ny * J.nz;
        if (J.n < 0) return chan_bad(k, "a negative count");
        if (span_outside(J.atom_first, J.n, n_points)) return chan_bad(k, "atoms outside xyz");
        if (span_outside(J.radius_first, J.n, n_radii)) return chan_bad(k, "radii outside the array");
        if (span_outside(J.out, 1, n_out)) return chan_bad(k, "the row is outside out");
        if (span_outside(J.comp_first, J.c_max, n_comps)) return chan_bad(k, "the rows are outside comps");
        if (J.mask_first < -1 || (J.mask_first >= 0 && span_outside(J.mask_first, rows, n_mask)))
            return chan_bad(k, "the words are outside mask");
        if (J.label_first < -1 || (J.label_first >= 0 && span_outside(J.label_first, chan_voxels(J), n_labels)))
            return chan_bad(k, "the bytes are outside labels");
        if ((J.n && (!xyz || !radii)) || (J.c_max && !comps) || (J.mask_first >= 0 && !mask) || (J.label_first >= 0 && !labels))
            return chan_bad(k, "null array");
        if (open_first && open_first[k] != -1 && (!open_words || span_outside(open_first[k], rows, n_open_words)))
            return chan_bad(k, "the open words are outside their array");
        bool finite = pw_finite(J.probe);
        for (int a = 0; a < 3; ++a) finite = finite && pw_finite(J.origin[a]);
        for (int a = 0; a < 6; ++a) finite = finite && pw_finite(J.step[a]);
        if (!finite) return chan_bad(k, "the origin, a step or the probe is not finite");
        if (!(J.step[0] > 0.0 && J.step[2] > 0.0 && J.step[5] > 0.0)) return chan_bad(k, "ax, by or cz <= 0");
        if (J.probe < 0.0) return chan_bad(k, "a negative probe");
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its radius)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_radii_check(ENTRY, k, radii, J.radius_first + a, 1));
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of comps with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].comp_first, (long)jobs[k].c_max}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares words of mask with an earlier job", [&](long k) {
        return OutSpan{(long)jobs[k].mask_first, jobs[k].mask_first >= 0 ? (long)jobs[k].ny * jobs[k].nz : 0};
    }));
    return shared_output(ENTRY, n_jobs, "shares bytes of labels with an earlier job", [&](long k) {
        return OutSpan{(long)jobs[k].label_first, jobs[k].label_first >= 0 ? chan_voxels(jobs[k]) : 0};
    });
}

// workspace_bytes: the budget of the open words, the masks and the labels of the jobs of one launch (0:
// CHAN_WORKSPACE_BYTES; at 1 every job is a launch of its own); kernel_ms: when not null, the time of the device work of
// the call from the first launch to the last, the copies between them included, by HIP events on the context's stream
int channels(pw_context* ctx, const pw_channels_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
             const double* radii, int64_t n_radii, pw_channels_out* out, int64_t n_out, pw_channels_comp* comps,
             int64_t n_comps, uint64_t* mask_, int64_t n_mask, uint8_t* labels, int64_t n_labels, const uint64_t* open_words_,
             const int64_t* open_first_, int64_t n_open_words, int64_t workspace_bytes, float* kernel_ms) {
    u64* mask = (u64*)mask_;
    const u64* open_words = (const u64*)open_words_;
    const long* open_first = (const long*)open_first_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_radii < 0 || n_out < 0 ||
        n_comps < 0 || n_mask < 0 || n_labels < 0 || n_open_words < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = chan_check(jobs, N, xyz, (long)n_points, radii, (long)n_radii, (long)n_out, comps, (long)n_comps, mask,
                              (long)n_mask, labels, (long)n_labels, open_words, open_first, (long)n_open_words);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_channels(jobs, N, xyz, radii, out, comps, mask, labels, open_words, open_first,
                                    pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // open words, masks and labels fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : CHAN_WORKSPACE_BYTES) / 8;
    Span atoms, atom_radii;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        atom_radii.widen((long)jobs[k].radius_first, (long)jobs[k].n);
    }
    std::vector<ChanJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long n_table = 0;
    for (long k = 0; k < N; ++k) {
        const pw_channels_job& J = jobs[k];
        const long rows = (long)J.ny * J.nz, label_words = J.label_first >= 0 ? (chan_voxels(J) + 7) / 8 : 0;
        const bool given = open_first && open_first[k] >= 0;
        const long mask_words = J.mask_first >= 0 ? rows : 0, words = mask_words + (given ? rows : 0) + label_words;
        place(groups, cur, budget_words, words + 1);                 // (a word more a job than it uses: no job is free)
        ChanJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.radius_first = atom_radii.rel((long)J.radius_first, (long)J.n);
        D.mask_first = mask_words ? cur.words : -1;                  // (masks of neighbours side by side: one copy)
        D.open_first = given ? cur.words + mask_words : -1;
        D.label_first = label_words ? cur.words + mask_words + (given ? rows : 0) : -1;
        D.comp_first = n_table;
        n_table += J.c_max;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        for (int a = 0; a < 6; ++a) D.s[a] = J.step[a];
        D.probe = J.probe; D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.c_max = J.c_max;
        cur.words += words; cur.cost += words + 1; cur.last += 1; cur.rows = rows > cur.rows ? rows : cur.rows;
    }
    groups.push_back(cur);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    STAT_TRY(hipFuncSetAttribute((const void*)pw_channels_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)chan_lds_bytes(CAVITY_MAX_G * CAVITY_MAX_G)));
    {
        StreamBuffers buf(st);
        ChanJobDev* d_jobs;
        double *d_xyz, *d_radii;
        u64* d_ws;
        pw_channels_comp* d_comps;
        pw_channels_out* d_out;
        const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), comps_bytes = sizeof(pw_channels_comp) * (size_t)n_table,
                     out_bytes = sizeof(pw_channels_out) * (size_t)N;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(ChanJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(ChanJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(atom_radii.upload(buf, &d_radii, radii, 1));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_comps, comps_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_comps, comps_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one may take the workspace over once the masks and
        // labels of this one are on their way; neighbours in the workspace and in the caller's array travel in one copy)
        for (const LaunchGroup& G : groups) {
            for (long k = G.first; k < G.last; ++k)
                if (devs[k].open_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].open_first, open_words + open_first[k],
                                            sizeof(u64) * (size_t)((long)jobs[k].ny * jobs[k].nz), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(pw_channels_kernel, dim3((unsigned)(G.last - G.first)), dim3(CAV_THREADS), chan_lds_bytes(G.rows), st,
                               d_jobs + G.first, d_xyz, d_radii, d_ws, d_comps, d_out + G.first);
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
            for (long k = G.first; k < G.last; ++k)                  // (labels start at a word: a copy a job)
                if (devs[k].label_first >= 0)
                    STAT_TRY(hipMemcpyAsync(labels + jobs[k].label_first, d_ws + devs[k].label_first, (size_t)chan_voxels(jobs[k]),
                                            hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(ev.stop(st));
        // (the compact results are in job order: neighbours in the caller's arrays come back in one copy)
        for (long k = 0; k < N;) {
            long e = k + 1;
            while (e < N && jobs[e].out == jobs[e - 1].out + 1) ++e;
            STAT_TRY(hipMemcpyAsync(out + jobs[k].out, d_out + k, sizeof(pw_channels_out) * (size_t)(e - k), hipMemcpyDeviceToHost, st));
            k = e;
        }
        for (long k = 0; k < N;) {
            long e = k + 1, count = (long)jobs[k].c_max;
            while (e < N && jobs[e].comp_first == jobs[e - 1].comp_first + jobs[e - 1].c_max) count += (long)jobs[e++].c_max;
            if (count)
                STAT_TRY(hipMemcpyAsync(comps + jobs[k].comp_first, d_comps + devs[k].comp_first, sizeof(pw_channels_comp) * (size_t)count,
                                        hipMemcpyDeviceToHost, st));
            k = e;
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_channels(pw_context* ctx, const pw_channels_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                           const double* radii, int64_t n_radii, pw_channels_out* out, int64_t n_out, pw_channels_comp* comps,
                           int64_t n_comps, uint64_t* mask, int64_t n_mask, uint8_t* labels, int64_t n_labels) {
    return channels(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, out, n_out, comps, n_comps, mask, n_mask, labels,
                    n_labels, nullptr, nullptr, 0, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_channels with ready-made open words for the jobs k whose
// open_first[k] >= 0 -- open_words[open_first[k] .. + ny * nz), one word a row, bits at i >= nx ignored -- in place of
// the classification of the atoms (open_first null or -1: classify); with the budget of the workspace of a launch given
// (0: the default; the result may not depend on it); and, when kernel_ms is not null, the device work timed by HIP events
extern "C" int pw_internal_channels(pw_context* ctx, const pw_channels_job* jobs, int64_t n_jobs, const double* xyz,
                                    int64_t n_points, const double* radii, int64_t n_radii, pw_channels_out* out, int64_t n_out,
                                    pw_channels_comp* comps, int64_t n_comps, uint64_t* mask, int64_t n_mask, uint8_t* labels,
                                    int64_t n_labels, const uint64_t* open_words, const int64_t* open_first,
                                    int64_t n_open_words, int64_t workspace_bytes, float* kernel_ms) {
    return channels(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, out, n_out, comps, n_comps, mask, n_mask, labels,
                    n_labels, open_words, open_first, n_open_words, workspace_bytes, kernel_ms);
}
