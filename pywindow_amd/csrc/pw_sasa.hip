// pw_sasa.hip -- gfx950 kernel and the C ABI entry of the accessible surface of a cage (include/pywindow_amd.h: pw_sasa;
// definition of the result, the cell search and the culling rule with its proof in pw_sasa.hpp).
//
// pw_sasa_kernel, a workgroup of four waves for SASA_BLOCK_ATOMS atoms of a job (a cage is one workgroup; a job of
// thousands of atoms takes several, which share nothing but two integer atomics at the end).  A wave takes the atoms
// i, i + 4, ... of its workgroup's range:
//   list      the atoms come 64 at a time, lane a loading atom base + a (coalesced, whatever n is) and testing whether
//             it can bury a point of i at all (sasa_far, conservative with a proof; j == i is dropped by its index);
//             one __ballot of that and a prefix popcount put the near atoms -- about 20 of a cage's 168 -- as
//             (X, Y, Z, R * R) into the wave's list in LDS, SASA_LIST_CAP entries.
//   points    lanes take the P test points 64 at a time and run down the list, every entry one broadcast read of LDS,
//             until no lane's point is left exposed; one __ballot and a popcount is the exposed count.  The exposed
//             lanes then find their grid cell by bisection (3 x at most 7 comparisons) and look at its corners in the
//             job's words -- in LDS when ny * nz <= SASA_LDS_WORDS, else read from global memory -- and a second
//             __ballot and popcount is the inside count.
//   overflow  a list that does not hold an atom's near atoms is not used for that atom: its points run over all n
//             atoms 64 at a time instead, culled and read from their lanes (v_readlane) as pw_cavity does it.  No
//             capacity in n; the integers cannot show which path ran.
// Lane 0 writes the atom's two counts; the wave's sums go to the job's row with one 64-bit integer atomicAdd each (the
// row is zeroed before the launch).  No floating-point atomics; every loop is bounded by n, P or the grid; no
// workgroup waits for another.  The directions are data (P x 3, transposed on upload so that lanes read neighbours):
// no transcendental is evaluated here.
// Occupancy: the compiler reports 39 VGPRs, 106 SGPRs (6 of them kept in lanes of a VGPR) and no scratch, and
// 7 waves a SIMD by registers; LDS is 16 KiB of lists plus at most 18 KiB of words a workgroup, so 4 workgroups =
// 16 waves a CU, 4 a SIMD, is what runs (a launch without words in LDS: 7 a SIMD).  SASA_LDS_WORDS is set where a
// cage's 46^2 .. 48^2 rows fit: larger grids keep that occupancy and pay a cached global read for a word instead.
// Launches follow one another on the context's stream; memory is allocated and released in stream order.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_sasa.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_sasa(const pw_sasa_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                const double* directions, long P, const unsigned long long* words, int* exposed,
                                int* inside, pw_sasa_out* out, int threads);   // pw_hostpath.cpp

static_assert(PW_SASA_MAX_POINTS == SASA_MAX_POINTS && PW_SASA_GRID == SASA_GRID, "the header's constants and the kernel's");
static_assert(sizeof(pw_sasa_job) == 104 && sizeof(pw_sasa_out) == 24, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int SASA_THREADS = 256;
constexpr int SASA_WAVES = SASA_THREADS / 64;
constexpr int SASA_LIST_CAP = 128;                               // near atoms a wave's list holds (4 doubles each)
constexpr long SASA_LDS_WORDS = 48 * 48;                         // a grid of at most this many rows goes to LDS
constexpr long SASA_BLOCK_ATOMS = 512;                           // atoms of a job a workgroup takes
constexpr size_t SASA_LIST_BYTES = sizeof(double) * 4 * SASA_LIST_CAP * SASA_WAVES;
constexpr size_t sasa_lds_bytes(long words) { return SASA_LIST_BYTES + 8 * (size_t)words; }   // (at most 48 KiB)

// a job as the kernel reads it: firsts relative to the spans of the arrays that were uploaded, counts compacted
struct SasaJobDev {
    long atom_first, n, radius_first, count_first;
    long word_first;           // the job's words in the uploaded span, or -1: no grid
    double o[3], h, probe, slack;
    int nx, ny, nz;
    int in_lds;                // the words are staged in LDS
};
// a workgroup: the atoms [a_begin, a_end) of a job
struct SasaBlock {
    long job, a_begin, a_end;
};

// the value that lane `from` of the wave holds; `from` is the wave's
__device__ inline double sasa_lane(double v, int from) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), from), __builtin_amdgcn_readlane(__double2loint(v), from));
}

// dirs: ux[0 .. P), uy[0 .. P), uz[0 .. P); counts: exposed[0 .. total), inside[0 .. total) of the compacted atoms
__global__ void __launch_bounds__(SASA_THREADS)
pw_sasa_kernel(const SasaBlock* __restrict__ blocks, const SasaJobDev* __restrict__ jobs, const double* __restrict__ xyz,
               const double* __restrict__ radii, const double* __restrict__ dirs, int P, const u64* __restrict__ words,
               int* __restrict__ counts, long total, pw_sasa_out* __restrict__ out, int list_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const SasaBlock B = blocks[blockIdx.x];
    const SasaJobDev& D = jobs[B.job];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* s_list = (double*)lds + 4 * SASA_LIST_CAP * wave;        // the wave's own
    u64* s_words = (u64*)(lds + SASA_LIST_BYTES);
    const int nx = D.nx, ny = D.ny, nz = D.nz;
    const bool grid = D.word_first >= 0, in_lds = D.in_lds != 0;
    const u64* g_words = words + (grid ? D.word_first : 0);
    if (in_lds)
        for (int r = tid; r < ny * nz; r += SASA_THREADS) s_words[r] = g_words[r];
    __syncthreads();                                                 // (B and D are the workgroup's: every thread is here)
    auto word = [&](int r) -> u64 { return in_lds ? s_words[r] : g_words[r]; };

    const long n = D.n;
    const double* atoms = xyz + 3 * D.atom_first;
    const double* reach = radii + D.radius_first;
    const double probe = D.probe, slack = D.slack, h = D.h;
    const double o[3] = {D.o[0], D.o[1], D.o[2]};
    const u64 below = (1ull << lane) - 1ull;                         // the lanes before this one
    long sum_exposed = 0, sum_inside = 0;
    for (long i = B.a_begin + wave; i < B.a_end; i += SASA_WAVES) {
        const double Xi = atoms[3 * i], Yi = atoms[3 * i + 1], Zi = atoms[3 * i + 2], Ri = sasa_reach(reach[i], probe);
        // ---- list
        int count = 0;
        bool overflow = false;
        for (long base = 0; base < n; base += 64) {
            const long a = base + lane;
            double X = 0.0, Y = 0.0, Z = 0.0, R = 0.0;
            bool near = false;
            if (a < n) {
                X = atoms[3 * a]; Y = atoms[3 * a + 1]; Z = atoms[3 * a + 2];
                R = sasa_reach(reach[a], probe);
                near = a != i && !sasa_far(Xi - X, Yi - Y, Zi - Z, Ri, R, slack);
            }
            const u64 mask = __ballot(near);
            const int more = __popcll(mask);
            if (count + more > list_cap) {
                overflow = true;
                break;
            }
            if (near) {
                double* e = s_list + 4 * (count + __popcll(mask & below));
                e[0] = X; e[1] = Y; e[2] = Z; e[3] = R * R;
            }
            count += more;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // (the list is the wave's: its lanes run together)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- points
        int n_exposed = 0, n_inside = 0;
        for (int kb = 0; kb < P; kb += 64) {
            const int k = kb + lane;
            bool exposed = k < P;
            double px = 0.0, py = 0.0, pz = 0.0;
            if (exposed) {
                px = sasa_point(Xi, Ri, dirs[k]);
                py = sasa_point(Yi, Ri, dirs[P + k]);
                pz = sasa_point(Zi, Ri, dirs[2 * P + k]);
            }
            if (!overflow) {
                for (int e = 0; e < count; ++e) {
                    if (!__ballot(exposed)) break;
                    const double* q = s_list + 4 * e;
                    exposed = exposed && sasa_exposed(px - q[0], py - q[1], pz - q[2], q[3]);
                }
            } else {
                for (long base = 0; base < n; base += 64) {
                    if (!__ballot(exposed)) break;
                    const long a = base + lane;
                    double X = 0.0, Y = 0.0, Z = 0.0, r2 = 0.0;
                    bool near = false;
                    if (a < n) {
                        X = atoms[3 * a]; Y = atoms[3 * a + 1]; Z = atoms[3 * a + 2];
                        const double R = sasa_reach(reach[a], probe);
                        r2 = R * R;
                        near = a != i && !sasa_far(Xi - X, Yi - Y, Zi - Z, Ri, R, slack);
                    }
                    for (u64 todo = __ballot(near); todo; todo &= todo - 1) {   // (at most 64 bits, one fewer a turn)
                        const int b = __ffsll((long long)todo) - 1;
                        exposed = exposed && sasa_exposed(px - sasa_lane(X, b), py - sasa_lane(Y, b), pz - sasa_lane(Z, b), sasa_lane(r2, b));
                    }
                }
            }
            const u64 open = __ballot(exposed);
            n_exposed += __popcll(open);
            if (grid && open) {
                const bool in = exposed && sasa_inside(px, py, pz, o, h, nx, ny, nz, word);
                n_inside += __popcll(__ballot(in));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // (the next atom's list overwrites this one)
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            counts[D.count_first + i] = n_exposed;
            counts[total + D.count_first + i] = n_inside;
        }
        sum_exposed += n_exposed;
        sum_inside += n_inside;
    }
    pw_sasa_out* row = out + B.job;                                  // (zeroed before the launch)
    if (lane == 0) {
        if (sum_exposed) atomicAdd((unsigned long long*)&row->exposed, (unsigned long long)sum_exposed);
        if (sum_inside) atomicAdd((unsigned long long*)&row->inside, (unsigned long long)sum_inside);
    }
    if (tid == 0 && B.a_begin == 0) row->flags = grid ? SASA_GRID : 0;
}

const char* const ENTRY = "pw_sasa";
int sasa_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

// Everything is checked before anything is launched or written.
int sasa_check(const pw_sasa_job* jobs, long n_jobs, const double* xyz, long n_points, const double* radii, long n_radii,
               const double* directions, long P, const u64* words, long n_words, const int* exposed, const int* inside,
               long n_counts, long n_out) {
    bool directions_checked = false;                                 // (they are the call's: the first job with atoms reads them)
    for (long k = 0; k < n_jobs; ++k) {
        const pw_sasa_job& J = jobs[k];
        const bool grid = J.word_first != -1;
        if (J.n < 0) return sasa_bad(k, "a negative count");
        if (span_outside(J.atom_first, J.n, n_points)) return sasa_bad(k, "atoms outside xyz");
        if (span_outside(J.radius_first, J.n, n_radii)) return sasa_bad(k, "radii outside the array");
        if (span_outside(J.count_first, J.n, n_counts)) return sasa_bad(k, "the counts are outside exposed and inside");
        if (span_outside(J.out, 1, n_out)) return sasa_bad(k, "the row is outside out");
        if (grid) {
            GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
            if (span_outside(J.word_first, (long)J.ny * J.nz, n_words)) return sasa_bad(k, "the words are outside their array");
        }
        if ((J.n && (!xyz || !radii || !exposed || !inside || !directions)) || (grid && !words)) return sasa_bad(k, "null array");
        if (!pw_finite(J.probe)) return sasa_bad(k, "the probe is not finite");
        if (J.probe < 0.0) return sasa_bad(k, "a negative probe");
        if (grid) GRID_CHECK(grid_frame_check(ENTRY, k, J.origin, J.spacing));
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its radius)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_radii_check(ENTRY, k, radii, J.radius_first + a, 1));
        }
        if (J.n && !directions_checked) {
            if (P < 1 || P > SASA_MAX_POINTS)
                return sasa_bad(k, "the number of directions is outside 1 .. PW_SASA_MAX_POINTS (4096)");
            char what[96];
            for (long d = 0; d < P; ++d) {
                const double* u = directions + 3 * d;
                const bool finite = pw_finite(u[0]) && pw_finite(u[1]) && pw_finite(u[2]);
                if (finite && sasa_unit(u[0], u[1], u[2])) continue;
                snprintf(what, sizeof what, finite ? "direction %ld is not a unit vector" : "direction %ld is not finite", d);
                return sasa_bad(k, what);
            }
            directions_checked = true;
        }
    }
    // outputs of two jobs: the later of the two is named.  (Of rows, all of length 1, stat_shared names the second
    // lowest job of a row that is shared, as the sweep over equal neighbours did.  The counts keep their sweep, which
    // orders spans of one first by job where stat_shared orders them by length: with three jobs at one first and the
    // lengths 1, 3, 2 this one names job 1 and stat_shared job 2 -- tests/test_sasa.py holds every such case.)
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    long bad = -1;
    std::vector<std::pair<long, long>> spans;
    for (long k = 0; k < n_jobs; ++k)
        if (jobs[k].n > 0) spans.push_back({(long)jobs[k].count_first, k});
    std::sort(spans.begin(), spans.end());
    long end = -1, owner = -1;                                       // the furthest end so far and the job it belongs to
    for (const auto& s : spans) {
        const long k = s.second, stop = s.first + (long)jobs[k].n;
        if (s.first < end) {
            const long later = k > owner ? k : owner;
            if (bad < 0 || later < bad) bad = later;
        }
        if (stop > end) {
            end = stop;
            owner = k;
        }
    }
    if (bad >= 0) return sasa_bad(bad, "shares entries of exposed and inside with an earlier job");
    return PW_OK;
}

// list_capacity: the entries of a wave's list (0: SASA_LIST_CAP; negative: none, every atom with a near atom takes
// the overflow path; larger values are cut to SASA_LIST_CAP); lds_words: the rows up to which a grid is staged in LDS
// (0: SASA_LDS_WORDS; negative: none; at most 64 * 64); block_atoms: the atoms of a job a workgroup takes (0:
// SASA_BLOCK_ATOMS); kernel_ms: when not null, the time of the kernel by HIP events on the context's stream
int sasa(pw_context* ctx, const pw_sasa_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points, const double* radii,
         int64_t n_radii, const double* directions, int64_t n_directions, const uint64_t* words_, int64_t n_words,
         int32_t* exposed, int32_t* inside, int64_t n_counts, pw_sasa_out* out, int64_t n_out, int64_t list_capacity,
         int64_t lds_words, int64_t block_atoms, float* kernel_ms) {
    const u64* words = (const u64*)words_;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_radii < 0 ||
        n_directions < 0 || n_words < 0 || n_counts < 0 || n_out < 0 || block_atoms < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs, P = (long)n_directions;
    const int rc = sasa_check(jobs, N, xyz, (long)n_points, radii, (long)n_radii, directions, P, words, (long)n_words,
                              exposed, inside, (long)n_counts, (long)n_out);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_sasa(jobs, N, xyz, radii, directions, P, words, exposed, inside, out,
                                pw_context_host_threads(ctx, 0));

    const int cap = list_capacity == 0 ? SASA_LIST_CAP : list_capacity < 0 ? 0 : (int)std::min<int64_t>(list_capacity, SASA_LIST_CAP);
    const long stage = lds_words == 0 ? SASA_LDS_WORDS : lds_words < 0 ? 0 : std::min<long>((long)lds_words, CAVITY_MAX_G * CAVITY_MAX_G);
    const long per_block = block_atoms ? (long)block_atoms : SASA_BLOCK_ATOMS;
    // the spans of the arrays that the jobs read, the compacted counts and the workgroups
    Span atoms, atom_radii, region;
    for (long k = 0; k < N; ++k) {
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        atom_radii.widen((long)jobs[k].radius_first, (long)jobs[k].n);
        if (jobs[k].word_first >= 0) region.widen((long)jobs[k].word_first, (long)jobs[k].ny * jobs[k].nz);
    }
    std::vector<SasaJobDev> devs((size_t)N);
    std::vector<SasaBlock> blocks;
    long total = 0, lds_rows = 0;
    for (long k = 0; k < N; ++k) {
        const pw_sasa_job& J = jobs[k];
        const bool grid = J.word_first >= 0;
        const long rows = grid ? (long)J.ny * J.nz : 0;
        SasaJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.radius_first = atom_radii.rel((long)J.radius_first, (long)J.n);
        D.count_first = total;
        D.word_first = grid ? (long)J.word_first - region.lo : -1;
        for (int a = 0; a < 3; ++a) D.o[a] = grid ? J.origin[a] : 0.0;
        D.h = grid ? J.spacing : 1.0;
        D.probe = J.probe;
        D.slack = J.n ? sasa_slack(sasa_magnitude(xyz + 3 * (long)J.atom_first, radii + (long)J.radius_first, (long)J.n, J.probe)) : -1.0;
        D.nx = grid ? J.nx : 1; D.ny = grid ? J.ny : 1; D.nz = grid ? J.nz : 1;
        D.in_lds = grid && rows <= stage;
        if (D.in_lds) lds_rows = std::max(lds_rows, rows);
        total += (long)J.n;
        blocks.push_back(SasaBlock{k, 0, std::min(per_block, (long)J.n)});           // (a job without atoms: its flags)
        for (long a = per_block; a < (long)J.n; a += per_block) blocks.push_back(SasaBlock{k, a, std::min(a + per_block, (long)J.n)});
    }
    if (blocks.size() > 0x7ffffff0ul) return sasa_bad(0, "more workgroups than a launch holds");
    const long Pd = total ? P : 0;                                   // (no job with atoms: nobody reads them)
    std::vector<double> dirs((size_t)(3 * Pd));                      // transposed: lanes read neighbours
    for (long d = 0; d < Pd; ++d)
        for (int c = 0; c < 3; ++c) dirs[(size_t)(c * Pd + d)] = directions[3 * d + c];

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        SasaBlock* d_blocks;
        SasaJobDev* d_jobs;
        double *d_xyz, *d_radii, *d_dirs;
        u64* d_words;
        int* d_counts;
        pw_sasa_out* d_out;
        const size_t counts_bytes = sizeof(int) * 2 * (size_t)total, out_bytes = sizeof(pw_sasa_out) * (size_t)N;
        STAT_TRY(buf.alloc(&d_blocks, sizeof(SasaBlock) * blocks.size()));
        STAT_TRY(buf.alloc(&d_jobs, sizeof(SasaJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_blocks, blocks.data(), sizeof(SasaBlock) * blocks.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(SasaJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(atom_radii.upload(buf, &d_radii, radii, 1));
        STAT_TRY(buf.alloc(&d_dirs, sizeof(double) * dirs.size()));
        if (Pd) STAT_TRY(hipMemcpyAsync(d_dirs, dirs.data(), sizeof(double) * dirs.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(region.upload(buf, &d_words, words, 1));
        STAT_TRY(buf.alloc(&d_counts, counts_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        STAT_TRY(poison_scratch(scratch_poisoned(), d_counts, counts_bytes, st));    // (test hook, pw_stat_host.hpp)
        STAT_TRY(hipMemsetAsync(d_out, 0, out_bytes, st));           // (the rows are sums by atomics: they start at 0)
        STAT_TRY(ev.start(st));
        hipLaunchKernelGGL(pw_sasa_kernel, dim3((unsigned)blocks.size()), dim3(SASA_THREADS), sasa_lds_bytes(lds_rows), st,
                           d_blocks, d_jobs, d_xyz, d_radii, d_dirs, (int)Pd, d_words, d_counts, total, d_out, cap);
        STAT_TRY(hipGetLastError());
        STAT_TRY(ev.stop(st));
        // (the counts are compacted in job order and the rows are in job order: neighbours in the caller's arrays come
        // back in one copy)
        for (long k = 0; k < N;) {
            if (jobs[k].n == 0) {
                ++k;
                continue;
            }
            long e = k, atoms = (long)jobs[k].n;
            for (long q = k + 1; q < N; ++q) {
                if (jobs[q].n == 0) continue;
                if (jobs[q].count_first != jobs[k].count_first + atoms) break;
                atoms += (long)jobs[q].n;
                e = q;
            }
            // (jobs without atoms between k and e take no room in either layout)
            STAT_TRY(hipMemcpyAsync(exposed + jobs[k].count_first, d_counts + devs[k].count_first, sizeof(int) * (size_t)atoms,
                                    hipMemcpyDeviceToHost, st));
            STAT_TRY(hipMemcpyAsync(inside + jobs[k].count_first, d_counts + total + devs[k].count_first,
                                    sizeof(int) * (size_t)atoms, hipMemcpyDeviceToHost, st));
            k = e + 1;
        }
        for (long k = 0; k < N;) {
            long e = k + 1;
            while (e < N && jobs[e].out == jobs[e - 1].out + 1) ++e;
            STAT_TRY(hipMemcpyAsync(out + jobs[k].out, d_out + k, sizeof(pw_sasa_out) * (size_t)(e - k), hipMemcpyDeviceToHost, st));
            k = e;
        }
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    return PW_OK;
}

}  // namespace

extern "C" int pw_sasa(pw_context* ctx, const pw_sasa_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                       const double* radii, int64_t n_radii, const double* directions, int64_t n_directions,
                       const uint64_t* words, int64_t n_words, int32_t* exposed, int32_t* inside, int64_t n_counts,
                       pw_sasa_out* out, int64_t n_out) {
    return sasa(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, directions, n_directions, words, n_words, exposed, inside,
                n_counts, out, n_out, 0, 0, 0, nullptr);
}

// measurement and test hook (not part of the header): pw_sasa with the kernel's alternative paths forced --
// list_capacity (0: the default; negative: no list at all, so every atom that has a near atom takes the overflow path;
// else the entries of a wave's list, at most the default), lds_words (0: the default; negative: every grid is read
// from global memory; else the rows up to which a grid is staged in LDS), block_atoms (0: the default; else the atoms
// of a job a workgroup takes, so that a job has several workgroups) -- none of which may show in the result; and,
// when kernel_ms is not null, the kernel timed by HIP events
extern "C" int pw_internal_sasa(pw_context* ctx, const pw_sasa_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                                const double* radii, int64_t n_radii, const double* directions, int64_t n_directions,
                                const uint64_t* words, int64_t n_words, int32_t* exposed, int32_t* inside, int64_t n_counts,
                                pw_sasa_out* out, int64_t n_out, int64_t list_capacity, int64_t lds_words,
                                int64_t block_atoms, float* kernel_ms) {
    return sasa(ctx, jobs, n_jobs, xyz, n_points, radii, n_radii, directions, n_directions, words, n_words, exposed, inside,
                n_counts, out, n_out, list_capacity, lds_words, block_atoms, kernel_ms);
}
