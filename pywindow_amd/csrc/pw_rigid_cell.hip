// pw_rigid_cell.hip -- gfx950 kernels and the C ABI entry of the orientation-averaged Boltzmann factor of a rigid linear
// guest at every voxel of a periodic cell (include/pywindow_amd.h: pw_rigid_cell; definition of the result, the skip and
// its proof in pw_rigid_cell.hpp), and of the same field with the Ewald sum of the framework's point charges
// (pw_rigid_cell_ewald; definition in pw_ewald.hpp, the two kernels of its reciprocal part in pw_ewald.hip, launched ahead
// of the main kernel, which is instantiated a second time for rows of three doubles).  Three kernels a launch group:
//   main     a work item is (job, group of 4 x 4 x 4 voxels), one wavefront an item, a lane a voxel.  Instantiated on the
//            number of sites as pw_rigid_kernel is (1, 2, 3, and a guarded form unrolled to 8 that serves 4 .. 8), so
//            that every per-site and per-orientation value has a register of its own: nothing private is indexed at run
//            time.  The job's directions (dynamic LDS, 24 bytes each) and offsets live in LDS.  THE NEAR LIST: the wave
//            goes over the job's atoms 64 at a time, a lane an atom, tests rcell_far against the group's centre and
//            compacts the survivors' indices into LDS by __ballot and a popcount of the lanes below, so the list is in
//            index order.  The survivors are staged AFF_TILE at a time with their S rows -- once an item when they fit
//            one tile, once per pass of RB orientations otherwise -- and per staged atom all S sites of RB orientations
//            are evaluated from one read of the atom.  A list that would outgrow RCELL_NEAR_CAP ends early; the wave then
//            takes the atoms segment by segment, rebuilding the list of a segment in every pass: every accumulator still
//            takes its terms in index order.  The lane writes its voxel's record (pw_rigid_cell.hpp).
//   sums     a work item is (job, chunk of 64 ranks): pw_rigid_kernel's end on the records -- the chunk tree with
//            __shfl_down, the minimum down the same tree with a strict <, the dead voxels by a popcount of __ballot --,
//            lane 0 writes the chunk's partial.
//   reduce   a wavefront a job, one lane a series of the partial.
// Every loop is bounded by n, M, the items, L or a constant; a workgroup is one wavefront and every barrier is reached
// with values that __ballot or the job made the same in every lane; nothing spins, no workgroup waits for another, no
// floating-point atomics (n_pairs, a diagnostic, is an integer atomic).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_affinity_dev.hpp"
#include "pw_ewald_dev.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_rigid_cell(const pw_rigid_cell_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                      const double* offsets, const double* dirs, const double* betas, double* maps,
                                      pw_affinity_level* levels, pw_rigid_out* out, long long* n_pairs, int skip,
                                      int threads, const EwaldHost* ew);   // pw_hostpath.cpp

static_assert(sizeof(pw_rigid_cell_job) == 200 && sizeof(pw_rigid_out) == 56 && sizeof(pw_rigid_cell_ewald_job) == 256,
              "the layouts of the header");
static_assert(RCELL_G * RCELL_G * RCELL_G == AFF_CHUNK && RCELL_NEAR_CAP % AFF_CHUNK == 0, "a group is a wavefront");

namespace {

typedef cavity_word u64;

constexpr int RCELL_RB = 2;                          // orientations held in registers at a time, S <= 3
constexpr int RCELL_CLASSES = 4;                     // 1, 2, 3, guarded 8

int rcell_class(int S) { return S <= 3 ? S - 1 : 3; }

// S_T sites unrolled; GUARD: the job has J.S <= S_T of them and every site is behind `s < S`; RB orientations a pass; W
// doubles a row of coef: 2 is pw_rigid_cell, 3 is pw_rigid_cell_ewald, whose charged jobs take pw_ewald.hpp's pair term
// behind a branch that is the same in every lane and add Urec from the workspace to the pose's energy
template <int S_T, bool GUARD, int RB, int W>
__global__ void __launch_bounds__(AFF_CHUNK)
pw_rigid_cell_kernel(const RCellJobDev* __restrict__ jobs, int n_jobs, long total, int cls, const double* __restrict__ xyz,
                     const double* __restrict__ coef, const double* __restrict__ offsets, const double* __restrict__ dirs,
                     const double* __restrict__ betas, u64* __restrict__ ws, unsigned long long* __restrict__ n_pairs) {
    __shared__ double s_xyz[3 * AFF_TILE];
    __shared__ double s_coef[W * S_T * AFF_TILE];                    // row (atom t, site s) at W * (t * S_T + s)
    __shared__ double s_off[RIGID_MAX_SITES];
    __shared__ int s_near[RCELL_NEAR_CAP];                           // the near list: atom indices of the job, ascending
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    extern __shared__ double s_dir[];                                // 3 M doubles: the launch sizes it for its largest M
    const int lane = threadIdx.x;
    const u64 below = (1ull << lane) - 1ull;
    for (int t = lane; t < 256; t += AFF_CHUNK) s_tab[t] = POW_EXP_TAB[t];
    for (long item = blockIdx.x; item < total; item += gridDim.x) {      // (the items of the launch)
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].item_first; });
        const RCellJobDev& J = jobs[k];
        if (J.cls != cls) continue;                                  // (the same in every lane: another instance's item)
        const long g = item - J.item_first, grow = g / J.gx;
        const int i0 = RCELL_G * (int)(g - grow * J.gx), j0 = RCELL_G * (int)(grow % J.gy), l0 = RCELL_G * (int)(grow / J.gy);
        const int nx = J.nx, ny = J.ny, L = J.L, M = J.M, S = GUARD ? J.S : S_T;
        const int i = i0 + (lane & 3), j = j0 + ((lane >> 2) & 3), l = l0 + (lane >> 4);
        const bool valid = i < nx && j < ny && l < J.nz;
        // (a lane without a voxel computes the group's first voxel and writes nothing)
        const int iv = valid ? i : i0, jv = valid ? j : j0, lv = valid ? l : l0;
        const double x = channels_x(J.o[0], iv, J.s[0], jv, J.s[1], lv, J.s[3]), y = channels_y(J.o[1], jv, J.s[2], lv, J.s[4]),
                     z = channels_z(J.o[2], lv, J.s[5]);
        const double gcx = rcell_centre_x(J.o, J.s, i0, j0, l0), gcy = rcell_centre_y(J.o, J.s, j0, l0),
                     gcz = rcell_centre_z(J.o, J.s, l0);
        const double core2 = J.core2, cutoff2 = J.cutoff2, reach2 = J.reach2, inv_M = rigid_inv(M);
        const long n = J.n;
        const double* atoms = xyz + 3 * J.atom_first;
        const double* rows_ab = coef + W * J.coef_first;
        const bool charged = W == 3 && J.charged != 0;               // (the same in every lane)
        const double alpha = J.alpha;
        const double* urec = charged && J.urec_first >= 0 ? (const double*)(ws + J.urec_first) : nullptr;
        // the near list of the atoms from `a` on, until they end or the list is full; the first atom it did not look at.
        // The caller puts the barriers around it.  count is the same in every lane
        auto build = [&](long a, int& count) {
            count = 0;
            long base = a;
            for (; base < n && count + AFF_CHUNK <= RCELL_NEAR_CAP; base += AFF_CHUNK) {   // (at most n / 64 + 1 turns)
                const long idx = base + lane;
                const bool keep = idx < n && !rcell_far(gcx, gcy, gcz, atoms[3 * idx], atoms[3 * idx + 1], atoms[3 * idx + 2], reach2);
                const u64 m = __ballot(keep);
                if (keep) s_near[count + cavity_popcount(m & below)] = (int)idx;
                count += cavity_popcount(m);
            }
            return base < n ? base : n;
        };
        // the survivors [q0, q0 + len) of the list and their S rows into LDS; the caller puts the barriers around it
        auto stage = [&](int q0, int len) {
            for (int t = lane; t < len; t += AFF_CHUNK) {            // (len <= AFF_TILE: two turns)
                const long idx = s_near[q0 + t];
                s_xyz[3 * t] = atoms[3 * idx];
                s_xyz[3 * t + 1] = atoms[3 * idx + 1];
                s_xyz[3 * t + 2] = atoms[3 * idx + 2];
#pragma unroll
                for (int s = 0; s < S_T; ++s) {
                    if (GUARD && s >= S) continue;
                    const double* src = rows_ab + W * ((long)s * n + idx);
                    s_coef[W * (t * S_T + s)] = src[0];
                    s_coef[W * (t * S_T + s) + 1] = src[1];
                    if (W == 3 && charged) s_coef[W * (t * S_T + s) + 2] = src[2];
                }
            }
        };
        __syncthreads();                                             // (the item before is done with the LDS)
        for (int t = lane; t < 3 * M; t += AFF_CHUNK) s_dir[t] = dirs[3 * J.dir_first + t];
        if (lane < S) s_off[lane] = offsets[J.site_first + lane];
        int count = 0;
        const long after = build(0, count);
        const bool single = after >= n;                              // the list holds every survivor of the job's atoms
        const bool once = single && count <= AFF_TILE;
        __syncthreads();
        if (once) {
            stage(0, count);
            __syncthreads();
        }
        long survivors = single ? count : 0;

        RigidFold fold[AFF_MAX_LEVELS];                              // (indexed by unrolled loops only: registers)
        double umin_v = aff_inf();
        int umin_o = -1, n_blocked = 0;
        bool clamped = false;
        for (int o0 = 0; o0 < M; o0 += RB) {                             // (the orientations, RB a pass)
            double px[RB][S_T], py[RB][S_T], pz[RB][S_T], U[RB][S_T];
            bool blocked[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int o = o0 + r < M ? o0 + r : M - 1;           // (past the end: the last one again, not used below)
                blocked[r] = false;
#pragma unroll
                for (int s = 0; s < S_T; ++s) {
                    U[r][s] = 0.0;
                    px[r][s] = py[r][s] = pz[r][s] = 0.0;
                    if (!GUARD || s < S) {
                        px[r][s] = rigid_site(x, s_off[s], s_dir[3 * o]);
                        py[r][s] = rigid_site(y, s_off[s], s_dir[3 * o + 1]);
                        pz[r][s] = rigid_site(z, s_off[s], s_dir[3 * o + 2]);
                    }
                }
            }
            long a = 0, next = after;
            int len_list = count;
            do {                                                     // (the segments: one when `single`; each takes 64 atoms or more)
                if (!single) {
                    __syncthreads();                                 // (the list of the segment before is done with)
                    next = build(a, len_list);
                    __syncthreads();
                    if (o0 == 0) survivors += len_list;
                }
                for (int q0 = 0; q0 < len_list; q0 += AFF_TILE) {        // (the tiles of the list)
                    const int len = len_list - q0 < AFF_TILE ? len_list - q0 : AFF_TILE;
                    if (!once) {
                        __syncthreads();                             // (the atoms staged before are done with)
                        stage(q0, len);
                        __syncthreads();
                    }
                    for (int t = 0; t < len; ++t) {
                        const double X = s_xyz[3 * t], Y = s_xyz[3 * t + 1], Z = s_xyz[3 * t + 2];
#pragma unroll
                        for (int s = 0; s < S_T; ++s) {
                            if (GUARD && s >= S) continue;
                            const double A = s_coef[W * (t * S_T + s)], B = s_coef[W * (t * S_T + s) + 1];
                            const double C = W == 3 && charged ? s_coef[W * (t * S_T + s) + 2] : 0.0;
#pragma unroll
                            for (int r = 0; r < RB; ++r) {
                                const double r2 = aff_r2(px[r][s] - X, py[r][s] - Y, pz[r][s] - Z);
                                blocked[r] = blocked[r] || aff_blocked(r2, core2);
                                double u = aff_pair(r2, A, B);
                                if (W == 3 && charged) {
                                    // (only a counting atom: alpha * r stays within the cutoff, the branch follows the lanes)
                                    if (aff_counts(r2, cutoff2)) U[r][s] = U[r][s] + ewald_pair(u, r2, C, alpha, s_tab);
                                } else {
                                    U[r][s] = aff_counts(r2, cutoff2) ? U[r][s] + u : U[r][s];
                                }
                            }
                        }
                    }
                }
                a = next;
            } while (a < n);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (o0 + r >= M) continue;                           // (the same in every lane)
                double Ut = U[r][0];
#pragma unroll
                for (int s = 1; s < S_T; ++s)
                    if (!GUARD || s < S) Ut = Ut + U[r][s];
                if (W == 3 && urec) Ut = Ut + urec[(long)(o0 + r) * J.V + ((long)(lv * ny + jv) * nx + iv)];
                const bool live = !blocked[r];
                n_blocked += blocked[r];
                if (live && Ut < umin_v) {
                    umin_v = Ut;
                    umin_o = o0 + r;
                }
#pragma unroll
                for (int b = 0; b < AFF_MAX_LEVELS; ++b) {
                    if (b >= L) continue;
                    bool over = false;
                    const double w = aff_weight(betas[J.beta_first + b], Ut, s_tab, over);
                    clamped = clamped || (live && over);
                    if (live) fold[b].add(w, Ut);
                }
            }
        }

        if (valid) {
            u64* rec = ws + J.rec_first + ((long)(l * ny + j) * nx + i);
#pragma unroll
            for (int b = 0; b < AFF_MAX_LEVELS; ++b) {
                if (b >= L) continue;
                rec[(long)b * J.V] = pw_d2bits(fold[b].zbar(inv_M));
                rec[(long)(L + 1 + b) * J.V] = pw_d2bits(fold[b].ebar(inv_M));
            }
            rec[(long)L * J.V] = pw_d2bits(umin_v);
            rec[(long)(2 * L + 1) * J.V] = rcell_info(n_blocked, clamped, umin_o);
        }
        const int n_valid = cavity_popcount(__ballot(valid));
        if (lane == 0) atomicAdd(n_pairs + k, (unsigned long long)(survivors * M * S * n_valid));
    }
}

__global__ void __launch_bounds__(AFF_CHUNK)
pw_rigid_cell_sums_kernel(const RCellJobDev* __restrict__ jobs, int n_jobs, long total, u64* __restrict__ ws) {
    const int lane = threadIdx.x;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {      // (the chunks of the launch)
        const int k = stat_find(n_jobs, item, [&](int q) { return jobs[q].chunk_first; });
        const RCellJobDev& J = jobs[k];
        const long chunk = item - J.chunk_first, rank = chunk * AFF_CHUNK + lane;
        const bool valid = rank < J.V;
        const int L = J.L;
        const u64* rec = ws + J.rec_first + (valid ? rank : 0);
        u64* part = ws + J.part_first + chunk * rigid_part_words(L);
        for (int b = 0; b < L; ++b) {                                    // (the levels)
            double sz = valid ? pw_bits2d(rec[(long)b * J.V]) : 0.0, se = valid ? pw_bits2d(rec[(long)(L + 1 + b) * J.V]) : 0.0;
            for (int s = 1; s < AFF_CHUNK; s <<= 1) {
                sz = sz + __shfl_down(sz, s);
                se = se + __shfl_down(se, s);
            }
            if (lane == 0) {
                part[2 * b] = pw_d2bits(sz);
                part[2 * b + 1] = pw_d2bits(se);
            }
        }
        const u64 info = valid ? rec[(long)(2 * L + 1) * J.V] : 0ull;
        double m = valid ? pw_bits2d(rec[(long)L * J.V]) : aff_inf();
        int m_lane = lane, m_o = rcell_info_dir(info), n_blocked = rcell_info_blocked(info);
        const bool dead_v = valid && m_o < 0;
        for (int s = 1; s < AFF_CHUNK; s <<= 1) {
            const double other = __shfl_down(m, s);
            const int other_lane = __shfl_down(m_lane, s), other_o = __shfl_down(m_o, s);
            n_blocked += __shfl_down(n_blocked, s);                  // (integers: lane 0 ends with the wave's total)
            if (other < m) {
                m = other;
                m_lane = other_lane;
                m_o = other_o;
            }
        }
        const u64 any_clamped = __ballot(rcell_info_clamped(info)), dead = __ballot(dead_v);
        if (lane == 0) {
            part[2 * L] = pw_d2bits(m);
            part[2 * L + 1] = (u64)(chunk * AFF_CHUNK + m_lane);
            part[2 * L + 2] = (u64)(long)m_o;
            part[2 * L + 3] = (u64)n_blocked;
            part[2 * L + 4] = (u64)cavity_popcount(dead);
            part[2 * L + 5] = any_clamped ? (u64)AFF_CLAMPED : 0ull;
        }
    }
}

__global__ void __launch_bounds__(AFF_CHUNK)
pw_rigid_cell_reduce_kernel(const RCellJobDev* __restrict__ jobs, const u64* __restrict__ ws, pw_rigid_out* __restrict__ out,
                            double* __restrict__ levels) {
    const RCellJobDev& J = jobs[blockIdx.x];
    const int t = threadIdx.x, L = J.L, stride = rigid_part_words(L);
    if (t >= stride || t == 2 * L + 1 || t == 2 * L + 2) return;     // (rank and direction go with the minimum)
    const u64* p = ws + J.part_first + t;
    pw_rigid_out& O = out[blockIdx.x];
    if (t < 2 * L) {
        double s = 0.0;
        for (long c = 0; c < J.chunks; ++c) s = s + pw_bits2d(p[c * stride]);
        levels[2 * J.level_first + t] = s;
    } else if (t == 2 * L) {
        double m = aff_inf();
        long rank = -1, dir = -1;
        for (long c = 0; c < J.chunks; ++c) {
            const double v = pw_bits2d(p[c * stride]);
            if (v < m) {
                m = v;
                rank = (long)p[c * stride + 1];
                dir = (long)p[c * stride + 2];
            }
        }
        const long row = rank >= 0 ? rank / J.nx : 0;
        O.u_min = m;
        O.min_voxel[0] = rank >= 0 ? (int)(rank - row * J.nx) : -1;
        O.min_voxel[1] = rank >= 0 ? (int)(row % J.ny) : -1;
        O.min_voxel[2] = rank >= 0 ? (int)(row / J.ny) : -1;
        O.min_dir = (int)dir;
    } else {
        unsigned long long s = 0;
        const bool flags = t == 2 * L + 5;
        for (long c = 0; c < J.chunks; ++c) s = flags ? s | p[c * stride] : s + p[c * stride];
        if (t == 2 * L + 3) {
            O.n_voxels = J.V;
            O.n_blocked_poses = (long)s;
        } else if (t == 2 * L + 4) {
            O.n_dead = (long)s;
        } else {
            O.flags = (int)s;
            O.reserved = 0;
        }
    }
}

// one instance over the items of a launch group; `lds`: the bytes of the directions of the group's largest M
void rcell_launch(int cls, bool wide, unsigned blocks, size_t lds, hipStream_t st, const RCellJobDev* jobs, int n_jobs,
                  long total, const double* xyz, const double* coef, const double* offsets, const double* dirs, const double* betas, u64* ws,
                  unsigned long long* n_pairs) {
#define RCELL_GO_W(S_T, GUARD, RB, W)                                                                                  \
    hipLaunchKernelGGL((pw_rigid_cell_kernel<S_T, GUARD, RB, W>), dim3(blocks), dim3(AFF_CHUNK), lds, st, jobs, n_jobs,  \
                       total, cls, xyz, coef, offsets, dirs, betas, ws, n_pairs)
#define RCELL_GO(S_T, GUARD, RB)                 \
    do {                                         \
        if (wide) RCELL_GO_W(S_T, GUARD, RB, 3); \
        else RCELL_GO_W(S_T, GUARD, RB, 2);      \
    } while (0)
    switch (cls) {
        case 0: RCELL_GO(1, false, RCELL_RB); break;
        case 1: RCELL_GO(2, false, RCELL_RB); break;
        case 2: RCELL_GO(3, false, RCELL_RB); break;
        default: RCELL_GO(RIGID_MAX_SITES, true, 1); break;
    }
#undef RCELL_GO
#undef RCELL_GO_W
}

// what pw_rigid_cell_ewald hands over beyond pw_rigid_cell's arguments; null for pw_rigid_cell
struct EwaldArgs {
    const pw_rigid_cell_ewald_job* jobs;
    const double *site_q, *cell, *kvecs;
    long n_site_q, n_cell, n_kvecs;
};

inline long rcell_voxels(const pw_rigid_cell_job& J) { return (long)J.nx * J.ny * J.nz; }
inline long rcell_map_words(const pw_rigid_cell_job& J) { return J.map_first >= 0 ? (J.n_betas + 1) * rcell_voxels(J) : 0; }

// Everything is checked before anything is launched or written
int rcell_check(const char* ENTRY, int W, const pw_rigid_cell_job* jobs, long n_jobs, const double* xyz, long n_points,
                const double* coef, long n_coef, const double* offsets, long n_offsets, const double* dirs, long n_dirs,
                const double* betas, long n_betas, const double* maps, long n_maps, const pw_affinity_level* levels, long n_levels,
                long n_out, const EwaldArgs* ew) {
    auto rcell_bad = [&](long k, const char* what) { return stat_bad(ENTRY, k, what); };
    for (long k = 0; k < n_jobs; ++k) {
        const pw_rigid_cell_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        const long L = (long)J.n_betas, S = (long)J.n_sites, M = (long)J.n_dirs;
        if (J.n < 0) return rcell_bad(k, "a negative count");
        if (J.n > 0x7fffffffl) return rcell_bad(k, "more than 2^31 - 1 atoms");
        GRID_CHECK(grid_n_betas_check(ENTRY, k, L));
        if (S < 1 || S > RIGID_MAX_SITES) return rcell_bad(k, "n_sites outside 1 .. PW_RIGID_MAX_SITES (8)");
        if (M < 1 || M > RIGID_MAX_DIRS) return rcell_bad(k, "n_dirs outside 1 .. PW_RIGID_MAX_DIRS (1024)");
        if (span_outside(J.atom_first, J.n, n_points)) return rcell_bad(k, "atoms outside xyz");
        if (span_outside(J.coef_first, S * J.n, n_coef)) return rcell_bad(k, "coefficients outside coef");   // (n < 2^31: no overflow)
        if (span_outside(J.site_first, S, n_offsets)) return rcell_bad(k, "sites outside offsets");
        if (span_outside(J.dir_first, M, n_dirs)) return rcell_bad(k, "directions outside dirs");
        if (span_outside(J.beta_first, L, n_betas)) return rcell_bad(k, "betas outside the array");
        if (span_outside(J.level_first, L, n_levels)) return rcell_bad(k, "the rows are outside levels");
        if (span_outside(J.out, 1, n_out)) return rcell_bad(k, "the row is outside out");
        if (J.map_first < -1 || (J.map_first >= 0 && span_outside(J.map_first, rcell_map_words(J), n_maps)))
            return rcell_bad(k, "the maps are outside their array");
        if ((J.n && (!xyz || !coef)) || !betas || !offsets || !dirs || !levels || (J.map_first >= 0 && !maps))
            return rcell_bad(k, "null array");
        bool finite = true;
        for (int a = 0; a < 3; ++a) finite = finite && pw_finite(J.origin[a]);
        for (int a = 0; a < 6; ++a) finite = finite && pw_finite(J.step[a]);
        if (!finite) return rcell_bad(k, "the origin or a step is not finite");
        if (!(J.step[0] > 0.0 && J.step[2] > 0.0 && J.step[5] > 0.0)) return rcell_bad(k, "ax, by or cz <= 0");
        if (J.cutoff2 == 0.0) return rcell_bad(k, "cutoff2 is 0: a cell has no \"no cutoff\"");
        GRID_CHECK(grid_core_check(ENTRY, k, J.core2, J.cutoff2));
        GRID_CHECK(grid_betas_check(ENTRY, k, betas, J.beta_first, L));
        for (long s = 0; s < S; ++s) {
            const double t = offsets[J.site_first + s];
            if (!pw_finite(t) || pw_abs(t) > RIGID_MAX_OFFSET) return rcell_bad(k, "an offset is not finite or beyond 16");
        }
        for (long c = 0; c < 3 * M; ++c) {
            const double d = dirs[3 * J.dir_first + c];
            if (!pw_finite(d) || pw_abs(d) > 1.0) return rcell_bad(k, "a direction's component is not finite or outside -1 .. 1");
        }
        GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first, J.n));   // (every coordinate, then every row)
        const bool charged = ew && ew->jobs[k].charged != 0;
        GRID_CHECK(grid_coef_check(ENTRY, k, coef, J.coef_first, S * J.n, W, charged));
        if (!ew) continue;
        const pw_rigid_cell_ewald_job& E = ew->jobs[k];
        if (E.charged != 0 && E.charged != 1) return rcell_bad(k, "charged is neither 0 nor 1");
        if (!charged) continue;                                      // (nothing else of the job is read)
        if (!pw_finite(E.alpha)) return rcell_bad(k, "alpha is not finite");
        if (E.alpha < 0.0) return rcell_bad(k, "alpha < 0");
        if (E.n_k < 0 || E.n_k > EWALD_MAX_K) return rcell_bad(k, "n_k outside 0 .. PW_EWALD_MAX_K (4096)");
        if (E.n_cell < 0 || E.n_cell > 0x7fffffffl) return rcell_bad(k, "n_cell is negative or above 2^31 - 1");
        if (span_outside(E.charge_first, S, ew->n_site_q)) return rcell_bad(k, "site charges outside site_q");
        if (span_outside(E.cell_first, E.n_cell, ew->n_cell)) return rcell_bad(k, "cell atoms outside cell");
        if (span_outside(E.k_first, E.n_k, ew->n_kvecs)) return rcell_bad(k, "rows outside kvecs");
        if (!ew->site_q || (E.n_cell && !ew->cell) || (E.n_k && !ew->kvecs)) return rcell_bad(k, "null array");
        for (long s = 0; s < S; ++s) {
            const double q = ew->site_q[E.charge_first + s];
            if (!pw_finite(q) || pw_abs(q) > AFF_MAX_COEF) return rcell_bad(k, "a site charge is not finite or beyond 1e100");
        }
        for (long c = 4 * E.cell_first; c < 4 * (E.cell_first + E.n_cell); ++c)
            if (!pw_finite(ew->cell[c]) || pw_abs(ew->cell[c]) > AFF_MAX_COEF)
                return rcell_bad(k, "a cell atom's coordinate or charge is not finite or beyond 1e100");
        for (long r = E.k_first; r < E.k_first + E.n_k; ++r) {
            const double* kv = ew->kvecs + 4 * r;
            for (int a = 0; a < 3; ++a)
                if (!pw_finite(kv[a]) || pw_abs(kv[a]) > (double)EWALD_MAX_INDEX || kv[a] != (double)(int)kv[a])
                    return rcell_bad(k, "an index of a row is not an integer within -PW_EWALD_MAX_INDEX .. PW_EWALD_MAX_INDEX (64)");
            if (!pw_finite(kv[3])) return rcell_bad(k, "a weight is not finite");
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of levels with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].level_first, (long)jobs[k].n_betas}; }));
    return shared_output(ENTRY, n_jobs, "shares maps with an earlier job",
                         [&](long k) { return OutSpan{(long)jobs[k].map_first, rcell_map_words(jobs[k])}; });
}

// workspace_bytes: the budget of the records and partials of the jobs of one launch (0: RCELL_WORKSPACE_BYTES; at 1 every
// job is a launch of its own); kernel_ms: when not null, the time of the device work of the call from the first launch to
// the last, the copies between them included, by HIP events on the context's stream; n_pairs: when not null, per job the
// pair terms that were evaluated (diagnostic: the paths differ); skip: 0 hands the kernels a reach of +inf, so that no
// atom is left out; instances: when not null, bit c is set iff instance c (1, 2, 3 sites, guarded) was launched
int rigid_cell(pw_context* ctx, const pw_rigid_cell_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
               const double* coef, int64_t n_coef, const double* offsets, int64_t n_offsets, const double* dirs, int64_t n_dirs,
               const double* betas, int64_t n_betas, double* maps, int64_t n_maps, pw_affinity_level* levels, int64_t n_levels,
               pw_rigid_out* out, int64_t n_out, int64_t workspace_bytes, float* kernel_ms, int64_t* n_pairs, int skip,
               int32_t* instances, const char* ENTRY = "pw_rigid_cell", const EwaldArgs* ew = nullptr) {
    const int W = ew ? 3 : 2;
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 || n_offsets < 0 ||
        n_dirs < 0 || n_betas < 0 || n_maps < 0 || n_levels < 0 || n_out < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (instances) *instances = 0;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = rcell_check(ENTRY, W, jobs, N, xyz, (long)n_points, coef, (long)n_coef, offsets, (long)n_offsets, dirs,
                               (long)n_dirs, betas, (long)n_betas, maps, (long)n_maps, levels, (long)n_levels, (long)n_out, ew);
    if (rc != PW_OK) return rc;
    std::vector<EwaldHostJob> ew_jobs((size_t)(ew ? N : 0));
    for (long k = 0; ew && k < N; ++k) {
        const pw_rigid_cell_ewald_job& E = ew->jobs[k];
        ew_jobs[k] = EwaldHostJob{(long)E.charge_first, (long)E.cell_first, (long)E.n_cell, (long)E.k_first, (long)E.n_k, E.alpha,
                                  E.charged};
    }
    if (pw_context_device(ctx) < 0) {
        const EwaldHost host{ew_jobs.data(), ew ? ew->site_q : nullptr, ew ? ew->cell : nullptr, ew ? ew->kvecs : nullptr};
        return pw_hostpath_rigid_cell(jobs, N, xyz, coef, offsets, dirs, betas, maps, levels, out, (long long*)n_pairs, skip,
                                      pw_context_host_threads(ctx, 0), ew ? &host : nullptr);
    }

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // records and partials fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : RCELL_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab, beta_span, site_span, dir_span, q_span, cell_span, k_span;
    for (long k = 0; k < N; ++k) {
        const pw_rigid_cell_job& J = jobs[k];
        atoms.widen((long)J.atom_first, (long)J.n);
        rows_ab.widen((long)J.coef_first, (long)J.n_sites * (long)J.n);
        beta_span.widen((long)J.beta_first, (long)J.n_betas);
        site_span.widen((long)J.site_first, (long)J.n_sites);
        dir_span.widen((long)J.dir_first, (long)J.n_dirs);
        if (!ew || !ew_jobs[k].charged) continue;
        q_span.widen(ew_jobs[k].charge_first, (long)J.n_sites);
        cell_span.widen(ew_jobs[k].cell_first, ew_jobs[k].n_cell);
        k_span.widen(ew_jobs[k].k_first, ew_jobs[k].n_k);
    }
    // betas, offsets and directions travel as one array (every job has some of each: the three spans have a lo), and
    // behind them what the charged jobs read: site charges, cell atoms and rows (h, k, l, w)
    const long n_beta_span = beta_span.count(), n_site_span = site_span.count(), n_dir_span = dir_span.count();
    const long n_q_span = q_span.count(), n_cell_span = cell_span.count(), n_k_span = k_span.count();
    const long q_at = n_beta_span + n_site_span + 3 * n_dir_span, cell_at = q_at + n_q_span, k_at = cell_at + 4 * n_cell_span;
    std::vector<double> params((size_t)(k_at + 4 * n_k_span));
    if (n_q_span) memcpy(params.data() + q_at, ew->site_q + q_span.lo, sizeof(double) * (size_t)n_q_span);
    if (n_cell_span) memcpy(params.data() + cell_at, ew->cell + 4 * cell_span.lo, sizeof(double) * 4 * (size_t)n_cell_span);
    if (n_k_span) memcpy(params.data() + k_at, ew->kvecs + 4 * k_span.lo, sizeof(double) * 4 * (size_t)n_k_span);
    memcpy(params.data(), betas + beta_span.lo, sizeof(double) * (size_t)n_beta_span);
    memcpy(params.data() + n_beta_span, offsets + site_span.lo, sizeof(double) * (size_t)n_site_span);
    memcpy(params.data() + n_beta_span + n_site_span, dirs + 3 * dir_span.lo, sizeof(double) * 3 * (size_t)n_dir_span);

    std::vector<RCellJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    long n_level_rows = 0, tiles = 0;                                // tiles: the items of the Urec kernel in `cur` so far
    for (long k = 0; k < N; ++k) {
        const pw_rigid_cell_job& J = jobs[k];
        const long L = (long)J.n_betas, V = rcell_voxels(J), chunks = (V + AFF_CHUNK - 1) / AFF_CHUNK;
        const long gx = rcell_groups(J.nx), gy = rcell_groups(J.ny), gz = rcell_groups(J.nz);
        const long rec_words = rcell_record_words(V, (int)L), part_words = chunks * rigid_part_words((int)L);
        const bool charged = ew && ew_jobs[k].charged;
        const long K = charged ? ew_jobs[k].n_k : 0, M = (long)J.n_dirs;
        const long table_words = K ? ewald_table_words(K, M) : 0, urec_words = K ? ewald_urec_words(V, M) : 0;
        const long need = rec_words + part_words + table_words + urec_words;
        place(groups, cur, budget_words, need);
        if (cur.last == cur.first) tiles = 0;                        // (a group was opened)
        RCellJobDev& D = devs[k];
        D.atom_first = atoms.rel((long)J.atom_first, (long)J.n);
        D.n = (long)J.n;
        D.coef_first = rows_ab.rel((long)J.coef_first, (long)J.n);
        D.rec_first = cur.words;
        D.part_first = cur.words + rec_words;
        D.table_first = cur.words + rec_words + part_words;
        D.urec_first = K ? D.table_first + table_words : -1;
        D.krow_first = cur.rows;                                     // (LaunchGroup's rows: the rows of the group's tables kernel)
        D.tile_first = tiles;
        D.charged = charged ? 1 : 0;
        D.alpha = charged ? ew_jobs[k].alpha : 0.0;
        D.q_first = charged ? ew_jobs[k].charge_first - q_span.lo_or_zero() : 0;
        D.cell_first = charged ? cell_span.rel(ew_jobs[k].cell_first, ew_jobs[k].n_cell) : 0;
        D.n_cell = charged ? ew_jobs[k].n_cell : 0;
        D.k_first = charged ? k_span.rel(ew_jobs[k].k_first, K) : 0;
        D.K = K;
        D.item_first = cur.items;
        D.chunk_first = cur.blocks;
        D.chunks = chunks;
        D.V = V;
        D.beta_first = (long)J.beta_first - beta_span.lo;
        D.site_first = (long)J.site_first - site_span.lo;
        D.dir_first = (long)J.dir_first - dir_span.lo;
        D.level_first = n_level_rows;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        for (int a = 0; a < 6; ++a) D.s[a] = J.step[a];
        D.core2 = J.core2; D.cutoff2 = J.cutoff2;
        D.reach2 = rcell_reach2(J.origin, J.step, J.cutoff2, offsets + J.site_first, (int)J.n_sites, dirs + 3 * J.dir_first,
                                (int)J.n_dirs, skip != 0);
        D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.gx = (int)gx; D.gy = (int)gy; D.L = (int)L; D.S = (int)J.n_sites; D.M = (int)J.n_dirs;
        D.cls = rcell_class((int)J.n_sites);
        n_level_rows += L;
        cur.words += need; cur.cost += need; cur.items += gx * gy * gz; cur.blocks += chunks; cur.last += 1;
        cur.rows += K;
        tiles += K ? gx * gy * gz * ((M + EWALD_OT - 1) / EWALD_OT) : 0;
    }
    groups.push_back(cur);

    // the compact result of the call: the rows of out in job order, then the rows of levels
    const size_t out_bytes = sizeof(pw_rigid_out) * (size_t)N, levels_bytes = sizeof(pw_affinity_level) * (size_t)n_level_rows,
                 res_bytes = out_bytes + levels_bytes, ws_bytes = sizeof(u64) * (size_t)most_words(groups),
                 pairs_bytes = sizeof(unsigned long long) * (size_t)N;
    std::vector<unsigned char> res(res_bytes);
    std::vector<unsigned long long> pairs((size_t)N);
    int ran = 0;

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        RCellJobDev* d_jobs;
        double *d_xyz, *d_coef, *d_params;
        u64* d_ws;
        unsigned long long* d_pairs;
        unsigned char* d_res;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(RCellJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(RCellJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, W));
        STAT_TRY(buf.alloc(&d_params, sizeof(double) * params.size()));
        STAT_TRY(hipMemcpyAsync(d_params, params.data(), sizeof(double) * params.size(), hipMemcpyHostToDevice, st));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_res, res_bytes));
        STAT_TRY(buf.alloc(&d_pairs, pairs_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_res, res_bytes, st));
        STAT_TRY(hipMemsetAsync(d_pairs, 0, pairs_bytes, st));
        pw_rigid_out* d_out = (pw_rigid_out*)d_res;
        double* d_levels = (double*)(d_res + out_bytes);
        const double *d_betas = d_params, *d_offsets = d_params + n_beta_span, *d_dirs = d_params + n_beta_span + n_site_span;
        STAT_TRY(ev.start(st));
        // (launches follow one another on the stream, so the next one takes the workspace over when this one is done and
        // its maps are on their way)
        for (const LaunchGroup& G : groups) {
            const unsigned n_group = (unsigned)(G.last - G.first);
            bool needed[RCELL_CLASSES] = {};
            int max_M = 1;
            for (long k = G.first; k < G.last; ++k) {
                needed[devs[k].cls] = true;
                max_M = devs[k].M > max_M ? devs[k].M : max_M;
            }
            const RCellJobDev& last = devs[G.last - 1];
            const long group_tiles = last.tile_first + (last.K ? (long)last.gx * last.gy * rcell_groups(last.nz) *
                                                                     ((last.M + EWALD_OT - 1) / EWALD_OT) : 0);
            STAT_TRY(ewald_launch(st, d_jobs + G.first, (int)n_group, G.rows, group_tiles, d_params + cell_at, d_params + k_at,
                                  d_params + q_at, d_offsets, d_dirs, d_ws));
            for (int cls = 0; cls < RCELL_CLASSES; ++cls) {
                if (!needed[cls]) continue;
                const long blocks = launch_blocks(G.items, 65536);   // (asked a launch: the test hook counts launches)
                rcell_launch(cls, W == 3, (unsigned)blocks, sizeof(double) * 3 * (size_t)max_M, st, d_jobs + G.first, (int)n_group,
                             G.items, d_xyz, d_coef, d_offsets, d_dirs, d_betas, d_ws, d_pairs + G.first);
                STAT_TRY(hipGetLastError());
                ran |= 1 << cls;
            }
            const long sum_blocks = launch_blocks(G.blocks, 65536);
            hipLaunchKernelGGL(pw_rigid_cell_sums_kernel, dim3((unsigned)sum_blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                               (int)n_group, G.blocks, d_ws);
            STAT_TRY(hipGetLastError());
            hipLaunchKernelGGL(pw_rigid_cell_reduce_kernel, dim3(n_group), dim3(AFF_CHUNK), 0, st, d_jobs + G.first, d_ws,
                               d_out + G.first, d_levels);
            STAT_TRY(hipGetLastError());
            for (long k = G.first; k < G.last; ++k)                  // (the map is the first L + 1 planes of the records)
                if (jobs[k].map_first >= 0)
                    STAT_TRY(hipMemcpyAsync(maps + jobs[k].map_first, d_ws + devs[k].rec_first,
                                            sizeof(double) * (size_t)rcell_map_words(jobs[k]), hipMemcpyDeviceToHost, st));
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res.data(), d_res, res_bytes, hipMemcpyDeviceToHost, st));
        STAT_TRY(hipMemcpyAsync(pairs.data(), d_pairs, pairs_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    // the caller's rows, job by job
    const pw_rigid_out* r_out = (const pw_rigid_out*)res.data();
    const pw_affinity_level* r_levels = (const pw_affinity_level*)(res.data() + out_bytes);
    for (long k = 0; k < N; ++k) {
        const pw_rigid_cell_job& J = jobs[k];
        out[J.out] = r_out[k];
        memcpy(levels + J.level_first, r_levels + devs[k].level_first, sizeof(pw_affinity_level) * (size_t)J.n_betas);
        if (n_pairs) n_pairs[k] = (int64_t)pairs[(size_t)k];
    }
    if (instances) *instances = ran;
    return PW_OK;
}

}  // namespace

extern "C" int pw_rigid_cell(pw_context* ctx, const pw_rigid_cell_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                             const double* coef, int64_t n_coef, const double* offsets, int64_t n_offsets, const double* dirs,
                             int64_t n_dirs, const double* betas, int64_t n_betas, double* maps, int64_t n_maps,
                             pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out, int64_t n_out) {
    return rigid_cell(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, offsets, n_offsets, dirs, n_dirs, betas, n_betas, maps, n_maps,
                      levels, n_levels, out, n_out, 0, nullptr, nullptr, 1, nullptr);
}

// measurement and test hook (not part of the header): pw_rigid_cell with the budget of the workspace of a launch given (0:
// the default; the result may not depend on it); the device work timed by HIP events when kernel_ms is not null; per job
// the pair terms evaluated in n_pairs[0 .. n_jobs) when that is not null; skip = 0: no atom is left out (the result may not
// depend on it); the instances of the main kernel that were launched, a bit each, when instances is not null
extern "C" int pw_internal_rigid_cell(pw_context* ctx, const pw_rigid_cell_job* jobs, int64_t n_jobs, const double* xyz,
                                      int64_t n_points, const double* coef, int64_t n_coef, const double* offsets,
                                      int64_t n_offsets, const double* dirs, int64_t n_dirs, const double* betas, int64_t n_betas,
                                      double* maps, int64_t n_maps, pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out,
                                      int64_t n_out, int64_t workspace_bytes, float* kernel_ms, int64_t* n_pairs, int skip,
                                      int32_t* instances) {
    return rigid_cell(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, offsets, n_offsets, dirs, n_dirs, betas, n_betas, maps, n_maps,
                      levels, n_levels, out, n_out, workspace_bytes, kernel_ms, n_pairs, skip, instances);
}

namespace {

// pw_rigid_cell_ewald: the embedded pw_rigid_cell jobs as an array of their own, then the one plan with the Ewald arguments
int rigid_cell_ewald(pw_context* ctx, const pw_rigid_cell_ewald_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                     const double* coef, int64_t n_coef, const double* offsets, int64_t n_offsets, const double* dirs,
                     int64_t n_dirs, const double* betas, int64_t n_betas, const double* site_q, int64_t n_site_q,
                     const double* cell, int64_t n_cell, const double* kvecs, int64_t n_kvecs, double* maps, int64_t n_maps,
                     pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out, int64_t n_out, int64_t workspace_bytes,
                     float* kernel_ms, int64_t* n_pairs, int skip, int32_t* instances) {
    if (n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && !jobs) || n_site_q < 0 || n_cell < 0 || n_kvecs < 0) return PW_E_BAD_ARG;
    std::vector<pw_rigid_cell_job> cells((size_t)n_jobs);
    for (int64_t k = 0; k < n_jobs; ++k) cells[(size_t)k] = jobs[k].cell;
    const EwaldArgs ew{jobs, site_q, cell, kvecs, (long)n_site_q, (long)n_cell, (long)n_kvecs};
    return rigid_cell(ctx, cells.data(), n_jobs, xyz, n_points, coef, n_coef, offsets, n_offsets, dirs, n_dirs, betas, n_betas, maps,
                      n_maps, levels, n_levels, out, n_out, workspace_bytes, kernel_ms, n_pairs, skip, instances,
                      "pw_rigid_cell_ewald", &ew);
}

}  // namespace

extern "C" int pw_rigid_cell_ewald(pw_context* ctx, const pw_rigid_cell_ewald_job* jobs, int64_t n_jobs, const double* xyz,
                                   int64_t n_points, const double* coef, int64_t n_coef, const double* offsets, int64_t n_offsets,
                                   const double* dirs, int64_t n_dirs, const double* betas, int64_t n_betas, const double* site_q,
                                   int64_t n_site_q, const double* cell, int64_t n_cell, const double* kvecs, int64_t n_kvecs,
                                   double* maps, int64_t n_maps, pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out,
                                   int64_t n_out) {
    return rigid_cell_ewald(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, offsets, n_offsets, dirs, n_dirs, betas, n_betas, site_q,
                            n_site_q, cell, n_cell, kvecs, n_kvecs, maps, n_maps, levels, n_levels, out, n_out, 0, nullptr, nullptr, 1,
                            nullptr);
}

// measurement and test hook (not part of the header): pw_rigid_cell_ewald with pw_internal_rigid_cell's knobs
extern "C" int pw_internal_rigid_cell_ewald(pw_context* ctx, const pw_rigid_cell_ewald_job* jobs, int64_t n_jobs, const double* xyz,
                                            int64_t n_points, const double* coef, int64_t n_coef, const double* offsets,
                                            int64_t n_offsets, const double* dirs, int64_t n_dirs, const double* betas,
                                            int64_t n_betas, const double* site_q, int64_t n_site_q, const double* cell,
                                            int64_t n_cell, const double* kvecs, int64_t n_kvecs, double* maps, int64_t n_maps,
                                            pw_affinity_level* levels, int64_t n_levels, pw_rigid_out* out, int64_t n_out,
                                            int64_t workspace_bytes, float* kernel_ms, int64_t* n_pairs, int skip,
                                            int32_t* instances) {
    return rigid_cell_ewald(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, offsets, n_offsets, dirs, n_dirs, betas, n_betas, site_q,
                            n_site_q, cell, n_cell, kvecs, n_kvecs, maps, n_maps, levels, n_levels, out, n_out, workspace_bytes,
                            kernel_ms, n_pairs, skip, instances);
}
