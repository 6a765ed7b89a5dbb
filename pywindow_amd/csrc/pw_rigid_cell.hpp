// pw_rigid_cell.hpp -- the orientation-averaged Boltzmann factor of a rigid linear guest at every voxel of the skewed
// grid of a periodic cell (include/pywindow_amd.h: pw_rigid_cell), single source for the gfx950 kernels
// (pw_rigid_cell.hip) and the host path (pw_hostpath.cpp).  It is pw_rigid.hpp's pose, weight and fold on
// pw_percolate.hpp's grid, with a cutoff that is always there -- and therefore with atoms that a group of voxels may
// leave out without changing a byte (THE SKIP, below).  The reference has no counterpart.
//
// DEFINED RESULT.  A job has the grid of a pw_percolation job (origin, step = (ax, bx, by, cx, cy, cz), nx, ny, nz <= 64,
// voxel centres by channels_x / _y / _z), n atoms X -- every periodic image that matters listed as an atom of its own --,
// core2 >= 1e-6, cutoff2 > core2 (0 is refused: a cell has no "no cutoff"), L <= 8 betas, and of a pw_rigid job the
// S <= RIGID_MAX_SITES offsets t_s (|t_s| <= 16), the M <= RIGID_MAX_DIRS directions d_o (data: components within
// [-1, 1], nothing normalises them) and rows (A, B) per (site, atom), row s * n + a, two doubles a row.  Uncharged only
// (pw_ewald.hpp defines the charged entry, pw_rigid_cell_ewald, on top of this one).
//   POSE, WEIGHT, VOXEL  pw_rigid.hpp's with charged = 0 and the voxel centre by channels_x / _y / _z: the site position
//            by rigid_site; per site the atoms in index order, aff_r2, aff_blocked, aff_counts, aff_pair, the per-site
//            accumulators from +0.0; U = U_0 + U_1 + ...; aff_weight with its clamp and AFF_CLAMPED; RigidFold over the
//            orientations in o order; zbar_b, ebar_b, and umin_v by strict < in o order; a voxel whose poses are all
//            blocked is DEAD.  Every voxel of the grid is a rank, (l * ny + j) * nx + i; V = nx * ny * nz.
//   SUMS     pw_affinity.hpp's, on the slots zbar_b and ebar_b: ranks by (l, j, i), chunks of 64 ranks, the tree 1, 2, 4,
//            8, 16, 32, the chunk sums added in chunk order from +0.0.  No floating-point atomics.
//   WRITTEN  row `out` (pw_rigid_out): n_voxels = V, n_blocked_poses, n_dead, u_min with min_voxel and min_dir (the
//            smallest pose energy, ties to the lowest rank, then the lowest o; +inf and -1s without one), the flags; rows
//            levels[level_first + b] = (Z_b, E_b); and, when map_first >= 0, L + 1 planes of V doubles from map_first:
//            zbar_0 .. zbar_{L-1}, then umin_v.
// With S = 1, t_0 = 0, M = 1 the umin_v plane is pw_percolation's map byte for byte (x + 0 * d == x unless x is -0.0,
// whose difference to an atom squares to the same bits).  On a cell with step = (h, 0, h, 0, 0, h) every output shared with
// pw_rigid_affinity over the whole grid with the same cutoff2 on the same atoms is that entry's bytes: (o + i*h) + j*0 + l*0
// is cavity_coord's value.
//
// A voxel's RECORD, as the main kernel and the host path leave it for the sums, is 2L + 2 eight-byte words in planes of V:
// planes [0, L) zbar_b, plane L umin_v (these L + 1 are the map), planes [L + 1, 2L + 1) ebar_b, plane 2L + 1 the INFO
// word: bits 0 .. 15 the voxel's blocked poses, bit 16 clamped, bits 32 .. 63 the direction of umin_v plus one (0: dead).
// A chunk's PARTIAL is pw_rigid.hpp's.
//
// THE SKIP.  A counting test that fails adds nothing to U, and a blocked test can only hold inside the cutoff
// (core2 < cutoff2).  So leaving an atom out for a GROUP of voxels changes no byte iff for every voxel of the group, every
// site and every direction of the job the computed aff_r2 exceeds cutoff2.  A group is a block of RCELL_G x RCELL_G x
// RCELL_G voxels, (i0 .. i0+3, j0 .. j0+3, l0 .. l0+3) cut at the grid's edges.  Its centre c = rcell_centre: the point of
// the lattice at the indices i0 + 1.5, j0 + 1.5, l0 + 1.5, in channels_x / _y / _z's association.  Per job
//     rho    = rcell_radius(step): 1.5 * the largest of |a + p b + q c| over the four signs (p, q), a = (ax, 0, 0),
//              b = (bx, by, 0), c = (cx, cy, cz) -- the half diagonals of the block, whose largest bounds the distance of
//              every lattice point (i0 + e, j0 + f, l0 + g), 0 <= e, f, g <= 3, to c, a norm being convex on the box;
//     tmax   = max_s |t_s| and dmax = max_o sqrt((dx*dx + dy*dy) + dz*dz): the norms as they are given;
//     reach  = ((sqrt(cutoff2) + tmax * dmax) + rho) + RCELL_MARGIN and reach2 = reach * reach.
// An atom is FAR from the group iff rcell_far: |X|, |Y|, |Z| <= RCELL_CAP and aff_r2(cx - X, cy - Y, cz - Z) > reach2; a far
// atom is left out.  reach2 is +inf -- nothing is far -- when rcell_extent(origin, step) = |ox| + |oy| + |oz| + 66 (|ax| +
// |bx| + |by| + |cx| + |cy| + |cz|) exceeds RCELL_CAP or cutoff2 exceeds RCELL_CAP^2, and when the caller of the internal
// entry turns the skip off.
// PROOF that a far atom has computed r2 > cutoff2 in every pose of the group, in floating point.  u = 2^-53; every value
// below is at most 2^22 in magnitude (coordinates of voxels, c and atoms <= RCELL_CAP = 2^20 by the two caps, |t d| <= 28,
// sqrt(cutoff2) <= 2^20), so one rounding errs by at most 2^22 u = 2^-31 =: e.  For a voxel v of the group with the
// computed centre p, a site s and a direction o with the computed site position P and the atom X:
//   (1) |P - (p + t_s d_o)| <= sqrt(3) * 2e (a product and a sum a coordinate), and |t_s d_o| <= tmax * |d_o|;
//   (2) the computed p and c each lie within sqrt(3) * 6e of their lattice points (three products and three sums a
//       coordinate at most), which are at most rho_exact apart; the computed rho is within 16e of rho_exact (a handful
//       of operations on values below 2^22), and the computed tmax * dmax within 8e of max |t_s| |d_o|;
//   (3) the computed aff_r2(c - X) = |c - X|^2 (1 + theta), |theta| <= 4u + O(u^2) (a difference, a square and two sums of
//       non-negative terms; no underflow matters: the value exceeds reach2 >= RCELL_MARGIN^2), the computed reach is within
//       4e of the sum it rounds, and its square within a factor 1 +- u: |c - X| > reach_exact_sum - 8e.
//   So |P - X| >= |c - X| - |c - p| - |p - P| > sqrt(cutoff2) (1 - u) + RCELL_MARGIN - 64e, and RCELL_MARGIN = 2^-20 = 2048e.
//   The computed r2 = |P - X|^2 (1 + theta'), |theta'| <= 4u + O(u^2), so r2 > cutoff2 (1 + 2^-41)^2 (1 - 5u) > cutoff2,
//   using sqrt(cutoff2) <= 2^20 for the relative size of the margin.
// The test costs a few percent of the reach in atoms and is the same on both paths; the result does not depend on whether a
// path applies it.  The survivors keep their index order, so every accumulator takes the terms it would have taken.
#pragma once
#include "pw_channels.hpp"
#include "pw_rigid.hpp"

namespace pw {

constexpr int RCELL_G = 4;                            // a group is RCELL_G^3 voxels: one wavefront
constexpr int RCELL_NEAR_CAP = 2048;                  // indices of the near list in LDS (pw_rigid_cell.hip); no result shows it
constexpr double RCELL_MARGIN = 9.5367431640625e-07;  // 2^-20
constexpr double RCELL_CAP = 1048576.0;               // 2^20
constexpr long RCELL_WORKSPACE_BYTES = 256l << 20;    // the records and partials of the jobs of one launch

// the words of a job in the workspace of its launch: the records, then the partials of its chunks
PW_HD inline long rcell_record_words(long V, int L) { return (2l * L + 2) * V; }
PW_HD inline long rcell_groups(int n) { return (n + RCELL_G - 1) / RCELL_G; }

PW_HD inline double rcell_extent(const double* o, const double* s) {
    return ((pw_abs(o[0]) + pw_abs(o[1])) + pw_abs(o[2])) +
           66.0 * (((((pw_abs(s[0]) + pw_abs(s[1])) + pw_abs(s[2])) + pw_abs(s[3])) + pw_abs(s[4])) + pw_abs(s[5]));
}
PW_HD inline double rcell_norm(double x, double y, double z) { return pw_sqrt((x * x + y * y) + z * z); }
PW_HD inline double rcell_radius(const double* s) {
    double most = 0.0;
    for (int q = 0; q < 4; ++q) {
        const double p = (q & 1) ? -1.0 : 1.0, r = (q & 2) ? -1.0 : 1.0;
        const double n = rcell_norm((s[0] + p * s[1]) + r * s[3], p * s[2] + r * s[4], r * s[5]);
        most = n > most ? n : most;
    }
    return 1.5 * most;
}
// the square of the reach of a job's groups; +inf: nothing is far.  ts: the S offsets, dd: the M directions
PW_HD inline double rcell_reach2(const double* o, const double* s, double cutoff2, const double* ts, int S, const double* dd,
                                 int M, bool skip) {
    if (!skip || !(rcell_extent(o, s) <= RCELL_CAP) || !(cutoff2 <= RCELL_CAP * RCELL_CAP)) return aff_inf();
    double tmax = 0.0, dmax = 0.0;
    for (int q = 0; q < S; ++q) tmax = pw_abs(ts[q]) > tmax ? pw_abs(ts[q]) : tmax;
    for (int q = 0; q < M; ++q) {
        const double n = rcell_norm(dd[3 * q], dd[3 * q + 1], dd[3 * q + 2]);
        dmax = n > dmax ? n : dmax;
    }
    const double reach = ((pw_sqrt(cutoff2) + tmax * dmax) + rcell_radius(s)) + RCELL_MARGIN;
    return reach * reach;
}
// a coordinate of the centre of the group whose first voxel is (i0, j0, l0)
PW_HD inline double rcell_centre_x(const double* o, const double* s, int i0, int j0, int l0) {
    return ((o[0] + ((double)i0 + 1.5) * s[0]) + ((double)j0 + 1.5) * s[1]) + ((double)l0 + 1.5) * s[3];
}
PW_HD inline double rcell_centre_y(const double* o, const double* s, int j0, int l0) {
    return (o[1] + ((double)j0 + 1.5) * s[2]) + ((double)l0 + 1.5) * s[4];
}
PW_HD inline double rcell_centre_z(const double* o, const double* s, int l0) { return o[2] + ((double)l0 + 1.5) * s[5]; }
PW_HD inline bool rcell_far(double cx, double cy, double cz, double X, double Y, double Z, double reach2) {
    return pw_abs(X) <= RCELL_CAP && pw_abs(Y) <= RCELL_CAP && pw_abs(Z) <= RCELL_CAP && aff_r2(cx - X, cy - Y, cz - Z) > reach2;
}

// the INFO word of a voxel's record
PW_HD inline unsigned long long rcell_info(int n_blocked, bool clamped, int umin_o) {
    return (unsigned long long)n_blocked | (clamped ? 1ull << 16 : 0ull) | ((unsigned long long)(unsigned)(umin_o + 1) << 32);
}
PW_HD inline int rcell_info_blocked(unsigned long long w) { return (int)(w & 0xffffull); }
PW_HD inline bool rcell_info_clamped(unsigned long long w) { return ((w >> 16) & 1ull) != 0; }
PW_HD inline int rcell_info_dir(unsigned long long w) { return (int)(w >> 32) - 1; }

}  // namespace pw
