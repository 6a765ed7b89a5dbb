// pw_rigid.hpp -- the orientation-averaged affinity of a cavity for a rigid linear guest (include/pywindow_amd.h:
// pw_rigid_affinity), single source for the gfx950 kernels (pw_rigid.hip) and the host path (pw_hostpath.cpp).  The pair
// term, the blocked and counts tests, the weight, the search of a rank's voxel and the chunk tree are pw_affinity.hpp's;
// this file adds the site position, the charged pair term and the fold over the orientations.  The reference has no
// counterpart.
//
// DEFINED RESULT.  A job has the grid, the REGION, core2, cutoff2 and the L betas of a pw_affinity job, n atoms X, and
//     S sites, 1 <= S <= RIGID_MAX_SITES, with the offsets t_s along the guest's axis, finite and |t_s| <= 16;
//     rows (A, B, C) per (site, atom), row s * n + a: 0 <= A, B <= 1e100, C finite with |C| <= 1e100;
//     charged (0 or 1): with 0 the column C is neither read nor evaluated;
//     M directions d_o, 1 <= M <= RIGID_MAX_DIRS, every component finite and within [-1, 1]; they are data: nothing
//     normalises them or checks their length.
//   POSE (v, o)  voxel v has the centre (x, y, z) by cavity_coord.  Site s sits at px = x + (t_s * dx), likewise py and
//            pz: the product is rounded, then the sum.  Per site the atoms go in index order: r2 = aff_r2(px - X,
//            py - Y, pz - Z); the POSE is BLOCKED iff aff_blocked(r2, core2) for any (site, atom); an atom COUNTS for a
//            site iff aff_counts(r2, cutoff2); for a counting atom u = aff_pair(r2, A, B) and, when charged,
//            u = u + C / sqrt(r2), square root and division correctly rounded; U_s = U_s + u from +0.0.  The pose's
//            energy is U = U_0, then U = U + U_s for s = 1 .. S - 1.  The accumulators are per site, so the nest of
//            the loops (atoms outside, sites inside) is free.
//   WEIGHT   per beta and pose that is not blocked: w = aff_weight(beta, U), the clamp at 700 and AFF_CLAMPED included;
//            the terms z = w and e = w * U.
//   VOXEL    per beta zs = +0.0 and es = +0.0; for o = 0 .. M - 1 in order zs = zs + z and es = es + e, blocked poses
//            skipped; zbar = zs * inv_M and ebar = es * inv_M with inv_M = 1.0 / (double)M.  umin_v is the smallest U of
//            the voxel's poses that are not blocked, by strict < in o order, +inf without one.  A voxel whose poses are
//            all blocked is DEAD.
//   SUMS     pw_affinity's, on the slots zbar and ebar: ranks by (l, j, i), chunks of 64 ranks, the tree k = 1, 2, 4,
//            8, 16, 32, the chunk sums added in chunk order from +0.0.  No floating-point atomics.
//   WRITTEN  n_voxels, n_blocked_poses, n_dead, u_min with min_voxel and min_dir (the smallest pose energy, ties to the
//            lowest rank and then the lowest o; +inf and -1s without one), the flags, (Z_b, E_b) per beta and, when
//            map_level >= 0, per rank the two doubles zbar at that level and umin_v.
// With S = 1, t_0 = 0, M = 1 and charged = 0 every shared output is pw_affinity's bytes: x + 0 * d == x, +0.0 + w == w
// and w * 1.0 == w.
//
// A chunk's PARTIAL is 2L + RIGID_PART_FIXED eight-byte words: [0, 2L) the chunk sums zbar_0, ebar_0, zbar_1, ...; then
// the bits of the chunk's smallest pose energy (+inf: none), its rank, its direction, the blocked poses, the dead
// voxels, the flags.
#pragma once
#include "pw_affinity.hpp"

namespace pw {

constexpr int RIGID_MAX_SITES = 8;                   // PW_RIGID_MAX_SITES
constexpr int RIGID_MAX_DIRS = 1024;                 // PW_RIGID_MAX_DIRS
constexpr int RIGID_PART_FIXED = 6;                  // u_min, its rank, its direction, blocked poses, dead voxels, flags
constexpr long RIGID_WORKSPACE_BYTES = 64l << 20;    // prefixes, partials and maps of the jobs of one launch
constexpr double RIGID_MAX_OFFSET = 16.0;

PW_HD inline int rigid_part_words(int L) { return 2 * L + RIGID_PART_FIXED; }

// a coordinate of a site: the centre's plus the rounded product of the offset and the direction's component
PW_HD inline double rigid_site(double x, double t, double d) {
    const double step = t * d;
    return x + step;
}

// the pair term of a counting atom; C is not touched when the job is not charged
template <bool CHARGED>
PW_HD inline double rigid_pair(double r2, double A, double B, double C) {
    const double u = aff_pair(r2, A, B);
    if constexpr (CHARGED) return u + C / pw_sqrt(r2);
    return u;
}

// the fold of one voxel over its orientations, one beta: add() takes the poses in o order, blocked ones left out
struct RigidFold {
    double zs = 0.0, es = 0.0;
    PW_HD inline void add(double w, double U) {
        zs = zs + w;
        es = es + w * U;
    }
    PW_HD inline double zbar(double inv_M) const { return zs * inv_M; }
    PW_HD inline double ebar(double inv_M) const { return es * inv_M; }
};
PW_HD inline double rigid_inv(int M) { return 1.0 / (double)M; }

}  // namespace pw
