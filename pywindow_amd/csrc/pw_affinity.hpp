// pw_affinity.hpp -- the Lennard-Jones energy map of a cavity for one guest and its Boltzmann sums (include/
// pywindow_amd.h: pw_affinity), single source for the gfx950 kernels (pw_affinity.hip) and the host path
// (pw_hostpath.cpp).  The reference has no counterpart.
//
// DEFINED RESULT.  A job has n atoms X with rows (A, B) of coefficients (A = 4 eps sigma^12 and B = 4 eps sigma^6 are
// the caller's; 0 <= A, B <= 1e100), the grid of pw_cavity (nx x ny x nz voxels, origin o, spacing h; voxel (i, j, l)
// has the centre x = o_x + (double)i * h, likewise y and z), a REGION -- the ny * nz words of a pw_cavity mask, bits
// at i >= nx ignored, or every voxel --, core2 >= 1e-6, cutoff2 (0.0: no cutoff, otherwise > core2), L inverse
// temperatures beta_b and E ascending edges.
//   ORDER    the voxels of the region are ranked by (l, j, i) ascending; V is their number.
//   ENERGY   per voxel, the atoms in index order, dx = x - X and so on, r2 = (dx*dx + dy*dy) + dz*dz.  The voxel is
//            BLOCKED iff some atom has r2 <= core2.  An atom COUNTS iff cutoff2 == 0.0 or r2 <= cutoff2; one that does
//            not is skipped, not added as zero.  For a counting atom q = 1.0 / r2 (correctly rounded), s = (q*q)*q,
//            u = s * (A*s - B), U = U + u from +0.0.  The bounds keep U of a voxel that is not blocked finite; U of a
//            blocked voxel is never used.
//   WEIGHT   per beta and voxel that is not blocked: x = -(beta * U); x > 700.0: x = 700.0 and the job's flag
//            AFF_CLAMPED; w = pw_exp(x); the terms z = w and e = w * U.
//   SUMS     chunk c holds the ranks 64c .. 64c + 63; a slot whose rank is >= V or whose voxel is blocked holds +0.0.
//            Within a chunk, for k = 1, 2, 4, 8, 16, 32 in turn slot[t] = slot[t] + slot[t + k] for every t that is a
//            multiple of 2k; the chunk's sum is slot[0].  The total starts at +0.0 and takes the chunk sums in chunk
//            order.  No floating-point atomics anywhere.
//   WRITTEN  n_voxels = V, n_blocked, u_min (the smallest U of a voxel that is not blocked, ties to the lowest rank,
//            by strict < in rank order; +inf and min_voxel = -1 without one), the flags; Z_b and E_b; hist[k] =
//            #{v not blocked : U_v < edge_k} by comparisons; and, when asked for, U of every rank (+inf where blocked).
// All of it FP64 without contraction in the association written, so device, host path and every split into launches
// return the same bytes.
//
// A chunk's PARTIAL is AFF_PART_FIXED + 2L + E eight-byte words: [0, 2L) the chunk sums z_0, e_0, z_1, e_1, ...;
// then the bits of the chunk's smallest U (+inf: none), the rank it belongs to, the number of blocked voxels, the
// flags; then the E counts.
#pragma once
#include "pw_cavity.hpp"
#include "pw_math.hpp"

namespace pw {

constexpr int AFF_MAX_LEVELS = 8;                    // PW_AFF_MAX_LEVELS
constexpr int AFF_MAX_EDGES = 16;                    // PW_AFF_MAX_EDGES
constexpr int AFF_CLAMPED = 1;                       // PW_AFF_CLAMPED
constexpr int AFF_CHUNK = 64;                        // ranks a chunk: one wavefront
constexpr int AFF_TILE = 128;                        // atoms staged in LDS at a time (pw_affinity.hip)
constexpr int AFF_PART_FIXED = 4;                    // u_min, its rank, n_blocked, flags
constexpr long AFF_WORKSPACE_BYTES = 64l << 20;      // prefixes, partials and energy maps of the jobs of one launch
constexpr double AFF_MIN_CORE2 = 1e-6;
constexpr double AFF_MAX_COEF = 1e100;
constexpr double AFF_CLAMP = 700.0;

PW_HD inline double aff_inf() { return pw_bits2d(0x7ff0000000000000ull); }
PW_HD inline int aff_part_words(int L, int E) { return 2 * L + AFF_PART_FIXED + E; }

PW_HD inline double aff_r2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
PW_HD inline bool aff_blocked(double r2, double core2) { return r2 <= core2; }
PW_HD inline bool aff_counts(double r2, double cutoff2) { return cutoff2 == 0.0 || r2 <= cutoff2; }
PW_HD inline double aff_pair(double r2, double A, double B) {
    const double q = 1.0 / r2;
    const double s = (q * q) * q;
    return s * (A * s - B);
}
// w of a voxel with the energy U at beta; `clamped` is set, never cleared
template <class Tab>
PW_HD inline double aff_weight(double beta, double U, Tab tab, bool& clamped) {
    double x = -(beta * U);
    if (x > AFF_CLAMP) {
        x = AFF_CLAMP;
        clamped = true;
    }
    return pw_exp_tab(x, tab);
}

// the position of the r-th set bit of w (r from 0), 0 <= r < popcount(w): six halvings
PW_HD inline int aff_select(cavity_word w, int r) {
    int pos = 0;
    for (int width = 32; width >= 1; width >>= 1) {
        const cavity_word low = w & ((1ull << width) - 1ull);
        const int c = cavity_popcount(low);
        if (r >= c) {
            r -= c;
            w >>= width;
            pos += width;
        } else {
            w = low;
        }
    }
    return pos;
}

// the voxel (i, row) of a rank < V.  word(r): the row's word as given; prefix(r): the number of voxels of the region in
// the rows before r, r = 0 .. rows (only read when masked).  The search halves [0, rows): at most 12 steps
template <class Word, class Prefix>
PW_HD inline void aff_voxel(long rank, bool masked, int nx, int rows, Word word, Prefix prefix, int& i, int& row) {
    if (!masked) {
        row = (int)(rank / nx);
        i = (int)(rank - (long)row * nx);
        return;
    }
    int lo = 0, hi = rows;                                           // prefix(lo) <= rank < prefix(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)prefix(mid) <= rank) lo = mid; else hi = mid;
    }
    row = lo;
    i = aff_select(word(lo) & cavity_row_mask(nx), (int)(rank - (long)prefix(lo)));
}

// the chunk tree over 64 slots, in place; the sum is slot[0]
inline double aff_tree(double* slot) {
    for (int k = 1; k < AFF_CHUNK; k <<= 1)
        for (int t = 0; t < AFF_CHUNK; t += 2 * k) slot[t] = slot[t] + slot[t + k];
    return slot[0];
}

}  // namespace pw
