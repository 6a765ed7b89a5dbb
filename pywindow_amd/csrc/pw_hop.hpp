// pw_hop.hpp -- the free-energy profile of a guest through a window of a cage: per slab of a grid laid along the window's
// axis, the Boltzmann sums over the 2-D component of allowed voxels round the axis (include/pywindow_amd.h: pw_hop),
// single source for the gfx950 kernels (pw_hop.hip) and the host path (pw_hostpath.cpp).  The reference has no
// counterpart.
//
// DEFINED RESULT.  A job is one (frame, window) in that window's own frame -- the caller has rotated atoms and planes so
// that the window's axis is z.  It has the grid of pw_cavity (nx x ny x nz voxels, each 1 .. 64, origin o, spacing h,
// voxel centres x = o_x + (double)i * h; voxel (i, j, l) has the rank (l, j, i)), a seed COLUMN (si, sj) inside the grid,
// m >= 0 planes (a, b, c, d), ALL of them held (the caller leaves its own window's plane out), a field U, a finite
// cap and 1 <= L <= 8 inverse temperatures.
//   FIELD    exactly pw_passage.hpp's: field_first == -1 is the Lennard-Jones energy of pw_affinity.hpp's ENERGY
//            paragraph (aff_r2, aff_blocked, aff_counts, aff_pair in that order and association), +inf where blocked;
//            otherwise the caller's field[field_first .. + nx*ny*nz), every value finite or +inf.
//   SLABS    every slab l = 0 .. nz - 1 on its own.  allowed(i, j): U is not +inf, ((a*x + b*y) + c*z) <= d for every
//            plane, and U <= cap.  C_l: the 4-connected component, in (i, j) only, of allowed that holds (si, sj); empty
//            when that voxel is not allowed.  n = |C_l|; n_face = the voxels of C_l with i == 0, i == nx - 1, j == 0 or
//            j == ny - 1, each counted once; u_min = the smallest U over C_l, ties (a -0.0 with a +0.0 too) to the
//            lowest (j, i), as the bits that voxel holds, with its (min_i, min_j); +inf, -1, -1 when C_l is empty.
//   SUMS     per beta, over the voxels of C_l ranked by (j, i): x = -(beta * U); x > 700.0: x = 700.0 and the job's flag
//            HOP_CLAMPED; w = pw_exp(x); the terms z = w and e = w * U.  Chunk c holds the ranks 64c .. 64c + 63, a slot
//            whose rank is >= n holds +0.0; within a chunk for k = 1, 2, .., 32 in turn slot[t] = slot[t] + slot[t + k]
//            for every t that is a multiple of 2k; the total starts at +0.0 and takes the chunk sums in order.  These are
//            pw_affinity's WEIGHT and SUMS paragraphs: with C_l handed to pw_affinity as a one-slab mask (nz = 1, o_z of
//            the slab) the pair (Z, E) is pw_affinity's, byte for byte.
//   WRITTEN  slabs[slab_first + l] = {n, n_face, u_min, min_i, min_j}; sums[sum_first + l * L + b] = (Z, E); row `out`:
//            the flags and the total of n; and, with word_first >= 0, words[word_first + l * ny + j] = row j of C_l, bit
//            i voxel i -- the layout of pw_cavity's mask.
// All of it FP64 without contraction in the association written, no floating-point atomics: device, host path and every
// split into launches return the same bytes.
//
// THE FILL.  Both paths keep a slab as ny 64-bit words and reach the least fixed point of
//     fill |= open & (fill << 1 | fill >> 1 | the rows above and below)
// over the seed bit by sweeps (pw_cavity.hpp: monotone, so the order of the work does not show).  Inside a row
// hop_fill_word spreads to saturation by doubling shifts: six steps to each side, the same word as pw_cavity.hpp's
// cavity_fill_word leaves after at most 64 single shifts.  A sweep that changes a word adds a voxel, so nx * ny + 1
// sweeps are the bound; a sweep that changes nothing proves the fixed point.
#pragma once
#include "pw_affinity.hpp"
#include "pw_cavity.hpp"
#include "pw_passage.hpp"

namespace pw {

constexpr int HOP_CLAMPED = 1;                       // PW_HOP_CLAMPED
constexpr int HOP_FIXED_WORDS = 5;                   // a slab's compact record: n, n_face, u_min, (min_i, min_j), flags
constexpr long HOP_WORKSPACE_BYTES = 64l << 20;      // the maps of the jobs of one launch

// a slab's compact record is HOP_FIXED_WORDS + 2L eight-byte words: the fixed ones, then z_0, e_0, z_1, e_1, ...
PW_HD inline int hop_record_words(int L) { return HOP_FIXED_WORDS + 2 * L; }

// `from` spread inside `open` to the fixed point of the x direction (every run of open bits that holds a bit of
// from & open, whole): an occluded fill by doubling shifts, six steps up and six down
PW_HD inline cavity_word hop_fill_word(cavity_word from, cavity_word open) {
    cavity_word up = from & open, down = up, pu = open, pd = open;
    for (int s = 1; s < 64; s <<= 1) {
        up |= pu & (up << s);
        pu &= pu << s;
        down |= pd & (down >> s);
        pd &= pd >> s;
    }
    return up | down;
}

// the voxels of row j of a slab's component, word f, that lie on a lateral face of the grid
PW_HD inline int hop_row_face(cavity_word f, int nx, int ny, int j) {
    return cavity_popcount(j == 0 || j == ny - 1 ? f : f & (1ull | (1ull << (nx - 1))));
}

// (U, position j * 64 + i) pairs order by U, then by the position: what a strict < in rank order leaves
PW_HD inline bool hop_before(double u, int pos, double best, int best_pos) {
    return u < best || (u == best && pos < best_pos);
}

// allowed but for the planes: not +inf and at or below the cap (a caller's field holds no NaN and no -inf)
PW_HD inline bool hop_admits(double U, double cap) { return U != aff_inf() && U <= cap; }

}  // namespace pw
