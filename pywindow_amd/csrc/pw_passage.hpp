// pw_passage.hpp -- the energy barrier a guest crosses at every window of a cage: the minimax (bottleneck) level of a
// scalar field between a seed voxel and the faces of its box (include/pywindow_amd.h: pw_passage), single source for the
// gfx950 kernels (pw_passage.hip) and the host path (pw_hostpath.cpp).  The reference has no counterpart.
//
// DEFINED RESULT.  A job has the grid of pw_cavity (nx x ny x nz voxels, origin o, spacing h, voxel centres
// x = o_x + (double)i * h), a seed voxel, m >= 0 planes (a, b, c, d) and a field U over every voxel of the grid, ranked
// (l, j, i) ascending as in pw_affinity:
//   FIELD    field_first == -1: the Lennard-Jones energy of pw_affinity.hpp's ENERGY paragraph from the job's atoms,
//            rows (A, B), core2 and cutoff2 -- aff_r2, aff_blocked, aff_counts and aff_pair in that order and
//            association --, +inf at a blocked voxel.  field_first >= 0: the caller's field[field_first .. + nx*ny*nz),
//            every value finite or +inf (+inf: blocked).
//   ROWS     R = max(m, 1) rows are written from out_first.  Row k leaves plane k out; with m == 0 the one row has no
//            plane.  held(v): ((a*x + b*y) + c*z) <= d for every plane j != k.
//   LEVELS   allowed_t(v): U_v is not +inf, held(v) and U_v <= t.  F(t): the 6-connected component of allowed_t that
//            holds the seed voxel, empty if the seed voxel is not allowed.  P(t): F(t) has a voxel on a face of the grid
//            (cavity_row_face).  P is monotone in t and changes only at voxel values.
//   WRITTEN  u_seed = U of the seed voxel.  PAS_SEED_CLOSED when the seed voxel is blocked or not held: barrier = well =
//            +inf, every voxel -1, every count 0.  Otherwise B = the smallest voxel value t with P(t); PAS_NO_EXIT and
//            B = +inf when P is false at the largest finite value.  n_fill = |F(B)|; saddle = the voxel of F(B) with
//            U == B of the lowest rank (-1, -1, -1 when B = +inf) and barrier = the bits of U at the saddle (+inf
//            without one), so a -0.0 that ties with a +0.0 comes back as whichever the saddle holds; well and
//            well_voxel = the smallest U over F(B), ties to the lowest rank by strict < in rank order; n_basin = the
//            size of the seed's component of {allowed, U < B}, 0 when U_seed == B.
// Everything is a comparison of doubles or an integer count, so device, host path and every split into launches return
// the same bytes.
//
// KEYS.  pas_key maps a double that is not a NaN to a 64-bit integer that orders as the doubles compare: the two zeros
// share one key (they compare equal), negative values have their bits inverted, the others their sign bit set.
// pas_unkey is its inverse up to the sign of zero (+0.0).  Both paths bisect the key: the lower bound is the seed's key
// (below it the seed is not allowed), the upper bound the largest key of a held voxel that is not blocked; a step fills
// at mid, and since P changes only at voxel values a step that passes lowers the upper bound to the largest key <= mid
// of a held voxel, and a step that fails raises the lower bound to the smallest key > mid of one -- the result is the
// same and an interval of keys halves every step: at most PAS_MAX_STEPS steps.
#pragma once
#include "pw_affinity.hpp"
#include "pw_cavity.hpp"

namespace pw {

constexpr int PAS_SEED_CLOSED = 1;                   // PW_PAS_SEED_CLOSED
constexpr int PAS_NO_EXIT = 2;                       // PW_PAS_NO_EXIT
constexpr int PAS_MAX_STEPS = 64;                    // bisection steps of a row: the keys have 64 bits
constexpr int PAS_FIELD_TILE = 128;                  // atoms staged in LDS at a time by the field kernel
constexpr long PAS_WORKSPACE_BYTES = 64l << 20;      // the maps of the jobs of one launch

constexpr unsigned long long PAS_KEY_INF = 0xFFF0000000000000ull;    // pas_key(+inf); every finite key is below
constexpr unsigned long long PAS_KEY_NONE = ~0ull;                   // no voxel: above every key

PW_HD inline unsigned long long pas_key(double v) {
    unsigned long long b = pw_d2bits(v);
    if (b == 0x8000000000000000ull) b = 0;                           // (-0.0 compares equal to +0.0)
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
PW_HD inline double pas_unkey(unsigned long long k) {
    return pw_bits2d((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k);
}
// a value a caller's field may hold: finite or +inf
PW_HD inline bool pas_value_ok(double v) { return v == v && v != -aff_inf(); }

PW_HD inline int pas_rows_out(long m) { return m > 1 ? (int)m : 1; }

// (key, rank) pairs order by the key, then by the rank: what a strict < in rank order leaves
PW_HD inline bool pas_before(unsigned long long key, long rank, unsigned long long best, long best_rank) {
    return key < best || (key == best && rank < best_rank);
}

}  // namespace pw
