// pw_percolate.hpp -- the energy levels at which the voids of a periodic cell connect for a guest: for each of six
// connection criteria the minimax (bottleneck) level of a scalar field over the cell's own grid (include/pywindow_amd.h:
// pw_percolation), single source for the gfx950 kernels (pw_percolate.hip) and the host path (pw_hostpath.cpp).  It is the
// composition of pw_channels.hpp (the periodic grid, the parity fills, the rank of a winding subspace) and
// pw_passage.hpp (the keys that order as doubles compare, the bisection on them) over the energy of pw_affinity.hpp.  The
// reference has no counterpart.
//
// DEFINED RESULT.  A job is one cell and one guest.
//   GRID     exactly pw_channels': nx x ny x nz voxels (1 .. 64 each), an origin and step = (ax, bx, by, cx, cy, cz), voxel
//            centres by channels_x / _y / _z, six neighbours with indices mod n_k, face crossings as defined there.
//   FIELD    U over every voxel, in rank (l * ny + j) * nx + i.  field_first == -1: the Lennard-Jones energy of the
//            job's atoms (every periodic image that matters listed as an atom of its own), rows (A, B), core2 and
//            cutoff2 -- aff_r2, aff_blocked, aff_counts and aff_pair in pw_field_dev.hpp's order and association: atom
//            after atom, U = U + aff_pair where aff_counts --, +inf at a blocked voxel.  field_first >= 0: the caller's
//            field[field_first .. + nx*ny*nz), every value finite or +inf (pas_value_ok).  map_first >= 0: the field is
//            also written to map[map_first .. + nx*ny*nz).
//   LEVELS   allowed_t(v): U_v is not +inf and U_v <= t.  For the periodic components of allowed_t, `wraps` and `rank` are
//            pw_channels'.
//   CRITERIA P_c(t), c = 0 .. 5: some component of allowed_t has rank >= 1, >= 2, >= 3 (c = 0, 1, 2) or has the bit of
//            phi = 1, 2, 4 set -- bits 0, 1 and 3 of wraps -- (c = 3, 4, 5): it holds a closed path that winds an odd
//            number of times along a, b or c.
//   WRITTEN  the job's row: n_blocked (voxels at +inf), u_min and u_min_voxel (the lowest rank on a tie, by strict < in
//            rank order; +inf and -1 without a finite voxel), flags (PERC_NEVER iff criterion 0 never holds).  Six rows,
//            one a criterion: level = B_c, the smallest voxel value t with P_c(t); +inf with PERC_NEVER when P_c is false
//            at the largest finite value.  C = the component of allowed_{B_c} that meets the criterion and has the lowest
//            first voxel: first, n_voxels, wraps, rank.  saddle = the voxel of C with U == B_c of the lowest rank, and
//            level carries the bits of U at the saddle (pw_passage's rule: a -0.0 that ties with a +0.0 comes back as
//            whichever the saddle holds).  well and well_voxel = the smallest U over C, ties to the lowest rank.
//            n_allowed = |allowed_{B_c}|.  With PERC_NEVER the voxels and first are -1, the counts, wraps and rank 0 and
//            well +inf.
// Everything is a comparison of doubles or an integer count over the field that is already defined, so the device, the
// host path, every launch grouping and every workspace budget return the same bytes.
//
// WHY P_c IS MONOTONE AND CHANGES ONLY AT VOXEL VALUES.  allowed_t grows with t and is constant between two consecutive
// voxel values.  For t' >= t a component of allowed_t is connected inside allowed_t', so it lies inside ONE component of
// allowed_t'; every closed walk of the smaller is a closed walk of the larger, so the larger's winding group, and with it
// the subspace W of residues mod 2 (pw_channels.hpp), contains the smaller's: its rank is no less and every set bit of
// wraps stays set (moving the base point of the walks along a path conjugates them, which changes no winding vector).
// So P_c(t) implies P_c(t'), and B_c is a voxel value.  B_0 <= B_1 <= B_2 and B_0 <= B_3, B_4, B_5 follow from the
// criteria: rank >= 2 implies rank >= 1, and a set bit implies rank >= 1.
//
// WHY THE SADDLE EXISTS.  Let C meet criterion c in allowed_{B_c} and suppose no voxel of C had U == B_c.  Then every
// voxel of C is allowed at t' = the largest value of a voxel of C, t' < B_c, and C -- connected, with the same closed
// walks -- lies inside one component of allowed_t' whose winding group contains C's: P_c(t') with t' < B_c, against the
// choice of B_c.
//
// THE CULL: FILLS ARE SEEDED AT FACE CANDIDATES ONLY (perc_candidates).  A CANDIDATE is an allowed voxel at index
// n_k - 1, for some k, whose +e_k neighbour is allowed.  A component that meets any criterion has a set bit of wraps, so it
// holds a closed walk with phi . w odd, which crosses some face k an odd number of times: at least once.  Every crossing
// step of a component is a step +e_k from index n_k - 1 between two of its voxels, or the reverse of one
// (pw_channels.hpp (1)), so the component holds a candidate.  An evaluation of a level therefore takes its seeds from the
// candidates alone -- the first candidate in rank order, the component filled from it, its candidates struck off, the
// next candidate -- and every component that can meet a criterion is found; the isolated low-energy wells that touch no
// face are never filled.  A component's first voxel is then the lowest set bit of its fill, not its seed.
// Within a component the fills that are not run are pw_channels' (channels_next), with its proofs.
//
// THE SEARCH (perc_search_*).  Per criterion an interval [lo_c, hi_c] of keys: hi_c is a voxel key with P_c(hi_c), and
// P_c is false below lo_c.  At the start lo_c = the smallest key and hi_c = the largest finite key, where P_c was
// evaluated (false there: never, and the criterion is closed with lo_c = hi_c = PAS_KEY_INF).  A step takes the first
// criterion with lo_c < hi_c, evaluates the level mid = lo_c + (hi_c - lo_c) / 2 and learns, for EVERY criterion d,
// from the six bits `met` of that one evaluation: met_d moves hi_d down to `below`, the largest voxel key <= mid (P_d is
// constant from it to mid); a bit that is clear after an evaluation that went through every candidate moves lo_d up to
// `above`, the smallest finite voxel key > mid.  An evaluation may stop as soon as every criterion d with
// lo_d <= mid < hi_d -- the only ones for which the answer is news -- is met; it is then not COMPLETE and its clear
// bits teach nothing.  The interval of the criterion that chose mid loses its upper or its lower half, mid included, so
// it takes at most PAS_MAX_STEPS steps and the search at most 6 * PAS_MAX_STEPS; nesting (B_0 <= B_1 <= B_2,
// B_0 <= B_3 ..) needs no code: the bits of one evaluation carry it.  At the end B_c = hi_c.
//
// WHAT IT LEAVES OUT.  (1) The mod-2 limit of pw_channels is inherited: a component whose windings are all even (the
// double helix of pitch two cells) reads as not winding, at every level.  (2) No guest-guest term and no charges: the
// landscape of ONE guest in the empty framework.  (3) The bottleneck is that of the grid's 6-connectivity at the chosen
// spacing: a pass narrower than a voxel between two blocked voxels is closed, and a saddle is a voxel centre.
#pragma once
#include "pw_channels.hpp"
#include "pw_passage.hpp"

namespace pw {

constexpr int PERC_NEVER = 1;                          // PW_PERC_NEVER
constexpr int PERC_CRITERIA = 6;                       // PW_PERC_CRITERIA
constexpr int PERC_MAX_STEPS = PERC_CRITERIA * PAS_MAX_STEPS;
constexpr long PERC_WORKSPACE_BYTES = 256l << 20;      // the maps of the jobs of one launch: 256 of 50^3 voxels, a job a CU

// the criteria a component with these wraps meets, bit c for criterion c
PW_HD inline int perc_criteria(int wraps) {
    const int rank = channels_rank(wraps);
    return (rank >= 1 ? 1 : 0) | (rank >= 2 ? 2 : 0) | (rank >= 3 ? 4 : 0) | ((wraps & 1) ? 8 : 0) | ((wraps & 2) ? 16 : 0) |
           ((wraps & 8) ? 32 : 0);
}

// the candidates of row (j, l), whose allowed word is `a`: its voxel nx - 1 when voxel 0 is allowed too, and on the last
// row along b or c the voxels whose +e_k neighbours -- in the rows (0, l) and (j, 0), words up_j and up_l -- are allowed
PW_HD inline cavity_word perc_candidates(cavity_word a, cavity_word up_j, cavity_word up_l, int nx, int ny, int nz, int j, int l) {
    return ((((a >> (nx - 1)) & a) & 1ull) << (nx - 1)) | (j == ny - 1 ? a & up_j : 0ull) | (l == nz - 1 ? a & up_l : 0ull);
}

// THE SEARCH, on lo[6], hi[6] wherever they live
PW_HD inline void perc_search_begin(unsigned long long* lo, unsigned long long* hi, unsigned long long kmin,
                                    unsigned long long kmax, int met_at_kmax) {
    for (int c = 0; c < PERC_CRITERIA; ++c) {
        const bool some = (met_at_kmax >> c) & 1;
        lo[c] = some ? kmin : PAS_KEY_INF;
        hi[c] = some ? kmax : PAS_KEY_INF;
    }
}
// the next level to evaluate and the criteria for which it is news; false: every criterion is closed
PW_HD inline bool perc_search_next(const unsigned long long* lo, const unsigned long long* hi, unsigned long long& mid, int& needed) {
    for (int c = 0; c < PERC_CRITERIA; ++c) {
        if (lo[c] >= hi[c]) continue;
        mid = lo[c] + ((hi[c] - lo[c]) >> 1);
        needed = 0;
        for (int d = 0; d < PERC_CRITERIA; ++d)
            if (lo[d] <= mid && mid < hi[d]) needed |= 1 << d;
        return true;
    }
    return false;
}
PW_HD inline void perc_search_learn(unsigned long long* lo, unsigned long long* hi, int met, bool complete,
                                    unsigned long long below, unsigned long long above) {
    for (int c = 0; c < PERC_CRITERIA; ++c) {
        if ((met >> c) & 1) {
            if (below < hi[c]) hi[c] = below;
        } else if (complete && above > lo[c] && above <= hi[c]) {
            lo[c] = above;                                           // (above <= hi[c] always: hi[c] is a voxel key > mid)
        }
    }
}

}  // namespace pw
