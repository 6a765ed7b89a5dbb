// pw_pores.hpp -- the probe-swept cavity of a cage for a ladder of probes: the probe-occupiable volume and the geometric
// pore size distribution (include/pywindow_amd.h: pw_pore_sizes), single source for the gfx950 kernel (pw_pores.hip) and
// the host path (pw_hostpath.cpp).  It stands on pw_cavity.hpp: a level's reach IS the cavity of pw_cavity for that
// probe.  The reference has no counterpart.
//
// DEFINED RESULT.  A job has the atoms, radii, planes, grid (nx, ny, nz in 1 .. 64, origin o, spacing h > 0) and seed
// voxel of a pw_cavity job and L probe radii 0 <= p_0 < p_1 < ... < p_{L-1}, 1 <= L <= PORES_MAX_LEVELS.  Per level l:
//     reach_l   the cavity of pw_cavity for the probe p_l (cavity_coord, cavity_reach2, cavity_free, cavity_inside, the
//               6-connected fill from the seed voxel); empty, with CAVITY_SEED_CLOSED, if the seed voxel is not open;
//     K_l       the largest integer k in [0, PORES_MAX_K2] with (double)k * (h * h) <= p_l * p_l, each product rounded
//               once (pores_k2: the left side is monotone in k, so it is a bisection and nothing is divided);
//     swept_l   the voxels v of the grid for which some c in reach_l has |v - c|^2 <= K_l in integers -- voxels outside
//               the grid do not exist: nothing wraps and nothing reaches the bits >= nx.
// domain = reach_0, and for v in domain cover(v) is the largest l with v in swept_l.  Written per level: n_reach and
// n_face (pw_cavity's n_voxels and n_face for that probe), n_swept = |swept_l & domain|, n_largest = #{cover = l},
// k2 = K_l and the flags; per job n_domain, n_none = #{v in domain without a cover} and n_levels, so that
// n_domain = n_none + sum n_largest.  The centre of a ball belongs to it whatever K is, so reach_0 is part of swept_0
// and swept_0 & domain = domain: level 0 is not swept, n_swept_0 = n_domain and n_none = 0 (it is counted all the same).
// A probe below h has K = 0 and sweeps nothing beyond its centres: the resolution in p is the grid's.
//
// THE SWEEP, bit-parallel and without floating point.  In the layout of pw_cavity.hpp (row (j, l) one word at
// l * ny + j) the swept word of a row is the OR, over the rows (j + dj, l + dl) inside the grid with dj^2 + dl^2 <= K,
// of their reach words spread along x by w = isqrt(K - dj^2 - dl^2): di^2 <= K - dj^2 - dl^2 iff |di| <= w.  A spread
// by s is the OR of the shifts -s .. s, built one side at a time by doubling: with U_c the OR of the shifts 0 .. c,
// U_{c+d} = U_c | U_c << d for d <= c + 1, at most 6 steps a side for s <= 63 (a larger s spreads no further than 63 in
// a word of 64).  Every bit only ever moves from its source towards its target, so no bit that counts is shifted out.
#pragma once
#include "pw_cavity.hpp"

namespace pw {

constexpr int PORES_MAX_LEVELS = 64;                  // PW_PORES_MAX_LEVELS
constexpr int PORES_MAX_K2 = 3 * 63 * 63;             // PW_PORES_MAX_K2: the farthest two voxels of a 64^3 grid
constexpr long PORES_WORKSPACE_BYTES = 64l << 20;     // open words and masks of the jobs of one launch (pw_pores.hip)

// K of a level (see DEFINED RESULT); k = 0 always holds, p * p being >= 0
PW_HD inline int pores_k2(double probe, double h) {
    const double h2 = h * h, p2 = probe * probe;
    int lo = 0, hi = PORES_MAX_K2;
    while (lo < hi) {                                  // (the interval halves: 14 turns)
        const int mid = lo + (hi - lo + 1) / 2;
        if ((double)mid * h2 <= p2) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the largest r with r * r <= v, 0 <= v <= PORES_MAX_K2 < 128 * 128
PW_HD inline int pores_isqrt(int v) {
    int r = 0;
    for (int b = 64; b; b >>= 1) {
        const int t = r + b;
        if (t * t <= v) r = t;
    }
    return r;
}

// the OR of the shifts -s .. s of a word whose bits >= nx are zero, masked to nx
PW_HD inline cavity_word pores_spread(cavity_word x, int s, cavity_word xmask) {
    if (s > 63) s = 63;
    cavity_word up = x, down = x;
    for (int c = 0; c < s;) {
        const int d = s - c < c + 1 ? s - c : c + 1;
        up |= up << d;
        down |= down >> d;
        c += d;
    }
    return (up | down) & xmask;
}

// the swept word of row (j, l) for K = k2; word_at(r) is the reach word of row r (bits >= nx zero).  At most ny * nz
// source rows; it stops early once every voxel of the row is swept.
template <class WordAt>
PW_HD inline cavity_word pores_dilate_row(WordAt word_at, int j, int l, int ny, int nz, int k2, cavity_word xmask) {
    const int R = pores_isqrt(k2);
    const int l_lo = l - R > 0 ? l - R : 0, l_hi = l + R < nz - 1 ? l + R : nz - 1;
    cavity_word out = 0;
    for (int ll = l_lo; ll <= l_hi; ++ll) {
        const int rest = k2 - (ll - l) * (ll - l), Rj = pores_isqrt(rest);
        const int j_lo = j - Rj > 0 ? j - Rj : 0, j_hi = j + Rj < ny - 1 ? j + Rj : ny - 1;
        for (int jj = j_lo; jj <= j_hi; ++jj) {
            const cavity_word f = word_at(ll * ny + jj);
            if (!f) continue;
            out |= pores_spread(f, pores_isqrt(rest - (jj - j) * (jj - j)), xmask);
        }
        if (out == xmask) break;
    }
    return out;
}

}  // namespace pw
