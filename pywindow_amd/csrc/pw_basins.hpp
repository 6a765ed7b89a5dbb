// pw_basins.hpp -- the energy basins of a guest's landscape in a periodic cell, the dividing surfaces between them and
// the Boltzmann sums over both (include/pywindow_amd.h: pw_basins).  Single source: the gfx950 kernels (pw_basins.hip)
// and the host path (pw_hostpath.cpp: pw_hostpath_basins) compile the functions below; this comment is the text of
// record.  The reference has no counterpart.
//
//   GRID     pw_percolation's: nx, ny, nz in 1 .. 64, origin, step, the centres by channels_x / _y / _z, rank
//            (l*ny + j)*nx + i.  FIELD: pw_percolation's -- field_first == -1: the Lennard-Jones field of the atoms in
//            pw_field_dev.hpp's order and association (+inf at a blocked voxel); field_first >= 0: the caller's field,
//            every value finite or +inf; map_first >= 0: the field is also written to map.
//   ALLOWED  U_v is not +inf and U_v <= cap (cap finite or +inf).  n_blocked counts the voxels at +inf, n_allowed the
//            allowed ones; u_min is the allowed voxel first in (key, rank), key = pas_key (the two zeros tie).
//   DESCENT  every allowed voxel v has one parent: of the candidates v itself, then its allowed neighbours in the order
//            -a, +a, -b, +b, -c, +c (indices mod n_k; with n_k == 1 the neighbour is v itself and no candidate), the one
//            with the smallest (key(U), rank, position in that order).  A step from index n_k - 1 to 0 along +e_k crosses
//            +e_k, the reverse step crosses -e_k; with n_k == 2 the two neighbours along k are one voxel through two
//            faces and tie in (key, rank), so the position decides: the step through the face of -e_k is taken -- it
//            crosses -e_k from index 0 and nothing from index 1.  A root has p(r) == r.  o(v), three integers, is the sum
//            of the crossings along the chain of parents from v to its root.  A plateau may hold several roots.
//   BASINS   the roots numbered 0 .. B-1 by ascending rank; basin(v) is the number of v's root.  Row of a basin: root,
//            n_voxels, u_min (the bits the root holds), and per beta (Z, E) with pw_affinity's WEIGHT: x = -(beta*U),
//            x > 700: x = 700 and PW_BAS_CLAMPED, w = pw_exp(x), terms w and w*U.  z[b], e[b] with b >= n_betas: +0.0.
//   EDGES    for every allowed v and k = 0, 1, 2 with v' = v + e_k allowed (n_k == 1: v' is v): c = e_k if v has index
//            n_k - 1 else 0, a = basin(v), b = basin(v'), d = c + o(v') - o(v).  The face is interior iff a == b and
//            d == 0; otherwise it belongs to the edge (a, b, d), made canonical: if a > b, or a == b and the first
//            non-zero component of d is negative, (b, a, -d).  The face's term is the larger of U_v, U_v' by key and on
//            a tie the bits of U_v.  Row of an edge: a, b, d, n_faces, saddle = the smallest term by key (its bits),
//            saddle_voxel (the rank of v) and saddle_k of the lowest (rank of v, k) among the faces whose term ties
//            with it, and per beta THREE sums s[b][k] = the sum of w(term) over the edge's faces across e_k: the rates
//            of the Python layer weigh a face by its area a_k, so the sums are kept per k (the edge's S is their sum
//            in the order k = 0, 1, 2).  Edges are written in ascending (a, b, d_a, d_b, d_c).
//   SUMS     no grouping shows.  A chunk is a row (j, l) of the grid, slots i = 0 .. 63; a slot holds +0.0 beyond nx,
//            where its voxel (its face (v, k), which sits in v's slot) is no member of the group, or is not allowed.
//            Within a chunk pw_affinity's tree: slot[t] += slot[t + k] for k = 1, 2, .. 32 and every t a multiple of
//            2k.  A total starts at +0.0 and takes its chunk sums in row order l*ny + j.  Every weight is >= +0.0, a
//            chunk of Z or S without a member is +0.0; a chunk of E without a member is +0.0 too and a total that
//            started at +0.0 is never -0.0, so a chunk without a member may be skipped.  No floating-point atomics.
//   RANGE    BAS_MAX_OFFSET = 255: a component of some o(v) or of some d beyond +-255 sets PW_BAS_RANGE; then no edge
//            is written, n_edges is 0 and every o of the labels is written as 0 (basins do not depend on o and are
//            written).  The device stores (parent, o) in one 8-byte word with 10 bits a component: the offset between
//            a voxel and an ancestor is a difference of two o, within +-510 when every o is in range.
//   OVERFLOW B > b_cap or E > e_cap sets PW_BAS_OVERFLOW: the first min(B, b_cap) basins are written and no edge;
//            n_basins and n_edges are the true counts either way (n_edges 0 under PW_BAS_RANGE only).
//   LABELS   label_first >= 0: per voxel basin(v) (-1 where not allowed) and o(v).
//
// PROOFS.  (1) Descent ends: the parent of v is v or a candidate that is before v in the strict total order (key, rank)
// of the voxels (a neighbour that ties in both is v itself and no candidate wins over v at position 0), so (key, rank)
// strictly falls along parents and a chain of V voxels ends at a root after fewer than V steps.
// (2) The in-place jumping is monotone: a word (q, t) of v always says "q is an ancestor of v (or v) and t is the sum of
// the crossings from v to q".  True at the start (q = p(v)).  A step reads (q, t) of v and (q', t') of q as ONE 8-byte
// word each, so (q', t') was true of q at some time and ancestors only move towards the root; it writes (q', t + t'),
// which is true of v.  A root's word never changes, a word that names a root is final, so a stale read can only delay;
// with synchronous rounds the distance to the root halves, and racy rounds are no slower: ceil(log2 V) + 1 rounds.
// (3) Levels: let allowed_t be the sub-level set and G_t the graph {basins with u_min <= t, edges with saddle <= t}.  A
// voxel of allowed_t reaches its root inside allowed_t (keys fall along parents), so basins with u_min <= t are exactly
// the basins that meet allowed_t and each is connected inside it.  A face between two voxels of allowed_t that is not
// interior is a face of an edge whose saddle (a minimum of terms) is <= its term = max(U_v, U_v') <= t; conversely an
// edge with saddle <= t has a face with both voxels in allowed_t.  So the components of allowed_t and of G_t correspond.
// Windings: replace every step of a closed walk in allowed_t by the descent chains: the crossing sum of a step v -> v'
// is o(v) + d - o(v') for its face's d (0 for an interior face), and the o telescope on a closed walk, so the walk's net
// crossing is the sum of the d of the edges it uses, signed: the winding groups agree as integers.
#pragma once
#include "pw_channels.hpp"
#include "pw_passage.hpp"

namespace pw {

constexpr int BAS_OVERFLOW = 1;                      // PW_BAS_OVERFLOW
constexpr int BAS_CLAMPED = 2;                       // PW_BAS_CLAMPED
constexpr int BAS_RANGE = 4;                         // PW_BAS_RANGE
constexpr int BAS_MAX_BETAS = 8;                     // PW_BAS_MAX_BETAS
constexpr int BAS_MAX_OFFSET = 255;                  // PW_BAS_MAX_OFFSET
constexpr long BAS_WORKSPACE_BYTES = 1l << 30;       // the workspaces of the jobs of one launch: a 50^3 job with the
                                                     // first capacities of the Python layer takes about 12 MB, and a
                                                     // launch should hold a workgroup for every compute unit or so

constexpr unsigned long long BAS_NONE = ~0ull;       // a word of a voxel that is not allowed; an empty slot; no key

PW_HD inline bool bas_allowed(double U, unsigned long long cap_key) {
    const unsigned long long key = pas_key(U);
    return key != PAS_KEY_INF && key <= cap_key;
}

// the voxel one step along direction q = 0 .. 5 (-a, +a, -b, +b, -c, +c) of (i, j, l) and what the step crosses
// (cross[k] in -1, 0, 1); false where n_k == 1
PW_HD inline bool bas_step(int q, int i, int j, int l, int nx, int ny, int nz, long& rank, int* cross) {
    const int k = q >> 1, up = q & 1;
    const int n = k == 0 ? nx : k == 1 ? ny : nz, at = k == 0 ? i : k == 1 ? j : l;
    cross[0] = cross[1] = cross[2] = 0;
    if (n == 1) return false;
    const int over = up ? (at == n - 1 ? 1 : 0) : (at == 0 ? -1 : 0);
    const int to = up ? (at == n - 1 ? 0 : at + 1) : (at == 0 ? n - 1 : at - 1);
    cross[0] = k == 0 ? over : 0;
    cross[1] = k == 1 ? over : 0;
    cross[2] = k == 2 ? over : 0;
    rank = ((long)(k == 2 ? to : l) * ny + (k == 1 ? to : j)) * nx + (k == 0 ? to : i);
    return true;
}

// the parent of the allowed voxel (i, j, l) of rank v and the crossing of the step to it; value(rank): U there
template <class Value>
PW_HD inline long bas_parent(int i, int j, int l, long v, int nx, int ny, int nz, unsigned long long cap_key, Value value, int* cross) {
    unsigned long long best = pas_key(value(v));
    long best_rank = v;
    cross[0] = cross[1] = cross[2] = 0;
    for (int q = 0; q < 6; ++q) {                                    // (the candidates in order: a strict < keeps the earlier)
        long r;
        int c[3];
        if (!bas_step(q, i, j, l, nx, ny, nz, r, c)) continue;
        const double U = value(r);
        if (!bas_allowed(U, cap_key)) continue;
        const unsigned long long key = pas_key(U);
        if (pas_before(key, r, best, best_rank)) {
            best = key;
            best_rank = r;
            cross[0] = c[0]; cross[1] = c[1]; cross[2] = c[2];
        }
    }
    return best_rank;
}

// the term of the face between v and v' = v + e_k: the larger by key, on a tie the bits of U_v
PW_HD inline double bas_term(double Uv, double Uw) { return pas_key(Uw) > pas_key(Uv) ? Uw : Uv; }

// the canonical form of the edge (a, b, d) in place
PW_HD inline void bas_canonical(int& a, int& b, int* d) {
    const int lead = d[0] ? d[0] : d[1] ? d[1] : d[2];
    if (a > b || (a == b && lead < 0)) {
        const int t = a;
        a = b;
        b = t;
        d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
    }
}

PW_HD inline bool bas_in_range(const int* d) {
    return d[0] >= -BAS_MAX_OFFSET && d[0] <= BAS_MAX_OFFSET && d[1] >= -BAS_MAX_OFFSET && d[1] <= BAS_MAX_OFFSET &&
           d[2] >= -BAS_MAX_OFFSET && d[2] <= BAS_MAX_OFFSET;
}

// an edge in range as one integer that orders as (a, b, d_a, d_b, d_c): 18 + 18 + 3 * 9 bits; never BAS_NONE
PW_HD inline unsigned long long bas_edge_key(int a, int b, const int* d) {
    return ((unsigned long long)a << 45) | ((unsigned long long)b << 27) | ((unsigned long long)(d[0] + 256) << 18) |
           ((unsigned long long)(d[1] + 256) << 9) | (unsigned long long)(d[2] + 256);
}
PW_HD inline void bas_edge_unkey(unsigned long long key, int& a, int& b, int* d) {
    a = (int)(key >> 45);
    b = (int)((key >> 27) & 0x3ffffull);
    d[0] = (int)((key >> 18) & 0x1ffull) - 256;
    d[1] = (int)((key >> 9) & 0x1ffull) - 256;
    d[2] = (int)(key & 0x1ffull) - 256;
}

}  // namespace pw
