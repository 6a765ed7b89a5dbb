// pw_cluster.hpp -- conformational clustering of frames by the gromos method (Daura et al. 1999; include/pywindow_amd.h:
// pw_cluster_gromos), single source for the gfx950 kernels (pw_cluster.hip) and the host path (pw_hostpath.cpp).  The
// reference has no counterpart.
//
// DEFINED RESULT.  A job has an n x n row-major matrix d of which ONLY the strict upper triangle is read, and a cutoff.
// Frames i != j are neighbours iff d[min(i, j)][max(i, j)] <= cutoff; every frame is a neighbour of itself; all frames
// start active.  While a frame is active: count for every active frame its active neighbours (itself included); the
// centre c is the active frame with the largest count, the smallest index among equals; cluster k (0, 1, ... in the
// order found) is c with its active neighbours -- labels[j] = k, centres[k] = c, sizes[k] = the count -- and its
// members become inactive.
//
// Every output is an integer, so the result is the definition itself whatever the order of the work.  Both paths take
// the bit-parallel form: the matrix is thresholded ONCE into a bit matrix bits[n][S] of 64-bit words, bit j % 64 of
// word j / 64 of row i set iff i and j are neighbours (the diagonal included; bits at columns >= n are zero), the lower
// triangle being the transpose of the upper by 64 x 64 bit tiles; S is the W = (n + 63) / 64 words of a row rounded up
// to an even number, so that a row is a whole number of 16-byte loads (the padding word is zero).  A count is
// sum_w popcount(bits[i][w] & active[w]), and centre and count come from the maximum of the keys
// (count << 32) | (0xFFFFFFFF - i): the larger count wins, then the smaller index; an integer maximum does not
// depend on the order it is taken in, and 0 is the key of no frame (a count is at least 1).
#pragma once
#include "pw_common.hpp"
#include "pw_gate.hpp"

namespace pw {

constexpr int CLUSTER_MAX_N = 32768;                 // PW_CLUSTER_MAX_N
constexpr long CLUSTER_SLAB_BYTES = 64l << 20;       // rows of the matrix on the device at a time (pw_cluster.hip)
constexpr long CLUSTER_BITS_BYTES = 256l << 20;      // bit matrices of the jobs that share the launches of a round
constexpr int CLUSTER_ROUNDS = 32;                   // count + pick rounds queued between two looks at the done flags

typedef unsigned long long cluster_word;

PW_HD inline long cluster_words(long n) { return (n + 63) / 64; }                 // W
PW_HD inline long cluster_stride(long n) { return (cluster_words(n) + 1) & ~1l; } // S

// the neighbour predicate of two different frames (a NaN distance never reaches this: the entry refuses it)
PW_HD inline bool cluster_neighbour(double d, double cutoff) { return d <= cutoff; }

// the bit of column `col` in row `row`'s word as the pack sees it: the diagonal, or an upper-triangle neighbour; `d`
// is only meaningful (and has only been read) when row < col < n
PW_HD inline bool cluster_pack_bit(long row, long col, long n, double d, double cutoff) {
    return col < n && (col == row || (col > row && cluster_neighbour(d, cutoff)));
}

PW_HD inline cluster_word cluster_key(unsigned count, unsigned row) {
    return ((cluster_word)count << 32) | (cluster_word)(0xFFFFFFFFu - row);
}
PW_HD inline unsigned cluster_key_count(cluster_word key) { return (unsigned)(key >> 32); }
PW_HD inline unsigned cluster_key_row(cluster_word key) { return 0xFFFFFFFFu - (unsigned)key; }

// the bits of word w that belong to columns < n: all ones below the last word, the low n % 64 in a last word that
// is cut short, zero from word W on (the padding word)
PW_HD inline cluster_word cluster_tail_mask(long n, long w) {
    const long left = n - 64 * w;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}

PW_HD inline int cluster_popcount(cluster_word v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

}  // namespace pw
