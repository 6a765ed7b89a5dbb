// pw_cavity.hpp -- the cavity of a cage as a voxel flood fill closed at its windows (include/pywindow_amd.h: pw_cavity),
// single source for the gfx950 kernel (pw_cavity.hip) and the host path (pw_hostpath.cpp).  The reference has no
// counterpart: its pore_volume is the volume of the largest inscribed sphere, a lower bound on the cavity.
//
// DEFINED RESULT.  A job has n atoms (X, radius), a probe radius, a grid of nx x ny x nz voxels (1 .. 64 each) with an
// origin o and a spacing h, m planes (a, b, c, d) and a seed voxel.  Voxel (i, j, l) has the centre
// x = o_x + (double)i * h (one product, one addition, no fma), likewise y and z.  It is FREE iff for every atom
//     (dx*dx + dy*dy) + dz*dz >= (radius + probe) * (radius + probe),   dx = x - X, ...      (equality is free)
// and OPEN iff it is free and ((a*x + b*y) + c*z) <= d for every plane.  The CAVITY is the 6-connected component of
// open voxels that holds the seed voxel, empty if the seed voxel is not open.  All of it FP64 without contraction in the
// association written; every output is an integer -- counts, sums of indices and of their products, a bounding box --
// so the result is the definition itself whatever the order of the work.
//
// Both paths take the bit-parallel form: a row (j, l) of the grid is ONE 64-bit word, bit i voxel i, at index
// l * ny + j; bits at i >= nx are zero.  The fill is the least fixed point of
//     fill |= open & (fill << 1 | fill >> 1 | the words of the four neighbour rows)
// over the seed bit.  The operator is monotone and only ever adds voxels of the component, so the fixed point does not
// depend on the order in which rows are visited or on which of a neighbour's earlier values a row saw; a sweep over
// all rows that changes no word has seen the final words and so proves the fixed point.  A sweep that changes a word
// adds a voxel: at most nx * ny * nz sweeps change something.
//
// CULLING.  A row may skip an atom when dy*dy + dz*dz >= r2: rounding is monotone and dx*dx >= 0, so
// fl(dx*dx + dy*dy) >= dy*dy and fl(fl(dx*dx + dy*dy) + dz*dz) >= fl(dy*dy + dz*dz) >= r2 -- every voxel of the row
// passes that atom's test.  Nothing else is culled.
#pragma once
#include "pw_common.hpp"

namespace pw {

constexpr int CAVITY_MAX_G = 64;                      // PW_CAVITY_MAX_G
constexpr int CAVITY_SEED_CLOSED = 1;                 // PW_CAV_SEED_CLOSED
constexpr long CAVITY_WORKSPACE_BYTES = 64l << 20;    // open words and masks of the jobs of one launch (pw_cavity.hip)

typedef unsigned long long cavity_word;

PW_HD inline double cavity_coord(double o, int i, double h) { return o + (double)i * h; }
PW_HD inline double cavity_reach2(double radius, double probe) {
    const double r = radius + probe;
    return r * r;
}
// every voxel of a row at (dy, dz) from the atom is free of it (see CULLING)
PW_HD inline bool cavity_row_clear(double dy, double dz, double r2) { return dy * dy + dz * dz >= r2; }
PW_HD inline bool cavity_free(double dx, double dy, double dz, double r2) { return (dx * dx + dy * dy) + dz * dz >= r2; }
PW_HD inline bool cavity_inside(double a, double b, double c, double d, double x, double y, double z) {
    return ((a * x + b * y) + c * z) <= d;
}
PW_HD inline bool cavity_inside(const double* plane, double x, double y, double z) {
    return cavity_inside(plane[0], plane[1], plane[2], plane[3], x, y, z);
}

// the bits of the voxels of a row: the low nx
PW_HD inline cavity_word cavity_row_mask(int nx) { return nx >= 64 ? ~0ull : (1ull << nx) - 1ull; }

// the voxel (i, j, l) of a rank = (l * ny + j) * nx + i into v[3]; (-1, -1, -1) for a negative rank: no such voxel
PW_HD inline void grid_voxel(long rank, int nx, int ny, int* v) {
    const long row = rank / nx;
    v[0] = rank >= 0 ? (int)(rank - row * nx) : -1;
    v[1] = rank >= 0 ? (int)(row % ny) : -1;
    v[2] = rank >= 0 ? (int)(row / ny) : -1;
}

PW_HD inline int cavity_popcount(cavity_word v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// `from` (the row's own fill and its neighbour rows' words, OR-ed) spread inside the open word to the fixed point of
// the x direction; a step that changes something adds a bit, so 64 steps are the bound
PW_HD inline cavity_word cavity_fill_word(cavity_word from, cavity_word open) {
    cavity_word g = from & open;
    for (int step = 0; step < 64; ++step) {
        const cavity_word next = g | (((g << 1) | (g >> 1)) & open);
        if (next == g) break;
        g = next;
    }
    return g;
}

// of the set bits i of a word: how many, the sum of i and the sum of i * i, from popcounts -- with i = sum_b 2^b i_b,
// sum i = sum_b 2^b |w & M_b| and sum i^2 = sum_b sum_c 2^(b+c) |w & M_b & M_c|, M_b the positions whose bit b is set
PW_HD inline void cavity_word_sums(cavity_word w, long& count, long& sum, long& sum2) {
    constexpr cavity_word M[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                  0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    count = cavity_popcount(w);
    long s = 0, s2 = 0;
    for (int b = 0; b < 6; ++b) {
        const cavity_word wb = w & M[b];
        s += (long)cavity_popcount(wb) << b;
        s2 += (long)cavity_popcount(wb) << (2 * b);
        for (int c = b + 1; c < 6; ++c) s2 += (long)cavity_popcount(wb & M[c]) << (b + c + 1);
    }
    sum = s;
    sum2 = s2;
}

// the voxels of row (j, l) of the cavity, word f, that lie on a face of the grid
PW_HD inline long cavity_row_face(cavity_word f, int nx, int ny, int nz, int j, int l) {
    const bool edge_row = j == 0 || j == ny - 1 || l == 0 || l == nz - 1;
    return cavity_popcount(edge_row ? f : f & (1ull | (1ull << (nx - 1))));
}

// what a row of the cavity adds to a job's result.  f: the row's word; ym, yp (rows j -+ 1) and zm, zp (rows l -+ 1):
// the neighbour rows' words, 0 outside the grid.  The sums are in the order of pw_cavity_out.
struct CavityRow {
    long n, surface, face;
    long first[3];
    long second[6];
};
PW_HD inline void cavity_row_sums(cavity_word f, cavity_word ym, cavity_word yp, cavity_word zm, cavity_word zp, int nx,
                                  int ny, int nz, int j, int l, CavityRow& r) {
    long n, si, sii;
    cavity_word_sums(f, n, si, sii);
    const cavity_word inner = f & (f << 1) & (f >> 1) & ym & yp & zm & zp;   // (bit nx of f is zero, and so is "bit -1")
    r.n = n;
    r.surface = cavity_popcount(f & ~inner);
    r.face = cavity_row_face(f, nx, ny, nz, j, l);
    r.first[0] = si;
    r.first[1] = n * j;
    r.first[2] = n * l;
    r.second[0] = sii;
    r.second[1] = n * j * j;
    r.second[2] = n * l * l;
    r.second[3] = si * j;
    r.second[4] = si * l;
    r.second[5] = n * j * l;
}

}  // namespace pw
