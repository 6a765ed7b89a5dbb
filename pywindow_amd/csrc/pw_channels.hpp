// pw_channels.hpp -- the void of a periodic cell as a network: its connected components under periodic neighbours and,
// for each, in how many dimensions it connects to its own periodic images (include/pywindow_amd.h: pw_channels), single
// source for the gfx950 kernel (pw_channels.hip) and the host path (pw_hostpath.cpp).  The reference has no counterpart.
//
// DEFINED RESULT.  A job is one cell at one probe.
//   atoms    n >= 0 atoms (X, radius) and a probe >= 0.  The job lists every periodic image that matters as an atom of
//            its own: the classification knows nothing of periodicity, only the fill wraps.
//   grid     nx x ny x nz voxels (1 .. 64 each), an origin o and six step components ax; bx, by; cx, cy, cz -- the
//            steps along the cell's first vector (along x), its second (in the xy plane) and its third; ax, by, cz
//            finite and > 0, the rest finite.  Voxel (i, j, l) has the centre
//                z = oz + (double)l*cz
//                y = (oy + (double)j*by) + (double)l*cy
//                x = ((ox + (double)i*ax) + (double)j*bx) + (double)l*cx
//            every product rounded, the sums from left to right, no contraction (channels_x / _y / _z below).
//   free     exactly pw_cavity's test: cavity_free(x - X, y - Y, z - Z, cavity_reach2(radius, probe)), equality is
//            free.  There are no planes: OPEN = FREE.  A row (j, l) runs along x, so y and z are constant over it and
//            cavity_row_clear(y - Y, z - Z, r2) with its proof (pw_cavity.hpp: CULLING) holds unchanged.
//   words    a row (j, l) is one 64-bit word at index l * ny + j, bit i voxel i, as in pw_cavity.  A job may bring
//            ready-made open words in place of the classification; their bits at i >= nx are ignored.
//   neighbours  voxel v has the six neighbours v +- e_k with indices taken mod n_k.  A step +e_k from index n_k - 1, or
//            -e_k from index 0, CROSSES face k.  With n_k = 1 every step along k crosses and the voxel is its own
//            neighbour; with n_k = 2 the two steps reach the same voxel, one crossing and one not.
//   components  the connected components of the open voxels under these neighbours, numbered in the order of their
//            first voxel in rank ((l * ny + j) * nx + i) ascending.
//   winding  for a functional phi in 1 .. 7 (bit 0 = a, bit 1 = b, bit 2 = c) the nodes are (voxel, parity) and a step
//            changes parity iff it crosses a face k whose bit is set in phi.  Bit phi - 1 of a component's `wraps` is
//            set iff (first voxel, 1) is reachable from (first voxel, 0).  A closed walk from the first voxel that
//            crosses face k c_k times in all has the winding vector w in Z^3 with w_k = c_k mod 2 (crossings up minus
//            crossings down has the parity of their sum), and ends at parity phi . w mod 2: the bit is 1 iff the
//            component holds a closed path with phi . w odd.  rank = 3 - log2(1 + number of clear bits).
//
// WHY THE CLEAR BITS FORM A SUBSPACE.  The winding vectors of the closed walks from the first voxel form a group
// (walks concatenate and reverse); their residues mod 2 are a subspace W of (Z/2)^3.  Bit phi - 1 is clear iff phi is
// orthogonal to all of W, so the clear phi with 0 are the subspace K orthogonal to W, of 1, 2, 4 or 8 elements, and
// rank = dim W: 0 a pocket, 1 a channel, 2 a layer, 3 a network.  It is the rank mod 2 of the winding lattice.
// LIMIT.  A component all of whose winding vectors are even reads as a pocket: a double helix of pitch two cells, each
// strand of which comes back to itself only after two cells, is the example.  The same words tiled twice along the
// axis read as rank 1.
//
// THE FILL.  Two bit grids p0, p1 (the two parities) over the words `open`; the fill for phi is the least fixed point of
//     p_q |= open & (the words of p_q, or of p_(1-q) where the step crosses a face of phi, of the row itself shifted by
//                    one bit either way circularly over nx bits and of the four neighbour rows (j +- 1) mod ny,
//                    (l +- 1) mod nz)
// over the bit of the first voxel in p0.  As in pw_cavity.hpp the operator is monotone and only adds nodes reachable
// from the seed, so the fixed point depends neither on the order of the rows nor on which earlier value of a neighbour
// a row saw, and a sweep that changes no word proves it.  A sweep that changes a word adds a node: at most
// 2 * nx * ny * nz sweeps change something.  p0 | p1 is the component, whatever phi is.
//
// FILLS THAT ARE NOT RUN (channels_infer).  n_cross[k] counts the component's voxels at index n_k - 1 whose +e_k
// neighbour is in the component.
//   (1) Every crossing step of the component is such a step or its reverse, so with n_cross[k] == 0 no step of the
//       component crosses face k, and the parity graphs of phi and of phi without bit k are the same graph: bit phi
//       equals bit (phi & cross), cross the set of k with n_cross[k] > 0, and it is 0 when phi & cross == 0.
//   (2) K is a subspace: two clear bits force the bit of their XOR clear, and a clear bit a and a set bit b force the
//       bit of a ^ b set (a ^ b in K would put b = a ^ (a ^ b) in K).
// The first fill of a component runs with phi = 7 and finds the component itself; a pocket that crosses no face costs
// that one fill.
#pragma once
#include "pw_cavity.hpp"

namespace pw {

constexpr int CHAN_MAX_COMPONENTS = 254;              // PW_CHAN_MAX_COMPONENTS
constexpr int CHAN_TRUNCATED = 1;                     // PW_CHAN_TRUNCATED
constexpr int CHAN_LABEL_BEYOND = 254, CHAN_LABEL_CLOSED = 255;
constexpr long CHAN_WORKSPACE_BYTES = 64l << 20;      // open words, masks and labels of the jobs of one launch

PW_HD inline double channels_z(double oz, int l, double cz) { return oz + (double)l * cz; }
PW_HD inline double channels_y(double oy, int j, double by, int l, double cy) { return (oy + (double)j * by) + (double)l * cy; }
PW_HD inline double channels_x(double ox, int i, double ax, int j, double bx, int l, double cx) {
    return ((ox + (double)i * ax) + (double)j * bx) + (double)l * cx;
}

// The x direction of a row taken to its fixed point inside the word, circularly over nx bits: g0 and g1 are the row's
// two parities with what the neighbour rows gave (`from`), kept inside `open`; a step from bit nx - 1 up to bit 0 or from
// bit 0 down to bit nx - 1 crosses face a and changes parity iff swap.  A step that changes something adds one of the
// 2 * nx bits, so after 2 * nx steps nothing is left to add.
PW_HD inline void channels_fill_words(cavity_word from0, cavity_word from1, cavity_word open, int nx, bool swap,
                                      cavity_word& out0, cavity_word& out1) {
    const cavity_word mask = cavity_row_mask(nx);
    cavity_word g0 = from0 & open, g1 = from1 & open;
    for (int step = 0; step < 2 * nx; ++step) {
        const cavity_word in0 = ((g0 << 1) & mask) | (g0 >> 1), in1 = ((g1 << 1) & mask) | (g1 >> 1);
        const cavity_word around0 = ((g0 >> (nx - 1)) & 1ull) | ((g0 & 1ull) << (nx - 1));
        const cavity_word around1 = ((g1 >> (nx - 1)) & 1ull) | ((g1 & 1ull) << (nx - 1));
        const cavity_word n0 = g0 | ((in0 | (swap ? around1 : around0)) & open);
        const cavity_word n1 = g1 | ((in1 | (swap ? around0 : around1)) & open);
        if (n0 == g0 && n1 == g1) break;
        g0 = n0;
        g1 = n1;
    }
    out0 = g0;
    out1 = g1;
}

// What the four neighbour rows of row (j, l) give it: load(q, row) is the word of parity q of a row; a row reached
// across a face of phi gives its other parity.  (With ny == 1 the row is its own neighbour both ways, across face b.)
template <class Load>
PW_HD inline void channels_gather(Load load, int j, int l, int ny, int nz, int phi, cavity_word& from0, cavity_word& from1) {
    auto take = [&](int row, bool swap) {
        const cavity_word a = load(0, row), b = load(1, row);
        from0 |= swap ? b : a;
        from1 |= swap ? a : b;
    };
    take(l * ny + (j > 0 ? j - 1 : ny - 1), j == 0 && (phi & 2));
    take(l * ny + (j + 1 < ny ? j + 1 : 0), j == ny - 1 && (phi & 2));
    take((l > 0 ? l - 1 : nz - 1) * ny + j, l == 0 && (phi & 4));
    take((l + 1 < nz ? l + 1 : 0) * ny + j, l == nz - 1 && (phi & 4));
}

// What is known of a component's seven bits: bit phi - 1 of `known` says that bit phi - 1 of `wraps` is final.
// channels_close draws every conclusion of (2); channels_next returns the next phi in 1 .. 7 whose fill has to be run, or
// 0 when all seven are known, after drawing the conclusions of (1) and (2).  `cross`: bit k set iff n_cross[k] > 0.
PW_HD inline void channels_close(int& known, int& wraps) {
    for (int round = 0; round < 7; ++round) {                        // (a round that learns nothing ends it; 7 bits to learn)
        const int before = known;
        for (int a = 1; a <= 7; ++a) {
            if (!((known >> (a - 1)) & 1) || ((wraps >> (a - 1)) & 1)) continue;      // a: known and clear
            for (int b = 1; b <= 7; ++b) {
                if (b == a || !((known >> (b - 1)) & 1)) continue;
                const int c = a ^ b;
                if ((known >> (c - 1)) & 1) continue;
                known |= 1 << (c - 1);
                wraps |= ((wraps >> (b - 1)) & 1) << (c - 1);
            }
        }
        if (known == before) break;
    }
}
PW_HD inline int channels_next(int cross, int& known, int& wraps) {
    for (int phi = 1; phi <= 7; ++phi) {
        channels_close(known, wraps);
        if ((known >> (phi - 1)) & 1) continue;
        const int same = phi & cross;
        if (same == phi) return phi;
        // (1): the bit of `same`, which is 0 or a smaller phi -- and every smaller phi is known by now
        known |= 1 << (phi - 1);
        if (same) wraps |= ((wraps >> (same - 1)) & 1) << (phi - 1);
    }
    channels_close(known, wraps);
    return 0;
}
// the result of the fill for phi.  (After the first fill, phi = 7, the caller also learns the bit of `cross`: by (1) the
// two are one graph.)
PW_HD inline void channels_learn(int phi, bool reached, int& known, int& wraps) {
    known |= 1 << (phi - 1);
    if (reached) wraps |= 1 << (phi - 1);
}

// what the walk of a component returns, on the host (pw_hostpath.cpp: channels_host_walk) and on the device
// (pw_channels_dev.hpp: chan_walk)
struct ChannelsWalk {
    int wraps, fills;                  // the winding bits; the fills that were run (1 .. 7)
    long n_voxels, n_cross[3];         // of the component, from the first fill
};

PW_HD inline int channels_rank(int wraps) {
    const int clear = 7 - cavity_popcount((cavity_word)(wraps & 127));
    return clear == 7 ? 0 : clear == 3 ? 1 : clear == 1 ? 2 : 3;     // (clear + 1 is 8, 4, 2 or 1)
}

// the voxels of row (j, l) of a component, word f, at index n_k - 1 whose +e_k neighbour is in the component; up_j and
// up_l: the component's words of the rows (0, l) and (j, 0)
PW_HD inline void channels_row_cross(cavity_word f, cavity_word up_j, cavity_word up_l, int nx, int ny, int nz, int j, int l,
                                     long cross[3]) {
    cross[0] = (long)(((f >> (nx - 1)) & f) & 1ull);
    cross[1] = j == ny - 1 ? cavity_popcount(f & up_j) : 0;
    cross[2] = l == nz - 1 ? cavity_popcount(f & up_l) : 0;
}

}  // namespace pw
