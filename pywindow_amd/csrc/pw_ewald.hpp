// pw_ewald.hpp -- the Ewald sum of a framework's point charges, added to the pose energy of a rigid linear guest at every
// voxel of a periodic cell (include/pywindow_amd.h: pw_rigid_cell_ewald), single source for the gfx950 kernels
// (pw_ewald.hip, pw_rigid_cell.hip) and the host path (pw_hostpath.cpp).  It is pw_rigid_cell.hpp's definition with one
// more pair term and one more term a pose; this file is the text of record of both.  Every association of every sum and
// product is written out below; nothing is fused (-ffp-contract=off, no pw_fma here).  The reference has no counterpart.
//
// DEFINED RESULT.  A job is a pw_rigid_cell job (grid, listed atoms X with their images, core2, cutoff2, L betas, S offsets
// t_s, M directions d_o) and
//     charged (0 or 1);
//     alpha >= 0, finite, in 1 / Angstrom;
//     rows (A, B, C) per (site, listed atom), row s * n + a, THREE doubles a row, the layout of pw_rigid_affinity;
//     C = coulomb * q_site * q_atom in kJ/mol Angstrom, finite, |C| <= 1e100;
//     S site charges q_s, finite, |q_s| <= 1e100;
//     n_cell CELL ATOMS, rows (x, y, z, q): the atoms of the primary cell only, in the job's triangular frame, finite,
//     |q| <= 1e100.  They make the structure factors; the listed atoms with their images make the real-space part;
//     K rows (h, k, l, w), 0 <= K <= EWALD_MAX_K: integer-valued doubles |h|, |k|, |l| <= EWALD_MAX_INDEX and a finite
//     weight w.  They are data, as the directions are: nothing derives them, orders them or checks that they are a half
//     space or that w is the weight of (h, k, l).
//   With charged == 0 the job is pw_rigid_cell's definition verbatim: C, q_s, the cell atoms, alpha and the K rows are
//   neither read nor evaluated, and the entry returns that entry's bytes.  The rest is for charged == 1.
//   REAL SPACE  in the per-site pair loop a counting atom (aff_counts(r2, cutoff2)) contributes ewald_pair:
//            u = aff_pair(r2, A, B); r = pw_sqrt(r2); e = pw_erfc(alpha * r); u = u + (C * e) / r -- the products are
//            rounded, then the division is taken.  The truncation at cutoff2 by aff_counts is part of the definition.
//            pw_erfc(0.0) == 1.0 exactly and (C * 1.0) / r == C / r, so alpha == 0 with K == 0 on a cell with step =
//            (h, 0, h, 0, 0, h) gives the bytes of a charged pw_rigid_affinity job over the whole grid.
//            THE SKIP of pw_rigid_cell.hpp needs no new proof: an atom that is left out has r2 > cutoff2 in every pose of
//            the group, does not count and contributes nothing, whatever the pair term is.
//   RECIPROCAL SPACE  per job, for K > 0, in this order:
//     (1) the wave vector of row k, ewald_kvec: with a1 = nx * ax, b1 = ny * bx, b2 = ny * by, c1 = nz * cx, c2 = nz * cy,
//         c3 = nz * cz (the cell's edges from step) the reciprocal rows a* = (1 / a1, -(b1 / (a1 * b2)), (b1 * c2 - b2 * c1) /
//         ((a1 * b2) * c3)), b* = (0, 1 / b2, -(c2 / (b2 * c3))), c* = (0, 0, 1 / c3) and kx = 2pi * (h * a*x), ky = 2pi *
//         (h * a*y + k * b*y), kz = 2pi * ((h * a*z + k * b*z) + l * c*z); k . p = (kx * px + ky * py) + kz * pz (ewald_dot).
//         A sine and cosine are ewald_sincos: pw_sincos, and NaN for both when the angle is beyond 1.05e8 or not a
//         number (pw_sincos is not specified there);
//     (2) the STRUCTURE FACTORS Sc_k = sum_j q_j cos(k . x_j) and Ss_k = sum_j q_j sin(k . x_j) over the cell atoms: 64
//         strided accumulators from +0.0, accumulator t takes j = t, t + 64, ... in order as acc = acc + q_j * cos, then
//         the 64 are folded pairwise by pw_affinity.hpp's tree (1, 2, 4, 8, 16, 32);
//     (3) the guest's FORM FACTORS per orientation, Fc_ok = sum_s q_s cos(phi) and Fs_ok = sum_s q_s sin(phi) with phi =
//         ewald_dot(k, t_s * dx, t_s * dy, t_s * dz) -- rigid_site's rounded products --, s in order from +0.0 as F = F +
//         q_s * cos;
//     (4) the tables P_ok = w_k * (Sc_k * Fc_ok + Ss_k * Fs_ok) and Q_ok = w_k * (Ss_k * Fc_ok - Sc_k * Fs_ok), and the
//         phase of the origin (c0_k, s0_k) = ewald_sincos(ewald_dot(k, origin));
//     (5) per pose Urec(v, o) = sum_k (P_ok * c_kv + Q_ok * s_kv): k in list order, one accumulator from +0.0, the term
//         (P * c) + (Q * s) added as acc = acc + term.  (c_kv, s_kv) are the cosine and sine of k . x_v.  The grid is the
//         cell cut into nx x ny x nz, so k . x_v = k . origin + 2pi (h i / nx + k j / ny + l m / nz) for the voxel (i, j, m),
//         and they are built from per-axis tables of exact integers, pw_dft.hpp's idiom: ewald_axis(n, q) = ewald_sincos((2pi
//         * (double)q) / (double)n) at q = (h * i) mod nx, (k * j) mod ny and (l * m) mod nz (the non-negative residue),
//         combined by angle addition in the order ((origin + x) + y) + z with ewald_add: c = ca * cb - sa * sb, s = sa * cb
//         + ca * sb.
//   POSE ENERGY  U = U_0 + U_1 + ... as in pw_rigid_cell, then, for K > 0, U = U + Urec(v, o) last.  (With K == 0 the sum
//            is empty and nothing is added: a pose energy is never -0.0, so adding +0.0 would change no bit either.)
//            The weight, the fold, the sums, the record, the partial and everything written are pw_rigid_cell's.
// The same bytes result on the device, on a device == -1 context, with the skip on or off and in any launch geometry or
// grouping of the jobs.
//
// EWALD_MAX_K = 4096.  A cubic cell of edge a at a real-space cutoff rc and tolerance tol needs about (2/3) pi (kmax a /
// 2pi)^3 half-space rows, kmax = 2 * (-ln tol) / rc: 1700 for the 25 Angstrom cell of CC3 at 12 Angstrom and 1e-6.  4096
// leaves room for 1e-8 on that cell or for a cutoff of 9 Angstrom at 1e-6, and keeps the tables P and Q of a job of 1024
// orientations at 64 MiB.  EWALD_MAX_INDEX = 64 = the grid's cap: an index times a voxel index stays an exact small integer.
//
// LEFT OUT BY DESIGN.  The guest's interaction with its own periodic images: infinite dilution.  Any self or background
// term: there is none in a framework-guest energy when the framework is neutral, which the Python layer enforces and this
// entry does not check.  Non-linear guests.  The charges are given: periodic charge equilibration is an entry of its own,
// pw_charges_cell (pw_charges_cell.hpp), which takes this file's wave vectors and phase arithmetic.
#pragma once
#include "pw_rigid_cell.hpp"

namespace pw {

constexpr int EWALD_MAX_K = 4096;                    // PW_EWALD_MAX_K
constexpr int EWALD_MAX_INDEX = 64;                  // PW_EWALD_MAX_INDEX
constexpr int EWALD_OT = 4;                          // orientations a register tile of the reciprocal kernel; no result shows it
constexpr double EWALD_TWO_PI = 6.283185307179586;
constexpr double EWALD_MAX_ANGLE = 1.05e8;           // pw_sincos's range (pw_math.hpp)

// the pair term of a counting atom of a charged job, on top of u = aff_pair(r2, A, B)
template <class Tab>
PW_HD inline double ewald_pair(double u, double r2, double C, double alpha, Tab tab) {
    const double r = pw_sqrt(r2);
    const double e = pw_erfc_tab(alpha * r, tab);
    const double ce = C * e;
    return u + ce / r;
}

struct EwaldK {
    double x, y, z;
};
PW_HD inline EwaldK ewald_kvec(const double* s, int nx, int ny, int nz, double h, double k, double l) {
    const double a1 = (double)nx * s[0], b1 = (double)ny * s[1], b2 = (double)ny * s[2];
    const double c1 = (double)nz * s[3], c2 = (double)nz * s[4], c3 = (double)nz * s[5];
    const double ax = 1.0 / a1, ay = -(b1 / (a1 * b2)), az = (b1 * c2 - b2 * c1) / ((a1 * b2) * c3);
    const double by = 1.0 / b2, bz = -(c2 / (b2 * c3)), cz = 1.0 / c3;
    EwaldK K;
    K.x = EWALD_TWO_PI * (h * ax);
    K.y = EWALD_TWO_PI * (h * ay + k * by);
    K.z = EWALD_TWO_PI * ((h * az + k * bz) + l * cz);
    return K;
}
PW_HD inline double ewald_dot(const EwaldK& K, double px, double py, double pz) { return (K.x * px + K.y * py) + K.z * pz; }

struct EwaldCS {
    double c, s;
};
PW_HD inline EwaldCS ewald_sincos(double angle) {
    EwaldCS r;
    if (!(pw_abs(angle) <= EWALD_MAX_ANGLE)) {
        r.c = r.s = pw_bits2d(0x7ff8000000000000ull);
        return r;
    }
    pw_sincos(angle, &r.s, &r.c);
    return r;
}
// entry q of the table of an axis cut into n: 0 <= q < n
PW_HD inline EwaldCS ewald_axis(int n, int q) { return ewald_sincos((EWALD_TWO_PI * (double)q) / (double)n); }
// the non-negative residue of index * voxel modulo n: |index| <= EWALD_MAX_INDEX, 0 <= voxel < n <= 64
PW_HD inline int ewald_residue(int index, int voxel, int n) {
    const int m = (int)((unsigned)((index < 0 ? -index : index) * voxel) % (unsigned)n);
    return index < 0 && m ? n - m : m;
}
PW_HD inline EwaldCS ewald_add(EwaldCS a, EwaldCS b) {
    EwaldCS r;
    r.c = a.c * b.c - a.s * b.s;
    r.s = a.s * b.c + a.c * b.s;
    return r;
}

// step (3) and (4) for one (k, o): the form factors of the guest and the row's entries of P and Q
PW_HD inline void ewald_pq(const EwaldK& K, double w, double Sc, double Ss, const double* ts, const double* qs, int S, double dx,
                           double dy, double dz, double* P, double* Q) {
    double Fc = 0.0, Fs = 0.0;
    for (int s = 0; s < S; ++s) {
        const EwaldCS f = ewald_sincos(ewald_dot(K, ts[s] * dx, ts[s] * dy, ts[s] * dz));
        Fc = Fc + qs[s] * f.c;
        Fs = Fs + qs[s] * f.s;
    }
    *P = w * (Sc * Fc + Ss * Fs);
    *Q = w * (Ss * Fc - Sc * Fs);
}

// one term of step (5)
PW_HD inline double ewald_term(double P, double Q, EwaldCS v) { return (P * v.c) + (Q * v.s); }

// the words of a charged job with K > 0 in the workspace of its launch, after pw_rigid_cell's records and partials: the
// three axis tables (64 pairs each), per row (c0, s0), then (P, Q) per (orientation, row); then Urec per (orientation,
// voxel).  (The host path keeps the axis tables of a group in vectors of its own.)
constexpr int EWALD_AXIS_WORDS = 6 * EWALD_MAX_INDEX;
PW_HD inline long ewald_table_words(long K, long M) { return EWALD_AXIS_WORDS + 2 * K + 2 * M * K; }
PW_HD inline long ewald_urec_words(long V, long M) { return M * V; }

// what the host path takes beyond pw_rigid_cell's arguments (pw_hostpath.cpp: pw_hostpath_rigid_cell); the firsts of a job
// index these arrays as the caller's arrays of pw_rigid_cell_ewald
struct EwaldHostJob {
    long charge_first, cell_first, n_cell, k_first, n_k;
    double alpha;
    int charged;
};
struct EwaldHost {
    const EwaldHostJob* jobs;
    const double* site_q;
    const double* cell;          // rows (x, y, z, q)
    const double* kvecs;         // rows (h, k, l, w)
};

}  // namespace pw
