// pw_charges_cell.hpp -- partial charges of a periodic crystal cell by charge equilibration (include/pywindow_amd.h:
// pw_charges_cell), single source for the gfx950 kernels (pw_charges_cell.hip) and the host path (pw_hostpath.cpp).  It is
// pw_charges.hpp's model on a cell: Ohno-Klopman shielding at short range, switched smoothly to the point-charge law, whose
// lattice sum is Ewald's (pw_ewald.hpp's wave vectors and phase arithmetic).  The reference has no counterpart.
//
// WHY THE SWITCH.  The shielding correction K / sqrt(r^2 + a^2) - K / r falls off as r^-3 and a_ij is not separable, so a
// neutral cell does not cancel it: cut at the Ewald cutoff the charges never settle.  Gaussian shielding matched at r = 0
// is indefinite on the neutral subspace with the bundled parameters.  With the correction taken to zero between shield_on
// and shield_off the matrix is positive definite on the neutral subspace of the CC3 cell (0.65 .. 244 eV) and the charges
// no longer depend on the cutoff or on the Ewald tolerance.  The switch range is a MODEL PARAMETER of the job.
//
// DEFINED RESULT.  A job has n >= 1 atoms x_i in the triangular frame of the cell's edges (a1, b1, b2, c1, c2, c3) -- the
// lattice vectors a = (a1, 0, 0), b = (b1, b2, 0), c = (c1, c2, c3) --, rows (chi_i, J_i) in eV, K = coulomb in eV
// Angstrom, alpha >= 0, cutoff2, shield_on2 < shield_off2 <= cutoff2, n_k rows (h, k, l, w) with w in eV, tol, max_iter.
// The atoms are taken as they are: wrapping them into the cell is the caller's.  The charges minimise sum chi_i q_i + 1/2
// q^T A q at sum q = 0, A = D + R + G.
//
//   D  D_i = J_i - (K * alpha) * 1.1283791670955126 (2 / sqrt(pi) as this literal): chc_self.
//   R  row i is the LIST of its counting terms: the candidates (j, m), j = 0 .. n - 1 ascending and for each j the image m =
//      0 .. 26 ascending, m = 9 (la + 1) + 3 (lb + 1) + (lc + 1) with la, lb, lc in {-1, 0, 1}; the candidate (i, 13) -- the
//      atom itself -- is left out, an atom's own images (j == i, m != 13) are candidates.  The shift of image m is chc_shift:
//      tx = ((double)la * a1 + (double)lb * b1) + (double)lc * c1, ty = (double)lb * b2 + (double)lc * c2, tz = (double)lc *
//      c3; d = (x_i - x_j) + t component by component, r2 = fma(dz, dz, fma(dy, dy, dx * dx)).  A candidate COUNTS when r2 <=
//      cutoff2 (equality counts).  Its value is chc_term:
//          u = (r2 - on2) / (off2 - on2) clamped to [0, 1];  s = 1.0 - ((u * u) * u) * ((10.0 - 15.0 * u) + (6.0 * u) * u);
//          r2 > 0:  r = sqrt(r2), a = (2.0 * K) / (J_i + J_j),
//                   value = s * (K / sqrt(r2 + a * a) - K / r) + (K * pw_erfc(alpha * r)) / r;
//          r2 == 0: value = s * ((J_i + J_j) / 2.0) - (K * alpha) * 1.1283791670955126 (the limit; finite, as coincident
//                   atoms are in pw_charges).
//      TWENTY-SEVEN IMAGES SUFFICE when the atoms are wrapped and sqrt(cutoff2) is at most the cell's smallest
//      perpendicular width: two wrapped atoms differ by less than one in every fractional coordinate, so an image with an
//      |index| >= 2 along an axis is more than one whole cell away along it, farther than that axis' perpendicular width.
//      The entry does not check either condition; the Python layer enforces both.
//   G  G_ij = sum_k w_k cos(k . (x_i - x_j)), the diagonal included, never formed.  THE PHASES ARE BUILT ONCE A JOB from
//      per-atom per-axis tables: with H, Kx, Lx the largest |h|, |k|, |l| of the job's rows, E_a[m][j] = ewald_sincos(
//      ewald_dot(ewald_kvec(edges, 1, 1, 1, m, 0, 0), x_j)) for m = 0 .. H, and likewise (0, m, 0) for m = 0 .. Kx and (0, 0, m)
//      for m = 0 .. Lx.  The entry of a negative index is that of its magnitude with the sine negated (c, -s).  The phase of
//      (row k, atom j) is chc_phase: ewald_add(ewald_add(E_a[h], E_b[k]), E_c[l]).  Whether a phase is kept or combined
//      again at every product cannot show.
//   PRODUCT  y = A p:  Sc_k = sum_j p_j c_kj and Ss_k = sum_j p_j s_kj by the rule of the sums with acc = fma(p_j, c_kj, acc);
//      real_i = the rule over the entries e = 0, 1, ... of row i's list with acc = fma(value_e, p_column(e), acc);
//      rec_i = the rule over the rows k with acc = fma(w_k, c_ki * Sc_k + s_ki * Ss_k, acc) (products rounded, then their
//      sum);  y_i = (D_i * p_i + real_i) + rec_i.
//   SUMS  pw_charges.hpp's rule: SUP_ACC = 64 accumulators from +0.0, accumulator l takes the terms l, l + 64, ... in rising
//      index, folded by sup_fold's order.  A plain sum is acc = acc + v.
//   SOLVER  projected, Jacobi-preconditioned conjugate gradients on the neutral subspace, one system.
//      sJ = sum of 1.0 / J_i (plain sum).  The preconditioned residual of r: u_i = r_i / J_i, lambda = (sum u) / sJ,
//      z_i = u_i - lambda / J_i, and r.z is taken as the rule's sum with acc = fma(r_i - lambda, z_i, acc).  (In exact
//      arithmetic sum z = 0 and the two are equal.  In floating point sum z is a rounding residue, and the plain r.z would
//      carry lambda times that residue: first order in the rounding where the true value is second order.  Held against
//      (tol * tol) * rz0 that term keeps a converged job running on directions that are noise, and 12 atoms without a pair
//      end at the unconstrained minimum, sum q = -6.9 e.)  Start: q = 0, r = -chi, z and lambda from r, p = z, rz = r.z,
//      rz0 = rz.  At step k = 0, 1, ...:
//        1. the job freezes with iterations = k when rz <= (tol * tol) * rz0;
//        2. else when k == max_iter it ends with iterations = k and CHG_NOT_CONVERGED, the charges of the last step written;
//        3. else y = A p and pAp = p.y; when !(pAp > 0) it ends with iterations = k and CHG_BREAKDOWN;
//        4. else al = rz / pAp, q_i = fma(al, p_i, q_i), r_i = fma(-al, y_i, r_i), z and lambda from r, rz' = r.z, beta = rz' /
//           rz, p_i = fma(beta, p_i, z_i), rz = rz'.
//   RESULT  mu = -lambda of the last residual (the equalised electronegativity; it does not depend on alpha), energy = 0.5 *
//      chi.q, q_min and q_max by pw_charges' accumulators and fold, iterations, flags (CHG_NOT_CONVERGED, CHG_BREAKDOWN, and
//      CHG_NO_SUM for !(sJ > 0)).  With one of the last two the charges, mu, energy, q_min and q_max are NaN.  Every double
//      leaves through chg_canon.  No dipole: a periodic cell has none that survives re-wrapping.  No total charge: the cell
//      is neutral, and a neutralising background drops out of q and of mu.
//
// Only + - * / sqrt, fma, pw_erfc and pw_sincos occur, the same code on both paths (-ffp-contract=off): the device, the
// host path and a restatement return the same bytes whatever the launch geometry, the grouping of the jobs into launches,
// where the vectors live and whether a row or a phase is stored or recomputed.  No atomics, no MFMA.
//
// CHC_LDS_ATOMS.  The solver's six vectors (q, r, z, p, y, J) are 48 bytes an atom.  The 160 KB of a CU hold 3413 atoms; two
// workgroups a CU, so that one's barrier does not idle the CU, leave 1706 each; 1536 = 24 * 64 is the multiple of the 64
// accumulators below that (72 KB).  The 1344 atoms of the CC3 cell fit.  Larger jobs keep the vectors in the workspace.
//
// LEFT OUT BY DESIGN.  Slater integrals, the hydrogen hardness correction, any dependence on a guest.
#pragma once
#include "pw_charges.hpp"
#include "pw_ewald.hpp"

namespace pw {

constexpr int CHC_VECTORS = 6;                        // q, r, z, p, y, J
constexpr int CHC_LDS_ATOMS = 1536;
// rows, tables and structure factors of the jobs of one launch: a CC3 frame at 12 Angstrom keeps about 11 MB, so 4 GiB are
// some 370 frames a launch, more workgroups than the device has CUs
constexpr long CHC_WORKSPACE_BYTES = 4096l << 20;
constexpr int CHC_IMAGES = 27, CHC_SELF_IMAGE = 13;
constexpr double CHC_TWO_OVER_SQRT_PI = 1.1283791670955126;

PW_HD inline double chc_self(double K, double alpha) { return (K * alpha) * CHC_TWO_OVER_SQRT_PI; }

// the shift of image m by the edges e = (a1, b1, b2, c1, c2, c3)
PW_HD inline void chc_shift(const double* e, int m, double* tx, double* ty, double* tz) {
    const double la = (double)(m / 9 - 1), lb = (double)((m / 3) % 3 - 1), lc = (double)(m % 3 - 1);
    *tx = (la * e[0] + lb * e[1]) + lc * e[3];
    *ty = lb * e[2] + lc * e[4];
    *tz = lc * e[5];
}

PW_HD inline double chc_r2(double xi, double yi, double zi, double xj, double yj, double zj, double tx, double ty, double tz) {
    const double dx = (xi - xj) + tx, dy = (yi - yj) + ty, dz = (zi - zj) + tz;
    return pw_fma(dz, dz, pw_fma(dy, dy, dx * dx));
}

PW_HD inline double chc_switch(double r2, double on2, double off2) {
    double u = (r2 - on2) / (off2 - on2);
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    return 1.0 - ((u * u) * u) * ((10.0 - 15.0 * u) + (6.0 * u) * u);
}

// the value of a counting candidate
PW_HD inline double chc_term(double r2, double Ji, double Jj, double K, double alpha, double on2, double off2) {
    const double s = chc_switch(r2, on2, off2);
    if (r2 == 0.0) return s * ((Ji + Jj) / 2.0) - chc_self(K, alpha);
    const double r = pw_sqrt(r2);
    const double a = (2.0 * K) / (Ji + Jj);
    const double shielded = K / pw_sqrt(r2 + a * a);
    const double point = K / r;
    const double e = pw_erfc(alpha * r);
    return s * (shielded - point) + (K * e) / r;
}

// the wave vector whose indices are m along `axis` and 0 along the other two
PW_HD inline EwaldK chc_axis_kvec(const double* e, int axis, int m) {
    return ewald_kvec(e, 1, 1, 1, axis == 0 ? (double)m : 0.0, axis == 1 ? (double)m : 0.0, axis == 2 ? (double)m : 0.0);
}

// the table entry of a signed index from that of its magnitude
PW_HD inline EwaldCS chc_signed(double c, double s, int index) {
    EwaldCS r;
    r.c = c;
    r.s = index < 0 ? -s : s;
    return r;
}

// the tables of a job: for axis a the entries m = 0 .. top[a] of the n atoms, cosines then sines: entry (a, m, j) has its
// cosine at first[a] + (2 * m) * n + j and its sine n further
struct ChcTables {
    long first[3];
    int top[3];
};
PW_HD inline long chc_table_words(const int* top, long n) { return 2 * n * ((long)top[0] + top[1] + top[2] + 3); }
PW_HD inline void chc_tables_layout(ChcTables& T, long n) {
    T.first[0] = 0;
    T.first[1] = 2 * n * ((long)T.top[0] + 1);
    T.first[2] = T.first[1] + 2 * n * ((long)T.top[1] + 1);
}
template <class I>
PW_HD inline EwaldCS chc_phase(const double* tab, const ChcTables& T, I n, I j, int h, int k, int l) {
    const double* A = tab + T.first[0] + (long)(2 * (h < 0 ? -h : h)) * n + j;
    const double* B = tab + T.first[1] + (long)(2 * (k < 0 ? -k : k)) * n + j;
    const double* C = tab + T.first[2] + (long)(2 * (l < 0 ? -l : l)) * n + j;
    return ewald_add(ewald_add(chc_signed(A[0], A[n], h), chc_signed(B[0], B[n], k)), chc_signed(C[0], C[n], l));
}

// one term of rec_i
PW_HD inline double chc_rec_term(EwaldCS ph, double Sc, double Ss) { return ph.c * Sc + ph.s * Ss; }

// the scalar state of the solver between two steps
struct ChcState {
    double rz, rz0, lambda;
    int iterations;
    bool ran_out, broke;
};

PW_HD inline int chc_flags(const ChcState& S, double sJ) {
    return (S.ran_out ? CHG_NOT_CONVERGED : 0) | (S.broke ? CHG_BREAKDOWN : 0) | (sJ > 0.0 ? 0 : CHG_NO_SUM);
}

}  // namespace pw
