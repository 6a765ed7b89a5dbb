// pw_charges.hpp -- partial charges of an isolated molecule by charge equilibration (include/pywindow_amd.h:
// pw_charges), single source for the gfx950 kernel (pw_charges.hip) and the host path (pw_hostpath.cpp).  The method
// is QEq (Rappe and Goddard 1991) with the Slater overlap integrals replaced by Ohno-Klopman shielding.  The reference
// has no counterpart.
//
// DEFINED RESULT.  A job has n atoms at x_i with parameters (chi_i, J_i) in eV, a total charge Q in e, Coulomb's constant
// K in eV Angstrom, a tolerance tol and a bound max_iter.  The charges minimise sum chi_i q_i + 1/2 q^T A q at sum q = Q.
//
//   MATRIX.  A_ii = J_i.  For i != j, A_ij = chg_pair(): with d = x_i - x_j, r2 = fma(dz, dz, fma(dy, dy, dx * dx)),
//   a = (2.0 * K) / (J_i + J_j), A_ij = K / sqrt(r2 + a * a) (the product rounded first).  Symmetric to the bit, and
//   (J_i + J_j) / 2 at r = 0: coincident atoms are finite.  Whether an element is stored or recomputed cannot show.
//
//   SUMS.  Every dot product, every row of y = A p and every sum over the atoms follows the rule of pw_superpose.hpp:
//   SUP_ACC = 64 accumulators that start at +0.0, accumulator l takes the terms l, l + 64, ... in rising index by
//   acc = fma(u, v, acc) (acc = acc + v for a plain sum), and the accumulators are folded by sup_fold's order.  The terms
//   of row i are A_ij * p_j over all j, the diagonal at its index.
//
//   SOLVER.  Two systems, A s = -chi (system 0) and A t = 1 (system 1), go through Jacobi-preconditioned conjugate
//   gradients in lockstep.  Each starts from x = 0, r = b, z_i = r_i / J_i, p = z, rz = r.z, bb = b.b, rr = bb.  At step
//   k = 0, 1, ..., for each system that is not frozen:
//     1. it freezes with iterations = k when rr <= (tol * tol) * bb;
//     2. otherwise Ap and pAp = p.Ap are taken;
//     3. it freezes with iterations = k and the breakdown flag when !(pAp > 0);
//     4. otherwise alpha = rz / pAp, x_i = fma(alpha, p_i, x_i), r_i = fma(-alpha, Ap_i, r_i), z_i = r_i / J_i,
//        rz' = r.z, rr = r.r, beta = rz' / rz, p_i = fma(beta, p_i, z_i), rz = rz'.
//   A frozen system is no longer touched.  The loop ends before step k when both are frozen, or when k == max_iter: then
//   the systems still running get iterations = max_iter and the not-converged flag is set.  Every loop is bounded.
//
//   RESULT.  S = sum s, T = sum t, mu = (Q - S) / T, q_i = fma(mu, t_i, s_i), energy = 0.5 * (chi.q + mu * Q),
//   dipole_a = sum of fma(q_i, x_ia, acc).  q_min and q_max go through the same 64 accumulators (+inf and -inf at the
//   start, acc = q < acc ? q : acc and acc = q > acc ? q : acc) and the same fold (acc[l] = acc[l + s] < acc[l] ?
//   acc[l + s] : acc[l], and > for the maximum).  flags: CHG_NOT_CONVERGED, CHG_BREAKDOWN, CHG_NO_SUM (!(T > 0)).  With
//   CHG_BREAKDOWN or CHG_NO_SUM the charges, mu, energy, dipole, q_min and q_max are NaN; sum_s and sum_t stay.  Every
//   double that leaves is passed through chg_canon(): a NaN, whatever made it, leaves as 0x7ff8000000000000 (the sign
//   of a NaN that an operation makes differs between the host and the device).
//
// Only + - * / sqrt and fma occur, all correctly rounded on both paths (-ffp-contract=off): the result does not depend
// on the device, the launch geometry, where the vectors live, how the jobs are cut into launches, the thread count of
// the host path or the run, and the two paths return the same bits.  No atomics, no MFMA.
#pragma once
#include "pw_superpose.hpp"   // SUP_ACC, sup_fold: the rule of the sums

namespace pw {

constexpr int CHG_NOT_CONVERGED = 1, CHG_BREAKDOWN = 2, CHG_NO_SUM = 4;
constexpr double CHG_TOL_MIN = 1e-14, CHG_TOL_MAX = 1e-2;
constexpr long CHG_MAX_ITER = 100000;
constexpr int CHG_VECTORS = 14;                     // doubles an atom of a job's state: x y z, J and five vectors a system
constexpr int CHG_LDS_ATOMS = 512;                  // a job of at most so many atoms keeps its state in LDS (56 KB)
constexpr long CHG_WORKSPACE_BYTES = 64l << 20;     // the state of the larger jobs of one launch (pw_charges.hip)

PW_HD inline double chg_nan() {
    union { unsigned long long u; double d; } c;
    c.u = 0x7ff8000000000000ull;
    return c.d;
}
PW_HD inline double chg_canon(double v) { return v != v ? chg_nan() : v; }

// A_ij, i != j
PW_HD inline double chg_pair(double xi, double yi, double zi, double Ji, double xj, double yj, double zj, double Jj, double K) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    const double r2 = pw_fma(dz, dz, pw_fma(dy, dy, dx * dx));
    const double a = (2.0 * K) / (Ji + Jj);
    return K / pw_sqrt(r2 + a * a);
}

// the scalar state of one system between two steps
struct ChgSystem {
    double rz, rr, bb;
    int iterations;
    bool frozen, broke;
};

// step 1 of SOLVER for system S at step k
PW_HD inline void chg_freeze_check(ChgSystem& S, double tol2, int k) {
    if (!S.frozen && S.rr <= tol2 * S.bb) {
        S.frozen = true;
        S.iterations = k;
    }
}

// step 3: true when the system goes on to step 4
PW_HD inline bool chg_curvature_ok(ChgSystem& S, double pAp, int k) {
    if (pAp > 0.0) return true;
    S.frozen = S.broke = true;
    S.iterations = k;
    return false;
}

PW_HD inline int chg_flags(const ChgSystem& s0, const ChgSystem& s1, bool ran_out, double T) {
    return (ran_out ? CHG_NOT_CONVERGED : 0) | (s0.broke || s1.broke ? CHG_BREAKDOWN : 0) | (T > 0.0 ? 0 : CHG_NO_SUM);
}

}  // namespace pw
