// pw_superpose.hpp -- least-squares superposition of two sets of points (include/pywindow_amd.h: pw_superpose),
// single source for the gfx950 kernels (pw_superpose.hip) and the host path (pw_hostpath.cpp).  The reference has
// no counterpart: it never brings two frames into one orientation.
//
// DEFINED RESULT.  For a job with mobile points x_i, target points y_i and weights w_i (1.0 where the job has
// none), i in [0, n):
//
//   SUMS.  Every sum over the atoms is taken by SUP_ACC = 64 accumulators: accumulator l starts at +0.0 and takes
//   the atoms i = l, l + 64, l + 128, ... in that order with the update written below; then the accumulators are
//   folded, acc[l] = acc[l] + acc[l + s] for l < s, with s = 32, 16, 8, 4, 2, 1, and acc[0] is the sum.  (IEEE
//   addition is commutative to the bit, so a butterfly acc[l] + acc[l ^ s] leaves that same sum in every lane.)
//
//   (a)  W   : acc = acc + w_i                      sx_a : acc = fma(w_i, x_ia, acc)     sy_a : acc = fma(w_i, y_ia, acc)
//        cx_a = sx_a / W,  cy_a = sy_a / W          (centre_mobile, centre_target)
//   (b)  dx_a = x_ia - cx_a,  dy_b = y_ib - cy_b    M[a][b] : acc = fma(w_i, dx_a * dy_b, acc)
//        (the product is rounded first, so that M is symmetric to the bit when mobile and target are the same rows)
//   HORN.  N is the symmetric 4 x 4 of sup_horn() below, every entry a sum or difference of entries of M in the
//   order written there.  Cyclic Jacobi (sup_jacobi): before every sweep off = the sum of |N[p][q]|, p < q, and
//   diag = the sum of |N[p][p]|; the iteration ends when off == 0, when off <= 1e-300 + 1e-22 * diag, or after
//   SUP_MAX_SWEEPS sweeps.  A sweep visits (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); an entry that is exactly 0
//   is passed over; otherwise theta = (N[q][q] - N[p][p]) / (2 N[p][q]), t = sign(theta) / (|theta| + sqrt(theta^2
//   + 1)), c = 1 / sqrt(t^2 + 1), s = t c, and rows and columns p, q of N and columns p, q of the eigenvector
//   matrix V (the identity at the start) are rotated as written in sup_rotate.  `sweeps` counts the sweeps done.
//   lambda[0] is the largest diagonal entry, the lowest index among equals, lambda[1] the largest of the other
//   three.  The quaternion is that column of V, negated when its first component that is not 0 is negative, and
//   divided by sqrt(fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0)))); the rotation is sup_rotation().  It is a
//   proper rotation whatever the input: n = 1 gives N = 0, no sweep and the identity.
//   (c)  dx, dy as in (b);  r_a = fma(R[a][2], dx_2, fma(R[a][1], dx_1, R[a][0] * dx_0));  e_a = r_a - dy_a;
//        E : acc = fma(w_i, fma(e_2, e_2, fma(e_1, e_1, e_0 * e_0)), acc);      rmsd = sqrt(E / W)
//        (a direct sum of residuals: G_x + G_y - 2 lambda cancels for similar structures)
//
// Only + - * / sqrt and fma occur, all of them correctly rounded on both paths (-ffp-contract=off), and the orders
// are written in the source: the result does not depend on the device, the launch geometry, how the jobs of a call
// are cut into launches to bound the workspace, the thread count of the host path or the run, and the two paths
// return the same bits.  No floating-point atomics, no MFMA.  Weights that are all exactly 1.0 give the bits of a
// job without weights (fma(1, x, acc) is acc + x); other equal weights scale W, the sums and M by roundings of
// their own and agree only to rounding.  A coordinate beyond about 1e150 overflows the products: not checked.
#pragma once
#include "pw_common.hpp"

namespace pw {

constexpr int SUP_ACC = 64;                         // accumulators of a sum: the lanes of a wave
constexpr int SUP_MAX_SWEEPS = 30;
constexpr long SUP_WORKSPACE_BYTES = 16l << 20;     // moments and rotations of one launch (pw_superpose.hip)
constexpr int SUP_MOMENT_FIELDS = 16;               // M[9], centre_mobile[3], centre_target[3], W
constexpr int SUP_SOLVE_FIELDS = 12;                // rotation[9], lambda[2], sweeps
constexpr long SUP_JOB_WORKSPACE = 8l * (SUP_MOMENT_FIELDS + SUP_SOLVE_FIELDS);

// ---- the per-atom updates of accumulator l: `w` null means weights of 1.0 -------------------------------------
struct SupSums {                 // pass (a)
    double w, x[3], y[3];
};
struct SupCentres {
    double cx[3], cy[3], W;
};

PW_HD inline double sup_weight(const double* w, long i) { return w ? w[i] : 1.0; }

PW_HD inline void sup_sums_zero(SupSums& s) {
    s.w = 0.0;
    for (int a = 0; a < 3; ++a) s.x[a] = s.y[a] = 0.0;
}

PW_HD inline void sup_sums_atom(SupSums& s, const double* x, const double* y, const double* w, long i) {
    const double wi = sup_weight(w, i);
    s.w = s.w + wi;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.x[a] = pw_fma(wi, x[3 * i + a], s.x[a]);
        s.y[a] = pw_fma(wi, y[3 * i + a], s.y[a]);
    }
}

PW_HD inline void sup_centres(const SupSums& s, SupCentres& c) {
    c.W = s.w;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c.cx[a] = s.x[a] / s.w;
        c.cy[a] = s.y[a] / s.w;
    }
}

// pass (b): m[3 * a + b]
PW_HD inline void sup_moment_atom(double (&m)[9], const SupCentres& c, const double* x, const double* y, const double* w,
                                  long i) {
    const double wi = sup_weight(w, i);
    double dx[3], dy[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        dx[a] = x[3 * i + a] - c.cx[a];
        dy[a] = y[3 * i + a] - c.cy[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) m[3 * a + b] = pw_fma(wi, dx[a] * dy[b], m[3 * a + b]);
}

// pass (c): r[3 * a + b] the rotation
PW_HD inline double sup_residual_atom(double acc, const double (&r)[9], const SupCentres& c, const double* x, const double* y,
                                      const double* w, long i) {
    const double wi = sup_weight(w, i);
    double dx[3], e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dx[a] = x[3 * i + a] - c.cx[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ra = pw_fma(r[3 * a + 2], dx[2], pw_fma(r[3 * a + 1], dx[1], r[3 * a] * dx[0]));
        e[a] = ra - (y[3 * i + a] - c.cy[a]);
    }
    return pw_fma(wi, pw_fma(e[2], e[2], pw_fma(e[1], e[1], e[0] * e[0])), acc);
}

// the fold of SUP_ACC accumulators held in an array (the host path; the device folds across lanes)
PW_HD inline double sup_fold(double* acc) {
    for (int s = SUP_ACC / 2; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) acc[l] = acc[l] + acc[l + s];
    return acc[0];
}

// ---- Horn's 4 x 4 from M (m[3 * a + b] = sum of w x_a y_b over the centred points) -----------------------------
PW_HD inline void sup_horn(const double (&m)[9], double (&N)[4][4]) {
    const double Sxx = m[0], Sxy = m[1], Sxz = m[2], Syx = m[3], Syy = m[4], Syz = m[5], Szx = m[6], Szy = m[7], Szz = m[8];
    N[0][0] = (Sxx + Syy) + Szz;
    N[1][1] = (Sxx - Syy) - Szz;
    N[2][2] = (Syy - Sxx) - Szz;
    N[3][3] = (Szz - Sxx) - Syy;
    N[0][1] = N[1][0] = Syz - Szy;
    N[0][2] = N[2][0] = Szx - Sxz;
    N[0][3] = N[3][0] = Sxy - Syx;
    N[1][2] = N[2][1] = Sxy + Syx;
    N[1][3] = N[3][1] = Szx + Sxz;
    N[2][3] = N[3][2] = Syz + Szy;
}

// one Jacobi rotation in the (P, Q) plane; indices are compile-time so that a and v stay in registers
template <int P, int Q>
PW_HD inline void sup_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (pw_abs(theta) + pw_sqrt(theta * theta + 1.0));
    const double c = 1.0 / pw_sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = a[r][P], arq = a[r][Q];
            a[r][P] = a[P][r] = c * arp - s * arq;
            a[r][Q] = a[Q][r] = s * arp + c * arq;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = v[r][P], vrq = v[r][Q];
        v[r][P] = c * vrp - s * vrq;
        v[r][Q] = s * vrp + c * vrq;
    }
}

// eigenvalues on the diagonal of a, eigenvectors in the columns of v; returns the sweeps done
PW_HD inline int sup_jacobi(double (&a)[4][4], double (&v)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < SUP_MAX_SWEEPS; ++sweeps) {
        const double off = ((((pw_abs(a[0][1]) + pw_abs(a[0][2])) + pw_abs(a[0][3])) + pw_abs(a[1][2])) + pw_abs(a[1][3])) +
                           pw_abs(a[2][3]);
        const double diag = ((pw_abs(a[0][0]) + pw_abs(a[1][1])) + pw_abs(a[2][2])) + pw_abs(a[3][3]);
        if (off == 0.0 || off <= 1e-300 + 1e-22 * diag) break;
        sup_rotate<0, 1>(a, v);
        sup_rotate<0, 2>(a, v);
        sup_rotate<0, 3>(a, v);
        sup_rotate<1, 2>(a, v);
        sup_rotate<1, 3>(a, v);
        sup_rotate<2, 3>(a, v);
    }
    return sweeps;
}

// the rotation of a unit quaternion (q0, q1, q2, q3), r[3 * a + b]
PW_HD inline void sup_rotation(const double (&q)[4], double (&r)[9]) {
    const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
    r[0] = ((q0 * q0 + qx * qx) - qy * qy) - qz * qz;
    r[1] = 2.0 * (qx * qy - q0 * qz);
    r[2] = 2.0 * (qx * qz + q0 * qy);
    r[3] = 2.0 * (qx * qy + q0 * qz);
    r[4] = ((q0 * q0 - qx * qx) + qy * qy) - qz * qz;
    r[5] = 2.0 * (qy * qz - q0 * qx);
    r[6] = 2.0 * (qx * qz - q0 * qy);
    r[7] = 2.0 * (qy * qz + q0 * qx);
    r[8] = ((q0 * q0 - qx * qx) - qy * qy) + qz * qz;
}

// M -> rotation, the two largest eigenvalues and the sweeps: the whole of HORN above
PW_HD inline int sup_solve(const double (&m)[9], double (&r)[9], double (&lambda)[2]) {
    double a[4][4], v[4][4];
    sup_horn(m, a);
    const int sweeps = sup_jacobi(a, v);
    // the largest diagonal entry, the lowest index among equals; selects, no run-time index
    double best = a[0][0];
    double q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
    double second = -PW_INF;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool take = a[j][j] > best;
        const double lower = take ? best : a[j][j];
        second = lower > second ? lower : second;
        best = take ? a[j][j] : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = take ? v[i][j] : q[i];
    }
    lambda[0] = best;
    lambda[1] = second;
    const double lead = q[0] != 0.0 ? q[0] : q[1] != 0.0 ? q[1] : q[2] != 0.0 ? q[2] : q[3];
    const double norm = pw_sqrt(pw_fma(q[3], q[3], pw_fma(q[2], q[2], pw_fma(q[1], q[1], q[0] * q[0]))));
    const double sign = lead < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (sign * q[i]) / norm;
    sup_rotation(q, r);
    return sweeps;
}

}  // namespace pw
