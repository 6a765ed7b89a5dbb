// pw_sasa.hpp -- the solvent-accessible surface of a cage by Shrake and Rupley's test points, split into the part that
// faces the cavity and the part that faces the outside (include/pywindow_amd.h: pw_sasa), single source for the gfx950
// kernel (pw_sasa.hip) and the host path (pw_hostpath.cpp).  The reference has no counterpart.
//
// DEFINED RESULT.  A call has P unit directions u_k (1 <= P <= 4096), shared by its jobs.  A job has n atoms
// (X, radius), a probe radius and, optionally, a bit grid in the layout of pw_cavity's mask: nx x ny x nz voxels
// (1 .. 64 each), an origin o, a spacing h > 0 and ny * nz words, row (j, l) at index l * ny + j, bit i voxel i.
// Atom i has the reach R_i = radius_i + probe (one addition) and the test points
//     p = X_i + R_i * u_k            component by component: one product, one addition, no fma.
// A point is EXPOSED iff for every atom j != i -- excluded by its index, not by its position --
//     (dx*dx + dy*dy) + dz*dz >= R_j * R_j,   dx = p_x - X_j,x, ...                      (equality is exposed)
// and an exposed point is INSIDE iff the job has a grid and at least one of the up to eight voxels at the corners of the
// grid cell that holds p is set: along x, i0 is the largest i in [0, nx) with o_x + (double)i * h <= p_x (cavity_coord),
// -1 if there is none; the corners are i0 and i0 + 1, those outside [0, nx) dropped; likewise y and z.  cavity_coord is
// monotone in i (rounding is monotone and h > 0), so a bisection by comparisons finds i0 and nothing is divided.  Bits
// at i >= nx are never looked at.  All of it FP64 without contraction in the association written; the outputs are the
// numbers of exposed and of inside points of every atom and their sums over the job -- integers, so the result is the
// definition itself whatever the order of the work.
//
// CULLING.  Atom j may be skipped for atom i when sasa_far holds:
//     D2 = (ex*ex + ey*ey) + ez*ez >= (t * t) * (1 + 2^-26),   e = X_i - X_j,   t = (R_i + R_j) + s,   s = 2^-45 * M,
// M being the largest |coordinate| and the largest reach of the job, and only for 2^-400 <= M <= 2^400 (otherwise
// s = -1 and nothing is culled: sasa_slack).  Claim: then every test point of i passes j's test.  With eps = 2^-53:
//   (a) No operation above overflows (all magnitudes <= 2^402, squares <= 2^806).  t >= s >= 2^-445, so t * t and D2
//       are >= 2^-890: a product that underflows adds at most 2^-1074 to sums that large, a relative 2^-184, which the
//       factors below absorb.
//   (b) e_a = fl(X_i,a - X_j,a) has one rounding, so D2 <= |X_i - X_j|^2 (1 + eps)^5 and
//       |X_i - X_j|^2 >= D2 (1 - 6 eps) >= t^2 (1 + 2^-26)(1 - 8 eps) >= t^2 (1 + 1.4e-8), i.e.
//       |X_i - X_j| >= t (1 + 6.9e-9) >= (R_i + R_j)(1 + 6e-9) + s      (t >= ((R_i + R_j)(1 - eps) + s)(1 - eps)).
//   (c) The computed point: p_a = fl(X_i,a + fl(R_i u_a)) differs from X_i,a + R_i u_a by at most
//       eps (|X_i,a| + 2.1 R_i |u_a|) <= 3.2 eps M, and |u| <= 1 + 1e-9 (the entry checks |u|^2 to 1e-9), so
//       |p - X_i| <= R_i (1 + 1e-9) + 6 eps M and |p - X_j| >= |X_i - X_j| - |p - X_i| >= R_j (1 + 6e-9) + s - 6 eps M
//       >= R_j (1 + 6e-9) + 250 eps M                                                     (s = 256 eps M).
//   (d) The test computes d_a = fl(p_a - X_j,a) and fl(fl(d_x^2 + d_y^2) + d_z^2) >= |p - X_j|^2 (1 - eps)^5 (1 - 2^-180)
//       >= R_j^2 (1 + 1.1e-8) >= fl(R_j * R_j): the point passes.                                                   qed
// The rule is conservative by about 1e-8 of the distance: it only ever skips tests that pass, so the result does not
// show whether it ran, and there is no capacity in n.
#pragma once
#include "pw_cavity.hpp"

namespace pw {

constexpr int SASA_MAX_POINTS = 4096;                 // PW_SASA_MAX_POINTS
constexpr int SASA_GRID = 1;                          // PW_SASA_GRID
constexpr double SASA_UNIT_TOLERANCE = 1e-9;          // | |u|^2 - 1 | of a direction
constexpr double SASA_CULL_FACTOR = 1.0 + 0x1p-26;
constexpr double SASA_SLACK = 0x1p-45;
constexpr double SASA_BIG_MAX = 0x1p400;
constexpr double SASA_BIG_MIN = 0x1p-400;

PW_HD inline double sasa_reach(double radius, double probe) { return radius + probe; }
PW_HD inline double sasa_point(double X, double R, double u) { return X + R * u; }
PW_HD inline bool sasa_exposed(double dx, double dy, double dz, double r2) { return cavity_free(dx, dy, dz, r2); }
PW_HD inline bool sasa_unit(double ux, double uy, double uz) {
    const double d = ((ux * ux + uy * uy) + uz * uz) - 1.0;
    return d <= SASA_UNIT_TOLERANCE && -d <= SASA_UNIT_TOLERANCE;
}

// the s of CULLING for a job whose largest |coordinate| or reach is `big`; negative: nothing is culled
PW_HD inline double sasa_slack(double big) { return big >= SASA_BIG_MIN && big <= SASA_BIG_MAX ? big * SASA_SLACK : -1.0; }
// every test point of an atom with the reach Ri passes the test of an atom with the reach Rj at e = X_i - X_j (see CULLING)
PW_HD inline bool sasa_far(double ex, double ey, double ez, double Ri, double Rj, double slack) {
    const double t = (Ri + Rj) + slack;
    return slack >= 0.0 && (ex * ex + ey * ey) + ez * ez >= (t * t) * SASA_CULL_FACTOR;
}

// the largest i in [0, n) with cavity_coord(o, i, h) <= p, -1 if there is none: at most 7 halvings of [-1, n)
PW_HD inline int sasa_cell(double o, double h, int n, double p) {
    int lo = -1, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;                              // (lo + hi >= 0 here: lo = -1 meets hi >= 1)
        if (cavity_coord(o, mid, h) <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// one of the corners of the cell that holds p is set; word(r): the word of row r = l * ny + j
template <class Words>
PW_HD inline bool sasa_inside(double px, double py, double pz, const double* o, double h, int nx, int ny, int nz, Words word) {
    const int i0 = sasa_cell(o[0], h, nx, px), j0 = sasa_cell(o[1], h, ny, py), l0 = sasa_cell(o[2], h, nz, pz);
    cavity_word bits = 0;                                            // (i0 <= nx - 1 <= 63: both shifts are defined)
    if (i0 >= 0) bits |= 1ull << i0;
    if (i0 + 1 < nx) bits |= 1ull << (i0 + 1);
    cavity_word any = 0;
    for (int l = l0 < 0 ? 0 : l0; l <= l0 + 1 && l < nz; ++l)
        for (int j = j0 < 0 ? 0 : j0; j <= j0 + 1 && j < ny; ++j) any |= word(l * ny + j) & bits;
    return any != 0;
}

// the M of CULLING: the largest |coordinate| and the largest reach of a job (host side of both paths)
PW_HD inline double sasa_magnitude(const double* atoms, const double* radii, long n, double probe) {
    double big = 0.0;
    for (long a = 0; a < n; ++a) {
        for (int c = 0; c < 3; ++c) big = pw_max(big, pw_abs(atoms[3 * a + c]));
        big = pw_max(big, sasa_reach(radii[a], probe));
    }
    return big;
}

}  // namespace pw
