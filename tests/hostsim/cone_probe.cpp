// tests/hostsim/cone_probe.cpp -- the cone and lattice helpers of team_ray_tests (pywindow_amd/csrc/pw_unit.hpp) for
// tests/test_cone_lattice.py: one atom's candidates as the kernel's lanes enumerate them, piece by piece, beside the
// rays of its band that pass the kernel's dot test.  Test infrastructure only.
#include <vector>
#include "../../pywindow_amd/csrc/pw_unit.hpp"
using namespace pw;
// One atom at rel (from the centre) with radius vr, a sphere of P rays of radius R, cn = |centre|.
// cand[0 .. return value): the candidates (at most cap are stored); info = {klo, khi, narrowed, pieces, loop iterations};
// brute[k] = 1 for every k of the band with dot >= thr (one-sided bands) -- P bytes.  A band that is not narrowed has
// every k of it for candidates.
extern "C" int hs_cone_candidates(int P, double R, const double* rel, double vr, double cn, int* cand, int cap,
                                  int* info, unsigned char* brute) {
    Sphere sp;
    sp.init(R, P);
    ConeBand b;
    ConeLattice L;
    const int pieces = cone_of_atom(rel[0], rel[1], rel[2], vr, cn, sp, true, &b, &L);
    const bool narrowed = b.klo < 0;
    const bool two_sided = b.khi < 0;
    const int klo = narrowed ? ~b.klo : b.klo, khi = two_sided ? -b.khi - 1 : b.khi;
    int m = 0, iters = 0;
    if (narrowed) {
        for (int g = 0; g < pieces; ++g) {
            const int k0 = klo + g * (int)L.plen;
            const int kend = k0 + (int)L.plen - 1 < khi ? k0 + (int)L.plen - 1 : khi;
            ConeLatticeWalk wk;
            wk.enter(L, k0, kend);
            iters += wk.k - k0;
            while (wk.k <= kend) {
                if (m < cap) cand[m] = wk.k;
                ++m; ++iters;
                wk.next();
            }
        }
        if (pieces > 0 && klo + pieces * (int)L.plen <= khi) m = -1;      // (the pieces must cover the band)
    } else {
        for (int k = klo; k <= khi; ++k) { if (m < cap) cand[m] = k; ++m; }
    }
    info[0] = klo; info[1] = khi; info[2] = narrowed ? 1 : 0; info[3] = pieces; info[4] = iters; info[5] = two_sided ? 1 : 0;
    for (int k = 0; k < P; ++k) {
        brute[k] = 0;
        if (k < klo || k > khi) continue;
        double px, py, pz;
        sp.point(k, &px, &py, &pz);
        const double dot = pw_fma(pz, rel[2], pw_fma(px, rel[0], py * rel[1]));
        brute[k] = (two_sided ? pw_abs(dot) >= b.thr : dot >= b.thr) ? 1 : 0;
    }
    return m;
}
// the table of steps: q[i], s[i] for i < return value
extern "C" int hs_cone_table(int* q, double* s) {
    for (int i = 0; i < ConeLatticeTable::N; ++i) { q[i] = CONE_LATTICE_TABLE.q[i]; s[i] = CONE_LATTICE_TABLE.s[i]; }
    return ConeLatticeTable::N;
}
