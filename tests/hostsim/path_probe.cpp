// tests/hostsim/path_probe.cpp -- one path of the window search's sampling stage (pywindow_amd/csrc/pw_unit.hpp) by both
// of its forms for tests/test_path_brackets.py: path_scan_thread, every point against every listed atom, and
// path_bracket_thread, each atom at the two points that bracket it, behind the guard of path_steps.  Test infrastructure only.
#include <vector>
#include "../../pywindow_amd/csrc/pw_unit.hpp"
using namespace pw;
// n atoms at xyz (n x 3) with radii vdw, a path from the origin to v, step length inc.  use_list != 0: through the
// candidate list of wave_path_candidates (a one-path wave), as the stage does where the list fits.
// res[0], res[1] = ok and the bits of 2 * best of the plain scan; res[2], res[3] = the same of the form the stage takes
// (the bracket form where the guard holds, the plain scan otherwise); res[4] = 1 where the guard held;
// res[5] = (atom, point) evaluations of the bracket form; res[6] = atoms gone through; res[7] = chunks;
// res[8], res[9] = n_eval of the two forms; res[10] = groups of radii (0: ungrouped).  2 * best is 0 where ok is not.
extern "C" int hs_path_both(int n, const double* xyz, const double* vdw, const double* v, double inc, int use_list,
                            long long* res) {
    if (n < 1) return -1;
    const size_t npad = (size_t)((n + 1) & ~1);
    std::vector<double> mass(n, 1.0), x(npad), y(npad), z(npad), xx(npad);
    std::vector<unsigned char> blob(template_groups_bytes(n));
    template_groups_build(vdw, mass.data(), n, blob.data());
    const ClassInfo* cls = (const ClassInfo*)blob.data();
    const int* inv = (const int*)(blob.data() + ((sizeof(ClassInfo) + 7) & ~(size_t)7));
    const int* perm = inv + npad;
    const double* vs = (const double*)(perm + npad);
    for (int i = 0; i < n; ++i) {
        const int p = inv[i];
        x[p] = xyz[3 * i]; y[p] = xyz[3 * i + 1]; z[p] = xyz[3 * i + 2];
        xx[p] = sq3(x[p], y[p], z[p]);
    }
    Frame F;
    F.x = x.data(); F.y = y.data(); F.z = z.data(); F.xx = xx.data();
    F.vdw = vs; F.perm = perm; F.cls = cls;
    const double m0 = wave_gap_value<HostTeam>(F, n, 0.0, 0.0, 0.0);
    std::vector<int> list((size_t)n + PW_KCLS + 2);
    int* cand = nullptr;
    int* coff = nullptr;
    if (use_list && wave_path_candidates<HostTeam>(F, n, true, v[0], v[1], v[2], inc, m0, list.data(), list.data() + n)) {
        cand = list.data();
        coff = cand + n;
    }
    double xx_max = 0.0;
    for (int i = 0; i < n; ++i) xx_max = __builtin_fmax(xx_max, xx[i]);
    // the plain scan
    double g2 = 0.0, chunk[3];
    int pos = 0, ev_a = 0, ev_b = 0;
    const bool ok_a = path_scan_thread(F, n, v[0], v[1], v[2], inc, m0, &g2, &pos, chunk, &ev_a, cand, coff);
    if (!ok_a) g2 = 0.0;
    // the stage's statements
    const PathSteps s = path_steps(F, v[0], v[1], v[2], inc, xx_max);
    double h2 = 0.0;
    long terms = 0;
    bool ok_b;
    if (s.bracket) {
        ok_b = path_bracket_thread(F, n, s.cx, s.cy, s.cz, s.chunks, s.rinv, m0, &h2, &ev_b, cand, coff, &terms);
    } else {
        ok_b = path_scan_thread(F, n, v[0], v[1], v[2], inc, m0, &h2, &pos, chunk, &ev_b, cand, coff);
    }
    if (!ok_b) h2 = 0.0;
    long long bits_a, bits_b;
    memcpy(&bits_a, &g2, 8);
    memcpy(&bits_b, &h2, 8);
    res[0] = ok_a ? 1 : 0; res[1] = bits_a;
    res[2] = ok_b ? 1 : 0; res[3] = bits_b;
    res[4] = s.bracket ? 1 : 0;
    res[5] = terms;
    res[6] = cand ? coff[cls->k] - coff[0] : n;
    res[7] = (long long)np_floordiv(norm3(v[0], v[1], v[2]), inc);
    res[8] = ev_a; res[9] = ev_b;
    res[10] = cls->k;
    return 0;
}
