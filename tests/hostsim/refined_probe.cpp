// tests/hostsim/refined_probe.cpp -- one path by the plain walk (every point against every atom, the first point with the
// smallest gap: the statements of wave_window's step (ii) for a one-lane team) and by the wave-level bracket scan
// (wave_path_bracket behind the guard of path_steps, pywindow_amd/csrc/pw_unit.hpp) for tests/test_refined_brackets.py;
// and the unit probe (unit_probe.cpp, included whole) with one more entry: the stage capture under given parameters.
// Test infrastructure only.
#include "unit_probe.cpp"
// hs_analysis_debug with the knobs of pw_params (increment2 among them)
extern "C" int hs_analysis_debug_params(long n_units, const long* off, const double* xyz, const double* vdw,
                                        const double* mass, unsigned stages, pw_unit_out* out, const pw_params* params,
                                        pw_unit_debug* dbg) {
    memset(dbg, 0, sizeof(pw_unit_debug) * (size_t)n_units);
    return run_batch(n_units, off, xyz, vdw, mass, stages, out, params, dbg);
}
// n atoms at xyz (n x 3) with radii vdw, a path from the origin to v in steps of inc, its points k_first .. chunks.
// res[0..2] = ok, the bits of the smallest gap and the first point that has it, by the plain walk;
// res[3..5] = the same by the form the pipeline takes (the bracket scan where the guard holds, the plain walk otherwise);
// res[6] = 1 where the guard held; res[7] = (atom, point) evaluations of the bracket scan; res[8] = chunks;
// res[9] = groups of radii (0: ungrouped).
extern "C" int hs_refined_both(int n, const double* xyz, const double* vdw, const double* v, double inc, int k_first,
                               long long* res) {
    if (n < 1 || k_first < 0 || k_first > 1) return -1;
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
    double xx_max = 0.0;
    for (int i = 0; i < n; ++i) xx_max = __builtin_fmax(xx_max, xx[i]);
    // wave_window's statements
    const double nrm = norm3(v[0], v[1], v[2]);
    const double fd = np_floordiv(nrm, inc);
    const int chunks = fd >= 0.0 && fd <= PW_PATH_POINTS_MAX ? (int)fd : 0;
    const double cx = v[0] / (double)chunks, cy = v[1] / (double)chunks, cz = v[2] / (double)chunks;
    auto plain = [&](bool* ok, double* best, int* pos) {
        *ok = true; *best = PW_INF; *pos = 0x7fffffff;
        for (int k = k_first; k <= chunks; ++k) {
            const double m = point_gap_value(F, n, cx * (double)k, cy * (double)k, cz * (double)k);
            if (!(m > 0.0)) *ok = false;
            if (m < *best) { *best = m; *pos = k; }
        }
    };
    bool ok_a, ok_b;
    double best_a, best_b;
    int pos_a, pos_b;
    plain(&ok_a, &best_a, &pos_a);
    const PathSteps s = path_steps(F, v[0], v[1], v[2], inc, xx_max);
    const bool guard = s.bracket && s.chunks == chunks && s.cx == cx && s.cy == cy && s.cz == cz;
    long terms = 0;
    if (guard) {
        const PathMin r = wave_path_bracket<HostTeam>(F, n, cx, cy, cz, chunks, s.rinv, k_first, &terms);
        best_b = r.gap; pos_b = r.k; ok_b = r.gap > 0.0;
    } else {
        plain(&ok_b, &best_b, &pos_b);
    }
    long long bits_a, bits_b;
    memcpy(&bits_a, &best_a, 8);
    memcpy(&bits_b, &best_b, 8);
    res[0] = ok_a ? 1 : 0; res[1] = bits_a; res[2] = pos_a;
    res[3] = ok_b ? 1 : 0; res[4] = bits_b; res[5] = pos_b;
    res[6] = guard ? 1 : 0;
    res[7] = terms;
    res[8] = chunks;
    res[9] = cls->k;
    return 0;
}
