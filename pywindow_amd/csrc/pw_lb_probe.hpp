// pw_lb_probe.hpp -- test instrumentation: one Lbfgsb<N> on one team, state in, state out (pw_internal_lb_probe).
//
// A case is the bytes of an LbMem<N>, the scalars of an Lbfgsb<N> (everything bind() does not set), a short list of
// operations and, for some of them, f and g.  The dispatcher below applies the operations -- the members of
// Lbfgsb<N> themselves, nothing restated -- and leaves the block, the scalars and every return value in the case.
// ONE text for any team: a device = -1 context runs it with HostTeam (pw_hostpath.cpp), and a device team can run
// the same text on a block in LDS (pw_lb_probe.hip says why none does yet), so the lists of operations and fields
// cannot drift; the field table is generated from the same lists.  The tests (tests/_lb_cases.py) fill and compare
// fields by name.
#pragma once
#include <stddef.h>
#include <string.h>

#include "pw_lbfgsb.hpp"

namespace pw {

enum LbProbeOp : int {
    LBP_SETUP = 1,      // setup() from in_x0, in_l, in_u, in_nbd and the case's factr, pgtol, maxls
    LBP_TABLES = 2,     // a = which (0..3)
    LBP_FACTOR = 3,     // a = which (1..3)
    LBP_FORMT = 4,
    LBP_FORMK = 5,
    LBP_BMV = 6,        // a = offset of v in wa, b = offset of p in wa (2 col entries each, not overlapping)
    LBP_CMPRLB = 7,
    LBP_SUBSM = 8,
    LBP_STEP = 9,       // f and g from in_f, in_g
    LBP_MINIMIZE = 10,  // a = objective, b = maxiter, c = maxfun
    LBP_OP_END = 11,
};
constexpr int LBP_MAX_OPS = 8;
constexpr int LBP_MAX_ITER = 500;       // maxiter, maxfun: a device that goes wrong ends
constexpr int LBP_MAX_LS = 64;          // maxls of an image
enum LbProbeFlag : int {
    LBP_F_DEVICE_ONLY = 1,  // written by device teams only (tables, lane exchange)
    LBP_F_SCRATCH = 2,      // defined only after returns of 0: a routine that gives up may leave part of a result
    LBP_F_CASE = 4,         // the case's inputs and outputs, not state of the optimiser
};

// ---- the scalars of Lbfgsb<N>, by name (bools travel as ints) ----
#define LB_PROBE_DBL(X) \
    X(f) X(factr) X(pgtol) X(theta) X(fold) X(tol) X(dnorm) X(epsmch) X(gd) X(stpmx) X(sbgnrm) X(stp) X(gdold) X(dtd)
#define LB_PROBE_INT(X)                                                                                            \
    X(maxls) X(task) X(msg) X(prjctd) X(cnstnd) X(boxed) X(updatd) X(nintol) X(itfile) X(iback) X(nskip) X(head)  \
    X(col) X(itail) X(iter) X(iupdat) X(nseg) X(nfgv) X(info) X(ifun) X(iword) X(nfree) X(nact) X(ileave)         \
    X(nenter) X(ls_task)
// ---- the arrays of LbMem<N>: X(member, flags) ----
#define LB_PROBE_MEM_D(X)                                                                                          \
    X(l, 0) X(u, 0) X(x, 0) X(g, 0) X(ws, 0) X(wy, 0) X(sy, 0) X(ss, 0) X(wt, 0) X(wn, 0) X(wn1d, 0) X(z, 0)      \
    X(r, 0) X(d, 0) X(t, 0) X(xp, 0) X(wa, LBP_F_SCRATCH) X(acc, LBP_F_DEVICE_ONLY) X(dsy, LBP_F_DEVICE_ONLY)     \
    X(rsy, LBP_F_DEVICE_ONLY) X(sqy, LBP_F_DEVICE_ONLY) X(rsq, LBP_F_DEVICE_ONLY) X(rwt, LBP_F_DEVICE_ONLY)       \
    X(rwn, LBP_F_DEVICE_ONLY) X(iwn, LBP_F_DEVICE_ONLY) X(tri, LBP_F_DEVICE_ONLY) X(le, 0) X(ue, 0)
#define LB_PROBE_MEM_I(X) X(pair, LBP_F_DEVICE_ONLY) X(cand, 0) X(nbd, 0) X(index, 0) X(iwhere, 0) X(indx2, 0)

struct LbProbeScal {
#define X(n) double n;
    LB_PROBE_DBL(X)
#undef X
#define X(n) int n;
    LB_PROBE_INT(X)
#undef X
};

template <int N>
struct LbProbeCase {
    LbMem<N> mem;
    LbProbeScal sc;
    double in_f, in_g[N], in_x0[N], in_l[N], in_u[N];
    int in_nbd[N];
    int nops, ops[LBP_MAX_OPS * 4];     // (code, a, b, c) per operation
    int ret[LBP_MAX_OPS];               // what each operation returned (0 where it returns nothing)
    int nit, nfev;                      // of the last MINIMIZE
};

struct LbProbeField {
    char name[12];
    int offset, count, type, flags;     // type: 0 double, 1 int
};

template <int N>
inline int lb_probe_fields(LbProbeField* out, int cap) {
    typedef LbProbeCase<N> C;
    int n = 0;
    auto put = [&](const char* name, size_t off, size_t bytes, int type, int flags) {
        if (n < cap) {
            LbProbeField& F = out[n];
            memset(&F, 0, sizeof(F));
            strncpy(F.name, name, sizeof(F.name) - 1);
            F.offset = (int)off;
            F.count = (int)(bytes / (type ? sizeof(int) : sizeof(double)));
            F.type = type;
            F.flags = flags;
        }
        ++n;
    };
    const size_t m0 = offsetof(C, mem), s0 = offsetof(C, sc);
#define X(n_, fl) put(#n_, m0 + offsetof(LbMem<N>, n_), sizeof(((LbMem<N>*)0)->n_), 0, fl);
    LB_PROBE_MEM_D(X)
#undef X
#define X(n_, fl) put(#n_, m0 + offsetof(LbMem<N>, n_), sizeof(((LbMem<N>*)0)->n_), 1, fl);
    LB_PROBE_MEM_I(X)
#undef X
    put("ls", m0 + offsetof(LbMem<N>, ls), 13 * sizeof(double), 0, 0);
    put("ls_i", m0 + offsetof(LbMem<N>, ls) + offsetof(LsState, brackt), 2 * sizeof(int), 1, 0);
#define X(n_) put(#n_, s0 + offsetof(LbProbeScal, n_), sizeof(double), 0, 0);
    LB_PROBE_DBL(X)
#undef X
#define X(n_) put(#n_, s0 + offsetof(LbProbeScal, n_), sizeof(int), 1, 0);
    LB_PROBE_INT(X)
#undef X
    put("in_f", offsetof(C, in_f), sizeof(double), 0, LBP_F_CASE);
    put("in_g", offsetof(C, in_g), sizeof(double) * N, 0, LBP_F_CASE);
    put("in_x0", offsetof(C, in_x0), sizeof(double) * N, 0, LBP_F_CASE);
    put("in_l", offsetof(C, in_l), sizeof(double) * N, 0, LBP_F_CASE);
    put("in_u", offsetof(C, in_u), sizeof(double) * N, 0, LBP_F_CASE);
    put("in_nbd", offsetof(C, in_nbd), sizeof(int) * N, 1, LBP_F_CASE);
    put("nops", offsetof(C, nops), sizeof(int), 1, LBP_F_CASE);
    put("ops", offsetof(C, ops), sizeof(int) * LBP_MAX_OPS * 4, 1, LBP_F_CASE);
    put("ret", offsetof(C, ret), sizeof(int) * LBP_MAX_OPS, 1, LBP_F_CASE);
    put("nit", offsetof(C, nit), sizeof(int), 1, LBP_F_CASE);
    put("nfev", offsetof(C, nfev), sizeof(int), 1, LBP_F_CASE);
    return n;
}

// pair[] as setup() of a wave leaves it: lane p owns (a, b), a > b, p = a (a - 1) / 2 + b; 255: no pair
PW_HD inline int lb_probe_pair(int p) {
    constexpr int M = LB_M;
    if (p >= M * (M - 1) / 2) return 255;
    int a = 1;
    while ((a + 1) * a / 2 <= p) ++a;
    return a | (p - a * (a - 1) / 2) << 8;
}

// ---- is the image safe to run?  Every index the routines form from the state stays inside the block. ----
template <int N>
inline bool lb_probe_safe(const LbProbeCase<N>& c) {
    const LbProbeScal& s = c.sc;
    if (s.col < 0 || s.col > LB_M) return false;
    if (s.head < 0 || s.head >= LB_M || s.itail < 0 || s.itail >= LB_M) return false;
    if (s.nfree < 0 || s.nfree > N || s.nenter < 0 || s.nenter > N || s.nact < 0 || s.nact > N) return false;
    // ileave: 1..N + 1, what freev() leaves; formk starts a loop over indx2 at ileave - 1.  The 0 of a run's start
    // (step(), minimize()) passes only while there is no correction pair: formk then reads nothing, and freev()
    // has run before the first pair exists.
    if (s.ileave > N + 1 || s.ileave < (s.col == 0 ? 0 : 1)) return false;
    if (s.maxls < 0 || s.maxls > LBP_MAX_LS) return false;
    // what step() reaches from here: matupd takes col = iupdat while iupdat <= m and writes row col - 1, column
    // (head + iupdat - 1) % m; past m it keeps col, which is m in every run.  The entry dispatch knows these tasks
    // and the line search these states.
    if (s.iupdat < 0 || s.iupdat > (1 << 20) || (s.iupdat >= LB_M && s.col != LB_M)) return false;
    if (s.iter < 0 || s.ls_task < 0 || s.ls_task > 4) return false;
    if (s.task != LB_START && s.task != LB_NEW_X && s.task != LB_FG && s.task != LB_CONVERGENCE && s.task != LB_STOP &&
        s.task != LB_WARNING && s.task != LB_ERROR && s.task != LB_ABNORMAL)
        return false;
    for (int i = 0; i < N; ++i) {
        if (c.mem.index[i] < 0 || c.mem.index[i] >= N || c.mem.indx2[i] < 0 || c.mem.indx2[i] >= N) return false;
        if (c.mem.nbd[i] < 0 || c.mem.nbd[i] > 3 || c.in_nbd[i] < 0 || c.in_nbd[i] > 3) return false;
    }
    // the lane-to-pair table indexes SY: the one setup() writes, or untouched (an image of a one-lane team)
    for (int p = 0; p < 64; ++p)
        if (c.mem.pair[p] != lb_probe_pair(p) && c.mem.pair[p] != 0) return false;
    if (c.nops < 0 || c.nops > LBP_MAX_OPS) return false;
    for (int k = 0; k < c.nops; ++k) {
        const int op = c.ops[4 * k], a = c.ops[4 * k + 1], b = c.ops[4 * k + 2], cc = c.ops[4 * k + 3];
        if (op < LBP_SETUP || op >= LBP_OP_END) return false;
        if (op == LBP_TABLES && (a < 0 || a > 3)) return false;
        if (op == LBP_FACTOR && (a < 1 || a > 3)) return false;
        if (op == LBP_BMV) {
            const int w = 2 * LB_M;     // (the widest product: whatever col an earlier operation of the list leaves)
            if (a < 0 || b < 0 || a + w > 8 * LB_M || b + w > 8 * LB_M) return false;
            if (a < b + w && b < a + w) return false;
        }
        if (op == LBP_MINIMIZE) {
            if (N == 3 ? (a < 0 || a > 3) : a != 4) return false;
            if (b < 1 || b > LBP_MAX_ITER || cc < 1 || cc > LBP_MAX_ITER) return false;
        }
    }
    return true;
}

// ---- analytic objectives of MINIMIZE: polynomials (and |.|) with explicit gradients, products and sums only, so
// host and device round alike; tests/_lb_cases.py has the same statements in Python ----
template <int N>
struct LbProbeObjective {
    int id, nfev;
    PW_HD static double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }
    PW_HD void operator()(const double* x, double& f, double* g) {
        nfev += 1;
        if constexpr (N == 3) {
            const double x0 = x[0], x1 = x[1], x2 = x[2];
            if (id == 0) {              // Rosenbrock, chained
                const double a = x1 - x0 * x0, b = 1.0 - x0, c = x2 - x1 * x1, e = 1.0 - x1;
                f = 100.0 * a * a + b * b + 100.0 * c * c + e * e;
                g[0] = -400.0 * a * x0 - 2.0 * b;
                g[1] = 200.0 * a - 400.0 * c * x1 - 2.0 * e;
                g[2] = 200.0 * c;
            } else if (id == 1) {       // quadratic, condition 1e12
                f = 0.5 * (x0 * x0 + 1e6 * x1 * x1 + 1e-6 * x2 * x2) + x0 * x2 * 1e-3;
                g[0] = x0 + x2 * 1e-3;
                g[1] = 1e6 * x1;
                g[2] = 1e-6 * x2 + x0 * 1e-3;
            } else if (id == 2) {       // kinks
                const double q = x2 - 1.0;
                f = pw_abs(x0) + 10.0 * pw_abs(x1 - 0.3) + q * q + 0.1 * x0 * x1;
                g[0] = sgn(x0) + 0.1 * x1;
                g[1] = 10.0 * sgn(x1 - 0.3) + 0.1 * x0;
                g[2] = 2.0 * q;
            } else {                    // Powell's singular function, three variables
                const double a = x0 + 10.0 * x1, b = x2 - x0, c = x1 - 2.0 * x2, d = x0 - x2;
                const double c2 = c * c, d2 = d * d, c3 = c2 * c, d3 = d2 * d;
                f = a * a + 5.0 * b * b + c2 * c2 + 10.0 * (d2 * d2);
                g[0] = 2.0 * a - 10.0 * b + 40.0 * d3;
                g[1] = 20.0 * a + 4.0 * c3;
                g[2] = 10.0 * b - 8.0 * c3 - 40.0 * d3;
            }
        } else {
            const double z = x[0], q = z * z - 2.0;
            f = q * q + 0.1 * z + pw_abs(z - 1.3);
            g[0] = 4.0 * z * q + 0.1 + sgn(z - 1.3);
        }
    }
};

// ---- the dispatcher: cs in the caller's memory, m the team's block (already holding cs->mem) ----
template <class T, int N>
PW_HD inline void lb_probe_run(LbProbeCase<N>* cs, LbMem<N>* m) {
    PW_ASSUME_LDS(m);
    Lbfgsb<N> S;
    S.bind(m);
    S.prof = nullptr;
#if defined(PW_PROFILE) && defined(PW_LB_FINE)
    m->prof_fine = nullptr;
#endif
#define X(n) S.n = cs->sc.n;
    LB_PROBE_DBL(X)
#undef X
#define X(n) S.n = (decltype(S.n))cs->sc.n;
    LB_PROBE_INT(X)
#undef X
    const int nops = T::uniform_i(cs->nops);
    int nit = 0, nfev = 0;
    for (int k = 0; k < nops; ++k) {
        const int op = T::uniform_i(cs->ops[4 * k]), a = T::uniform_i(cs->ops[4 * k + 1]),
                  b = T::uniform_i(cs->ops[4 * k + 2]), c = T::uniform_i(cs->ops[4 * k + 3]);
        int ret = 0;
        if (op == LBP_SETUP) {
            S.template setup<T>(m, cs->in_x0, cs->in_l, cs->in_u, cs->in_nbd, cs->sc.factr, cs->sc.pgtol, cs->sc.maxls);
            if (T::WSIZE == 1)
                for (int p = 0; p < 64; ++p) m->pair[p] = lb_probe_pair(p);     // (the image serves a wave as well)
        } else if (op == LBP_TABLES) {
            S.template tables<T>(a);
        } else if (op == LBP_FACTOR) {
            ret = S.template factor<T>(a);
        } else if (op == LBP_FORMT) {
            ret = S.template formt<T>();
        } else if (op == LBP_FORMK) {
            ret = S.template formk<T>();
        } else if (op == LBP_BMV) {
            ret = S.template bmv<T>(S.wa + a, S.wa + b);
        } else if (op == LBP_CMPRLB) {
            ret = S.template cmprlb<T>();
        } else if (op == LBP_SUBSM) {
            ret = S.template subsm<T>();
        } else if (op == LBP_STEP) {
            S.f = cs->in_f;
            T::wave_sync();
            if (T::lane() == 0)
                for (int i = 0; i < N; ++i) S.g[i] = cs->in_g[i];
            T::wave_sync();
            S.template step<T>();
        } else if (op == LBP_MINIMIZE) {
            LbProbeObjective<N> fg{a, 0};
            S.template minimize<T>(fg, b, c, &nit);
            nfev = fg.nfev;
        }
        T::wave_sync();
        if (T::lane() == 0) cs->ret[k] = ret;
    }
    T::wave_sync();
    if (T::lane() == 0) {
#define X(n) cs->sc.n = S.n;
        LB_PROBE_DBL(X)
#undef X
#define X(n) cs->sc.n = (int)S.n;
        LB_PROBE_INT(X)
#undef X
        cs->nit = nit;
        cs->nfev = nfev;
    }
}

}  // namespace pw
