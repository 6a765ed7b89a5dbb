// pw_hostpath.cpp -- the `device = -1` path of the C ABI (include/pywindow_amd.h): the SAME unit pipeline
// (pw_unit.hpp, single source with the gfx950 kernels) compiled by g++ for a one-lane team and run by host
// threads over the units of a batch.  Explicit choice only -- pw_context_create(-1); nothing ever falls back
// to it.  It is what makes BASELINE.json's configs[0] ("CC3 single-frame full_analysis() on CPU") runnable
// through the product's own boundary, and what bench.py times as the same-source CPU figure.
//
// Reference for the path: Molecule.full_analysis (molecular.py:156-202) per unit, the per-frame loop of
// Trajectory._analysis_serial (trajectory.py:496-522) over the batch; `threads` plays the role of
// analysis(ncpus=...) (trajectory.py:553-586).
//
// Built with g++ -O2 -ffp-contract=off -mfma (fused multiply-adds only where the source writes them).
#define pw pw_cpu          // a namespace of its own: nothing here merges with the HIP translation units' host code
#include "pw_unit.hpp"
#include "pw_kde.hpp"
#include "pw_corr.hpp"
#include "pw_dft.hpp"
#include "pw_gate.hpp"
#include "pw_trans.hpp"
#include "pw_superpose.hpp"
#include "pw_cluster.hpp"
#include "pw_cov.hpp"
#include "pw_affinity.hpp"
#include "pw_rigid.hpp"
#include "pw_rigid_body.hpp"
#include "pw_rigid_cell.hpp"
#include "pw_ewald.hpp"
#include "pw_cavity.hpp"
#include "pw_sasa.hpp"
#include "pw_pores.hpp"
#include "pw_passage.hpp"
#include "pw_hop.hpp"
#include "pw_charges.hpp"
#include "pw_charges_cell.hpp"
#include "pw_channels.hpp"
#include "pw_percolate.hpp"
#include "pw_basins.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

using namespace pw;

namespace {

// neighbour tables of the sampling sphere (pw_unit.hpp), built per vector count on first use
struct HostTables {
    std::mutex lock;
    // bumped (release) after a table has been appended: a worker copies `off` under the lock when the version
    // it last saw is stale, and reads rows only through its copy -- every row it can reach was complete before
    // the version it acquired (no plain read of memory another thread may be writing)
    std::atomic<unsigned> version{0};
    std::vector<unsigned> off = std::vector<unsigned>(PW_NB_PMAX + 1, PW_NB_NONE);
    // one allocation per P (pointers handed to running threads must stay valid): offsets index `rows`
    std::vector<unsigned short> idx;
    std::vector<double> bound;
    HostTables() {
        // room for every P up front would be 84 MB; tables are appended instead and the vectors reserved
        // generously so that appending never moves them while other threads read
        idx.reserve((size_t)64 * PW_NB_PMAX * PW_NB_K);
        bound.reserve((size_t)64 * PW_NB_PMAX);
    }
    void ensure(int P) {
        if (P < PW_NB_PMIN || P > PW_NB_PMAX) return;
        std::lock_guard<std::mutex> g(lock);
        if (off[P] != PW_NB_NONE) return;
        const size_t first = bound.size();
        if (first + (size_t)P > bound.capacity()) return;          // (64 distinct counts seen: no more tables)
        std::vector<double> ux(P), uy(P), uz(P);
        Sphere sp;
        sp.init(1.0, P);
        for (int k = 0; k < P; ++k) sp.point(k, &ux[k], &uy[k], &uz[k]);
        idx.resize((first + P) * PW_NB_K);
        bound.resize(first + P);
        for (int k = 0; k < P; ++k)
            nb_build_point(P, k, ux.data(), uy.data(), uz.data(), idx.data() + (first + k) * PW_NB_K, bound.data() + first + k);
        off[P] = (unsigned)first;
        version.fetch_add(1, std::memory_order_release);
    }
    // the worker's private view of `off` (see `version`)
    void snapshot(std::vector<unsigned>& mine, unsigned& seen) {
        const unsigned v = version.load(std::memory_order_acquire);
        if (v == seen && !mine.empty()) return;
        std::lock_guard<std::mutex> g(lock);
        mine = off;
        seen = version.load(std::memory_order_relaxed);
    }
};
HostTables g_tables;
unsigned g_rsq[65536];
std::once_flag g_rsq_once;

// How every entry below pw_hostpath_run shares its work: f(piece) for piece = 0 .. pieces - 1, by at most `threads`
// threads, each taking the next piece that nobody has; one thread is the calling thread.  Which thread runs a piece and
// in which order the pieces finish is not defined, so a piece writes only what is its own and keeps its scratch to itself.
template <class F>
void host_share(long pieces, int threads, F f) {
    std::atomic<long> next{0};
    auto worker = [&]() {
        for (;;) {
            const long p = next.fetch_add(1);
            if (p >= pieces) break;
            f(p);
        }
    };
    const int count = (long)threads > pieces ? (int)std::max(1l, pieces) : std::max(1, threads);
    if (count == 1) {
        worker();
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < count; ++t) pool.emplace_back(worker);
        for (auto& t : pool) t.join();
    }
}

// The (job, block) pieces of the statistical entries: job k has blocks_of_job(k) blocks (0: the job has no work), and
// f(k, block) runs once for every block of every job, shared out by host_share.  A piece finds its job by bisection in
// the table of first pieces, so it does not matter which pieces the thread had before.
template <class B, class F>
void host_share_blocks(long n_jobs, int threads, B blocks_of_job, F f) {
    std::vector<long> first((size_t)n_jobs + 1, 0);
    for (long k = 0; k < n_jobs; ++k) first[k + 1] = first[k] + blocks_of_job(k);
    host_share(first[n_jobs], threads, [&](long w) {
        const long k = (std::upper_bound(first.begin(), first.end(), w) - first.begin()) - 1;   // the last job with first[k] <= w
        f(k, w - first[k]);
    });
}

// the blocks of `block` that `count` outputs make
inline long host_blocks(long count, long block) { return (count + block - 1) / block; }

}  // namespace

// One batch on the host.  Returns 0 or PW_E_NOMEM.  extra: windows beyond PW_W_MAX, appended unsorted.
extern "C" int pw_hostpath_run(const pw_batch_in* in, unsigned stages, pw_unit_out* out, const pw_params* prm_in,
                               int p_cap, int threads, pw_unit_debug* dbg, pw_extra_window* xw, unsigned xw_cap,
                               unsigned* xw_count) {
    std::call_once(g_rsq_once, [] { rsqrt14_decode(g_rsq); });
    const pw_params prm = prm_in ? *prm_in : default_params();
    const long n_units = (long)in->n_units;
    int nmax = 0;
    for (long u = 0; u < n_units; ++u) nmax = std::max(nmax, (int)(in->atom_offset[u + 1] - in->atom_offset[u]));
    p_cap = round_p_cap(p_cap);
    if (threads < 1) threads = 1;
    if ((long)threads > n_units) threads = (int)std::max(1l, n_units);
    std::atomic<long> next{0};
    std::atomic<int> failed{0};
    unsigned xcount = 0;            // (bumped with atomic increments: pw_unit.hpp team_atomic_inc)
    const int vstride = in->template_atoms > 0 ? 0 : 1;
    auto worker = [&]() {
        const size_t bytes = UnitShared::bytes(nmax, 1, 8, 2, false, p_cap);
        unsigned char* lds = (unsigned char*)aligned_alloc(16, (bytes + 15) & ~(size_t)15);
        TeamWorkspace* ws = (TeamWorkspace*)calloc(1, sizeof(TeamWorkspace));
        unsigned char* slab = (unsigned char*)malloc(team_slab_bytes(p_cap));
        unsigned long long* adj = (unsigned long long*)malloc(sizeof(unsigned long long) * team_adj_words(p_cap));
        if (!lds || !ws || !slab || !adj) {
            failed = 1;
            free(lds); free(ws); free(slab); free(adj);
            return;
        }
        bind_team_slab(ws, slab, p_cap);
        ws->adj = adj;
        ws->rsq = g_rsq;
        ws->dbg_base = dbg;
        ws->xwin = xw; ws->xwin_cap = xw_cap; ws->xwin_count = &xcount;
        std::vector<unsigned> nb_off;
        unsigned nb_seen = 0;
        for (;;) {
            const long u = next.fetch_add(1);
            if (u >= n_units) break;
            ws->unit = u;
            g_tables.snapshot(nb_off, nb_seen);
            ws->nb_off = nb_off.data(); ws->nb_idx = g_tables.idx.data(); ws->nb_bound = g_tables.bound.data();
            memset(lds, 0, bytes);
            UnitShared sh;
            sh.carve(lds, nmax, 1, 8, 2, false, p_cap);
            const long a0 = (long)in->atom_offset[u];
            const int n = (int)(in->atom_offset[u + 1] - a0);
            memset(&out[u], 0, sizeof(pw_unit_out));
            analyse_unit<HostTeam>(sh, ws, n, in->xyz + 3 * a0, in->vdw + a0 * vstride, in->mass + a0 * vstride, stages,
                                   &out[u], prm);

            if ((stages & PW_STAGE_WINDOWS) && out[u].n_points >= PW_NB_PMIN) g_tables.ensure(out[u].n_points);
        }
        free(adj); free(slab); free(ws); free(lds);
    };
    if (threads == 1) {
        worker();
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t) pool.emplace_back(worker);
        for (auto& t : pool) t.join();
    }
    if (xw_count) *xw_count = xcount;
    return failed ? PW_E_NOMEM : PW_OK;
}

extern "C" int pw_hostpath_default_threads(void) {
    const char* e = getenv("PW_CPU_THREADS");
    if (e && atoi(e) > 0) return atoi(e);
    unsigned hc = std::thread::hardware_concurrency();
    return hc ? (int)hc : 1;
}

// pw_kde_sums on the host (pw_kde.hip checks the arguments and sends device == -1 contexts here): the
// chunks of pw_kde.hpp in the same order as the kernels, so the sums have the device's bits.  Threads
// share out blocks of grid points; how they do has no part in the result.
extern "C" int pw_hostpath_kde(const pw_kde_job* jobs, long n_jobs, const double* samples, const double* points,
                               double* sums, int threads) {
    constexpr long BLOCK = 8;                      // grid points of one piece of work
    host_share_blocks(n_jobs, threads, [&](long k) { return host_blocks((long)jobs[k].n_points, BLOCK); }, [&](long k, long block) {
        const pw_kde_job& J = jobs[k];
        const long j0 = block * BLOCK, j1 = std::min(j0 + BLOCK, (long)J.n_points);
        const double* x = samples + J.sample_first;
        for (long j = j0; j < j1; ++j) {
            const double g = points[J.point_first + j];
            double s = 0.0;
            for (long i0 = 0; i0 < (long)J.n_samples; i0 += KDE_CHUNK) {
                const int len = (int)std::min((long)KDE_CHUNK, (long)J.n_samples - i0);
                const double p = kde_chunk_sum(g, x + i0, len, J.inv_bandwidth, POW_EXP_TAB);
                s = i0 == 0 ? p : s + p;
            }
            sums[J.point_first + j] = s;
        }
    });
    return PW_OK;
}

// pw_kde2_sums on the host, the same way: threads over (job, block of points), a point's chunks in order
extern "C" int pw_hostpath_kde2(const pw_kde2_job* jobs, long n_jobs, const double* samples, const double* points,
                                double* sums, int threads) {
    constexpr long BLOCK = 8;                      // points of one piece of work
    host_share_blocks(n_jobs, threads, [&](long k) { return host_blocks((long)jobs[k].n_points, BLOCK); }, [&](long k, long block) {
        const pw_kde2_job& J = jobs[k];
        const long j0 = block * BLOCK, j1 = std::min(j0 + BLOCK, (long)J.n_points);
        const double* xy = samples + 2 * J.sample_first;
        for (long j = j0; j < j1; ++j) {
            const double g0 = points[2 * (J.point_first + j)], g1 = points[2 * (J.point_first + j) + 1];
            double s = 0.0;
            for (long i0 = 0; i0 < (long)J.n_samples; i0 += KDE_CHUNK) {
                const int len = (int)std::min((long)KDE_CHUNK, (long)J.n_samples - i0);
                const double p = kde2_chunk_sum(g0, g1, xy + 2 * i0, len, J.w00, J.w10, J.w11, POW_EXP_TAB);
                s = i0 == 0 ? p : s + p;
            }
            sums[J.point_first + j] = s;
        }
    });
    return PW_OK;
}

// pw_kde_wsums on the host (pw_kdew.hip checks the arguments and sends device == -1 contexts here): threads over
// (job, block of points); a point's term is computed once and goes to every replica's sum, chunks in order
extern "C" int pw_hostpath_kdew(const pw_kdew_job* jobs, long n_jobs, const double* samples, const double* points,
                                const double* weights, double* sums, int threads) {
    constexpr long BLOCK = 8;                      // grid points of one piece of work
    host_share_blocks(n_jobs, threads, [&](long k) { return host_blocks((long)jobs[k].n_points, BLOCK); }, [&](long k, long block) {
        const pw_kdew_job& J = jobs[k];
        const long n = (long)J.n_samples, m = (long)J.n_points, nb = (long)J.n_replicas;
        const long j0 = block * BLOCK, j1 = std::min(j0 + BLOCK, m);
        const double* x = samples + J.sample_first;
        const double* wt = weights + J.weight_first;
        std::vector<double> s((size_t)nb, 0.0), p((size_t)nb, 0.0);   // (the piece's own: a pair a block of points)
        for (long j = j0; j < j1; ++j) {
            const double g = points[J.point_first + j];
            for (long b = 0; b < nb; ++b) s[b] = 0.0;
            for (long i0 = 0; i0 < n; i0 += KDE_CHUNK) {
                const int len = (int)std::min((long)KDE_CHUNK, n - i0);
                kdew_chunk_sums(g, x + i0, wt + i0 * nb, nb, len, nb, J.inv_bandwidth, POW_EXP_TAB, p.data());
                for (long b = 0; b < nb; ++b) s[b] = i0 == 0 ? p[b] : s[b] + p[b];
            }
            for (long b = 0; b < nb; ++b) sums[J.out_first + b * m + j] = s[b];
        }
    });
    return PW_OK;
}

// pw_corr_sums on the host (pw_corr.hip checks the arguments and sends device == -1 contexts here): the chunks
// of pw_corr.hpp, a lag's chunks in order, so the sums have the device's bits.  Threads share out blocks of
// BLOCK consecutive lags; a block's lags go through a chunk side by side (independent accumulators, each in
// its own t order) as far as the shortest of them reaches, and finish one by one.
extern "C" int pw_hostpath_corr(const pw_corr_job* jobs, long n_jobs, const double* series, double* sums, int threads) {
    constexpr long BLOCK = 16;                     // lags of one piece of work
    auto blocks = [&](long k) { return jobs[k].n ? host_blocks((long)jobs[k].n_lags, BLOCK) : 0; };
    host_share_blocks(n_jobs, threads, blocks, [&](long k, long block) {
        const pw_corr_job& J = jobs[k];
        const long n = (long)J.n, l0 = block * BLOCK, l1 = std::min(l0 + BLOCK, (long)J.n_lags);
        const double* a = series + J.a_first;
        const double* b = series + J.b_first;
        double s[BLOCK];
        for (long c = 0; c * CORR_CHUNK < n - l0; ++c) {
            const long t0 = c * CORR_CHUNK;
            double p[BLOCK];
            for (long j = 0; j < BLOCK; ++j) p[j] = 0.0;
            long t = 0;
            if (l1 - l0 == BLOCK) {
                const long all = std::max(0l, corr_chunk_len(n, l1 - 1, c));   // terms every lag of the block has
                const double* bb = b + t0 + l0;
                for (; t < all; ++t) {
                    const double av = a[t0 + t];
                    for (long j = 0; j < BLOCK; ++j) p[j] = pw_fma(av, bb[t + j], p[j]);
                }
            }
            for (long j = 0; j < l1 - l0; ++j) {
                const long len = corr_chunk_len(n, l0 + j, c);
                if (len <= 0) continue;            // the chunk does not exist for this lag
                double q = p[j];
                for (long u = t; u < len; ++u) q = pw_fma(a[t0 + u], b[t0 + u + l0 + j], q);
                s[j] = c == 0 ? q : s[j] + q;
            }
        }
        for (long j = 0; j < l1 - l0; ++j) sums[J.out_first + l0 + j] = s[j];
    });
    return PW_OK;
}

// pw_dft_sums on the host (pw_dft.hip checks the arguments and sends device == -1 contexts here): the definition
// of pw_dft.hpp, a frequency's chunks in order, so the sums have the device's bits.  Threads share out blocks of
// BLOCK consecutive frequencies of a job; a block's twiddles are computed once ([r][frequency], as the device's
// table) and its frequencies go through a chunk side by side (independent accumulators, each in its own r order).
extern "C" int pw_hostpath_dft(const pw_dft_job* jobs, long n_jobs, const double* series, double* re, double* im,
                               int threads) {
    constexpr long BLOCK = 8;                      // frequencies of one piece of work
    auto blocks = [&](long k) { return jobs[k].n && jobs[k].n_freq ? host_blocks((long)jobs[k].n_freq, BLOCK) : 0; };
    host_share_blocks(n_jobs, threads, blocks, [&](long k, long block) {
        const pw_dft_job& J = jobs[k];
        const long n = (long)J.n, M = (long)J.period;
        const long q0 = block * BLOCK, count = std::min(BLOCK, (long)J.n_freq - q0);
        const long steps = std::min(n, (long)DFT_CHUNK);
        double cA[DFT_CHUNK * BLOCK], sA[DFT_CHUNK * BLOCK];         // (the piece's own twiddles, 32 KiB each: no allocation)
        long j[BLOCK];
        for (long f = 0; f < BLOCK; ++f) j[f] = (long)J.j_first + (q0 + std::min(f, count - 1)) * (long)J.j_step;
        for (long r = 0; r < steps; ++r)
            for (long f = 0; f < BLOCK; ++f) dft_phase(j[f], r, M, &cA[r * BLOCK + f], &sA[r * BLOCK + f]);
        const double* a = series + J.a_first;
        double sr[BLOCK], si[BLOCK];
        for (long f = 0; f < BLOCK; ++f) sr[f] = si[f] = 0.0;
        for (long t0 = 0; t0 < n; t0 += DFT_CHUNK) {
            const long len = std::min((long)DFT_CHUNK, n - t0);
            double pc[BLOCK], ps[BLOCK];
            for (long f = 0; f < BLOCK; ++f) pc[f] = ps[f] = 0.0;
            for (long r = 0; r < len; ++r) {
                const double av = a[t0 + r];
                const double* c = &cA[r * BLOCK];
                const double* s = &sA[r * BLOCK];
                for (long f = 0; f < BLOCK; ++f) {
                    pc[f] = pw_fma(av, c[f], pc[f]);
                    ps[f] = pw_fma(av, s[f], ps[f]);
                }
            }
            for (long f = 0; f < count; ++f) {
                double cB, sB, x, y;
                dft_phase(j[f], t0, M, &cB, &sB);
                dft_rotate(cB, sB, pc[f], ps[f], &x, &y);
                sr[f] = sr[f] + x;
                si[f] = si[f] + y;
            }
        }
        for (long f = 0; f < count; ++f) {
            re[J.out_first + q0 + f] = sr[f];
            im[J.out_first + q0 + f] = si[f];
        }
    });
    return PW_OK;
}

// pw_gate_counts on the host (pw_gate.hip checks the arguments and sends device == -1 contexts here): the chunks,
// summaries and merge of pw_gate.hpp, the very functions the kernels run.  Threads share out (job, block of BLOCK
// consecutive thresholds) pairs; a threshold goes through the series chunk by chunk, and its row is its own.
extern "C" int pw_hostpath_gate(const pw_gate_job* jobs, long n_jobs, const double* series, const double* thresholds,
                                long n_bins, long* counts, long* hist, int threads) {
    constexpr long BLOCK = 16;                     // thresholds of one piece of work
    auto blocks = [&](long k) { return jobs[k].n && jobs[k].n_thr ? host_blocks((long)jobs[k].n_thr, BLOCK) : 0; };
    host_share_blocks(n_jobs, threads, blocks, [&](long k, long block) {
        const pw_gate_job& J = jobs[k];
        const long n = (long)J.n, q0 = block * BLOCK, q1 = std::min(q0 + BLOCK, (long)J.n_thr);
        const double* a = series + J.a_first;
        for (long q = q0; q < q1; ++q) {
            const double d = thresholds[J.d_first + q];
            const long row = (long)J.out_first + q;
            long* h = n_bins > 0 ? hist + row * 2 * n_bins : nullptr;
            for (long i = 0; i < 2 * n_bins; ++i) h[i] = 0;
            auto bin = [&](int s, long len) {
                if (n_bins > 0) h[s * n_bins + std::min(len, n_bins) - 1] += 1;
            };
            GateWalk W;
            GateTally<long> T;
            for (long t0 = 0; t0 < n; t0 += GATE_CHUNK)
                gate_merge(W, gate_chunk(a + t0, (int)std::min((long)GATE_CHUNK, n - t0), d, T, bin), T, bin);
            gate_finish(W, T, bin);
            long* c = counts + row * GATE_FIELDS;
            c[0] = T.n_open; c[1] = T.n_closed; c[2] = T.open_runs; c[3] = T.closed_runs;
            c[4] = T.longest_open; c[5] = T.longest_closed; c[6] = T.openings; c[7] = T.closings;
            c[8] = T.complete_open_runs; c[9] = T.complete_closed_runs;
            c[10] = T.complete_open_frames; c[11] = T.complete_closed_frames;
        }
    });
    return PW_OK;
}

// pw_trans_counts on the host (pw_trans.hip checks the arguments and sends device == -1 contexts here): the masks,
// funnel shift and popcount of pw_trans.hpp with 64-bit words.  First the threads share out the jobs and classify every
// entry once (trans_state) into one mask a reachable state, [state][word] with a word of zeros after the last; then
// they share out (job, block of BLOCK consecutive lags) pairs, and a lag's row is its own.
extern "C" int pw_hostpath_trans(const pw_trans_job* jobs, long n_jobs, const double* series, const double* edges,
                                 long n_states, long* counts, int threads) {
    typedef unsigned long long u64;
    constexpr long BLOCK = 16;                     // lags of one piece of work
    const long S = n_states;
    auto live = [&](long k) { return jobs[k].n && jobs[k].n_lags; };
    std::vector<long> m_first((size_t)n_jobs + 1, 0);
    for (long k = 0; k < n_jobs; ++k)
        m_first[k + 1] = m_first[k] + (live(k) ? ((long)jobs[k].n_edges + 1) * (((long)jobs[k].n + 63) / 64 + 1) : 0);
    std::vector<u64> masks((size_t)m_first[n_jobs], 0);
    host_share(n_jobs, threads, [&](long k) {                        // the masks, a job a piece
        const pw_trans_job& J = jobs[k];
        if (!live(k)) return;
        const long n = (long)J.n, stride = (n + 63) / 64 + 1;
        const double* a = series + J.a_first;
        u64* M = masks.data() + m_first[k];
        for (long t = 0; t < n; ++t) {
            const int s = trans_state(a[t], J.n_edges ? edges + J.e_first : nullptr, (int)J.n_edges);
            if (s != TRANS_GAP) M[s * stride + t / 64] |= 1ull << (t % 64);
        }
    });
    auto blocks = [&](long k) { return live(k) ? host_blocks((long)jobs[k].n_lags, BLOCK) : 0; };
    host_share_blocks(n_jobs, threads, blocks, [&](long k, long block) {   // the lags
        const pw_trans_job& J = jobs[k];
        const long n = (long)J.n, nw = (n + 63) / 64, stride = nw + 1, ns = (long)J.n_edges + 1;
        const long q0 = block * BLOCK, q1 = std::min(q0 + BLOCK, (long)J.n_lags);
        const u64* M = masks.data() + m_first[k];
        for (long q = q0; q < q1; ++q) {
            const long lag = (long)J.lag_first + q * (long)J.lag_step;
            long c[TRANS_MAX_STATES][TRANS_MAX_STATES] = {};
            if (lag < n) {
                const long ko = lag / 64;
                const unsigned r = (unsigned)(lag % 64);
                for (long x = 0; x + ko < nw; ++x)
                    for (long j = 0; j < ns; ++j) {
                        const u64 partner = trans_funnel(M[j * stride + x + ko + 1], M[j * stride + x + ko], r);
                        for (long i = 0; i < ns; ++i) trans_count(c[i][j], M[i * stride + x] & partner);
                    }
            }
            long* row = counts + ((long)J.out_first + q) * S * S;
            for (long i = 0; i < S; ++i)
                for (long j = 0; j < S; ++j) row[i * S + j] = c[i][j];
        }
    });
    return PW_OK;
}

// pw_superpose on the host (pw_superpose.hip checks the arguments and sends device == -1 contexts here): the 64
// accumulators of pw_superpose.hpp as arrays, atom i going to accumulator i % 64, folded by sup_fold.  The threads
// share out blocks of BLOCK jobs; a job's row is its own.
extern "C" int pw_hostpath_superpose(const pw_superpose_job* jobs, long n_jobs, const double* xyz, const double* weights,
                                     pw_superpose_out* out, int threads) {
    constexpr long BLOCK = 16;
    auto one = [&](const pw_superpose_job& J) {
        const long n = (long)J.n;
        const double* x = xyz + 3 * (long)J.mobile_first;
        const double* y = xyz + 3 * (long)J.target_first;
        const double* w = J.weight_first < 0 ? nullptr : weights + (long)J.weight_first;
        SupSums acc[SUP_ACC];
        double lanes[SUP_ACC];
        for (int l = 0; l < SUP_ACC; ++l) sup_sums_zero(acc[l]);
        for (long i = 0; i < n; ++i) sup_sums_atom(acc[i % SUP_ACC], x, y, w, i);
        SupSums s;
        auto fold = [&](auto field) {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = field(l);
            return sup_fold(lanes);
        };
        s.w = fold([&](int l) { return acc[l].w; });
        for (int a = 0; a < 3; ++a) {
            s.x[a] = fold([&](int l) { return acc[l].x[a]; });
            s.y[a] = fold([&](int l) { return acc[l].y[a]; });
        }
        SupCentres c;
        sup_centres(s, c);
        double macc[SUP_ACC][9] = {};
        for (long i = 0; i < n; ++i) sup_moment_atom(macc[i % SUP_ACC], c, x, y, w, i);
        double m[9], r[9], lambda[2];
        for (int k = 0; k < 9; ++k) m[k] = fold([&](int l) { return macc[l][k]; });
        const int sweeps = sup_solve(m, r, lambda);
        for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
        for (long i = 0; i < n; ++i) lanes[i % SUP_ACC] = sup_residual_atom(lanes[i % SUP_ACC], r, c, x, y, w, i);
        const double e = sup_fold(lanes);
        pw_superpose_out* o = out + (long)J.out;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) o->rotation[a][b] = r[3 * a + b];
            o->centre_mobile[a] = c.cx[a];
            o->centre_target[a] = c.cy[a];
        }
        o->rmsd = pw_sqrt(e / c.W);
        o->lambda[0] = lambda[0];
        o->lambda[1] = lambda[1];
        o->sweeps = sweeps;
        o->reserved = 0;
    };
    host_share(host_blocks(n_jobs, BLOCK), threads, [&](long p) {
        for (long k = p * BLOCK; k < std::min((p + 1) * BLOCK, n_jobs); ++k) one(jobs[k]);
    });
    return PW_OK;
}

// pw_cluster_gromos on the host (pw_cluster.hip checks the arguments and sends device == -1 contexts here): the bit
// matrix, the keys and the tail mask of pw_cluster.hpp.  The threads of a call are started once and woken a piece of
// work (a round of counts is too short to start threads for): they share out the rows of the pack, the tile rows of the
// mirror and the rows of every round's counts, each keeping the largest key of its rows; the largest of those is the
// centre, whatever the number of threads.  A round with little to count is taken by the calling thread alone.
namespace {
struct ClusterCrew {
    int threads;
    std::vector<std::thread> pool;
    std::mutex m;
    std::condition_variable go, back;
    std::function<void(int)> work;
    long generation = 0;
    int pending = 0;
    bool stop = false;
    explicit ClusterCrew(int t) : threads(t < 1 ? 1 : t) {
        for (int i = 1; i < threads; ++i) pool.emplace_back([this, i] { serve(i); });
    }
    ~ClusterCrew() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        go.notify_all();
        for (auto& t : pool) t.join();
    }
    void serve(int me) {
        long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> g(m);
            go.wait(g, [&] { return stop || generation != seen; });
            if (stop) return;
            seen = generation;
            g.unlock();
            work(me);
            g.lock();
            if (--pending == 0) back.notify_one();
        }
    }
    // f(t) for t = 0 .. threads - 1, t = 0 on the calling thread; returns when all have
    void run(const std::function<void(int)>& f) {
        if (threads == 1) return f(0);
        {
            std::lock_guard<std::mutex> g(m);
            work = f;
            pending = threads - 1;
            ++generation;
        }
        go.notify_all();
        f(0);
        std::unique_lock<std::mutex> g(m);
        back.wait(g, [&] { return pending == 0; });
    }
};
}  // namespace

extern "C" int pw_hostpath_cluster(const pw_cluster_job* jobs, long n_jobs, const double* dist, int* labels, int* centres,
                                   int* sizes, long* n_clusters, int threads) {
    typedef cluster_word u64;
    constexpr long SMALL = 4096;                   // words of a round below which the calling thread counts alone
    long n_max = 0;
    for (long k = 0; k < n_jobs; ++k) n_max = std::max(n_max, (long)jobs[k].n);
    if (threads < 1) threads = 1;
    if ((long)threads > (n_max + 63) / 64) threads = (int)std::max(1l, (n_max + 63) / 64);
    ClusterCrew crew(threads);
    const int T = crew.threads;
    std::vector<u64> bits, active;
    std::vector<u64> best((size_t)T);
    for (long k = 0; k < n_jobs; ++k) {
        const pw_cluster_job& J = jobs[k];
        const long n = (long)J.n, W = cluster_words(n), S = cluster_stride(n);
        n_clusters[k] = 0;
        if (n == 0) continue;
        const double* d = dist + J.d_first;
        const double cutoff = J.cutoff;
        int* lab = labels + J.out_first;
        int* cen = centres + J.out_first;
        int* siz = sizes + J.out_first;
        bits.assign((size_t)(n * S), 0);
        active.resize((size_t)S);
        u64* B = bits.data();
        // pack: the diagonal and the strict upper triangle, rows shared out in blocks of 64
        crew.run([&](int t) {
            for (long I = t; I < W; I += T)
                for (long i = 64 * I; i < std::min(64 * I + 64, n); ++i) {
                    B[i * S + i / 64] |= 1ull << (i % 64);
                    for (long j = i + 1; j < n; ++j)
                        if (cluster_pack_bit(i, j, n, d[i * n + j], cutoff)) B[i * S + j / 64] |= 1ull << (j % 64);
                }
        });
        // mirror: tile (I, Jt), I <= Jt, transposed into tile (Jt, I); a thread owns the tile rows Jt it writes
        crew.run([&](int t) {
            for (long Jt = t; Jt < W; Jt += T)
                for (long I = 0; I <= Jt; ++I) {
                    u64 a[64], tr[64];
                    for (long l = 0; l < 64; ++l) a[l] = 64 * I + l < n ? B[(64 * I + l) * S + Jt] : 0;
                    for (int c = 0; c < 64; ++c) {
                        u64 v = 0;
                        for (int l = 0; l < 64; ++l) v |= ((a[l] >> c) & 1ull) << l;
                        tr[c] = v;
                    }
                    for (long c = 0; c < 64 && 64 * Jt + c < n; ++c) {
                        u64& out = B[(64 * Jt + c) * S + I];
                        out = I == Jt ? (out | tr[c]) : tr[c];
                    }
                }
        });
        for (long w = 0; w < S; ++w) active[w] = cluster_tail_mask(n, w);
        for (long j = 0; j < n; ++j) {
            cen[j] = -1;
            siz[j] = 0;
        }
        const u64* A = active.data();
        long left = n, found = 0;
        while (left > 0) {
            auto count_rows = [&](long lo, long hi) {
                u64 mine = 0;
                for (long i = lo; i < hi; ++i) {
                    if (!((A[i >> 6] >> (i & 63)) & 1)) continue;
                    unsigned count = 0;
                    for (long w = 0; w < W; ++w) count += (unsigned)cluster_popcount(B[i * S + w] & A[w]);
                    mine = std::max(mine, cluster_key(count, (unsigned)i));
                }
                return mine;
            };
            u64 key = 0;
            if (T == 1 || left * W < SMALL) {
                key = count_rows(0, n);
            } else {
                crew.run([&](int t) { best[t] = count_rows(n * t / T, n * (t + 1) / T); });
                for (int t = 0; t < T; ++t) key = std::max(key, best[t]);
            }
            const long c = (long)cluster_key_row(key);
            cen[found] = (int)c;
            siz[found] = (int)cluster_key_count(key);
            for (long w = 0; w < W; ++w) {
                u64 m = B[c * S + w] & active[w];
                active[w] &= ~m;
                for (; m; m &= m - 1) lab[64 * w + __builtin_ctzll(m)] = (int)found;
            }
            left -= (long)cluster_key_count(key);
            ++found;
        }
        n_clusters[k] = found;
    }
    return PW_OK;
}

// pw_covariance and pw_project on the host (pw_cov.hip checks the arguments and sends device == -1 contexts here): the
// values, chunks and orders of pw_cov.hpp.  A job's values y are computed once into a buffer of the job, rows shared
// out among the threads; then blocks of columns take their chunk sums in order, the rows are centred in place, and
// the blocks of COV_HOST_BLOCK x COV_HOST_BLOCK entries on or above the diagonal take their chunk partials in order
// and are written to both triangles.  An entry's sums are its own, whatever the number of threads.
namespace {
constexpr long COV_HOST_BLOCK = 32;

// y[t][a] of the job's rows, or z = y - mean when mean is not null
void cov_host_values(const double* x, const double* tr, long T, long D, const double* mean, int threads, double* y) {
    constexpr long ROWS = 64;
    host_share((T + ROWS - 1) / ROWS, threads, [&](long p) {
        for (long t = p * ROWS; t < std::min((p + 1) * ROWS, T); ++t) {
            const double* trow = tr ? tr + t * COV_TRANSFORM_DOUBLES : nullptr;
            for (long a = 0; a < D; ++a) {
                const double v = cov_y(x + t * D, trow, a);
                y[t * D + a] = mean ? v - mean[a] : v;
            }
        }
    });
}
}  // namespace

extern "C" int pw_hostpath_covariance(const pw_cov_job* jobs, long n_jobs, const double* data, const double* transforms,
                                      double* mean, double* scatter, int threads) {
    std::vector<double> y;
    for (long k = 0; k < n_jobs; ++k) {
        const pw_cov_job& J = jobs[k];
        const long T = (long)J.T, D = (long)J.D, chunks = (T + COV_CHUNK - 1) / COV_CHUNK;
        const double* x = data + (long)J.x_first;
        const double* tr = J.transform_first < 0 ? nullptr : transforms + (long)J.transform_first * COV_TRANSFORM_DOUBLES;
        double* m = mean + (long)J.mean_first;
        y.resize((size_t)(T * D));
        cov_host_values(x, tr, T, D, nullptr, threads, y.data());
        const long col_blocks = (D + COV_HOST_BLOCK - 1) / COV_HOST_BLOCK;
        host_share(col_blocks, threads, [&](long p) {
            const long a0 = p * COV_HOST_BLOCK, w = std::min(COV_HOST_BLOCK, D - a0);
            double total[COV_HOST_BLOCK];
            for (long c = 0; c < chunks; ++c) {
                double s[COV_HOST_BLOCK];
                for (long i = 0; i < w; ++i) s[i] = 0.0;
                for (long t = c * COV_CHUNK; t < std::min((c + 1) * COV_CHUNK, T); ++t)
                    for (long i = 0; i < w; ++i) s[i] = s[i] + y[t * D + a0 + i];
                for (long i = 0; i < w; ++i) total[i] = c == 0 ? s[i] : total[i] + s[i];
            }
            for (long i = 0; i < w; ++i) m[a0 + i] = total[i] / (double)T;
        });
        if (J.s_first < 0) continue;
        host_share((T + 63) / 64, threads, [&](long p) {
            for (long t = p * 64; t < std::min((p + 1) * 64, T); ++t)
                for (long a = 0; a < D; ++a) y[t * D + a] = y[t * D + a] - m[a];
        });
        double* S = scatter + (long)J.s_first;
        host_share(col_blocks * (col_blocks + 1) / 2, threads, [&](long p) {
            int ba, bb;
            cov_tile_of(p, (int)col_blocks, ba, bb);
            const long a0 = ba * COV_HOST_BLOCK, b0 = bb * COV_HOST_BLOCK;
            const long wa = std::min(COV_HOST_BLOCK, D - a0), wb = std::min(COV_HOST_BLOCK, D - b0);
            double s[COV_HOST_BLOCK][COV_HOST_BLOCK], part[COV_HOST_BLOCK][COV_HOST_BLOCK];
            for (long c = 0; c < chunks; ++c) {
                for (long i = 0; i < wa; ++i)
                    for (long j = 0; j < wb; ++j) part[i][j] = 0.0;
                for (long t = c * COV_CHUNK; t < std::min((c + 1) * COV_CHUNK, T); ++t) {
                    const double* za = y.data() + t * D + a0;
                    const double* zb = y.data() + t * D + b0;
                    for (long i = 0; i < wa; ++i) {
                        const double zi = za[i];
                        for (long j = 0; j < wb; ++j) part[i][j] = pw_fma(zi, zb[j], part[i][j]);
                    }
                }
                for (long i = 0; i < wa; ++i)
                    for (long j = 0; j < wb; ++j) s[i][j] = c == 0 ? part[i][j] : s[i][j] + part[i][j];
            }
            for (long i = 0; i < wa; ++i)
                for (long j = 0; j < wb; ++j) {
                    if (a0 + i > b0 + j) continue;             // (below the diagonal of a diagonal block: the mirror writes it)
                    S[(a0 + i) * D + b0 + j] = s[i][j];
                    S[(b0 + j) * D + a0 + i] = s[i][j];
                }
        });
    }
    return PW_OK;
}

extern "C" int pw_hostpath_project(const pw_project_job* jobs, long n_jobs, const double* data, const double* transforms,
                                   const double* mean, const double* vectors, double* proj, int threads) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_project_job& J = jobs[k];
        const long T = (long)J.T, D = (long)J.D, K = (long)J.k;
        const double* x = data + (long)J.x_first;
        const double* tr = J.transform_first < 0 ? nullptr : transforms + (long)J.transform_first * COV_TRANSFORM_DOUBLES;
        const double* m = mean + (long)J.mean_first;
        const double* V = vectors + (long)J.v_first;
        double* P = proj + (long)J.p_first;
        constexpr long ROWS = 16;
        host_share((T + ROWS - 1) / ROWS, threads, [&](long p) {
            std::vector<double> z((size_t)D);
            for (long t = p * ROWS; t < std::min((p + 1) * ROWS, T); ++t) {
                const double* trow = tr ? tr + t * COV_TRANSFORM_DOUBLES : nullptr;
                for (long a = 0; a < D; ++a) z[a] = cov_y(x + t * D, trow, a) - m[a];
                for (long j = 0; j < K; ++j) {
                    double acc[COV_PROJ_ACC];
                    for (int l = 0; l < COV_PROJ_ACC; ++l) acc[l] = 0.0;
                    for (long a = 0; a < D; ++a) acc[a % COV_PROJ_ACC] = pw_fma(z[a], V[j * D + a], acc[a % COV_PROJ_ACC]);
                    static_assert(COV_PROJ_ACC == SUP_ACC, "sup_fold folds SUP_ACC accumulators");
                    P[t * K + j] = sup_fold(acc);
                }
            }
        });
    }
    return PW_OK;
}

// pw_cavity on the host (pw_cavity.hip checks the arguments and sends device == -1 contexts here): the voxel, plane
// and row-culling tests, the spread inside a word and the sums of a row of pw_cavity.hpp.  The threads share out the
// jobs; a job is a plain loop over its rows -- classify, then sweeps forwards and backwards over the words until one
// changes nothing (at most nx * ny * nz + 1 of them), then the sums of the rows.  A job's row of the result is its own.
namespace {
// a grid and what it is classified against (the fields that pw_cavity_job and pw_pores_job have in common)
struct CavityHostGrid {
    const double *atoms, *reach, *cuts;
    long n, m;
    const double* origin;
    double h;
    int nx, ny, nz;
    const int* seed;
};

// the open words of the grid for a probe
void cavity_host_open(const CavityHostGrid& G, double probe, std::vector<cavity_word>& open) {
    const int nx = G.nx, ny = G.ny, rows = G.ny * G.nz;
    for (int r = 0; r < rows; ++r) {
        const double y = cavity_coord(G.origin[1], r % ny, G.h), z = cavity_coord(G.origin[2], r / ny, G.h);
        cavity_word word = cavity_row_mask(nx);
        for (long a = 0; a < G.n && word; ++a) {
            const double r2 = cavity_reach2(G.reach[a], probe);
            const double dy = y - G.atoms[3 * a + 1], dz = z - G.atoms[3 * a + 2];
            if (cavity_row_clear(dy, dz, r2)) continue;
            for (int i = 0; i < nx; ++i)
                if (!cavity_free(cavity_coord(G.origin[0], i, G.h) - G.atoms[3 * a], dy, dz, r2)) word &= ~(1ull << i);
        }
        for (long q = 0; q < G.m && word; ++q)
            for (int i = 0; i < nx; ++i)
                if (!cavity_inside(G.cuts + 4 * q, cavity_coord(G.origin[0], i, G.h), y, z)) word &= ~(1ull << i);
        open[r] = word;
    }
}

// the component of the open words that holds the seed voxel into `fill`; false, and fill all zero, if the seed is closed
bool cavity_host_fill(const CavityHostGrid& G, const std::vector<cavity_word>& open, std::vector<cavity_word>& fill) {
    const int nx = G.nx, ny = G.ny, nz = G.nz, rows = ny * nz;
    std::fill(fill.begin(), fill.end(), 0);
    const int seed_row = G.seed[2] * ny + G.seed[1];
    const cavity_word seed_bit = 1ull << G.seed[0];
    const bool seed_open = (open[seed_row] & seed_bit) != 0;
    if (seed_open) fill[seed_row] = seed_bit;
    auto word_of = [&](int j, int l) -> cavity_word { return j < 0 || j >= ny || l < 0 || l >= nz ? 0 : fill[l * ny + j]; };
    auto visit = [&](int r) {
        if (!open[r]) return false;
        const int j = r % ny, l = r / ny;
        const cavity_word g = cavity_fill_word(fill[r] | word_of(j - 1, l) | word_of(j + 1, l) | word_of(j, l - 1) | word_of(j, l + 1),
                                               open[r]);
        const bool changed = g != fill[r];
        fill[r] = g;
        return changed;
    };
    const long max_sweeps = (long)nx * ny * nz + 1;
    for (long sweep = 0; seed_open && sweep < max_sweeps; ++sweep) {
        bool changed = false;
        for (int r = 0; r < rows; ++r) changed = visit(r) || changed;
        for (int r = rows - 1; r >= 0; --r) changed = visit(r) || changed;
        if (!changed) break;
    }
    return seed_open;
}
}  // namespace

extern "C" int pw_hostpath_cavity(const pw_cavity_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                  const double* planes, pw_cavity_out* out, unsigned long long* mask,
                                  const unsigned long long* open_words, const long* open_first, int threads) {
    typedef cavity_word u64;
    host_share(n_jobs, threads, [&](long k) {
        const pw_cavity_job& J = jobs[k];
        const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz;
        const CavityHostGrid G{xyz + 3 * (long)J.atom_first, radii + (long)J.radius_first, planes + 4 * (long)J.plane_first,
                               (long)J.n, (long)J.m, J.origin, J.spacing, nx, ny, nz, J.seed};
        std::vector<u64> open((size_t)rows), fill((size_t)rows, 0);
        if (open_first && open_first[k] >= 0) {
            for (int r = 0; r < rows; ++r) open[r] = open_words[open_first[k] + r] & cavity_row_mask(nx);
        } else {
            cavity_host_open(G, J.probe, open);
        }
        const bool seed_open = cavity_host_fill(G, open, fill);
        auto word_of = [&](int j, int l) -> u64 { return j < 0 || j >= ny || l < 0 || l >= nz ? 0 : fill[l * ny + j]; };
        pw_cavity_out o{};
        u64 any = 0;
        int box[4] = {CAVITY_MAX_G, -1, CAVITY_MAX_G, -1};
        for (int r = 0; r < rows; ++r) {
            o.n_open += cavity_popcount(open[r]);
            const u64 f = fill[r];
            if (J.mask_first >= 0) mask[(long)J.mask_first + r] = f;
            if (!f) continue;
            const int j = r % ny, l = r / ny;
            CavityRow R;
            cavity_row_sums(f, word_of(j - 1, l), word_of(j + 1, l), word_of(j, l - 1), word_of(j, l + 1), nx, ny, nz, j, l, R);
            o.n_voxels += R.n;
            o.n_surface += R.surface;
            o.n_face += R.face;
            for (int a = 0; a < 3; ++a) o.first[a] += R.first[a];
            for (int a = 0; a < 6; ++a) o.second[a] += R.second[a];
            any |= f;
            box[0] = std::min(box[0], j); box[1] = std::max(box[1], j);
            box[2] = std::min(box[2], l); box[3] = std::max(box[3], l);
        }
        o.box[0] = any ? __builtin_ctzll(any) : -1;
        o.box[1] = any ? 63 - __builtin_clzll(any) : -1;
        for (int a = 0; a < 4; ++a) o.box[2 + a] = any ? box[a] : -1;
        o.flags = seed_open ? 0 : CAVITY_SEED_CLOSED;
        o.reserved = 0;
        out[(long)J.out] = o;
    });
    return PW_OK;
}

// pw_pore_sizes on the host (pw_pores.hip checks the arguments and sends device == -1 contexts here): a level's reach
// by the steps of pw_cavity above, K, the spread and the swept word of a row of pw_pores.hpp.  The threads share out
// the jobs; a job runs its levels from the first to the last, keeps every level's swept words inside the domain, and
// then hands every voxel of the domain to the largest level that covers it, from the last level down.
extern "C" int pw_hostpath_pore_sizes(const pw_pores_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                      const double* planes, const double* probes, pw_pores_level* levels,
                                      pw_pores_out* out, unsigned long long* mask, const unsigned long long* open_words,
                                      const long* open_first, int threads) {
    typedef cavity_word u64;
    host_share(n_jobs, threads, [&](long k) {
        const pw_pores_job& J = jobs[k];
        const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz, L = (int)J.n_levels;
        const u64 xmask = cavity_row_mask(nx);
        const CavityHostGrid G{xyz + 3 * (long)J.atom_first, radii + (long)J.radius_first, planes + 4 * (long)J.plane_first,
                               (long)J.n, (long)J.m, J.origin, J.spacing, nx, ny, nz, J.seed};
        std::vector<u64> open((size_t)rows), fill((size_t)rows), domain((size_t)rows, 0), swept((size_t)L * rows, 0);
        pw_pores_level* LV = levels + (long)J.level_first;
        for (int lv = 0; lv < L; ++lv) {
            const double probe = probes[(long)J.probe_first + lv];
            if (open_first && open_first[k] >= 0) {
                for (int r = 0; r < rows; ++r) open[r] = open_words[open_first[k] + (long)lv * rows + r] & xmask;
            } else {
                cavity_host_open(G, probe, open);
            }
            const bool seed_open = cavity_host_fill(G, open, fill);
            if (lv == 0) domain = fill;
            pw_pores_level o{};
            o.k2 = pores_k2(probe, J.spacing);
            o.flags = seed_open ? 0 : CAVITY_SEED_CLOSED;
            u64* mine = swept.data() + (size_t)lv * rows;
            for (int r = 0; r < rows; ++r) {
                const int j = r % ny, l = r / ny;
                o.n_reach += cavity_popcount(fill[r]);
                o.n_face += cavity_row_face(fill[r], nx, ny, nz, j, l);
                if (seed_open && domain[r])
                    mine[r] = pores_dilate_row([&](int s) { return fill[s]; }, j, l, ny, nz, o.k2, xmask) & domain[r];
                o.n_swept += cavity_popcount(mine[r]);
            }
            LV[lv] = o;
        }
        std::vector<u64> assigned((size_t)rows, 0);
        for (int lv = L - 1; lv >= 0; --lv)
            for (int r = 0; r < rows; ++r) {
                const u64 taken = swept[(size_t)lv * rows + r] & ~assigned[r];
                LV[lv].n_largest += cavity_popcount(taken);
                assigned[r] |= taken;
            }
        pw_pores_out total{0, 0, L};
        for (int r = 0; r < rows; ++r) {
            total.n_domain += cavity_popcount(domain[r]);
            total.n_none += cavity_popcount(domain[r] & ~assigned[r]);
        }
        out[(long)J.out] = total;
        if (J.mask_first >= 0) memcpy(mask + (long)J.mask_first, swept.data(), sizeof(u64) * swept.size());
    });
    return PW_OK;
}

// pw_sasa on the host (pw_sasa.hip checks the arguments and sends device == -1 contexts here): the test point, the
// exposure test, the cell search, the corner test and the culling rule of pw_sasa.hpp.  The threads share out pieces of
// SASA_HOST_ATOMS atoms of a job; an atom collects the atoms that sasa_far does not rule out and runs its P points
// down that list.  An atom's counts are its own; a job's row is summed from them afterwards, in order.
extern "C" int pw_hostpath_sasa(const pw_sasa_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                const double* directions, long P, const unsigned long long* words, int* exposed,
                                int* inside, pw_sasa_out* out, int threads) {
    constexpr long SASA_HOST_ATOMS = 16;
    struct Piece { long job, a_begin, a_end; };
    std::vector<Piece> pieces;
    std::vector<double> slack((size_t)n_jobs);
    for (long k = 0; k < n_jobs; ++k) {
        const pw_sasa_job& J = jobs[k];
        slack[k] = J.n ? sasa_slack(sasa_magnitude(xyz + 3 * (long)J.atom_first, radii + (long)J.radius_first, (long)J.n, J.probe)) : -1.0;
        for (long a = 0; a < (long)J.n; a += SASA_HOST_ATOMS) pieces.push_back({k, a, std::min(a + SASA_HOST_ATOMS, (long)J.n)});
    }
    host_share((long)pieces.size(), threads, [&](long p) {
        const Piece& piece = pieces[p];
        const pw_sasa_job& J = jobs[piece.job];
        const double* atoms = xyz + 3 * (long)J.atom_first;
        const double* reach = radii + (long)J.radius_first;
        const bool grid = J.word_first >= 0;
        const cavity_word* w = grid ? words + (long)J.word_first : nullptr;
        std::vector<double> near;
        for (long i = piece.a_begin; i < piece.a_end; ++i) {
            const double Xi = atoms[3 * i], Yi = atoms[3 * i + 1], Zi = atoms[3 * i + 2], Ri = sasa_reach(reach[i], J.probe);
            near.clear();
            for (long a = 0; a < (long)J.n; ++a) {
                const double R = sasa_reach(reach[a], J.probe);
                if (a == i || sasa_far(Xi - atoms[3 * a], Yi - atoms[3 * a + 1], Zi - atoms[3 * a + 2], Ri, R, slack[piece.job])) continue;
                near.insert(near.end(), {atoms[3 * a], atoms[3 * a + 1], atoms[3 * a + 2], R * R});
            }
            int n_exposed = 0, n_inside = 0;
            for (long k = 0; k < P; ++k) {
                const double px = sasa_point(Xi, Ri, directions[3 * k]), py = sasa_point(Yi, Ri, directions[3 * k + 1]),
                             pz = sasa_point(Zi, Ri, directions[3 * k + 2]);
                bool open = true;
                for (size_t e = 0; e < near.size() && open; e += 4)
                    open = sasa_exposed(px - near[e], py - near[e + 1], pz - near[e + 2], near[e + 3]);
                if (!open) continue;
                ++n_exposed;
                if (grid && sasa_inside(px, py, pz, J.origin, J.spacing, J.nx, J.ny, J.nz, [&](int r) { return w[r]; })) ++n_inside;
            }
            exposed[(long)J.count_first + i] = n_exposed;
            inside[(long)J.count_first + i] = n_inside;
        }
    });
    for (long k = 0; k < n_jobs; ++k) {
        const pw_sasa_job& J = jobs[k];
        pw_sasa_out o{};
        for (long i = 0; i < (long)J.n; ++i) {
            o.exposed += exposed[(long)J.count_first + i];
            o.inside += inside[(long)J.count_first + i];
        }
        o.flags = J.word_first >= 0 ? SASA_GRID : 0;
        out[(long)J.out] = o;
    }
    return PW_OK;
}

// pw_affinity on the host (pw_affinity.hip checks the arguments, counts the voxels of every region and sends
// device == -1 contexts here): the pair term, the blocked and counts tests, the weight with its clamp, the chunk tree and
// the search of a rank's voxel of pw_affinity.hpp.  The threads share out (job, chunk) pieces, each of which leaves the
// partial of pw_affinity.hpp; then one ordered reduce a job.
extern "C" int pw_hostpath_affinity(const pw_affinity_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                    const double* coef, const unsigned long long* words, const double* betas,
                                    const double* edges, double* energies, pw_affinity_level* levels, long long* hist,
                                    pw_affinity_out* out, int threads) {
    typedef cavity_word u64;
    struct Plan { long piece_first, part_first, prefix_first; };
    std::vector<Plan> plan((size_t)n_jobs + 1);
    long pieces = 0, part_words = 0, prefix_ints = 0;
    for (long k = 0; k < n_jobs; ++k) {
        const pw_affinity_job& J = jobs[k];
        plan[k] = Plan{pieces, part_words, prefix_ints};
        const long chunks = (voxels[k] + AFF_CHUNK - 1) / AFF_CHUNK;
        pieces += chunks;
        part_words += chunks * aff_part_words((int)J.n_betas, (int)J.n_edges);
        if (J.word_first >= 0) prefix_ints += (long)J.ny * J.nz + 1;
    }
    plan[n_jobs] = Plan{pieces, part_words, prefix_ints};
    std::vector<u64> part((size_t)part_words);
    std::vector<int> prefix((size_t)prefix_ints);
    for (long k = 0; k < n_jobs; ++k) {
        const pw_affinity_job& J = jobs[k];
        if (J.word_first < 0) continue;
        int* p = prefix.data() + plan[k].prefix_first;
        const int rows = J.ny * J.nz;
        p[0] = 0;
        for (int r = 0; r < rows; ++r) p[r + 1] = p[r] + cavity_popcount(words[(long)J.word_first + r] & cavity_row_mask(J.nx));
    }
    // the voxel of a rank of job k
    auto voxel_of = [&](long k, long rank, int& i, int& row) {
        const pw_affinity_job& J = jobs[k];
        const u64* w = J.word_first >= 0 ? words + (long)J.word_first : nullptr;
        const int* p = prefix.data() + plan[k].prefix_first;
        aff_voxel(rank, J.word_first >= 0, J.nx, J.ny * J.nz, [&](int r) { return w[r]; }, [&](int r) { return p[r]; }, i, row);
    };
    host_share(pieces, threads, [&](long piece) {
        long k = 0, hi = n_jobs;                                     // the last job with piece_first <= piece
        while (hi - k > 1) {
            const long mid = (k + hi) / 2;
            if (plan[mid].piece_first <= piece) k = mid; else hi = mid;
        }
        const pw_affinity_job& J = jobs[k];
        const int L = (int)J.n_betas, E = (int)J.n_edges, stride = aff_part_words(L, E);
        const long chunk = piece - plan[k].piece_first, V = voxels[k];
        const double* atoms = xyz + 3 * (long)J.atom_first;
        const double* ab = coef + 2 * (long)J.coef_first;
        double U[AFF_CHUNK], slot_z[AFF_CHUNK], slot_e[AFF_CHUNK];
        bool live[AFF_CHUNK];
        long n_blocked = 0;
        for (int t = 0; t < AFF_CHUNK; ++t) {
            const long rank = chunk * AFF_CHUNK + t;
            U[t] = 0.0;
            live[t] = false;
            if (rank >= V) continue;
            int i, row;
            voxel_of(k, rank, i, row);
            const double x = cavity_coord(J.origin[0], i, J.spacing), y = cavity_coord(J.origin[1], row % J.ny, J.spacing),
                         z = cavity_coord(J.origin[2], row / J.ny, J.spacing);
            double u_sum = 0.0;
            bool blocked = false;
            for (long a = 0; a < (long)J.n && !blocked; ++a) {
                const double r2 = aff_r2(x - atoms[3 * a], y - atoms[3 * a + 1], z - atoms[3 * a + 2]);
                blocked = aff_blocked(r2, J.core2);
                if (!blocked && aff_counts(r2, J.cutoff2)) u_sum = u_sum + aff_pair(r2, ab[2 * a], ab[2 * a + 1]);
            }
            n_blocked += blocked;
            live[t] = !blocked;
            U[t] = u_sum;
            if (J.energy_first >= 0) energies[(long)J.energy_first + rank] = blocked ? aff_inf() : u_sum;
        }
        u64* P = part.data() + plan[k].part_first + chunk * stride;
        bool clamped = false;
        for (int b = 0; b < L; ++b) {
            for (int t = 0; t < AFF_CHUNK; ++t) {
                slot_z[t] = slot_e[t] = 0.0;
                if (!live[t]) continue;
                const double w = aff_weight(betas[(long)J.beta_first + b], U[t], POW_EXP_TAB, clamped);
                slot_z[t] = w;
                slot_e[t] = w * U[t];
            }
            P[2 * b] = pw_d2bits(aff_tree(slot_z));
            P[2 * b + 1] = pw_d2bits(aff_tree(slot_e));
        }
        double m = aff_inf();
        long m_rank = chunk * AFF_CHUNK;
        for (int t = 0; t < AFF_CHUNK; ++t)
            if (live[t] && U[t] < m) {
                m = U[t];
                m_rank = chunk * AFF_CHUNK + t;
            }
        P[2 * L] = pw_d2bits(m);
        P[2 * L + 1] = (u64)m_rank;
        P[2 * L + 2] = (u64)n_blocked;
        P[2 * L + 3] = clamped ? (u64)AFF_CLAMPED : 0ull;
        for (int e = 0; e < E; ++e) {
            long below = 0;
            for (int t = 0; t < AFF_CHUNK; ++t) below += live[t] && U[t] < edges[(long)J.edge_first + e];
            P[2 * L + AFF_PART_FIXED + e] = (u64)below;
        }
    });
    host_share(n_jobs, threads, [&](long k) {
        const pw_affinity_job& J = jobs[k];
        const int L = (int)J.n_betas, E = (int)J.n_edges, stride = aff_part_words(L, E);
        const long chunks = plan[k + 1].piece_first - plan[k].piece_first;
        const u64* P = part.data() + plan[k].part_first;
        for (int b = 0; b < L; ++b) {
            double sz = 0.0, se = 0.0;
            for (long c = 0; c < chunks; ++c) {
                sz = sz + pw_bits2d(P[c * stride + 2 * b]);
                se = se + pw_bits2d(P[c * stride + 2 * b + 1]);
            }
            levels[(long)J.level_first + b] = pw_affinity_level{sz, se};
        }
        pw_affinity_out o{voxels[k], 0, aff_inf(), {-1, -1, -1}, 0};
        long rank = -1;
        for (long c = 0; c < chunks; ++c) {
            const double v = pw_bits2d(P[c * stride + 2 * L]);
            if (v < o.u_min) {
                o.u_min = v;
                rank = (long)P[c * stride + 2 * L + 1];
            }
            o.n_blocked += (long)P[c * stride + 2 * L + 2];
            o.flags |= (int)P[c * stride + 2 * L + 3];
        }
        if (rank >= 0) {
            int i, row;
            voxel_of(k, rank, i, row);
            o.min_voxel[0] = i;
            o.min_voxel[1] = row % J.ny;
            o.min_voxel[2] = row / J.ny;
        }
        out[(long)J.out] = o;
        for (int e = 0; e < E; ++e) {
            long long s = 0;
            for (long c = 0; c < chunks; ++c) s += (long long)P[c * stride + 2 * L + AFF_PART_FIXED + e];
            hist[(long)J.hist_first + e] = s;
        }
    });
    return PW_OK;
}

// pw_rigid_affinity on the host (pw_rigid.hip checks the arguments, counts the voxels of every region and sends
// device == -1 contexts here): the site position, the charged pair term and the fold over the orientations of
// pw_rigid.hpp on the pair term, the tests, the weight, the chunk tree and the search of a rank's voxel of
// pw_affinity.hpp.  The threads share out (job, chunk) pieces, each of which leaves the partial of pw_rigid.hpp; then one
// ordered reduce a job.  pw_rigid_body_affinity (pw_rigid_body.hip) is the same walk with the site position read from
// the job's pose table (pw_rigid_body.hpp), so both entries go through rigid_on_host: `site(J, o, s, x, y, z, px, py,
// pz)` places site s of pose o of job J at the voxel centre (x, y, z).
template <class Job, class Site>
static int rigid_on_host(const Job* jobs, long n_jobs, const long* voxels, const double* xyz, const double* coef,
                         const unsigned long long* words, const double* betas, double* maps, pw_affinity_level* levels,
                         pw_rigid_out* out, int threads, Site site) {
    typedef cavity_word u64;
    struct Plan { long piece_first, part_first, prefix_first; };
    std::vector<Plan> plan((size_t)n_jobs + 1);
    long pieces = 0, part_words = 0, prefix_ints = 0;
    for (long k = 0; k < n_jobs; ++k) {
        const Job& J = jobs[k];
        plan[k] = Plan{pieces, part_words, prefix_ints};
        const long chunks = (voxels[k] + AFF_CHUNK - 1) / AFF_CHUNK;
        pieces += chunks;
        part_words += chunks * rigid_part_words((int)J.n_betas);
        if (J.word_first >= 0) prefix_ints += (long)J.ny * J.nz + 1;
    }
    plan[n_jobs] = Plan{pieces, part_words, prefix_ints};
    std::vector<u64> part((size_t)part_words);
    std::vector<int> prefix((size_t)prefix_ints);
    for (long k = 0; k < n_jobs; ++k) {
        const Job& J = jobs[k];
        if (J.word_first < 0) continue;
        int* p = prefix.data() + plan[k].prefix_first;
        const int rows = J.ny * J.nz;
        p[0] = 0;
        for (int r = 0; r < rows; ++r) p[r + 1] = p[r] + cavity_popcount(words[(long)J.word_first + r] & cavity_row_mask(J.nx));
    }
    auto voxel_of = [&](long k, long rank, int& i, int& row) {
        const Job& J = jobs[k];
        const u64* w = J.word_first >= 0 ? words + (long)J.word_first : nullptr;
        const int* p = prefix.data() + plan[k].prefix_first;
        aff_voxel(rank, J.word_first >= 0, J.nx, J.ny * J.nz, [&](int r) { return w[r]; }, [&](int r) { return p[r]; }, i, row);
    };
    host_share(pieces, threads, [&](long piece) {
        long k = 0, hi = n_jobs;                                     // the last job with piece_first <= piece
        while (hi - k > 1) {
            const long mid = (k + hi) / 2;
            if (plan[mid].piece_first <= piece) k = mid; else hi = mid;
        }
        const Job& J = jobs[k];
        const int L = (int)J.n_betas, S = (int)J.n_sites, M = (int)J.n_dirs, stride = rigid_part_words(L);
        const long chunk = piece - plan[k].piece_first, V = voxels[k], n = (long)J.n;
        const bool charged = J.charged != 0;
        const double* atoms = xyz + 3 * (long)J.atom_first;
        const double* abc = coef + 3 * (long)J.coef_first;
        const double inv_M = rigid_inv(M);
        double slot_z[AFF_MAX_LEVELS][AFF_CHUNK], slot_e[AFF_MAX_LEVELS][AFF_CHUNK];
        double m = aff_inf();
        long m_rank = chunk * AFF_CHUNK, m_dir = 0, n_blocked = 0, n_dead = 0;
        bool clamped = false;
        for (int t = 0; t < AFF_CHUNK; ++t) {
            for (int b = 0; b < L; ++b) slot_z[b][t] = slot_e[b][t] = 0.0;
            const long rank = chunk * AFF_CHUNK + t;
            if (rank >= V) continue;
            int i, row;
            voxel_of(k, rank, i, row);
            const double x = cavity_coord(J.origin[0], i, J.spacing), y = cavity_coord(J.origin[1], row % J.ny, J.spacing),
                         z = cavity_coord(J.origin[2], row / J.ny, J.spacing);
            RigidFold fold[AFF_MAX_LEVELS];
            double umin_v = aff_inf();
            int n_live = 0;
            for (int o = 0; o < M; ++o) {
                bool blocked = false;
                double U = 0.0;
                for (int s = 0; s < S && !blocked; ++s) {
                    double px, py, pz;
                    site(J, o, s, x, y, z, px, py, pz);
                    const double* rows = abc + 3 * (long)s * n;
                    double Us = 0.0;
                    for (long a = 0; a < n && !blocked; ++a) {
                        const double r2 = aff_r2(px - atoms[3 * a], py - atoms[3 * a + 1], pz - atoms[3 * a + 2]);
                        blocked = aff_blocked(r2, J.core2);
                        if (blocked || !aff_counts(r2, J.cutoff2)) continue;
                        Us = Us + (charged ? rigid_pair<true>(r2, rows[3 * a], rows[3 * a + 1], rows[3 * a + 2])
                                           : rigid_pair<false>(r2, rows[3 * a], rows[3 * a + 1], 0.0));
                    }
                    U = s ? U + Us : Us;
                }
                if (blocked) {
                    ++n_blocked;
                    continue;
                }
                ++n_live;
                if (U < umin_v) umin_v = U;
                if (U < m) {
                    m = U;
                    m_rank = rank;
                    m_dir = o;
                }
                for (int b = 0; b < L; ++b) fold[b].add(aff_weight(betas[(long)J.beta_first + b], U, POW_EXP_TAB, clamped), U);
            }
            n_dead += n_live == 0;
            for (int b = 0; b < L; ++b) {
                slot_z[b][t] = fold[b].zbar(inv_M);
                slot_e[b][t] = fold[b].ebar(inv_M);
            }
            if (J.map_level >= 0) {
                maps[(long)J.map_first + 2 * rank] = fold[J.map_level].zbar(inv_M);
                maps[(long)J.map_first + 2 * rank + 1] = umin_v;
            }
        }
        u64* P = part.data() + plan[k].part_first + chunk * stride;
        for (int b = 0; b < L; ++b) {
            P[2 * b] = pw_d2bits(aff_tree(slot_z[b]));
            P[2 * b + 1] = pw_d2bits(aff_tree(slot_e[b]));
        }
        P[2 * L] = pw_d2bits(m);
        P[2 * L + 1] = (u64)m_rank;
        P[2 * L + 2] = (u64)m_dir;
        P[2 * L + 3] = (u64)n_blocked;
        P[2 * L + 4] = (u64)n_dead;
        P[2 * L + 5] = clamped ? (u64)AFF_CLAMPED : 0ull;
    });
    host_share(n_jobs, threads, [&](long k) {
        const Job& J = jobs[k];
        const int L = (int)J.n_betas, stride = rigid_part_words(L);
        const long chunks = plan[k + 1].piece_first - plan[k].piece_first;
        const u64* P = part.data() + plan[k].part_first;
        for (int b = 0; b < L; ++b) {
            double sz = 0.0, se = 0.0;
            for (long c = 0; c < chunks; ++c) {
                sz = sz + pw_bits2d(P[c * stride + 2 * b]);
                se = se + pw_bits2d(P[c * stride + 2 * b + 1]);
            }
            levels[(long)J.level_first + b] = pw_affinity_level{sz, se};
        }
        pw_rigid_out o{voxels[k], 0, 0, aff_inf(), {-1, -1, -1}, -1, 0, 0};
        long rank = -1;
        for (long c = 0; c < chunks; ++c) {
            const double v = pw_bits2d(P[c * stride + 2 * L]);
            if (v < o.u_min) {
                o.u_min = v;
                rank = (long)P[c * stride + 2 * L + 1];
                o.min_dir = (int)P[c * stride + 2 * L + 2];
            }
            o.n_blocked_poses += (long)P[c * stride + 2 * L + 3];
            o.n_dead += (long)P[c * stride + 2 * L + 4];
            o.flags |= (int)P[c * stride + 2 * L + 5];
        }
        if (rank >= 0) {
            int i, row;
            voxel_of(k, rank, i, row);
            o.min_voxel[0] = i;
            o.min_voxel[1] = row % J.ny;
            o.min_voxel[2] = row / J.ny;
        }
        out[(long)J.out] = o;
    });
    return PW_OK;
}

extern "C" int pw_hostpath_rigid(const pw_rigid_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                 const double* coef, const double* offsets, const double* dirs,
                                 const unsigned long long* words, const double* betas, double* maps,
                                 pw_affinity_level* levels, pw_rigid_out* out, int threads) {
    return rigid_on_host(jobs, n_jobs, voxels, xyz, coef, words, betas, maps, levels, out, threads,
                         [&](const pw_rigid_job& J, int o, int s, double x, double y, double z, double& px, double& py, double& pz) {
                             const double t = offsets[(long)J.site_first + s];
                             const double* d = dirs + 3 * ((long)J.dir_first + o);
                             px = rigid_site(x, t, d[0]);
                             py = rigid_site(y, t, d[1]);
                             pz = rigid_site(z, t, d[2]);
                         });
}

extern "C" int pw_hostpath_rigid_body(const pw_rigid_body_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                      const double* coef, const double* poses, const unsigned long long* words,
                                      const double* betas, double* maps, pw_affinity_level* levels, pw_rigid_out* out,
                                      int threads) {
    return rigid_on_host(jobs, n_jobs, voxels, xyz, coef, words, betas, maps, levels, out, threads,
                         [&](const pw_rigid_body_job& J, int o, int s, double x, double y, double z, double& px, double& py, double& pz) {
                             const double* p = poses + 3 * ((long)J.pose_first + (long)o * (long)J.n_sites + s);
                             px = rigid_body_site(x, p[0]);
                             py = rigid_body_site(y, p[1]);
                             pz = rigid_body_site(z, p[2]);
                         });
}

// pw_rigid_cell on the host (pw_rigid_cell.hip checks the arguments and sends device == -1 contexts here): the pose, the
// weight and the fold of pw_rigid.hpp on the grid of pw_channels.hpp, with the near list of pw_rigid_cell.hpp -- the same
// test against the same group centre, so n_pairs is the device's unless `skip` is 0.  The threads share out (job, group)
// pieces, each of which leaves the records of its voxels; then (job, chunk) pieces leave the partials of pw_rigid.hpp;
// then one ordered reduce a job.  n_pairs (may be null): per job, diagnostic.  With `ew` (pw_rigid_cell_ewald; null for
// pw_rigid_cell) the rows of coef are (A, B, C) and a charged job takes pw_ewald.hpp's pair term and reciprocal sum.
extern "C" int pw_hostpath_rigid_cell(const pw_rigid_cell_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                      const double* offsets, const double* dirs, const double* betas, double* maps,
                                      pw_affinity_level* levels, pw_rigid_out* out, long long* n_pairs, int skip, int threads,
                                      const EwaldHost* ew) {
    typedef cavity_word u64;
    struct Plan { long group_first, chunk_first, rec_first, part_first; };
    // pw_rigid_cell_ewald (pw_ewald.hpp): rows of three and, per charged job with rows of the reciprocal sum, the tables
    // (c0, s0) a row and (P, Q) per (orientation, row), made before the groups that read them
    const int W = ew ? 3 : 2;
    struct Rec { long first, krow_first; };
    std::vector<Rec> recp((size_t)n_jobs + 1);
    long table_words = 0, krows = 0;
    for (long k = 0; k < n_jobs; ++k) {
        recp[k] = Rec{table_words, krows};
        if (ew && ew->jobs[k].charged && ew->jobs[k].n_k > 0) {
            table_words += ewald_table_words(ew->jobs[k].n_k, (long)jobs[k].n_dirs);
            krows += ew->jobs[k].n_k;
        }
    }
    recp[n_jobs] = Rec{table_words, krows};
    std::vector<double> tables((size_t)table_words);
    host_share(krows, threads, [&](long piece) {
        long k = 0, hi = n_jobs;                                     // the last job with krow_first <= piece
        while (hi - k > 1) {
            const long mid = (k + hi) / 2;
            if (recp[mid].krow_first <= piece) k = mid; else hi = mid;
        }
        const pw_rigid_cell_job& J = jobs[k];
        const EwaldHostJob& E = ew->jobs[k];
        const long row = piece - recp[k].krow_first, K = E.n_k, M = (long)J.n_dirs;
        const double* kv = ew->kvecs + 4 * (E.k_first + row);
        const EwaldK kk = ewald_kvec(J.step, J.nx, J.ny, J.nz, kv[0], kv[1], kv[2]);
        double slot_c[AFF_CHUNK], slot_s[AFF_CHUNK];
        for (int t = 0; t < AFF_CHUNK; ++t) {
            double sc = 0.0, ss = 0.0;
            for (long j = t; j < E.n_cell; j += AFF_CHUNK) {
                const double* a = ew->cell + 4 * (E.cell_first + j);
                const EwaldCS f = ewald_sincos(ewald_dot(kk, a[0], a[1], a[2]));
                sc = sc + a[3] * f.c;
                ss = ss + a[3] * f.s;
            }
            slot_c[t] = sc;
            slot_s[t] = ss;
        }
        const double Sc = aff_tree(slot_c), Ss = aff_tree(slot_s);
        double* T = tables.data() + recp[k].first;
        const EwaldCS e0 = ewald_sincos(ewald_dot(kk, J.origin[0], J.origin[1], J.origin[2]));
        T[2 * row] = e0.c;
        T[2 * row + 1] = e0.s;
        const double* dd = dirs + 3 * (long)J.dir_first;
        for (long o = 0; o < M; ++o)
            ewald_pq(kk, kv[3], Sc, Ss, offsets + (long)J.site_first, ew->site_q + E.charge_first, (int)J.n_sites, dd[3 * o],
                     dd[3 * o + 1], dd[3 * o + 2], T + 2 * K + 2 * (o * K + row), T + 2 * K + 2 * (o * K + row) + 1);
    });
    std::vector<Plan> plan((size_t)n_jobs + 1);
    std::vector<double> reach2((size_t)n_jobs);
    long n_groups = 0, n_chunks = 0, rec_words = 0, part_words = 0;
    for (long k = 0; k < n_jobs; ++k) {
        const pw_rigid_cell_job& J = jobs[k];
        plan[k] = Plan{n_groups, n_chunks, rec_words, part_words};
        const long V = (long)J.nx * J.ny * J.nz, chunks = (V + AFF_CHUNK - 1) / AFF_CHUNK;
        n_groups += rcell_groups(J.nx) * rcell_groups(J.ny) * rcell_groups(J.nz);
        n_chunks += chunks;
        rec_words += rcell_record_words(V, (int)J.n_betas);
        part_words += chunks * rigid_part_words((int)J.n_betas);
        reach2[k] = rcell_reach2(J.origin, J.step, J.cutoff2, offsets + (long)J.site_first, (int)J.n_sites,
                                 dirs + 3 * (long)J.dir_first, (int)J.n_dirs, skip != 0);
    }
    plan[n_jobs] = Plan{n_groups, n_chunks, rec_words, part_words};
    std::vector<u64> rec((size_t)rec_words), part((size_t)part_words);
    std::vector<std::atomic<long long>> pairs((size_t)n_jobs);
    for (auto& p : pairs) p.store(0, std::memory_order_relaxed);
    host_share(n_groups, threads, [&](long piece) {
        long k = 0, hi = n_jobs;                                     // the last job with group_first <= piece
        while (hi - k > 1) {
            const long mid = (k + hi) / 2;
            if (plan[mid].group_first <= piece) k = mid; else hi = mid;
        }
        const pw_rigid_cell_job& J = jobs[k];
        const int L = (int)J.n_betas, S = (int)J.n_sites, M = (int)J.n_dirs, nx = J.nx, ny = J.ny, nz = J.nz;
        const long n = (long)J.n, V = (long)nx * ny * nz, g = piece - plan[k].group_first;
        const long gx = rcell_groups(nx), gy = rcell_groups(ny), grow = g / gx;
        const int i0 = RCELL_G * (int)(g - grow * gx), j0 = RCELL_G * (int)(grow % gy), l0 = RCELL_G * (int)(grow / gy);
        const double* atoms = xyz + 3 * (long)J.atom_first;
        const double* ab = coef + W * (long)J.coef_first;
        const double* ts = offsets + (long)J.site_first;
        const double* dd = dirs + 3 * (long)J.dir_first;
        const double inv_M = rigid_inv(M);
        const bool charged = ew && ew->jobs[k].charged;
        const double alpha = charged ? ew->jobs[k].alpha : 0.0;
        const long K = charged ? ew->jobs[k].n_k : 0;
        const double* kv = K ? ew->kvecs + 4 * ew->jobs[k].k_first : nullptr;
        const double* T = K ? tables.data() + recp[k].first : nullptr;
        std::vector<EwaldCS> wave((size_t)K), axis_x((size_t)(K ? nx : 0)), axis_y((size_t)(K ? ny : 0)), axis_z((size_t)(K ? nz : 0));
        for (int q = 0; K && q < nx; ++q) axis_x[q] = ewald_axis(nx, q);
        for (int q = 0; K && q < ny; ++q) axis_y[q] = ewald_axis(ny, q);
        for (int q = 0; K && q < nz; ++q) axis_z[q] = ewald_axis(nz, q);
        const double gcx = rcell_centre_x(J.origin, J.step, i0, j0, l0), gcy = rcell_centre_y(J.origin, J.step, j0, l0),
                     gcz = rcell_centre_z(J.origin, J.step, l0);
        std::vector<long> near_list;
        for (long a = 0; a < n; ++a)
            if (!rcell_far(gcx, gcy, gcz, atoms[3 * a], atoms[3 * a + 1], atoms[3 * a + 2], reach2[k])) near_list.push_back(a);
        u64* R = rec.data() + plan[k].rec_first;
        long n_valid = 0;
        for (int l = l0; l < l0 + RCELL_G && l < nz; ++l)
            for (int j = j0; j < j0 + RCELL_G && j < ny; ++j)
                for (int i = i0; i < i0 + RCELL_G && i < nx; ++i) {
                    ++n_valid;
                    const long rank = ((long)l * ny + j) * nx + i;
                    const double x = channels_x(J.origin[0], i, J.step[0], j, J.step[1], l, J.step[3]),
                                 y = channels_y(J.origin[1], j, J.step[2], l, J.step[4]), z = channels_z(J.origin[2], l, J.step[5]);
                    RigidFold fold[AFF_MAX_LEVELS];
                    double umin_v = aff_inf();
                    int umin_o = -1, n_blocked = 0;
                    bool clamped = false;
                    for (long r = 0; r < K; ++r) {                   // (c_kv, s_kv) of the voxel, row by row
                        const EwaldCS e0{T[2 * r], T[2 * r + 1]};
                        wave[r] = ewald_add(ewald_add(ewald_add(e0, axis_x[ewald_residue((int)kv[4 * r], i, nx)]),
                                                      axis_y[ewald_residue((int)kv[4 * r + 1], j, ny)]),
                                            axis_z[ewald_residue((int)kv[4 * r + 2], l, nz)]);
                    }
                    for (int o = 0; o < M; ++o) {
                        bool blocked = false;
                        double U = 0.0;
                        for (int s = 0; s < S && !blocked; ++s) {
                            const double px = rigid_site(x, ts[s], dd[3 * o]), py = rigid_site(y, ts[s], dd[3 * o + 1]),
                                         pz = rigid_site(z, ts[s], dd[3 * o + 2]);
                            const double* rows = ab + W * (long)s * n;
                            double Us = 0.0;
                            for (size_t q = 0; q < near_list.size() && !blocked; ++q) {
                                const long a = near_list[q];
                                const double r2 = aff_r2(px - atoms[3 * a], py - atoms[3 * a + 1], pz - atoms[3 * a + 2]);
                                blocked = aff_blocked(r2, J.core2);
                                if (blocked || !aff_counts(r2, J.cutoff2)) continue;
                                const double u = aff_pair(r2, rows[W * a], rows[W * a + 1]);
                                Us = Us + (charged ? ewald_pair(u, r2, rows[W * a + 2], alpha, POW_EXP_TAB) : u);
                            }
                            U = s ? U + Us : Us;
                        }
                        if (blocked) {
                            ++n_blocked;
                            continue;
                        }
                        if (K) {
                            const double* PQ = T + 2 * K + 2 * (long)o * K;
                            double urec = 0.0;
                            for (long r = 0; r < K; ++r) urec = urec + ewald_term(PQ[2 * r], PQ[2 * r + 1], wave[r]);
                            U = U + urec;
                        }
                        if (U < umin_v) {
                            umin_v = U;
                            umin_o = o;
                        }
                        for (int b = 0; b < L; ++b) fold[b].add(aff_weight(betas[(long)J.beta_first + b], U, POW_EXP_TAB, clamped), U);
                    }
                    for (int b = 0; b < L; ++b) {
                        R[(long)b * V + rank] = pw_d2bits(fold[b].zbar(inv_M));
                        R[(long)(L + 1 + b) * V + rank] = pw_d2bits(fold[b].ebar(inv_M));
                    }
                    R[(long)L * V + rank] = pw_d2bits(umin_v);
                    R[(long)(2 * L + 1) * V + rank] = rcell_info(n_blocked, clamped, umin_o);
                }
        pairs[(size_t)k].fetch_add((long long)near_list.size() * M * S * n_valid, std::memory_order_relaxed);
    });
    host_share(n_chunks, threads, [&](long piece) {
        long k = 0, hi = n_jobs;                                     // the last job with chunk_first <= piece
        while (hi - k > 1) {
            const long mid = (k + hi) / 2;
            if (plan[mid].chunk_first <= piece) k = mid; else hi = mid;
        }
        const pw_rigid_cell_job& J = jobs[k];
        const int L = (int)J.n_betas, stride = rigid_part_words(L);
        const long V = (long)J.nx * J.ny * J.nz, chunk = piece - plan[k].chunk_first;
        const u64* R = rec.data() + plan[k].rec_first;
        u64* P = part.data() + plan[k].part_first + chunk * stride;
        double slot_z[AFF_CHUNK], slot_e[AFF_CHUNK];
        for (int b = 0; b < L; ++b) {
            for (int t = 0; t < AFF_CHUNK; ++t) {
                const long rank = chunk * AFF_CHUNK + t;
                slot_z[t] = rank < V ? pw_bits2d(R[(long)b * V + rank]) : 0.0;
                slot_e[t] = rank < V ? pw_bits2d(R[(long)(L + 1 + b) * V + rank]) : 0.0;
            }
            P[2 * b] = pw_d2bits(aff_tree(slot_z));
            P[2 * b + 1] = pw_d2bits(aff_tree(slot_e));
        }
        double m = aff_inf();
        long m_rank = chunk * AFF_CHUNK, m_dir = -1, n_blocked = 0, n_dead = 0;
        bool clamped = false;
        for (int t = 0; t < AFF_CHUNK; ++t) {
            const long rank = chunk * AFF_CHUNK + t;
            if (rank >= V) break;
            const u64 info = R[(long)(2 * L + 1) * V + rank];
            const double v = pw_bits2d(R[(long)L * V + rank]);
            n_blocked += rcell_info_blocked(info);
            n_dead += rcell_info_dir(info) < 0;
            clamped = clamped || rcell_info_clamped(info);
            if (v < m) {
                m = v;
                m_rank = rank;
                m_dir = rcell_info_dir(info);
            }
        }
        P[2 * L] = pw_d2bits(m);
        P[2 * L + 1] = (u64)m_rank;
        P[2 * L + 2] = (u64)m_dir;
        P[2 * L + 3] = (u64)n_blocked;
        P[2 * L + 4] = (u64)n_dead;
        P[2 * L + 5] = clamped ? (u64)AFF_CLAMPED : 0ull;
    });
    host_share(n_jobs, threads, [&](long k) {
        const pw_rigid_cell_job& J = jobs[k];
        const int L = (int)J.n_betas, stride = rigid_part_words(L);
        const long V = (long)J.nx * J.ny * J.nz, chunks = plan[k + 1].chunk_first - plan[k].chunk_first;
        const u64* P = part.data() + plan[k].part_first;
        for (int b = 0; b < L; ++b) {
            double sz = 0.0, se = 0.0;
            for (long c = 0; c < chunks; ++c) {
                sz = sz + pw_bits2d(P[c * stride + 2 * b]);
                se = se + pw_bits2d(P[c * stride + 2 * b + 1]);
            }
            levels[(long)J.level_first + b] = pw_affinity_level{sz, se};
        }
        pw_rigid_out o{V, 0, 0, aff_inf(), {-1, -1, -1}, -1, 0, 0};
        long rank = -1;
        for (long c = 0; c < chunks; ++c) {
            const double v = pw_bits2d(P[c * stride + 2 * L]);
            if (v < o.u_min) {
                o.u_min = v;
                rank = (long)P[c * stride + 2 * L + 1];
                o.min_dir = (int)P[c * stride + 2 * L + 2];
            }
            o.n_blocked_poses += (long)P[c * stride + 2 * L + 3];
            o.n_dead += (long)P[c * stride + 2 * L + 4];
            o.flags |= (int)P[c * stride + 2 * L + 5];
        }
        if (rank >= 0) {
            const long row = rank / J.nx;
            o.min_voxel[0] = (int)(rank - row * J.nx);
            o.min_voxel[1] = (int)(row % J.ny);
            o.min_voxel[2] = (int)(row / J.ny);
        }
        out[(long)J.out] = o;
        if (J.map_first >= 0) memcpy(maps + (long)J.map_first, rec.data() + plan[k].rec_first, sizeof(double) * (size_t)((L + 1) * V));
        if (n_pairs) n_pairs[k] = pairs[(size_t)k].load(std::memory_order_relaxed);
    });
    return PW_OK;
}

// The Lennard-Jones energy maps of pw_passage, pw_hop and pw_percolation on the host: one pair loop, the two kinds of
// voxel centres, and the batches the maps are computed in.
namespace {
constexpr long FIELD_HOST_SLAB = 4096;                               // voxels of a map in one piece of work

// the energy of a guest at (x, y, z) among the job's atoms: pw_affinity.hpp's pair terms in atom order (pw_field_dev.hpp's
// and pw_field_cell_dev.hpp's order); the atoms after one that blocks the point add nothing to +inf
template <class Job>
inline double field_value_at(const Job& J, const double* atoms, const double* ab, double x, double y, double z) {
    double u_sum = 0.0;
    bool blocked = false;
    for (long a = 0; a < (long)J.n && !blocked; ++a) {
        const double r2 = aff_r2(x - atoms[3 * a], y - atoms[3 * a + 1], z - atoms[3 * a + 2]);
        blocked = aff_blocked(r2, J.core2);
        if (!blocked && aff_counts(r2, J.cutoff2)) u_sum = u_sum + aff_pair(r2, ab[2 * a], ab[2 * a + 1]);
    }
    return blocked ? aff_inf() : u_sum;
}

// ... at the voxel `rank` of the grid around a molecule (pw_passage_job, pw_hop_job): pw_cavity.hpp's centres.  (This and
// the next are objects without state, not functions, so that host_field_batches is compiled with the loop inside it.)
struct GridFieldValue {
    template <class Job>
    double operator()(const Job& J, const double* atoms, const double* ab, long rank) const {
        const int row = (int)(rank / J.nx), i = (int)(rank - (long)row * J.nx);
        return field_value_at(J, atoms, ab, cavity_coord(J.origin[0], i, J.spacing), cavity_coord(J.origin[1], row % J.ny, J.spacing),
                              cavity_coord(J.origin[2], row / J.ny, J.spacing));
    }
};

// ... at the voxel `rank` of the grid of a periodic cell (pw_percolation_job, pw_basins_job): pw_channels.hpp's centres
struct CellFieldValue {
    template <class Job>
    double operator()(const Job& J, const double* atoms, const double* ab, long rank) const {
        const int row = (int)(rank / J.nx), i = (int)(rank - (long)row * J.nx), j = row % J.ny, l = row / J.ny;
        return field_value_at(J, atoms, ab, channels_x(J.origin[0], i, J.step[0], j, J.step[1], l, J.step[3]),
                              channels_y(J.origin[1], j, J.step[2], l, J.step[4]), channels_z(J.origin[2], l, J.step[5]));
    }
};

// Jobs go in order in batches [first, last): a batch takes jobs while the maps of those without a field of their own
// (field_first == -1) fit workspace_bytes, and a job that alone does not fit is a batch.  The threads share out slabs of
// FIELD_HOST_SLAB voxels of the batch's maps, value(J, atoms, ab, rank) a voxel; then phase(first, last, field_of) does
// the entry's own work on the batch, field_of(k) being job k's map or the caller's field, which is read in place.
template <class Job, class Value, class Phase>
void host_field_batches(const Job* jobs, long n_jobs, const double* xyz, const double* coef, const double* field,
                        long workspace_bytes, int threads, Value value, Phase phase) {
    struct Slab { long job, a, b; };
    std::vector<double> maps;
    std::vector<long> map_first((size_t)n_jobs);
    for (long first = 0; first < n_jobs;) {
        long last = first, words = 0;
        std::vector<Slab> slabs;
        for (; last < n_jobs; ++last) {
            const Job& J = jobs[last];
            const long V = (long)J.nx * J.ny * J.nz;
            if (last > first && J.field_first == -1 && words + V > workspace_bytes / 8) break;
            map_first[last] = words;
            if (J.field_first != -1) continue;
            words += V;
            for (long a = 0; a < V; a += FIELD_HOST_SLAB) slabs.push_back({last, a, std::min(a + FIELD_HOST_SLAB, V)});
        }
        maps.resize((size_t)words);
        host_share((long)slabs.size(), threads, [&](long s) {
            const Slab& piece = slabs[s];
            const Job& J = jobs[piece.job];
            const double* atoms = xyz + 3 * (long)J.atom_first;
            const double* ab = coef + 2 * (long)J.coef_first;
            double* U = maps.data() + map_first[piece.job];
            for (long rank = piece.a; rank < piece.b; ++rank) U[rank] = value(J, atoms, ab, rank);
        });
        phase(first, last, [&](long k) -> const double* {
            return jobs[k].field_first == -1 ? maps.data() + map_first[k] : field + (long)jobs[k].field_first;
        });
        first = last;
    }
}
}  // namespace

// pw_passage on the host (pw_passage.hip checks the arguments and sends device == -1 contexts here): the plane test and
// the fill of pw_cavity.hpp, the keys and the bisection of pw_passage.hpp, on the maps of host_field_batches within
// PAS_WORKSPACE_BYTES.  A batch's (job, row) pieces are shared out; a piece builds its held words, then runs level after
// level: the allowed words from the map, the fill, the face test.
extern "C" int pw_hostpath_passage(const pw_passage_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                   const double* planes, const double* field, pw_passage_out* out, int* fills,
                                   int threads) {
    typedef cavity_word u64;
    struct Piece { long job, row; };
    host_field_batches(jobs, n_jobs, xyz, coef, field, PAS_WORKSPACE_BYTES, threads, GridFieldValue(),
                       [&](long first, long last, auto field_of) {
        std::vector<Piece> pieces;
        for (long job = first; job < last; ++job)
            for (long k = 0; k < pas_rows_out((long)jobs[job].m); ++k) pieces.push_back({job, k});
        host_share((long)pieces.size(), threads, [&](long p) {
            const pw_passage_job& J = jobs[pieces[p].job];
            const long k = pieces[p].row;
            const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz;
            const double* U = field_of(pieces[p].job);
            const double* cuts = planes + 4 * (long)J.plane_first;
            const CavityHostGrid G{nullptr, nullptr, nullptr, 0, 0, J.origin, J.spacing, nx, ny, nz, J.seed};
            std::vector<u64> held((size_t)rows), open((size_t)rows), fill((size_t)rows);
            for (int r = 0; r < rows; ++r) {
                const double y = cavity_coord(J.origin[1], r % ny, J.spacing), z = cavity_coord(J.origin[2], r / ny, J.spacing);
                u64 word = cavity_row_mask(nx);
                for (long q = 0; q < (long)J.m && word; ++q) {
                    if (q == k) continue;
                    for (int i = 0; i < nx; ++i)
                        if (!cavity_inside(cuts + 4 * q, cavity_coord(J.origin[0], i, J.spacing), y, z)) word &= ~(1ull << i);
                }
                held[r] = word;
            }
            const int seed_row = J.seed[2] * ny + J.seed[1];
            const long seed_rank = (long)seed_row * nx + J.seed[0];
            const u64 seed_key = pas_key(U[seed_rank]);
            pw_passage_out o{};
            o.u_seed = U[seed_rank];
            int n_fills = 0;
            // the level `mid`: open, below, above as the kernel's level pass; then the fill; true iff it is on a face
            u64 below = 0, above = PAS_KEY_NONE;
            auto level = [&](u64 mid) {
                below = 0;
                above = PAS_KEY_NONE;
                for (int r = 0; r < rows; ++r) {
                    u64 word = 0;
                    for (u64 todo = held[r]; todo; todo &= todo - 1) {
                        const int i = __builtin_ctzll(todo);
                        const u64 key = pas_key(U[(long)r * nx + i]);
                        if (key <= mid) {
                            word |= 1ull << i;
                            below = std::max(below, key);
                        } else if (key < PAS_KEY_INF) {
                            above = std::min(above, key);
                        }
                    }
                    open[r] = word;
                }
                cavity_host_fill(G, open, fill);
                ++n_fills;
                long face = 0;
                for (int r = 0; r < rows; ++r) face += cavity_row_face(fill[r], nx, ny, nz, r % ny, r / ny);
                return face != 0;
            };
            auto count = [&]() {
                long n = 0;
                for (int r = 0; r < rows; ++r) n += cavity_popcount(fill[r]);
                return n;
            };
            if (!((held[seed_row] >> J.seed[0]) & 1ull) || seed_key == PAS_KEY_INF) {
                o.barrier = o.well = aff_inf();
                for (int a = 0; a < 3; ++a) o.saddle[a] = o.well_voxel[a] = -1;
                o.flags = PAS_SEED_CLOSED;
            } else {
                u64 B = PAS_KEY_NONE;
                if (!level(PAS_KEY_INF - 1)) {
                    o.flags = PAS_NO_EXIT;
                    o.n_fill = o.n_basin = count();
                } else {
                    u64 lo = seed_key, hi = below;
                    for (int step = 0; step < PAS_MAX_STEPS && lo < hi; ++step) {
                        const u64 mid = lo + ((hi - lo) >> 1);
                        if (level(mid)) {
                            hi = below;
                        } else {
                            if (above > hi) break;
                            lo = above;
                        }
                    }
                    B = hi;
                    if (seed_key < B) {
                        level(B - 1);
                        o.n_basin = count();
                    }
                    level(B);
                    o.n_fill = count();
                }
                u64 well_key = PAS_KEY_NONE;
                long well_rank = -1, saddle_rank = -1;
                for (int r = 0; r < rows; ++r)
                    for (u64 todo = fill[r]; todo; todo &= todo - 1) {
                        const long rank = (long)r * nx + __builtin_ctzll(todo);
                        const u64 key = pas_key(U[rank]);
                        if (key < well_key) {
                            well_key = key;
                            well_rank = rank;
                        }
                        if (key == B && saddle_rank < 0) saddle_rank = rank;
                    }
                o.barrier = saddle_rank >= 0 ? U[saddle_rank] : aff_inf();
                o.well = U[well_rank];
                grid_voxel(saddle_rank, nx, ny, o.saddle);
                grid_voxel(well_rank, nx, ny, o.well_voxel);
            }
            out[(long)J.out_first + k] = o;
            if (fills) fills[(long)J.out_first + k] = n_fills;
        });
    });
    return PW_OK;
}

// pw_hop on the host (pw_hop.hip checks the arguments and sends device == -1 contexts here): the plane test of
// pw_cavity.hpp, the fill, the minimum and the sums of pw_hop.hpp, on the maps of host_field_batches within
// HOP_WORKSPACE_BYTES.  A batch's (job, slab) pieces are shared out; a job's row of out is put together from its pieces'
// counts and flags afterwards.
extern "C" int pw_hostpath_hop(const pw_hop_job* jobs, long n_jobs, const double* xyz, const double* coef,
                               const double* planes, const double* field, const double* betas, pw_hop_slab* slabs,
                               pw_affinity_level* sums, pw_hop_out* out, unsigned long long* words, int threads) {
    typedef cavity_word u64;
    struct Piece { long job, slab; };
    host_field_batches(jobs, n_jobs, xyz, coef, field, HOP_WORKSPACE_BYTES, threads, GridFieldValue(),
                       [&](long first, long last, auto field_of) {
        std::vector<Piece> pieces;
        for (long job = first; job < last; ++job)
            for (long l = 0; l < jobs[job].nz; ++l) pieces.push_back({job, l});
        std::vector<int> piece_flags(pieces.size(), 0);
        host_share((long)pieces.size(), threads, [&](long p) {
            const pw_hop_job& J = jobs[pieces[p].job];
            const int l = (int)pieces[p].slab, nx = J.nx, ny = J.ny, L = (int)J.n_betas;
            const double* U = field_of(pieces[p].job) + (long)l * ny * nx;
            const double* cuts = planes + 4 * (long)J.plane_first;
            const double z = cavity_coord(J.origin[2], l, J.spacing);
            u64 open[CAVITY_MAX_G], fill[CAVITY_MAX_G];
            for (int j = 0; j < ny; ++j) {
                const double y = cavity_coord(J.origin[1], j, J.spacing);
                u64 word = 0;
                for (int i = 0; i < nx; ++i) {
                    bool ok = hop_admits(U[(long)j * nx + i], J.cap);
                    const double x = cavity_coord(J.origin[0], i, J.spacing);
                    for (long q = 0; q < (long)J.m && ok; ++q) ok = cavity_inside(cuts + 4 * q, x, y, z);
                    if (ok) word |= 1ull << i;
                }
                open[j] = word;
                fill[j] = 0;
            }
            fill[J.seed[1]] = open[J.seed[1]] & (1ull << J.seed[0]);
            const long max_sweeps = (long)nx * ny + 1;
            for (long sweep = 0; sweep < max_sweeps; ++sweep) {
                bool changed = false;
                for (int j = 0; j < ny; ++j) {                       // (in place: a row may see this sweep's neighbour)
                    const u64 from = fill[j] | (j > 0 ? fill[j - 1] : 0) | (j + 1 < ny ? fill[j + 1] : 0);
                    const u64 g = hop_fill_word(from, open[j]);
                    changed = changed || g != fill[j];
                    fill[j] = g;
                }
                if (!changed) break;
            }
            pw_hop_slab s{0, 0, aff_inf(), -1, -1};
            int best_pos = 0x7fffffff;
            for (int j = 0; j < ny; ++j) {
                s.n += cavity_popcount(fill[j]);
                s.n_face += hop_row_face(fill[j], nx, ny, j);
                if (words && J.word_first >= 0) words[(long)J.word_first + (long)l * ny + j] = fill[j];
            }
            // the voxels in rank order, 64 a chunk
            double z_total[AFF_MAX_LEVELS], e_total[AFF_MAX_LEVELS], u[AFF_CHUNK], slot_z[AFF_CHUNK], slot_e[AFF_CHUNK];
            for (int b = 0; b < L; ++b) z_total[b] = e_total[b] = 0.0;
            bool clamped = false;
            int held = 0, j = 0;
            u64 todo = ny ? fill[0] : 0;
            for (long done = 0; done < s.n;) {
                for (held = 0; held < AFF_CHUNK && done < s.n;) {
                    while (!todo) todo = fill[++j];                  // (done < n: a voxel is left in a later row)
                    const int i = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    u[held] = U[(long)j * nx + i];
                    if (hop_before(u[held], j * 64 + i, s.u_min, best_pos)) {
                        s.u_min = u[held];
                        best_pos = j * 64 + i;
                    }
                    ++held;
                    ++done;
                }
                for (int b = 0; b < L; ++b) {
                    for (int t = 0; t < AFF_CHUNK; ++t) {
                        slot_z[t] = slot_e[t] = 0.0;
                        if (t >= held) continue;
                        const double w = aff_weight(betas[(long)J.beta_first + b], u[t], POW_EXP_TAB, clamped);
                        slot_z[t] = w;
                        slot_e[t] = w * u[t];
                    }
                    z_total[b] = z_total[b] + aff_tree(slot_z);
                    e_total[b] = e_total[b] + aff_tree(slot_e);
                }
            }
            if (s.n) {
                s.min_i = best_pos & 63;
                s.min_j = best_pos >> 6;
            }
            slabs[(long)J.slab_first + l] = s;
            for (int b = 0; b < L; ++b) sums[(long)J.sum_first + (long)l * L + b] = pw_affinity_level{z_total[b], e_total[b]};
            piece_flags[(size_t)p] = clamped ? HOP_CLAMPED : 0;
        });
        for (size_t p = 0; p < pieces.size();) {                     // (a job's pieces follow one another)
            const pw_hop_job& J = jobs[pieces[p].job];
            pw_hop_out o{0, 0, 0};
            for (long l = 0; l < J.nz; ++l, ++p) {
                o.n += slabs[(long)J.slab_first + l].n;
                o.flags |= piece_flags[p];
            }
            out[(long)J.out] = o;
        }
    });
    return PW_OK;
}

// pw_charges on the host (pw_charges.hip checks the arguments and sends device == -1 contexts here): the solver of
// pw_charges.hpp step by step, the 64 accumulators of a sum as an array, term i going to accumulator i % 64, folded by
// sup_fold.  Every element of the matrix is recomputed where it is needed, so nothing but the job's ten vectors is held.
// The threads share out the jobs; a job's row and charges are its own.
extern "C" int pw_hostpath_charges(const pw_charges_job* jobs, long n_jobs, const double* xyz, const double* params,
                                   double* charges, pw_charges_out* out, int threads) {
    auto one = [&](const pw_charges_job& J) {
        const long n = (long)J.n;
        const double* X = xyz + 3 * (long)J.xyz_first;
        const double* P = params + 2 * (long)J.param_first;
        const double K = J.coulomb, Q = J.total_charge, tol2 = J.tol * J.tol;
        std::vector<double> state((size_t)(10 * n));
        double* v[2][5];                                             // x, r, z, p, Ap of the two systems
        for (int s = 0; s < 2; ++s)
            for (int f = 0; f < 5; ++f) v[s][f] = state.data() + (5 * s + f) * n;
        double lanes[SUP_ACC];
        auto dot = [&](const double* a, const double* b) {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
            for (long i = 0; i < n; ++i) lanes[i % SUP_ACC] = pw_fma(a[i], b[i], lanes[i % SUP_ACC]);
            return sup_fold(lanes);
        };
        auto sum = [&](const double* a) {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
            for (long i = 0; i < n; ++i) lanes[i % SUP_ACC] = lanes[i % SUP_ACC] + a[i];
            return sup_fold(lanes);
        };
        ChgSystem sys[2];
        for (int s = 0; s < 2; ++s) {
            double *x = v[s][0], *r = v[s][1], *z = v[s][2], *p = v[s][3];
            for (long i = 0; i < n; ++i) {
                x[i] = 0.0;
                r[i] = s == 0 ? -P[2 * i] : 1.0;
                p[i] = z[i] = r[i] / P[2 * i + 1];
            }
            sys[s].rz = dot(r, z);
            sys[s].rr = sys[s].bb = dot(r, r);
            sys[s].iterations = 0;
            sys[s].frozen = sys[s].broke = false;
        }
        bool ran_out = false;
        for (int k = 0;; ++k) {
            chg_freeze_check(sys[0], tol2, k);
            chg_freeze_check(sys[1], tol2, k);
            if (sys[0].frozen && sys[1].frozen) break;
            if (k == J.max_iter) {
                ran_out = true;
                for (int s = 0; s < 2; ++s)
                    if (!sys[s].frozen) sys[s].iterations = k;
                break;
            }
            const bool on0 = !sys[0].frozen, on1 = !sys[1].frozen;
            double acc0[SUP_ACC], acc1[SUP_ACC];
            for (long i = 0; i < n; ++i) {
                for (int l = 0; l < SUP_ACC; ++l) acc0[l] = acc1[l] = 0.0;
                const double xi = X[3 * i], yi = X[3 * i + 1], zi = X[3 * i + 2], Ji = P[2 * i + 1];
                for (long j = 0; j < n; ++j) {
                    const double a = j == i ? Ji : chg_pair(xi, yi, zi, Ji, X[3 * j], X[3 * j + 1], X[3 * j + 2], P[2 * j + 1], K);
                    if (on0) acc0[j % SUP_ACC] = pw_fma(a, v[0][3][j], acc0[j % SUP_ACC]);
                    if (on1) acc1[j % SUP_ACC] = pw_fma(a, v[1][3][j], acc1[j % SUP_ACC]);
                }
                if (on0) v[0][4][i] = sup_fold(acc0);
                if (on1) v[1][4][i] = sup_fold(acc1);
            }
            for (int s = 0; s < 2; ++s) {
                ChgSystem& S = sys[s];
                if (S.frozen) continue;
                double *x = v[s][0], *r = v[s][1], *z = v[s][2], *p = v[s][3], *Ap = v[s][4];
                const double pAp = dot(p, Ap);
                if (!chg_curvature_ok(S, pAp, k)) continue;
                const double alpha = S.rz / pAp;
                for (long i = 0; i < n; ++i) {
                    x[i] = pw_fma(alpha, p[i], x[i]);
                    r[i] = pw_fma(-alpha, Ap[i], r[i]);
                    z[i] = r[i] / P[2 * i + 1];
                }
                const double rz_new = dot(r, z);
                S.rr = dot(r, r);
                const double beta = rz_new / S.rz;
                for (long i = 0; i < n; ++i) p[i] = pw_fma(beta, p[i], z[i]);
                S.rz = rz_new;
            }
        }
        const double *s_vec = v[0][0], *t_vec = v[1][0];
        const double S = sum(s_vec), T = sum(t_vec);
        const int flags = chg_flags(sys[0], sys[1], ran_out, T);
        const bool lost = (flags & (CHG_BREAKDOWN | CHG_NO_SUM)) != 0;
        const double mu = (Q - S) / T;
        double* q = charges + (long)J.charge_first;
        double e[SUP_ACC], d[3][SUP_ACC], lo[SUP_ACC], hi[SUP_ACC];
        for (int l = 0; l < SUP_ACC; ++l) {
            e[l] = d[0][l] = d[1][l] = d[2][l] = 0.0;
            lo[l] = PW_INF;
            hi[l] = -PW_INF;
        }
        for (long i = 0; i < n; ++i) {
            const int l = (int)(i % SUP_ACC);
            const double qi = pw_fma(mu, t_vec[i], s_vec[i]);
            e[l] = pw_fma(P[2 * i], qi, e[l]);
            for (int a = 0; a < 3; ++a) d[a][l] = pw_fma(qi, X[3 * i + a], d[a][l]);
            lo[l] = qi < lo[l] ? qi : lo[l];
            hi[l] = qi > hi[l] ? qi : hi[l];
            q[i] = lost ? chg_nan() : chg_canon(qi);
        }
        for (int s = SUP_ACC / 2; s >= 1; s >>= 1)
            for (int l = 0; l < s; ++l) {
                lo[l] = lo[l + s] < lo[l] ? lo[l + s] : lo[l];
                hi[l] = hi[l + s] > hi[l] ? hi[l + s] : hi[l];
            }
        pw_charges_out* o = out + (long)J.out;
        const double nan = chg_nan();
        o->mu = lost ? nan : chg_canon(mu);
        o->sum_s = chg_canon(S);
        o->sum_t = chg_canon(T);
        o->energy = lost ? nan : chg_canon(0.5 * (sup_fold(e) + mu * Q));
        for (int a = 0; a < 3; ++a) o->dipole[a] = lost ? nan : chg_canon(sup_fold(d[a]));
        o->q_min = lost ? nan : chg_canon(lo[0]);
        o->q_max = lost ? nan : chg_canon(hi[0]);
        o->iterations[0] = sys[0].iterations;
        o->iterations[1] = sys[1].iterations;
        o->flags = flags;
        o->reserved = 0;
    };
    host_share(n_jobs, threads, [&](long k) { one(jobs[k]); });
    return PW_OK;
}

// pw_charges_cell on the host (pw_charges_cell.hip checks the arguments and sends device == -1 contexts here): the
// definition of pw_charges_cell.hpp step by step.  A job's rows of R are built once as lists, its phases once as (n_k, n)
// arrays -- the definition lets either be kept or recomputed --, and the sums are pw_hostpath_charges'.  The threads share
// out the jobs.
extern "C" int pw_hostpath_charges_cell(const pw_charges_cell_job* jobs, long n_jobs, const double* xyz, const double* params,
                                        const double* kvecs, double* charges, pw_charges_cell_out* out, int threads) {
    auto one = [&](const pw_charges_cell_job& J) {
        const long n = (long)J.n, nk = (long)J.n_k;
        const double* X = xyz + 3 * (long)J.xyz_first;
        const double* P = params + 2 * (long)J.param_first;
        const double* KV = kvecs + 4 * (long)J.k_first;
        const double K = J.coulomb, alpha = J.alpha, tol2 = J.tol * J.tol;
        // R: the lists
        double shift[CHC_IMAGES][3];
        for (int m = 0; m < CHC_IMAGES; ++m) chc_shift(J.edges, m, &shift[m][0], &shift[m][1], &shift[m][2]);
        std::vector<long> first((size_t)n + 1, 0);
        std::vector<double> value;
        std::vector<int> column;
        for (long i = 0; i < n; ++i) {
            const double xi = X[3 * i], yi = X[3 * i + 1], zi = X[3 * i + 2], Ji = P[2 * i + 1];
            for (long j = 0; j < n; ++j)
                for (int m = 0; m < CHC_IMAGES; ++m) {
                    if (j == i && m == CHC_SELF_IMAGE) continue;
                    const double r2 = chc_r2(xi, yi, zi, X[3 * j], X[3 * j + 1], X[3 * j + 2], shift[m][0], shift[m][1], shift[m][2]);
                    if (!(r2 <= J.cutoff2)) continue;
                    value.push_back(chc_term(r2, Ji, P[2 * j + 1], K, alpha, J.shield_on2, J.shield_off2));
                    column.push_back((int)j);
                }
            first[(size_t)i + 1] = (long)value.size();
        }
        // G: the tables and the phases
        ChcTables T;
        T.top[0] = T.top[1] = T.top[2] = 0;
        for (long k = 0; k < nk; ++k)
            for (int a = 0; a < 3; ++a) {
                const int v = (int)KV[4 * k + a];
                T.top[a] = std::max(T.top[a], v < 0 ? -v : v);
            }
        chc_tables_layout(T, n);
        std::vector<double> tab((size_t)chc_table_words(T.top, n));
        for (int a = 0; a < 3; ++a)
            for (int m = 0; m <= T.top[a]; ++m) {
                const EwaldK kv = chc_axis_kvec(J.edges, a, m);
                for (long j = 0; j < n; ++j) {
                    const EwaldCS e = ewald_sincos(ewald_dot(kv, X[3 * j], X[3 * j + 1], X[3 * j + 2]));
                    tab[(size_t)(T.first[a] + 2l * m * n + j)] = e.c;
                    tab[(size_t)(T.first[a] + 2l * m * n + n + j)] = e.s;
                }
            }
        std::vector<double> pc((size_t)(nk * n)), ps((size_t)(nk * n)), Sc((size_t)nk), Ss((size_t)nk);
        for (long k = 0; k < nk; ++k)
            for (long j = 0; j < n; ++j) {
                const EwaldCS ph = chc_phase(tab.data(), T, n, j, (int)KV[4 * k], (int)KV[4 * k + 1], (int)KV[4 * k + 2]);
                pc[(size_t)(k * n + j)] = ph.c;
                ps[(size_t)(k * n + j)] = ph.s;
            }
        std::vector<double> state((size_t)(5 * n));
        double *q = state.data(), *r = q + n, *z = r + n, *p = z + n, *y = p + n;
        double lanes[SUP_ACC], lanes2[SUP_ACC];
        auto dot = [&](const double* a, const double* b, long count) {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
            for (long i = 0; i < count; ++i) lanes[i % SUP_ACC] = pw_fma(a[i], b[i], lanes[i % SUP_ACC]);
            return sup_fold(lanes);
        };
        for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
        for (long i = 0; i < n; ++i) lanes[i % SUP_ACC] = lanes[i % SUP_ACC] + 1.0 / P[2 * i + 1];
        const double sJ = sup_fold(lanes);
        // z and lambda from r
        auto precondition = [&]() {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
            for (long i = 0; i < n; ++i) {
                z[i] = r[i] / P[2 * i + 1];
                lanes[i % SUP_ACC] = lanes[i % SUP_ACC] + z[i];
            }
            const double lambda = sup_fold(lanes) / sJ;
            for (long i = 0; i < n; ++i) z[i] = z[i] - lambda / P[2 * i + 1];
            return lambda;
        };
        ChcState S;
        for (long i = 0; i < n; ++i) {
            q[i] = 0.0;
            r[i] = -P[2 * i];
        }
        S.lambda = precondition();
        for (long i = 0; i < n; ++i) p[i] = z[i];
        // r.z with the residual's constant part taken out (pw_charges_cell.hpp, SOLVER)
        auto projected_dot = [&](double lambda) {
            for (int l = 0; l < SUP_ACC; ++l) lanes[l] = 0.0;
            for (long i = 0; i < n; ++i) lanes[i % SUP_ACC] = pw_fma(r[i] - lambda, z[i], lanes[i % SUP_ACC]);
            return sup_fold(lanes);
        };
        S.rz = S.rz0 = projected_dot(S.lambda);
        S.iterations = 0;
        S.ran_out = S.broke = false;
        const double self = chc_self(K, alpha);
        for (int k = 0;; ++k) {
            S.iterations = k;
            if (S.rz <= tol2 * S.rz0) break;
            if (k == J.max_iter) {
                S.ran_out = true;
                break;
            }
            for (long kr = 0; kr < nk; ++kr) {
                for (int l = 0; l < SUP_ACC; ++l) lanes[l] = lanes2[l] = 0.0;
                const double *c = pc.data() + kr * n, *s = ps.data() + kr * n;
                for (long j = 0; j < n; ++j) {
                    lanes[j % SUP_ACC] = pw_fma(p[j], c[j], lanes[j % SUP_ACC]);
                    lanes2[j % SUP_ACC] = pw_fma(p[j], s[j], lanes2[j % SUP_ACC]);
                }
                Sc[(size_t)kr] = sup_fold(lanes);
                Ss[(size_t)kr] = sup_fold(lanes2);
            }
            for (long i = 0; i < n; ++i) {
                for (int l = 0; l < SUP_ACC; ++l) lanes[l] = lanes2[l] = 0.0;
                for (long e = first[(size_t)i], t = 0; e < first[(size_t)i + 1]; ++e, ++t)
                    lanes[t % SUP_ACC] = pw_fma(value[(size_t)e], p[column[(size_t)e]], lanes[t % SUP_ACC]);
                const double real = sup_fold(lanes);
                for (long kr = 0; kr < nk; ++kr) {
                    EwaldCS ph;
                    ph.c = pc[(size_t)(kr * n + i)];
                    ph.s = ps[(size_t)(kr * n + i)];
                    lanes2[kr % SUP_ACC] = pw_fma(KV[4 * kr + 3], chc_rec_term(ph, Sc[(size_t)kr], Ss[(size_t)kr]), lanes2[kr % SUP_ACC]);
                }
                const double rec = sup_fold(lanes2);
                y[i] = ((P[2 * i + 1] - self) * p[i] + real) + rec;
            }
            const double pAp = dot(p, y, n);
            if (!(pAp > 0.0)) {
                S.broke = true;
                break;
            }
            const double al = S.rz / pAp;
            for (long i = 0; i < n; ++i) {
                q[i] = pw_fma(al, p[i], q[i]);
                r[i] = pw_fma(-al, y[i], r[i]);
            }
            S.lambda = precondition();
            const double rz_new = projected_dot(S.lambda);
            const double beta = rz_new / S.rz;
            for (long i = 0; i < n; ++i) p[i] = pw_fma(beta, p[i], z[i]);
            S.rz = rz_new;
        }
        const int flags = chc_flags(S, sJ);
        const bool lost = (flags & (CHG_BREAKDOWN | CHG_NO_SUM)) != 0;
        const double nan = chg_nan();
        double e[SUP_ACC], lo[SUP_ACC], hi[SUP_ACC];
        for (int l = 0; l < SUP_ACC; ++l) {
            e[l] = 0.0;
            lo[l] = PW_INF;
            hi[l] = -PW_INF;
        }
        double* Q = charges + (long)J.charge_first;
        for (long i = 0; i < n; ++i) {
            const int l = (int)(i % SUP_ACC);
            e[l] = pw_fma(P[2 * i], q[i], e[l]);
            lo[l] = q[i] < lo[l] ? q[i] : lo[l];
            hi[l] = q[i] > hi[l] ? q[i] : hi[l];
            Q[i] = lost ? nan : chg_canon(q[i]);
        }
        for (int s = SUP_ACC / 2; s >= 1; s >>= 1)
            for (int l = 0; l < s; ++l) {
                lo[l] = lo[l + s] < lo[l] ? lo[l + s] : lo[l];
                hi[l] = hi[l + s] > hi[l] ? hi[l + s] : hi[l];
            }
        pw_charges_cell_out* o = out + (long)J.out;
        o->mu = lost ? nan : chg_canon(-S.lambda);
        o->energy = lost ? nan : chg_canon(0.5 * sup_fold(e));
        o->q_min = lost ? nan : chg_canon(lo[0]);
        o->q_max = lost ? nan : chg_canon(hi[0]);
        o->iterations = S.iterations;
        o->flags = flags;
    };
    host_share(n_jobs, threads, [&](long k) { one(jobs[k]); });
    return PW_OK;
}

// The component of a seed voxel in the open words of a periodic grid and how it winds (pw_channels.hpp), for
// pw_hostpath_channels and pw_hostpath_percolation: chan_walk of pw_channels_dev.hpp as a plain loop.
namespace {
// From the bit seed_bit of row seed_row, which is open: up to seven fills for the phi that channels_next asks for, phi = 7
// first, channels_learn after each; the first fill also gives the voxels and the three crossing counts of the component
// (channels_row_cross) and `cross`.  A fill is sweeps forwards and backwards over the rows until one changes nothing, at
// most 2 * nx * ny * nz + 1 of them.  On return p0 | p1 is the component.
// A row is skipped when the words gathered for it miss its open word.  That changes nothing: the row's own p0, p1 are
// among the gathered words and lie inside its open word (the seed is open, every other store is a result of
// channels_fill_words), so they are zero then, and the fill of nothing gives g0 = g1 = 0 as well.  chan_fill on the
// device skips the same rows.
ChannelsWalk channels_host_walk(const std::vector<cavity_word>& open, std::vector<cavity_word>& p0, std::vector<cavity_word>& p1,
                                int seed_row, cavity_word seed_bit, int nx, int ny, int nz) {
    typedef cavity_word u64;
    const int rows = ny * nz;
    const long max_sweeps = 2 * (long)nx * ny * nz + 1;
    auto load = [&](int q, int row) { return q ? p1[row] : p0[row]; };
    ChannelsWalk W{0, 0, 0, {0, 0, 0}};
    int known = 0, cross = 0, phi = 7;
    for (; W.fills < 7 && phi; ++W.fills) {
        std::fill(p0.begin(), p0.end(), 0);
        std::fill(p1.begin(), p1.end(), 0);
        p0[seed_row] = seed_bit;
        auto visit = [&](int r) {
            if (!open[r]) return false;
            u64 from0 = p0[r], from1 = p1[r], g0, g1;
            channels_gather(load, r % ny, r / ny, ny, nz, phi, from0, from1);
            if (!((from0 | from1) & open[r])) return false;
            channels_fill_words(from0, from1, open[r], nx, (phi & 1) != 0, g0, g1);
            const bool changed = g0 != p0[r] || g1 != p1[r];
            p0[r] = g0;
            p1[r] = g1;
            return changed;
        };
        for (long sweep = 0; sweep < max_sweeps; ++sweep) {
            bool changed = false;
            for (int r = 0; r < rows; ++r) changed = visit(r) || changed;
            for (int r = rows - 1; r >= 0; --r) changed = visit(r) || changed;
            if (!changed) break;
        }
        const bool reached = (p1[seed_row] & seed_bit) != 0;
        channels_learn(phi, reached, known, W.wraps);
        if (W.fills == 0) {
            for (int r = 0; r < rows; ++r) {
                const u64 f = p0[r] | p1[r];
                if (!f) continue;
                const int j = r % ny, l = r / ny;
                long c[3];
                channels_row_cross(f, p0[l * ny] | p1[l * ny], p0[j] | p1[j], nx, ny, nz, j, l, c);
                W.n_voxels += cavity_popcount(f);
                for (int a = 0; a < 3; ++a) W.n_cross[a] += c[a];
            }
            for (int a = 0; a < 3; ++a) cross |= (W.n_cross[a] > 0) << a;
            if (cross) channels_learn(cross, reached, known, W.wraps);
        }
        phi = channels_next(cross, known, W.wraps);
    }
    return W;
}
}  // namespace

// pw_channels on the host (pw_channels.hip checks the arguments and sends device == -1 contexts here): the centres and
// the rank of pw_channels.hpp, the components by channels_host_walk.  The threads share out the jobs; a job is a plain
// loop: classify, then component after component from the first set bit of todo.  A job's outputs are its own.
extern "C" int pw_hostpath_channels(const pw_channels_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                    pw_channels_out* out, pw_channels_comp* comps, unsigned long long* mask,
                                    unsigned char* labels, const unsigned long long* open_words, const long* open_first,
                                    int threads) {
    typedef cavity_word u64;
    host_share(n_jobs, threads, [&](long k) {
        const pw_channels_job& J = jobs[k];
        const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz;
        std::vector<u64> todo((size_t)rows), p0((size_t)rows), p1((size_t)rows), acc((size_t)rows, 0);
        if (open_first && open_first[k] >= 0) {
            for (int r = 0; r < rows; ++r) todo[r] = open_words[open_first[k] + r] & cavity_row_mask(nx);
        } else {
            const double* atoms = xyz + 3 * (long)J.atom_first;
            const double* reach = radii + (long)J.radius_first;
            for (int r = 0; r < rows; ++r) {
                const int j = r % ny, l = r / ny;
                const double y = channels_y(J.origin[1], j, J.step[2], l, J.step[4]), z = channels_z(J.origin[2], l, J.step[5]);
                u64 word = cavity_row_mask(nx);
                for (long a = 0; a < (long)J.n && word; ++a) {
                    const double r2 = cavity_reach2(reach[a], J.probe);
                    const double dy = y - atoms[3 * a + 1], dz = z - atoms[3 * a + 2];
                    if (cavity_row_clear(dy, dz, r2)) continue;
                    for (int i = 0; i < nx; ++i)
                        if (!cavity_free(channels_x(J.origin[0], i, J.step[0], j, J.step[1], l, J.step[3]) - atoms[3 * a], dy, dz, r2))
                            word &= ~(1ull << i);
                }
                todo[r] = word;
            }
        }
        pw_channels_out o{};
        unsigned char* label = J.label_first >= 0 ? labels + (long)J.label_first : nullptr;
        for (int r = 0; r < rows; ++r) {
            o.n_open += cavity_popcount(todo[r]);
            if (label)
                for (int i = 0; i < nx; ++i)
                    if (!((todo[r] >> i) & 1ull)) label[(long)r * nx + i] = (unsigned char)CHAN_LABEL_CLOSED;
        }
        pw_channels_comp* table = comps + (long)J.comp_first;
        long count = 0;
        for (int seed_row = 0; seed_row < rows;) {
            if (!todo[seed_row]) {
                ++seed_row;
                continue;
            }
            const int seed_i = __builtin_ctzll(todo[seed_row]);
            const ChannelsWalk W = channels_host_walk(todo, p0, p1, seed_row, 1ull << seed_i, nx, ny, nz);
            pw_channels_comp C{};
            C.first = (long)seed_row * nx + seed_i;
            C.n_voxels = W.n_voxels;
            for (int a = 0; a < 3; ++a) C.n_cross[a] = W.n_cross[a];
            C.wraps = W.wraps;
            C.rank = channels_rank(W.wraps);
            const unsigned char name = (unsigned char)(count < J.c_max ? count : CHAN_LABEL_BEYOND);
            for (int r = 0; r < rows; ++r) {
                const u64 f = p0[r] | p1[r];
                if (!f) continue;
                todo[r] &= ~f;
                if (C.rank >= 1) acc[r] |= f;
                if (label)
                    for (int i = 0; i < nx; ++i)
                        if ((f >> i) & 1ull) label[(long)r * nx + i] = name;
            }
            if (count < J.c_max) table[count] = C;
            o.n_voxels_by_rank[C.rank] += C.n_voxels;
            o.n_components_by_rank[C.rank] += 1;
            ++count;
        }
        for (long c = count; c < J.c_max; ++c) {
            pw_channels_comp none{};
            none.first = -1;
            table[c] = none;
        }
        if (J.mask_first >= 0)
            for (int r = 0; r < rows; ++r) mask[(long)J.mask_first + r] = acc[r];
        o.n_components = count;
        o.n_recorded = count < J.c_max ? count : J.c_max;
        o.flags = count > J.c_max ? CHAN_TRUNCATED : 0;
        o.reserved = 0;
        out[(long)J.out] = o;
    });
    return PW_OK;
}

// pw_percolation on the host (pw_percolate.hip checks the arguments and sends device == -1 contexts here): the keys of
// pw_passage.hpp, the candidates and the search of pw_percolate.hpp, on the maps of host_field_batches within
// PERC_WORKSPACE_BYTES.  A batch's jobs are shared out.  A job is a plain loop: the scan of its map, the search -- an
// evaluation is the allowed words from the map, the candidates, then component after component from the first candidate
// by channels_host_walk --, and one evaluation at each distinct level for the rows.  n_evaluations, n_fills (may be
// null): per job, diagnostic.
extern "C" int pw_hostpath_percolation(const pw_percolation_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                       const double* field, double* map, pw_percolation_level* levels, pw_percolation_out* out,
                                       int* n_evaluations, int* n_fills, int threads) {
    typedef cavity_word u64;
    constexpr long NO_RANK = 0x7fffffffffffffffl;
    host_field_batches(jobs, n_jobs, xyz, coef, field, PERC_WORKSPACE_BYTES, threads, CellFieldValue(),
                       [&](long first, long last, auto field_of) {
        host_share(last - first, threads, [&](long q) {
            const long k = first + q;
            const pw_percolation_job& J = jobs[k];
            const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz;
            const long V = (long)nx * rows;
            const double* U = field_of(k);
            if (J.map_first >= 0)
                for (long v = 0; v < V; ++v) map[(long)J.map_first + v] = U[v];
            pw_percolation_level* R = levels + (long)J.level_first;
            // the scan
            u64 kmin = PAS_KEY_NONE, kmax = 0;
            long min_rank = NO_RANK, n_blocked = 0;
            for (long v = 0; v < V; ++v) {
                const u64 key = pas_key(U[v]);
                if (key == PAS_KEY_INF) {
                    ++n_blocked;
                    continue;
                }
                if (pas_before(key, v, kmin, min_rank)) {
                    kmin = key;
                    min_rank = v;
                }
                kmax = key > kmax ? key : kmax;
            }
            const bool some = min_rank != NO_RANK;
            std::vector<u64> allowed((size_t)rows), todo((size_t)rows), p0((size_t)rows), p1((size_t)rows);
            long best[PERC_CRITERIA];
            int evaluations = 0, fills = 0;
            // an evaluation (pw_percolate.hip: perc_evaluate)
            auto evaluate = [&](u64 level, int asked, bool final, bool& complete, u64& below, u64& above) {
                ++evaluations;
                below = 0;
                above = PAS_KEY_NONE;
                long n_allowed = 0;
                for (int r = 0; r < rows; ++r) {
                    u64 word = 0;
                    for (int i = 0; i < nx; ++i) {
                        const u64 key = pas_key(U[(long)r * nx + i]);
                        if (key <= level) {
                            word |= 1ull << i;
                            below = key > below ? key : below;
                        } else if (key < PAS_KEY_INF) {
                            above = key < above ? key : above;
                        }
                    }
                    allowed[r] = word;
                    n_allowed += cavity_popcount(word);
                }
                for (int r = 0; r < rows; ++r) {
                    const int j = r % ny, l = r / ny;
                    todo[r] = perc_candidates(allowed[r], allowed[l * ny], allowed[j], nx, ny, nz, j, l);
                }
                int met = 0;
                complete = true;
                for (int seed_row = 0; seed_row < rows;) {               // (a turn strikes a candidate off, or moves on)
                    if (!todo[seed_row]) {
                        ++seed_row;
                        continue;
                    }
                    const u64 seed_bit = 1ull << __builtin_ctzll(todo[seed_row]);
                    const ChannelsWalk W = channels_host_walk(allowed, p0, p1, seed_row, seed_bit, nx, ny, nz);
                    const int wraps = W.wraps;
                    const long n_voxels = W.n_voxels;
                    fills += W.fills;
                    const int crit = perc_criteria(wraps);
                    met |= crit;
                    long comp_first = -1;
                    for (int r = 0; r < rows; ++r) {
                        const u64 f = p0[r] | p1[r];
                        if (!f) continue;
                        if (comp_first < 0) comp_first = (long)r * nx + __builtin_ctzll(f);
                        todo[r] &= ~f;
                    }
                    if (!final) {
                        if ((met & asked) == asked) {
                            complete = false;
                            break;
                        }
                        continue;
                    }
                    int lead = 0;
                    for (int c = 0; c < PERC_CRITERIA; ++c)
                        if (((crit & asked) >> c) & 1) lead |= (comp_first < best[c]) << c;
                    if (!lead) continue;
                    u64 well_key = PAS_KEY_NONE;
                    long well_rank = NO_RANK, saddle_rank = -1;
                    for (int r = 0; r < rows; ++r) {
                        const u64 f = p0[r] | p1[r];
                        for (int i = 0; f && i < nx; ++i) {
                            if (!((f >> i) & 1ull)) continue;
                            const long rank = (long)r * nx + i;
                            const u64 key = pas_key(U[rank]);
                            if (pas_before(key, rank, well_key, well_rank)) {
                                well_key = key;
                                well_rank = rank;
                            }
                            if (key == level && saddle_rank < 0) saddle_rank = rank;
                        }
                    }
                    for (int c = 0; c < PERC_CRITERIA; ++c) {
                        if (!((lead >> c) & 1)) continue;
                        best[c] = comp_first;
                        pw_percolation_level& O = R[c];
                        O.level = saddle_rank >= 0 ? U[saddle_rank] : aff_inf();
                        O.well = U[well_rank];
                        O.first = comp_first;
                        O.n_voxels = n_voxels;
                        grid_voxel(saddle_rank, nx, ny, O.saddle);
                        grid_voxel(well_rank, nx, ny, O.well_voxel);
                        O.wraps = wraps;
                        O.rank = channels_rank(wraps);
                        O.flags = 0;
                        O.reserved = 0;
                    }
                }
                if (final)
                    for (int c = 0; c < PERC_CRITERIA; ++c)
                        if ((asked >> c) & 1) R[c].n_allowed = n_allowed;
                return met;
            };
            bool complete;
            u64 below, above, lo[PERC_CRITERIA], hi[PERC_CRITERIA];
            const int met_at_top = some ? evaluate(kmax, 63, false, complete, below, above) : 0;
            pw_percolation_out& O = out[(long)J.out];
            O.n_blocked = n_blocked;
            O.u_min = some ? U[min_rank] : aff_inf();
            grid_voxel(some ? min_rank : -1, nx, ny, O.u_min_voxel);
            O.flags = (met_at_top & 1) ? 0 : PERC_NEVER;
            for (int c = 0; c < PERC_CRITERIA; ++c) {
                pw_percolation_level none{};
                none.level = none.well = aff_inf();
                none.first = -1;
                for (int a = 0; a < 3; ++a) none.saddle[a] = none.well_voxel[a] = -1;
                none.flags = PERC_NEVER;
                R[c] = none;
                best[c] = NO_RANK;
            }
            perc_search_begin(lo, hi, kmin, kmax, met_at_top);
            for (int step = 0; some && step < PERC_MAX_STEPS; ++step) {
                u64 mid = 0;
                int needed = 0;
                if (!perc_search_next(lo, hi, mid, needed)) break;
                const int met = evaluate(mid, needed, false, complete, below, above);
                perc_search_learn(lo, hi, met, complete, below, above);
            }
            for (int c = 0; some && c < PERC_CRITERIA; ++c) {
                int asked = 0;
                bool seen = false;
                for (int d = 0; d < PERC_CRITERIA; ++d) {
                    if (hi[d] != hi[c]) continue;
                    asked |= 1 << d;
                    seen = seen || d < c;
                }
                if (hi[c] == PAS_KEY_INF || seen) continue;
                evaluate(hi[c], asked, true, complete, below, above);
            }
            if (n_evaluations) n_evaluations[k] = evaluations;
            if (n_fills) n_fills[k] = fills;
        });
    });
    return PW_OK;
}

// pw_basins on the host (pw_basins.hip checks the arguments and sends device == -1 contexts here): the definition of
// pw_basins.hpp as plain loops, a job a piece of work.  The parents by bas_parent; the roots numbered in rank order; a
// voxel's basin and offset by walking its chain down to a voxel that has them already; the faces by their packed keys,
// sorted; every sum by aff_tree over the 64 slots of a row, the rows in order.  n_rounds, n_faces (may be null): per
// job, diagnostic.
extern "C" int pw_hostpath_basins(const pw_basins_job* jobs, long n_jobs, const double* xyz, const double* coef, const double* field,
                                  double* map, pw_basins_basin* basins, pw_basins_edge* edges, pw_basins_label* labels,
                                  pw_basins_out* out, int* n_rounds, int* n_faces, int threads) {
    typedef cavity_word u64;
    host_share(n_jobs, threads, [&](long job) {
        const pw_basins_job& J = jobs[job];
        const int nx = J.nx, ny = J.ny, nz = J.nz, rows = ny * nz, L = J.n_betas;
        const long V = (long)nx * rows;
        std::vector<double> own;
        const double* U = field + (long)J.field_first;
        if (J.field_first == -1) {
            own.resize((size_t)V);
            for (long v = 0; v < V; ++v) own[v] = CellFieldValue()(J, xyz + 3 * (long)J.atom_first, coef + 2 * (long)J.coef_first, v);
            U = own.data();
        }
        if (J.map_first >= 0)
            for (long v = 0; v < V; ++v) map[(long)J.map_first + v] = U[v];
        const u64 cap_key = pas_key(J.cap);
        pw_basins_out O{};
        // the scan and the parents
        u64 kmin = PAS_KEY_NONE;
        long min_rank = -1;
        std::vector<long> parent((size_t)V, -1);
        std::vector<int> step((size_t)(3 * V), 0), o((size_t)(3 * V), 0), id((size_t)V, -1);
        for (long v = 0; v < V; ++v) {
            const u64 key = pas_key(U[v]);
            O.n_blocked += key == PAS_KEY_INF;
            if (!bas_allowed(U[v], cap_key)) continue;
            ++O.n_allowed;
            if (min_rank < 0 || pas_before(key, v, kmin, min_rank)) {
                kmin = key;
                min_rank = v;
            }
            const long row = v / nx;
            parent[v] = bas_parent((int)(v - row * nx), (int)(row % ny), (int)(row / ny), v, nx, ny, nz, cap_key,
                                   [&](long r) { return U[r]; }, &step[3 * v]);
        }
        long B = 0;
        for (long v = 0; v < V; ++v)
            if (parent[v] == v) id[v] = (int)B++;
        bool range = false;
        std::vector<long> chain;
        for (long v = 0; v < V; ++v) {
            if (parent[v] < 0 || id[v] >= 0) continue;
            chain.clear();
            long u = v;
            for (; id[u] < 0; u = parent[u]) chain.push_back(u);         // (fewer than V steps: proof (1))
            for (long q = (long)chain.size() - 1; q >= 0; --q) {
                const long c = chain[q], p = parent[c];
                id[c] = id[p];
                for (int a = 0; a < 3; ++a) {
                    o[3 * c + a] = step[3 * c + a] + o[3 * p + a];
                    range = range || o[3 * c + a] > BAS_MAX_OFFSET || o[3 * c + a] < -BAS_MAX_OFFSET;
                }
            }
        }
        // the faces
        struct Face { u64 key; long vk; double term; };
        std::vector<Face> faces;
        std::vector<u64> keys;
        for (long v = 0; v < V && !range; ++v) {
            if (id[v] < 0) continue;
            const long row = v / nx;
            const int i = (int)(v - row * nx), j = (int)(row % ny), l = (int)(row / ny);
            for (int k = 0; k < 3; ++k) {
                long r = v;
                int c[3];
                if (!bas_step(2 * k + 1, i, j, l, nx, ny, nz, r, c)) {
                    r = v;
                    c[k] = 1;
                }
                if (id[r] < 0) continue;
                int a = id[v], b = id[r], d[3];
                for (int q = 0; q < 3; ++q) d[q] = c[q] + o[3 * r + q] - o[3 * v + q];
                if (a == b && !d[0] && !d[1] && !d[2]) continue;
                bas_canonical(a, b, d);
                if (!bas_in_range(d)) {
                    range = true;
                    continue;
                }
                faces.push_back({bas_edge_key(a, b, d), 4 * v + k, bas_term(U[v], U[r])});
                keys.push_back(faces.back().key);
            }
        }
        const long n_boundary = (long)faces.size();
        if (range) {
            faces.clear();
            keys.clear();
        }
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        const long E = (long)keys.size();
        const bool overflow = B > (long)J.b_cap || E > (long)J.e_cap;
        const long b_written = std::min(B, (long)J.b_cap), e_written = overflow ? 0 : E;
        // the basins' rows and sums
        pw_basins_basin* R = basins + (long)J.basin_first;
        for (long v = 0; v < V; ++v) {
            if (id[v] < 0 || id[v] >= b_written) continue;
            pw_basins_basin& Q = R[id[v]];
            if (parent[v] == v) {
                Q.root = v;
                Q.n_voxels = 0;
                Q.u_min = U[v];
                for (int b = 0; b < BAS_MAX_BETAS; ++b) Q.z[b] = Q.e[b] = 0.0;
            }
        }
        for (long v = 0; v < V; ++v)
            if (id[v] >= 0 && id[v] < b_written) ++R[id[v]].n_voxels;
        bool clamped = false;
        double wt[AFF_CHUNK], slot[AFF_CHUNK];
        std::vector<int> seen;
        for (int r = 0; r < rows; ++r) {
            const long v0 = (long)r * nx;
            seen.clear();
            for (int t = 0; t < nx; ++t) {
                const int a = id[v0 + t];
                if (a >= 0 && std::find(seen.begin(), seen.end(), a) == seen.end()) seen.push_back(a);
            }
            if (seen.empty()) continue;
            for (int b = 0; b < L; ++b) {
                for (int t = 0; t < nx; ++t)
                    wt[t] = id[v0 + t] >= 0 ? aff_weight(J.betas[b], U[v0 + t], POW_EXP_TAB, clamped) : 0.0;
                for (int a : seen) {
                    if (a >= b_written) continue;
                    for (int kind = 0; kind < 2; ++kind) {
                        for (int t = 0; t < AFF_CHUNK; ++t)
                            slot[t] = t < nx && id[v0 + t] == a ? (kind ? wt[t] * U[v0 + t] : wt[t]) : 0.0;
                        double& total = kind ? R[a].e[b] : R[a].z[b];
                        total = total + aff_tree(slot);
                    }
                }
            }
        }
        // the edges' rows and sums
        if (e_written) {
            pw_basins_edge* G = edges + (long)J.edge_first;
            std::vector<u64> saddle_key((size_t)E, PAS_KEY_NONE);
            std::vector<int> face_edge((size_t)(3 * V), -1);
            for (long e = 0; e < E; ++e) {
                pw_basins_edge& Q = G[e];
                bas_edge_unkey(keys[e], Q.a, Q.b, Q.d);
                Q.saddle_k = 0;
                Q.n_faces = 0;
                Q.saddle_voxel = -1;
                Q.saddle = 0.0;
                for (int b = 0; b < BAS_MAX_BETAS; ++b) Q.s[b][0] = Q.s[b][1] = Q.s[b][2] = 0.0;
            }
            for (const Face& F : faces) {                                // (ascending in (v, k): the first of a tie stays)
                const long e = std::lower_bound(keys.begin(), keys.end(), F.key) - keys.begin();
                pw_basins_edge& Q = G[e];
                ++Q.n_faces;
                face_edge[(F.vk & 3) * V + (F.vk >> 2)] = (int)e;
                if (pas_key(F.term) < saddle_key[e]) {
                    saddle_key[e] = pas_key(F.term);
                    Q.saddle = F.term;
                    Q.saddle_voxel = F.vk >> 2;
                    Q.saddle_k = (int)(F.vk & 3);
                }
            }
            bool unused = false;
            for (int b = 0; b < L; ++b)
                for (int k = 0; k < 3; ++k)
                    for (int r = 0; r < rows; ++r) {
                        const long v0 = (long)r * nx;
                        seen.clear();
                        for (int t = 0; t < nx; ++t) {
                            const int e = face_edge[k * V + v0 + t];
                            wt[t] = 0.0;
                            if (e < 0) continue;
                            if (std::find(seen.begin(), seen.end(), e) == seen.end()) seen.push_back(e);
                            long rr = v0 + t;
                            int c[3];
                            const long row = rr / nx;
                            if (!bas_step(2 * k + 1, t, (int)(row % ny), (int)(row / ny), nx, ny, nz, rr, c)) rr = v0 + t;
                            wt[t] = aff_weight(J.betas[b], bas_term(U[v0 + t], U[rr]), POW_EXP_TAB, unused);
                        }
                        for (int e : seen) {
                            for (int t = 0; t < AFF_CHUNK; ++t) slot[t] = t < nx && face_edge[k * V + v0 + t] == e ? wt[t] : 0.0;
                            G[e].s[b][k] = G[e].s[b][k] + aff_tree(slot);
                        }
                    }
        }
        if (J.label_first >= 0)
            for (long v = 0; v < V; ++v) {
                pw_basins_label& Q = labels[(long)J.label_first + v];
                Q.basin = id[v];
                for (int a = 0; a < 3; ++a) Q.o[a] = id[v] < 0 || range ? 0 : o[3 * v + a];
            }
        O.n_basins = B;
        O.n_edges = E;
        O.n_basins_written = b_written;
        O.n_edges_written = e_written;
        O.u_min = min_rank >= 0 ? U[min_rank] : aff_inf();
        grid_voxel(min_rank, nx, ny, O.u_min_voxel);
        O.flags = (overflow ? BAS_OVERFLOW : 0) | (clamped ? BAS_CLAMPED : 0) | (range ? BAS_RANGE : 0);
        out[(long)J.out] = O;
        if (n_rounds) n_rounds[job] = 0;
        if (n_faces) n_faces[job] = (int)n_boundary;
    });
    return PW_OK;
}

// the phases of pw_dft.hpp for arbitrary k (test instrumentation, pw_dft.hip: pw_internal_dft_twiddles)
extern "C" void pw_hostpath_dft_twiddles(long j, long M, const long* k, long n, double* c, double* s) {
    for (long i = 0; i < n; ++i) dft_phase(j, k[i], M, &c[i], &s[i]);
}

// pw_exp over an array (test instrumentation, pw_kde.hip: pw_internal_exp)
extern "C" void pw_hostpath_exp(const double* x, long n, double* y) {
    for (long i = 0; i < n; ++i) y[i] = pw_exp(x[i]);
}

// one function of pw_math.hpp over an array, with the reciprocal-square-root table the analysis above uses
// (test instrumentation, pw_kernels.hip: pw_internal_math); y is null for the functions of one argument
extern "C" void pw_hostpath_math(int which, const double* x, const double* y, long n, double* out) {
    std::call_once(g_rsq_once, [] { rsqrt14_decode(g_rsq); });
    for (long i = 0; i < n; ++i) out[i] = pw_math_probe(which, x[i], y ? y[i] : 0.0, g_rsq);
}

// pw_erfc element by element (test instrumentation, pw_ewald.hip: pw_internal_erfc)
extern "C" void pw_hostpath_erfc(const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = pw_erfc(x[i]);
}

// a batch of optimiser cases on a one-lane team (test instrumentation, pw_lb_probe.hip: pw_internal_lb_probe, which
// has checked that every image is safe to run); the block is a copy, as the device's is
#include "pw_lb_probe.hpp"
template <int N>
static void lb_probe_host(void* cases, long n_cases) {
    LbProbeCase<N>* cs = (LbProbeCase<N>*)cases;
    for (long u = 0; u < n_cases; ++u) {
        LbMem<N> block = cs[u].mem;
        lb_probe_run<HostTeam, N>(&cs[u], &block);
#if defined(PW_PROFILE) && defined(PW_LB_FINE)
        block.prof_fine = nullptr;      // (a diagnostic build's pointer member: pointers never leave the library)
#endif
        cs[u].mem = block;
    }
}
extern "C" int pw_hostpath_lb_probe(int n, void* cases, long n_cases) {
    if (n == 3) lb_probe_host<3>(cases, n_cases);
    else lb_probe_host<1>(cases, n_cases);
    return PW_OK;
}
