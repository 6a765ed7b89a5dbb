// stat_sanitize.cpp -- the host paths of the statistical entries (pw_hostpath.cpp: pw_hostpath_kde, _kde2, _kdew, _corr,
// _dft, _gate, _trans, _superpose) in a stand-alone program, to be built with -fsanitize=address,undefined or
// -fsanitize=thread together with pw_hostpath.cpp and run with the thread count as its argument.  Every entry is called
// twice: with nine jobs -- series of 0 .. 1100 entries across the chunk of 512, 0 .. 37 outputs across the blocks of 8 and
// 16, so jobs without a piece of work and last blocks cut short -- and with three jobs that make fewer pieces than 16
// threads; pw_superpose with 37 jobs and with 3.  Outputs go from the back to the front into arrays filled with a
// sentinel, and one FNV-1a checksum covers every output byte, which must be the same at every thread count.  Host code
// only: it is not loaded into Python and needs no device.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/stat_sanitize/stat_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o stat_sanitize && ./stat_sanitize 16
// Expected at every thread count, with either sanitizer or none (x86-64, glibc): checksum 7c5bae0f3b427772.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" {
int pw_hostpath_kde(const pw_kde_job* jobs, long n_jobs, const double* samples, const double* points, double* sums, int threads);
int pw_hostpath_kde2(const pw_kde2_job* jobs, long n_jobs, const double* samples, const double* points, double* sums, int threads);
int pw_hostpath_kdew(const pw_kdew_job* jobs, long n_jobs, const double* samples, const double* points, const double* weights,
                     double* sums, int threads);
int pw_hostpath_corr(const pw_corr_job* jobs, long n_jobs, const double* series, double* sums, int threads);
int pw_hostpath_dft(const pw_dft_job* jobs, long n_jobs, const double* series, double* re, double* im, int threads);
int pw_hostpath_gate(const pw_gate_job* jobs, long n_jobs, const double* series, const double* thresholds, long n_bins,
                     long* counts, long* hist, int threads);
int pw_hostpath_trans(const pw_trans_job* jobs, long n_jobs, const double* series, const double* edges, long n_states,
                      long* counts, int threads);
int pw_hostpath_superpose(const pw_superpose_job* jobs, long n_jobs, const double* xyz, const double* weights,
                          pw_superpose_out* out, int threads);
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {                                             // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static double uniform() { return (double)(next() >> 11) / 9007199254740992.0; }   // in [0, 1)

static uint64_t g_hash = 0xCBF29CE484222325ull;
static void fnv(const void* p, size_t bytes) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) g_hash = (g_hash ^ c[i]) * 0x100000001B3ull;
}
template <class T>
static void fnv(const std::vector<T>& v) { fnv(v.data(), sizeof(T) * v.size()); }

struct Size { long n, m; };                                          // entries of a job's series, outputs of the job
static const std::vector<Size> MANY = {{700, 37}, {0, 5}, {513, 0}, {1, 1}, {512, 8}, {511, 9}, {1100, 16}, {64, 17}, {130, 33}};
static const std::vector<Size> FEW = {{0, 3}, {40, 3}, {5, 0}};

// values in [-1, 1), one in `gap_every` a NaN (0: none)
static std::vector<double> series_of(long n, int gap_every) {
    std::vector<double> a((size_t)n);
    for (long t = 0; t < n; ++t) a[t] = gap_every && next() % gap_every == 0 ? NAN : 2.0 * uniform() - 1.0;
    return a;
}

// where each job's `count[k]` outputs start, the last job's first
static std::vector<long> back_to_front(const std::vector<long>& count, long& total) {
    total = 0;
    for (long c : count) total += c;
    std::vector<long> first(count.size());
    long at = total;
    for (size_t k = 0; k < count.size(); ++k) first[k] = (at -= count[k]);
    return first;
}

static int run(const std::vector<Size>& sizes, int threads) {
    const long K = (long)sizes.size();
    long n_all = 0, total;
    std::vector<long> a_first, m_of;
    for (const Size& s : sizes) {
        a_first.push_back(n_all);
        n_all += s.n;
        m_of.push_back(s.m);
    }
    const std::vector<long> out_first = back_to_front(m_of, total);
    int rc = 0;
    {                                                                // kde, kde2: the points of a job in [-1, 1)
        const std::vector<double> samples = series_of(2 * n_all, 0), points = series_of(2 * total, 0);
        std::vector<pw_kde_job> jobs;
        std::vector<pw_kde2_job> jobs2;
        for (long k = 0; k < K; ++k) {
            jobs.push_back({a_first[k], sizes[k].n, out_first[k], sizes[k].m, 1.0 + 3.0 * uniform()});
            jobs2.push_back({a_first[k], sizes[k].n, out_first[k], sizes[k].m, 1.0 + uniform(), uniform() - 0.5, 2.0 + uniform()});
        }
        std::vector<double> sums((size_t)total, -777.0), sums2((size_t)total, -777.0);
        rc |= pw_hostpath_kde(jobs.data(), K, samples.data(), points.data(), sums.data(), threads);
        rc |= pw_hostpath_kde2(jobs2.data(), K, samples.data(), points.data(), sums2.data(), threads);
        fnv(sums);
        fnv(sums2);
    }
    {                                                                // kdew: one to three replicas a job
        const std::vector<double> samples = series_of(n_all, 0), points = series_of(total, 0);
        std::vector<double> weights;
        std::vector<long> count;
        for (long k = 0; k < K; ++k) count.push_back((1 + k % 3) * sizes[k].m);
        long n_sums;
        const std::vector<long> first = back_to_front(count, n_sums);
        std::vector<pw_kdew_job> jobs;
        for (long k = 0; k < K; ++k) {
            const long nb = 1 + k % 3;
            jobs.push_back({sizes[k].n, sizes[k].m, nb, a_first[k], out_first[k], (long)weights.size(), first[k], 1.0 + 3.0 * uniform()});
            for (long i = 0; i < sizes[k].n * nb; ++i) weights.push_back((double)(next() % 4));
        }
        std::vector<double> sums((size_t)n_sums, -777.0);
        rc |= pw_hostpath_kdew(jobs.data(), K, samples.data(), points.data(), weights.data(), sums.data(), threads);
        fnv(sums);
    }
    {                                                                // corr: 1 <= n_lags <= n
        const std::vector<double> series = series_of(n_all, 0);
        std::vector<long> count;
        for (long k = 0; k < K; ++k) count.push_back(sizes[k].n ? std::max(1l, std::min(sizes[k].m, sizes[k].n)) : 0);
        long n_sums;
        const std::vector<long> first = back_to_front(count, n_sums);
        std::vector<pw_corr_job> jobs;
        for (long k = 0; k < K; ++k) {                               // (b is a's range, or the first job's where that is as long)
            const long b_first = k % 2 == 0 && sizes[0].n >= sizes[k].n ? a_first[0] : a_first[k];
            jobs.push_back({a_first[k], b_first, sizes[k].n, first[k], count[k]});
        }
        std::vector<double> sums((size_t)n_sums, -777.0);
        rc |= pw_hostpath_corr(jobs.data(), K, series.data(), sums.data(), threads);
        fnv(sums);
    }
    {                                                                // dft: odd numerators below the period
        const std::vector<double> series = series_of(n_all, 0);
        std::vector<pw_dft_job> jobs;
        for (long k = 0; k < K; ++k)
            jobs.push_back({a_first[k], sizes[k].n, std::max(2 * sizes[k].n + 3, 2 * sizes[k].m + 2), 1, 2, sizes[k].m, out_first[k]});
        std::vector<double> re((size_t)total, -777.0), im((size_t)total, -777.0);
        rc |= pw_hostpath_dft(jobs.data(), K, series.data(), re.data(), im.data(), threads);
        fnv(re);
        fnv(im);
    }
    {                                                                // gate: gaps in the series, four bins
        const long n_bins = 4;
        const std::vector<double> series = series_of(n_all, 9), thresholds = series_of(total, 0);
        std::vector<pw_gate_job> jobs;
        for (long k = 0; k < K; ++k) jobs.push_back({a_first[k], sizes[k].n, out_first[k], sizes[k].m, out_first[k]});
        std::vector<long> counts((size_t)(total * PW_GATE_FIELDS), -777), hist((size_t)(total * 2 * n_bins), -777);
        rc |= pw_hostpath_gate(jobs.data(), K, series.data(), thresholds.data(), n_bins, counts.data(), hist.data(), threads);
        fnv(counts);
        fnv(hist);
    }
    {                                                                // trans: zero to three edges, lags past the series
        const long n_states = 5;
        const std::vector<double> series = series_of(n_all, 7);
        const double edges[3] = {-0.5, 0.0, 0.5};
        std::vector<pw_trans_job> jobs;
        for (long k = 0; k < K; ++k) jobs.push_back({a_first[k], sizes[k].n, 0, k % 4, k % 3, 1 + k % 2, sizes[k].m, out_first[k]});
        std::vector<long> counts((size_t)(total * n_states * n_states), -777);
        rc |= pw_hostpath_trans(jobs.data(), K, series.data(), edges, n_states, counts.data(), threads);
        fnv(counts);
    }
    return rc;
}

static int run_superpose(long K, int threads) {
    std::vector<pw_superpose_job> jobs;
    long rows = 0;
    for (long k = 0; k < K; ++k) {
        const long n = 1 + (7 * k) % 70;
        jobs.push_back({rows, rows + n, k % 3 ? -1 : rows, n, K - 1 - k});
        rows += 2 * n;
    }
    std::vector<double> xyz = series_of(3 * rows, 0), weights((size_t)rows);
    for (double& w : weights) w = 0.5 + uniform();
    std::vector<pw_superpose_out> out((size_t)K);                   // (no padding: 18 doubles and 2 int32, reserved written)
    memset(out.data(), 0x5A, sizeof(pw_superpose_out) * out.size());
    const int rc = pw_hostpath_superpose(jobs.data(), K, xyz.data(), weights.data(), out.data(), threads);
    fnv(out);
    return rc;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1;
    int rc = run(MANY, threads);
    rc |= run(FEW, threads);
    rc |= run_superpose(37, threads);
    rc |= run_superpose(3, threads);
    printf("rc %d, 8 entries, %zu and %zu jobs, threads %d, checksum %016llx\n", rc, MANY.size(), FEW.size(), threads,
           (unsigned long long)g_hash);
    return rc;
}
