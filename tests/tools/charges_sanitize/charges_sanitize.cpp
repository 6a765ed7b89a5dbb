// charges_sanitize.cpp -- pw_charges' host path (pw_hostpath.cpp: pw_hostpath_charges) in a stand-alone program, to be
// built with -fsanitize=address,undefined or -fsanitize=thread together with pw_hostpath.cpp and run with the thread
// count as its argument: 24 jobs of 1 .. 257 atoms that share three parameter sets -- several total charges, tolerances
// and bounds, one that runs out of steps, one that breaks down, outputs from the back to the front -- and an FNV-1a
// checksum of every output byte, which must be the same at every thread count.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/charges_sanitize/charges_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o charges_sanitize && ./charges_sanitize 16
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" int pw_hostpath_charges(const pw_charges_job* jobs, long n_jobs, const double* xyz, const double* params,
                                   double* charges, pw_charges_out* out, int threads);

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                                            // xorshift64*, in [0, 1)
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static uint64_t fnv(uint64_t h, const void* p, size_t bytes) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001B3ull;
    return h;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1;
    const long sizes[8] = {1, 2, 3, 63, 64, 65, 129, 257}, n_rows = 257;
    const double table[4][2] = {{4.528, 13.8904}, {5.343, 10.126}, {6.899, 11.760}, {8.741, 13.364}};
    std::vector<double> params(2 * 3 * n_rows);                      // three parameter sets of 257 rows
    for (long r = 0; r < 3 * n_rows; ++r) {
        const int e = (int)(4.0 * uniform());
        params[2 * r] = table[e][0];
        params[2 * r + 1] = table[e][1];
    }
    std::vector<pw_charges_job> jobs;
    std::vector<double> xyz;
    long n_charges = 0;
    for (int k = 0; k < 24; ++k) {
        pw_charges_job J;
        memset(&J, 0, sizeof J);
        J.n = sizes[k % 8];
        J.xyz_first = (long)xyz.size() / 3;
        J.param_first = (k % 3) * n_rows + (k % 2 ? n_rows - J.n : 0);
        J.total_charge = (double)(k % 4) - 1.0;
        J.coulomb = 14.399645;
        J.tol = k % 5 == 0 ? 1e-2 : k % 5 == 1 ? 1e-6 : 1e-10;
        J.max_iter = k == 7 ? 3 : 1000;
        for (long a = 0; a < 3 * J.n; ++a) xyz.push_back(20.0 * uniform());
        n_charges += J.n;
        jobs.push_back(J);
    }
    {                                                                // two atoms a hair apart with a huge constant: breakdown
        pw_charges_job& J = jobs[1];
        J.coulomb = 1e6;
        xyz[3 * J.xyz_first + 3] = xyz[3 * J.xyz_first] + 1e-3;
        xyz[3 * J.xyz_first + 4] = xyz[3 * J.xyz_first + 1];
        xyz[3 * J.xyz_first + 5] = xyz[3 * J.xyz_first + 2];
    }
    long at = n_charges;
    for (size_t k = 0; k < jobs.size(); ++k) {                       // outputs from the back to the front
        at -= jobs[k].n;
        jobs[k].charge_first = at;
        jobs[k].out = (int64_t)(jobs.size() - 1 - k);
    }
    std::vector<double> charges((size_t)n_charges, -1.0);
    std::vector<pw_charges_out> out(jobs.size());
    const int rc = pw_hostpath_charges(jobs.data(), (long)jobs.size(), xyz.data(), params.data(), charges.data(), out.data(), threads);
    uint64_t h = fnv(0xCBF29CE484222325ull, charges.data(), sizeof(double) * charges.size());
    h = fnv(h, out.data(), sizeof(pw_charges_out) * out.size());     // (no padding: 9 doubles and 4 int32, reserved written)
    int converged = 0, broke = 0, short_of = 0;
    for (const pw_charges_out& o : out) {
        converged += o.flags == 0;
        broke += (o.flags & PW_CHG_BREAKDOWN) != 0;
        short_of += (o.flags & PW_CHG_NOT_CONVERGED) != 0;
    }
    printf("rc %d, %zu jobs, %d converged, %d out of steps, %d broke down, threads %d, checksum %016llx\n", rc, jobs.size(),
           converged, short_of, broke, threads, (unsigned long long)h);
    return rc;
}
