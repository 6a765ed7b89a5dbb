// basins_sanitize.cpp -- pw_basins' host path (pw_hostpath.cpp: pw_hostpath_basins) in a stand-alone program, to be built
// with -fsanitize=address,undefined or -fsanitize=thread together with pw_hostpath.cpp and run with the thread count as
// its argument: 24 jobs on grids from 1 x 1 x 1 to 64 x 9 x 7 -- half of them with atoms on a skewed cell (with and
// without a cutoff), half with a field of the caller's made of few integer values, blocked voxels and the two zeros; one
// to eight inverse temperatures; finite caps and +inf; capacities that hold and that overflow; with and without maps and
// labels; outputs from the back to the front -- and an FNV-1a checksum of every output byte, which must be the same at
// every thread count.  Host code only: it is not loaded into Python and needs no device.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/basins_sanitize/basins_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o basins_sanitize \
//       && ./basins_sanitize 16
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" int pw_hostpath_basins(const pw_basins_job* jobs, long n_jobs, const double* xyz, const double* coef, const double* field,
                                  double* map, pw_basins_basin* basins, pw_basins_edge* edges, pw_basins_label* labels,
                                  pw_basins_out* out, int* n_rounds, int* n_faces, int threads);

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() {                                             // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static double uniform() { return (double)(next() >> 11) / 9007199254740992.0; }   // in [0, 1)

static uint64_t fnv(uint64_t h, const void* p, size_t bytes) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001B3ull;
    return h;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1;
    const int dims[8][3] = {{1, 1, 1}, {2, 2, 2}, {64, 9, 7}, {63, 5, 13}, {5, 1, 8}, {17, 16, 1}, {33, 8, 8}, {1, 64, 2}};
    std::vector<pw_basins_job> jobs;
    std::vector<double> xyz, coef, field;
    std::vector<long> map_size, label_size;
    long n_map = 0, n_labels = 0, n_basins = 0, n_edges = 0;
    for (int k = 0; k < 24; ++k) {
        pw_basins_job J;
        memset(&J, 0, sizeof J);
        J.nx = dims[k % 8][0]; J.ny = dims[k % 8][1]; J.nz = dims[k % 8][2];
        const double step[6] = {0.5, 0.125, 0.4375, -0.0625, 0.1875, 0.46875};
        for (int a = 0; a < 6; ++a) J.step[a] = step[a];
        for (int a = 0; a < 3; ++a) J.origin[a] = 0.25 * a;
        J.core2 = 0.09;
        J.cutoff2 = k % 4 == 0 ? 0.0 : 6.25;
        J.n_betas = 1 + k % 8;
        for (int b = 0; b < J.n_betas; ++b) J.betas[b] = 0.1 * (b + 1);
        J.cap = k % 5 == 0 ? 0.5 : INFINITY;
        const long voxels = (long)J.nx * J.ny * J.nz;
        J.b_cap = k % 7 == 3 ? 2 : voxels;                           // (some overflow)
        J.e_cap = k % 7 == 5 ? 1 : 3 * voxels;
        if (k % 2) {                                                 // a field of the caller's
            J.field_first = (long)field.size();
            const double values[6] = {-2.0, -1.0, -0.0, 0.0, 1.0, INFINITY};
            for (long v = 0; v < voxels; ++v) field.push_back(values[next() % (k % 3 ? 6 : 5)]);
        } else {
            J.field_first = -1;
            J.atom_first = J.coef_first = (long)(xyz.size() / 3);
            J.n = voxels / 40 + (k % 3 ? 1 : 0);                     // (some jobs without an atom)
            for (long a = 0; a < J.n; ++a) {
                const double f[3] = {uniform() * J.nx, uniform() * J.ny, uniform() * J.nz};
                xyz.push_back(f[0] * step[0] + f[1] * step[1] + f[2] * step[3]);
                xyz.push_back(f[1] * step[2] + f[2] * step[4]);
                xyz.push_back(f[2] * step[5]);
                const double eps = 0.2 + uniform(), s6 = pow(0.8 + 0.5 * uniform(), 6.0);
                coef.push_back(4.0 * eps * s6 * s6);
                coef.push_back(4.0 * eps * s6);
            }
        }
        map_size.push_back(k % 3 ? voxels : 0);
        label_size.push_back(k % 4 != 1 ? voxels : 0);
        n_map += map_size.back();
        n_labels += label_size.back();
        n_basins += J.b_cap;
        n_edges += J.e_cap;
        jobs.push_back(J);
    }
    long at_map = n_map, at_label = n_labels, at_basin = n_basins, at_edge = n_edges;
    for (size_t k = 0; k < jobs.size(); ++k) {                       // outputs from the back to the front
        pw_basins_job& J = jobs[k];
        J.map_first = map_size[k] ? (at_map -= map_size[k]) : -1;
        J.label_first = label_size[k] ? (at_label -= label_size[k]) : -1;
        J.basin_first = (at_basin -= J.b_cap);
        J.edge_first = (at_edge -= J.e_cap);
        J.out = (int64_t)(jobs.size() - 1 - k);
    }
    std::vector<pw_basins_out> out(jobs.size());
    std::vector<pw_basins_basin> basins((size_t)n_basins);
    std::vector<pw_basins_edge> edges((size_t)n_edges);
    std::vector<pw_basins_label> labels((size_t)n_labels);
    memset(basins.data(), 0x5a, sizeof(pw_basins_basin) * basins.size());      // (rows beyond what is written stay)
    memset(edges.data(), 0x5a, sizeof(pw_basins_edge) * edges.size());
    std::vector<double> map((size_t)n_map, -777.0);
    std::vector<int> n_rounds(jobs.size()), n_faces(jobs.size());
    const int rc = pw_hostpath_basins(jobs.data(), (long)jobs.size(), xyz.data(), coef.data(), field.data(), map.data(),
                                      basins.data(), edges.data(), labels.data(), out.data(), n_rounds.data(), n_faces.data(), threads);
    uint64_t h = fnv(0xCBF29CE484222325ull, out.data(), sizeof(pw_basins_out) * out.size());   // (no padding)
    h = fnv(h, basins.data(), sizeof(pw_basins_basin) * basins.size());
    h = fnv(h, edges.data(), sizeof(pw_basins_edge) * edges.size());
    h = fnv(h, labels.data(), sizeof(pw_basins_label) * labels.size());
    h = fnv(h, map.data(), 8 * map.size());
    long n_b = 0, n_e = 0, overflow = 0, faces = 0;
    for (const pw_basins_out& o : out) {
        n_b += o.n_basins;
        n_e += o.n_edges;
        overflow += (o.flags & PW_BAS_OVERFLOW) != 0;
    }
    for (size_t k = 0; k < jobs.size(); ++k) faces += n_faces[k];
    printf("rc %d, %zu jobs, %ld basins, %ld edges, %ld boundary faces, %ld jobs overflowed, threads %d, checksum %016llx\n", rc,
           jobs.size(), n_b, n_e, faces, overflow, threads, (unsigned long long)h);
    return rc;
}
