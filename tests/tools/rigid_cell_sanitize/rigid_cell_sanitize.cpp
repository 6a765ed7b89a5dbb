// rigid_cell_sanitize.cpp -- pw_rigid_cell's host path (pw_hostpath.cpp: pw_hostpath_rigid_cell) in a stand-alone program,
// to be built with -fsanitize=address,undefined or -fsanitize=thread together with pw_hostpath.cpp and run with the thread
// count as its argument: jobs of mixed skewed and orthorhombic grids -- 1 .. 8 sites, several betas, with maps and without,
// no atoms, grids that are no multiple of the group of 4 x 4 x 4 voxels, the skip on and off -- and an FNV-1a checksum of
// every output byte, which must be the same at every thread count.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/rigid_cell_sanitize/rigid_cell_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o rigid_cell_sanitize \
//       && ./rigid_cell_sanitize 16
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" int pw_hostpath_rigid_cell(const pw_rigid_cell_job* jobs, long n_jobs, const double* xyz, const double* coef,
                                      const double* offsets, const double* dirs, const double* betas, double* maps,
                                      pw_affinity_level* levels, pw_rigid_out* out, long long* n_pairs, int skip, int threads);

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
    const int dims[8][3] = {{1, 1, 1}, {64, 5, 2}, {13, 5, 4}, {63, 4, 3}, {64, 1, 1}, {5, 3, 9}, {33, 7, 3}, {8, 8, 8}};
    const int sites[8] = {1, 2, 3, 8, 5, 3, 2, 4}, n_dirs_of[8] = {1, 2, 65, 7, 64, 1024, 3, 16};
    const double skew[6] = {0.5, 0.125, 0.4375, -0.0625, 0.1875, 0.46875};
    const long n_atoms = 2300, n_all_dirs = 1024, n_betas = 8;
    std::vector<double> xyz(3 * n_atoms), coef(2 * 8 * n_atoms), offsets(8), dirs(3 * n_all_dirs), betas(n_betas);
    for (long a = 0; a < n_atoms; ++a)
        for (int d = 0; d < 3; ++d) xyz[3 * a + d] = -6.0 + 20.0 * uniform();
    for (long r = 0; r < 8 * n_atoms; ++r) {
        const double sigma = 0.8 + 0.8 * uniform(), eps = 0.1 + 0.9 * uniform(), s6 = sigma * sigma * sigma * sigma * sigma * sigma;
        coef[2 * r] = 4.0 * eps * s6 * s6;
        coef[2 * r + 1] = 4.0 * eps * s6;
    }
    for (int s = 0; s < 8; ++s) offsets[s] = -0.7 + 0.2 * s;
    for (long o = 0; o < n_all_dirs; ++o) {
        double v[3], len = 0.0;
        for (int d = 0; d < 3; ++d) {
            v[d] = -1.0 + 2.0 * uniform();
            len += v[d] * v[d];
        }
        len = sqrt(len) + 1e-9;
        for (int d = 0; d < 3; ++d) dirs[3 * o + d] = v[d] / len;
    }
    for (long b = 0; b < n_betas; ++b) betas[b] = 0.2 * (double)b;
    std::vector<pw_rigid_cell_job> jobs;
    long n_levels = 0, n_maps = 0;
    for (int k = 0; k < 16; ++k) {
        const int* d = dims[k % 8];
        pw_rigid_cell_job J;
        memset(&J, 0, sizeof J);
        J.n_sites = sites[(k + k / 8) % 8];
        J.n = k == 5 ? 0 : (k % 2 ? 300 : 129);
        J.n = k == 2 ? n_atoms : J.n;                                // (more atoms than a near list of the device holds)
        J.atom_first = k == 5 ? 0 : n_atoms - J.n;
        J.coef_first = 0;
        J.beta_first = k % 3;
        J.n_betas = 1 + (k * 5) % (int)(n_betas - 2);
        J.site_first = 0;
        J.dir_first = k % 4;
        J.n_dirs = n_dirs_of[k % 8] - (k % 4 && n_dirs_of[k % 8] == 1024 ? 4 : 0);
        J.n_dirs = k == 2 ? 3 : J.n_dirs;
        J.level_first = n_levels;
        J.out = k;
        for (int a = 0; a < 3; ++a) J.origin[a] = 0.1 * a;
        const double h = 8.0 / (double)(d[0] > d[1] ? d[0] : d[1]);
        for (int a = 0; a < 6; ++a) J.step[a] = k % 2 ? 2.0 * h * skew[a] : (a == 0 || a == 2 || a == 5 ? h : 0.0);
        J.core2 = 0.25;
        J.cutoff2 = k % 3 ? 16.0 : 6.25;
        J.nx = d[0]; J.ny = d[1]; J.nz = d[2];
        const long V = (long)d[0] * d[1] * d[2];
        J.map_first = k % 4 == 3 ? -1 : n_maps;
        n_levels += J.n_betas;
        n_maps += J.map_first >= 0 ? (J.n_betas + 1) * V : 0;
        jobs.push_back(J);
    }
    uint64_t sums[2];
    long live = 0;
    int rc = 0;
    for (int skip = 0; skip < 2; ++skip) {
        std::vector<double> maps((size_t)n_maps, -1.0);
        std::vector<pw_affinity_level> levels((size_t)n_levels);
        std::vector<pw_rigid_out> out(jobs.size());
        std::vector<long long> n_pairs(jobs.size());
        rc |= pw_hostpath_rigid_cell(jobs.data(), (long)jobs.size(), xyz.data(), coef.data(), offsets.data(), dirs.data(), betas.data(),
                                     maps.data(), levels.data(), out.data(), n_pairs.data(), skip, threads);
        uint64_t h = 0xCBF29CE484222325ull;
        h = fnv(h, maps.data(), sizeof(double) * maps.size());
        h = fnv(h, levels.data(), sizeof(pw_affinity_level) * levels.size());
        live = 0;
        for (const pw_rigid_out& o : out) {                          // (field by field: the padding is not the entry's)
            h = fnv(h, &o.n_voxels, 3 * sizeof(int64_t));
            h = fnv(h, &o.u_min, sizeof(double));
            h = fnv(h, o.min_voxel, 3 * sizeof(int32_t));
            h = fnv(h, &o.min_dir, 2 * sizeof(int32_t));
            live += o.n_voxels - o.n_dead;
        }
        sums[skip] = h;
    }
    if (sums[0] != sums[1]) rc |= 64;                                // (the skip may not show)
    printf("rc %d, %zu jobs, %ld voxels with a free pose, threads %d, checksum %016llx\n", rc, jobs.size(), live, threads,
           (unsigned long long)sums[1]);
    return rc;
}
