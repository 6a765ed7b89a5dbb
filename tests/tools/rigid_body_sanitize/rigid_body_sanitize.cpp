// rigid_body_sanitize.cpp -- pw_rigid_body_affinity's host path (pw_hostpath.cpp: pw_hostpath_rigid_body) in a stand-alone
// program, to be built with -fsanitize=address,undefined or -fsanitize=thread together with pw_hostpath.cpp and run with
// the thread count as its argument.  Twelve jobs of mixed grids -- with masks and without, 1 .. 8 sites, charged and not,
// 1 .. 1024 poses, several betas, with maps and without, no atoms, an empty region -- are linear guests: each goes through
// pw_hostpath_rigid with its offsets and directions and through pw_hostpath_rigid_body with the table p = t * d, and the
// two must write the same bytes.  An FNV-1a checksum of every output byte must be the same at every thread count.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/rigid_body_sanitize/rigid_body_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o rigid_body_sanitize \
//       && ./rigid_body_sanitize 16
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" int pw_hostpath_rigid(const pw_rigid_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                 const double* coef, const double* offsets, const double* dirs,
                                 const unsigned long long* words, const double* betas, double* maps,
                                 pw_affinity_level* levels, pw_rigid_out* out, int threads);
extern "C" int pw_hostpath_rigid_body(const pw_rigid_body_job* jobs, long n_jobs, const long* voxels, const double* xyz,
                                      const double* coef, const double* poses, const unsigned long long* words,
                                      const double* betas, double* maps, pw_affinity_level* levels, pw_rigid_out* out,
                                      int threads);

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

static bool same_row(const pw_rigid_out& a, const pw_rigid_out& b) {  // (field by field: the padding is not the entry's)
    return a.n_voxels == b.n_voxels && a.n_blocked_poses == b.n_blocked_poses && a.n_dead == b.n_dead &&
           !memcmp(&a.u_min, &b.u_min, sizeof(double)) && !memcmp(a.min_voxel, b.min_voxel, sizeof a.min_voxel) &&
           a.min_dir == b.min_dir && a.flags == b.flags;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 1;
    const int n_jobs = 12;
    const int dims[6][3] = {{1, 1, 1}, {64, 16, 2}, {13, 5, 4}, {63, 4, 4}, {64, 1, 1}, {5, 3, 9}};
    const int sites[8] = {1, 2, 3, 8, 5, 7, 4, 6}, poses_of[6] = {1, 2, 65, 7, 64, 1024};
    const long n_atoms = 200, n_all_dirs = 1024, n_betas = 8;
    std::vector<double> xyz(3 * n_atoms), coef(3 * 8 * n_atoms), offsets(8), dirs(3 * n_all_dirs), betas(n_betas), table;
    for (long a = 0; a < n_atoms; ++a)
        for (int d = 0; d < 3; ++d) xyz[3 * a + d] = -2.0 + 12.0 * uniform();
    for (long r = 0; r < 8 * n_atoms; ++r) {
        const double sigma = 0.8 + 0.8 * uniform(), eps = 0.1 + 0.9 * uniform(), s6 = sigma * sigma * sigma * sigma * sigma * sigma;
        coef[3 * r] = 4.0 * eps * s6 * s6;
        coef[3 * r + 1] = 4.0 * eps * s6;
        coef[3 * r + 2] = -2.0 + 4.0 * uniform();
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
    std::vector<pw_rigid_job> linear;
    std::vector<pw_rigid_body_job> body;
    std::vector<unsigned long long> words;
    std::vector<long> voxels;
    long n_levels = 0, n_maps = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const int* d = dims[k % 6];
        pw_rigid_job J;
        memset(&J, 0, sizeof J);
        J.n_sites = sites[k % 8];
        J.n = k == 5 ? 0 : (k % 2 ? n_atoms : 129);
        J.atom_first = k == 5 ? 0 : n_atoms - J.n;
        J.beta_first = k % 3;
        J.n_betas = 1 + (k * 5) % (int)(n_betas - 2);
        J.dir_first = k % 4;
        J.n_dirs = poses_of[k % 6] - (k % 4 && poses_of[k % 6] == 1024 ? 4 : 0);
        J.level_first = n_levels;
        J.out = k;
        for (int a = 0; a < 3; ++a) J.origin[a] = 0.1 * a;
        J.spacing = 8.0 / (double)(d[0] > d[1] ? d[0] : d[1]);
        J.core2 = 0.25;
        J.cutoff2 = k % 2 ? 16.0 : 0.0;
        J.nx = d[0]; J.ny = d[1]; J.nz = d[2];
        J.charged = (k / 2) % 2;
        long V = (long)d[0] * d[1] * d[2];
        J.word_first = -1;
        if (k % 3 != 1) {                                            // a mask, junk bits beyond nx; job 6: an empty region
            J.word_first = (long)words.size();
            V = 0;
            for (int r = 0; r < d[1] * d[2]; ++r) {
                unsigned long long w = k == 6 ? 0ull : (unsigned long long)(uniform() * 18446744073709551615.0);
                if (d[0] < 64) w |= ~0ull << d[0];
                words.push_back(w);
                V += __builtin_popcountll(d[0] < 64 ? w & ((1ull << d[0]) - 1ull) : w);
            }
        }
        J.map_level = k % 4 == 3 ? -1 : (int)((k * 3) % J.n_betas);
        J.map_first = J.map_level >= 0 ? n_maps : -1;
        n_levels += J.n_betas;
        n_maps += J.map_level >= 0 ? 2 * V : 0;
        voxels.push_back(V);
        linear.push_back(J);
        // the same job as a table: row o * S + s = t_s * d_o, one rounded product a component
        pw_rigid_body_job B;
        memset(&B, 0, sizeof B);
        B.atom_first = J.atom_first; B.n = J.n; B.coef_first = J.coef_first; B.word_first = J.word_first;
        B.beta_first = J.beta_first; B.n_betas = J.n_betas; B.n_sites = J.n_sites; B.n_dirs = J.n_dirs;
        B.level_first = J.level_first; B.map_first = J.map_first; B.out = J.out;
        for (int a = 0; a < 3; ++a) B.origin[a] = J.origin[a];
        B.spacing = J.spacing; B.core2 = J.core2; B.cutoff2 = J.cutoff2;
        B.nx = J.nx; B.ny = J.ny; B.nz = J.nz; B.charged = J.charged; B.map_level = J.map_level;
        B.pose_first = (long)(table.size() / 3);
        for (long o = 0; o < J.n_dirs; ++o)
            for (long s = 0; s < J.n_sites; ++s)
                for (int a = 0; a < 3; ++a) table.push_back(offsets[J.site_first + s] * dirs[3 * (J.dir_first + o) + a]);
        body.push_back(B);
    }
    std::vector<double> maps((size_t)n_maps, -1.0), maps_b((size_t)n_maps, -2.0);
    std::vector<pw_affinity_level> levels((size_t)n_levels), levels_b((size_t)n_levels);
    std::vector<pw_rigid_out> out(linear.size()), out_b(body.size());
    int rc = pw_hostpath_rigid(linear.data(), n_jobs, voxels.data(), xyz.data(), coef.data(), offsets.data(), dirs.data(),
                               words.data(), betas.data(), maps.data(), levels.data(), out.data(), threads);
    rc |= pw_hostpath_rigid_body(body.data(), n_jobs, voxels.data(), xyz.data(), coef.data(), table.data(), words.data(),
                                 betas.data(), maps_b.data(), levels_b.data(), out_b.data(), threads);
    bool same = !memcmp(maps.data(), maps_b.data(), sizeof(double) * maps.size()) &&
                !memcmp(levels.data(), levels_b.data(), sizeof(pw_affinity_level) * levels.size());
    for (int k = 0; k < n_jobs; ++k) same = same && same_row(out[k], out_b[k]);
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv(h, maps_b.data(), sizeof(double) * maps_b.size());
    h = fnv(h, levels_b.data(), sizeof(pw_affinity_level) * levels_b.size());
    long live = 0;
    for (const pw_rigid_out& o : out_b) {
        h = fnv(h, &o.n_voxels, 3 * sizeof(int64_t));
        h = fnv(h, &o.u_min, sizeof(double));
        h = fnv(h, o.min_voxel, 3 * sizeof(int32_t));
        h = fnv(h, &o.min_dir, 2 * sizeof(int32_t));
        live += o.n_voxels - o.n_dead;
    }
    printf("rc %d, %d jobs, %ld voxels with a free pose, threads %d, table == linear: %s, checksum %016llx\n", rc, n_jobs, live,
           threads, same ? "yes" : "NO", (unsigned long long)h);
    return rc || !same;
}
