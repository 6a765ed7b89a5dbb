// channels_sanitize.cpp -- pw_channels' host path (pw_hostpath.cpp: pw_hostpath_channels) in a stand-alone program, to be
// built with -fsanitize=address,undefined or -fsanitize=thread together with pw_hostpath.cpp and run with the thread
// count as its argument: 24 jobs on grids from 1 x 1 x 1 to 64 x 9 x 7 -- half of them classified from atoms on a skewed
// cell, half with ready-made open words whose bits beyond nx are set; c_max from 0 to 254; with and without masks and
// labels; outputs from the back to the front -- and an FNV-1a checksum of every output byte, which must be the same at
// every thread count.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tests/tools/channels_sanitize/channels_sanitize.cpp pywindow_amd/csrc/pw_hostpath.cpp -o channels_sanitize && ./channels_sanitize 16
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../../include/pywindow_amd.h"

extern "C" int pw_hostpath_channels(const pw_channels_job* jobs, long n_jobs, const double* xyz, const double* radii,
                                    pw_channels_out* out, pw_channels_comp* comps, unsigned long long* mask,
                                    unsigned char* labels, const unsigned long long* open_words, const long* open_first,
                                    int threads);

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
    const int caps[6] = {0, 1, 3, 16, 64, 254};
    std::vector<pw_channels_job> jobs;
    std::vector<double> xyz, radii;
    std::vector<unsigned long long> open_words;
    std::vector<long> open_first;
    long n_comps = 0, n_mask = 0, n_labels = 0;
    for (int k = 0; k < 24; ++k) {
        pw_channels_job J;
        memset(&J, 0, sizeof J);
        J.nx = dims[k % 8][0]; J.ny = dims[k % 8][1]; J.nz = dims[k % 8][2];
        J.c_max = caps[k % 6];
        const double step[6] = {0.5, 0.125, 0.4375, -0.0625, 0.1875, 0.46875};
        for (int a = 0; a < 6; ++a) J.step[a] = step[a];
        for (int a = 0; a < 3; ++a) J.origin[a] = 0.25 * a;
        J.probe = 0.1 * (k % 4);
        const long rows = (long)J.ny * J.nz, voxels = rows * J.nx;
        if (k % 2) {                                                 // ready-made open words, the bits beyond nx set
            open_first.push_back((long)open_words.size());
            for (long r = 0; r < rows; ++r) open_words.push_back(next() & next() | (J.nx < 64 ? ~0ull << J.nx : 0ull));
        } else {
            open_first.push_back(-1);
            J.atom_first = J.radius_first = (long)radii.size();
            J.n = voxels / 40 + 1;
            for (long a = 0; a < J.n; ++a) {
                const double f[3] = {uniform() * J.nx, uniform() * J.ny, uniform() * J.nz};
                xyz.push_back(f[0] * step[0] + f[1] * step[1] + f[2] * step[3]);
                xyz.push_back(f[1] * step[2] + f[2] * step[4]);
                xyz.push_back(f[2] * step[5]);
                radii.push_back(0.5 + uniform());
            }
        }
        J.mask_first = k % 3 ? rows : -1;                            // (for now the count; placed below)
        J.label_first = k % 4 ? voxels : -1;
        n_comps += J.c_max;
        n_mask += k % 3 ? rows : 0;
        n_labels += k % 4 ? voxels : 0;
        jobs.push_back(J);
    }
    long at_comp = n_comps, at_mask = n_mask, at_label = n_labels;
    for (size_t k = 0; k < jobs.size(); ++k) {                       // outputs from the back to the front
        pw_channels_job& J = jobs[k];
        at_comp -= J.c_max;
        J.comp_first = at_comp;
        if (J.mask_first >= 0) J.mask_first = (at_mask -= J.mask_first);
        if (J.label_first >= 0) J.label_first = (at_label -= J.label_first);
        J.out = (int64_t)(jobs.size() - 1 - k);
    }
    std::vector<pw_channels_out> out(jobs.size());
    std::vector<pw_channels_comp> comps((size_t)n_comps);
    std::vector<unsigned long long> mask((size_t)n_mask, 0x5555555555555555ull);
    std::vector<unsigned char> labels((size_t)n_labels, 0x77);
    const int rc = pw_hostpath_channels(jobs.data(), (long)jobs.size(), xyz.data(), radii.data(), out.data(), comps.data(),
                                        mask.data(), labels.data(), open_words.data(), open_first.data(), threads);
    uint64_t h = fnv(0xCBF29CE484222325ull, out.data(), sizeof(pw_channels_out) * out.size());   // (no padding: reserved written)
    h = fnv(h, comps.data(), sizeof(pw_channels_comp) * comps.size());
    h = fnv(h, mask.data(), 8 * mask.size());
    h = fnv(h, labels.data(), labels.size());
    long components = 0, winding = 0, truncated = 0, open = 0;
    for (const pw_channels_out& o : out) {
        components += o.n_components;
        winding += o.n_components - o.n_components_by_rank[0];
        truncated += (o.flags & PW_CHAN_TRUNCATED) != 0;
        open += o.n_open;
    }
    printf("rc %d, %zu jobs, %ld open voxels, %ld components, %ld of them wind, %ld jobs truncated, threads %d, checksum %016llx\n",
           rc, jobs.size(), open, components, winding, truncated, threads, (unsigned long long)h);
    return rc;
}
