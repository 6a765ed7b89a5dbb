// pw_basins.hip -- gfx950 kernels and the C ABI entry of the energy basins of a periodic cell, the dividing surfaces
// between them and their Boltzmann sums (include/pywindow_amd.h: pw_basins; the definition and the proofs in
// pw_basins.hpp).  Two kernels a launch group:
//   field    pw_percolate.hip's: field_items_cell (pw_field_cell_dev.hpp) for the jobs without a field of their own; a
//            caller's field is copied to the job's map in the workspace instead.
//   basins   a workgroup of eight waves a job; the map, an 8-byte (parent, offset) word per voxel, a hash table of
//            edge keys, their sorted list, an edge number per face and the job's rows live in the launch workspace.
//            (1) one scan: n_blocked, n_allowed, u_min, and every allowed voxel's parent by seven key comparisons.
//            (2) pointer jumping in place (pw_basins.hpp, proof (2)): the word is read and written as ONE 8-byte atomic.
//            (3) the roots of a row by ballot, the rows' counts prefixed in LDS, a root's number by popcount; then every
//            voxel takes its root's number.  (4) basin sums: wave s takes the sum s = 2 * beta + (Z | E) and walks the
//            rows IN ORDER; in a row it peels the distinct basins (the lowest live lane's number, a ballot of its
//            members), runs pw_affinity_kernel's shuffle tree with +0.0 in the other lanes and adds the chunk sum to
//            the basin's total: one wave owns a total, so the association is the defined one and there is no partial to
//            store.  (5) edges: every boundary face's packed key goes into the hash table by 64-bit compare-and-swap
//            (new keys counted: E), the keys are gathered, sorted by a bitonic network and looked up per face by binary
//            search; n_faces and the saddle by integer atomics (the key, then the lowest (v, k) among its ties); the
//            sums s[beta][k] as in (4), wave s = 3 * beta + k.
// Every branch that leads to a barrier depends on values read from LDS after a barrier or reduced over the workgroup,
// the same in every thread.  Every loop carries its bound; nothing spins, no workgroup waits for another, no
// floating-point atomics.  Launches follow one another on the context's stream.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/pywindow_amd.h"
#include "pw_field_cell_dev.hpp"
#include "pw_basins.hpp"
#include "pw_grid_host.hpp"

using namespace pw;

extern "C" int pw_hostpath_basins(const pw_basins_job* jobs, long n_jobs, const double* xyz, const double* coef, const double* field,
                                  double* map, pw_basins_basin* basins, pw_basins_edge* edges, pw_basins_label* labels,
                                  pw_basins_out* out, int* n_rounds, int* n_faces, int threads);   // pw_hostpath.cpp

static_assert(PW_BAS_OVERFLOW == BAS_OVERFLOW && PW_BAS_CLAMPED == BAS_CLAMPED && PW_BAS_RANGE == BAS_RANGE &&
              PW_BAS_MAX_BETAS == BAS_MAX_BETAS && PW_BAS_MAX_OFFSET == BAS_MAX_OFFSET && BAS_MAX_BETAS == AFF_MAX_LEVELS,
              "the header's constants and the kernel's");
static_assert(sizeof(pw_basins_job) == 264 && sizeof(pw_basins_basin) == 152 && sizeof(pw_basins_edge) == 240 &&
              sizeof(pw_basins_label) == 16 && sizeof(pw_basins_out) == 72, "the layouts of the header");

namespace {

typedef cavity_word u64;

constexpr int BAS_THREADS = 512, BAS_WAVES = BAS_THREADS / 64;
constexpr int BAS_MAX_ROWS = CAVITY_MAX_G * CAVITY_MAX_G;
constexpr int BAS_BASIN_WORDS = sizeof(pw_basins_basin) / 8, BAS_EDGE_WORDS = sizeof(pw_basins_edge) / 8, BAS_LABEL_WORDS = 2;
constexpr u64 BAS_NUMBERED = 1ull << 63;                            // the word holds the basin's number, not a rank
constexpr long BAS_NO_RANK = 0x7fffffffffffffffl;
constexpr int BAS_STORED = 511;                                     // what ten bits a component hold

// a job as the kernels read it: firsts relative to the spans that were uploaded and to the workspace of the launch
struct BasJobDev {
    long atom_first, n, coef_first;
    long map_first;            // V words
    long item_first, chunks;   // the job's chunks among the work items of the field kernel (none: a caller's field)
    long V;
    long word_first;           // V words
    long table_first, table_slots;     // a power of two > 3 V
    long list_first, list_slots;       // a power of two >= min(e_cap, 3 V), at least 1
    long face_first;           // 3 V ints
    long basin_first, edge_first, label_first;   // the job's rows (labels: -1 without)
    long b_cap, e_cap;         // as given, at most V and 3 V
    double o[3], s[6], core2, cutoff2;
    double betas[BAS_MAX_BETAS];
    u64 cap_key;
    int nx, ny, nz, L;
};

struct BasShared {
    u64 red_key[BAS_WAVES];
    long red_rank[BAS_WAVES], red_blocked[BAS_WAVES], red_allowed[BAS_WAVES];
    int row_count[BAS_MAX_ROWS];             // the roots of a row, then the roots before it
    unsigned long long n_edges, n_boundary;
    unsigned int list_fill;
    int flags, B;
};

__global__ void __launch_bounds__(AFF_CHUNK)
pw_basins_field_kernel(const BasJobDev* __restrict__ jobs, int n_jobs, long total, const double* __restrict__ xyz,
                       const double* __restrict__ coef, u64* __restrict__ ws) {
    field_items_cell(jobs, n_jobs, total, xyz, coef, ws);            // (pw_field_cell_dev.hpp: pw_percolation's field)
}

__device__ inline u64 bas_pack(long parent, int ox, int oy, int oz) {
    return (u64)parent | ((u64)(ox + 512) << 32) | ((u64)(oy + 512) << 42) | ((u64)(oz + 512) << 52);
}
__device__ inline long bas_low(u64 w) { return (long)(w & 0xffffffffull); }
__device__ inline int bas_o(u64 w, int k) { return (int)((w >> (32 + 10 * k)) & 0x3ffull) - 512; }
__device__ inline int bas_clamp(int o, bool& over) {
    over = over || o > BAS_STORED || o < -BAS_STORED;
    return o > BAS_STORED ? BAS_STORED : o < -BAS_STORED ? -BAS_STORED : o;
}
__device__ inline u64 bas_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void bas_store(u64* p, u64 w) { __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the face (v, k) after the numbering: false when v or v' = v + e_k is not allowed or the face is interior; otherwise
// the edge's key (in_range) and the face's term
__device__ inline bool bas_face(const u64* __restrict__ map, const u64* __restrict__ word, long v, int k, int nx, int ny, int nz,
                                u64& key, double& term, bool& in_range) {
    const u64 w = word[v];
    if (w == BAS_NONE) return false;
    const long row = v / nx;
    const int i = (int)(v - row * nx), j = (int)(row % ny), l = (int)(row / ny);
    long r = v;
    int c[3];
    if (!bas_step(2 * k + 1, i, j, l, nx, ny, nz, r, c)) {           // (n_k == 1: v' is v through the face of +e_k)
        r = v;
        c[0] = k == 0;
        c[1] = k == 1;
        c[2] = k == 2;
    }
    const u64 w2 = word[r];
    if (w2 == BAS_NONE) return false;
    int a = (int)bas_low(w), b = (int)bas_low(w2);
    int d[3] = {c[0] + bas_o(w2, 0) - bas_o(w, 0), c[1] + bas_o(w2, 1) - bas_o(w, 1), c[2] + bas_o(w2, 2) - bas_o(w, 2)};
    if (a == b && !d[0] && !d[1] && !d[2]) return false;
    bas_canonical(a, b, d);
    in_range = bas_in_range(d);
    key = in_range ? bas_edge_key(a, b, d) : 0;
    term = bas_term(pw_bits2d(map[v]), pw_bits2d(map[r]));
    return true;
}

// the chunk tree over the lanes (pw_affinity_kernel's): lane 0 holds the defined sum
__device__ inline double bas_tree(double x) {
    for (int s = 1; s < AFF_CHUNK; s <<= 1) x = x + __shfl_down(x, s);
    return x;
}

// diag: the rounds of the pointer jumping and the boundary faces of the job (diagnostic: not part of the defined result)
__global__ void __launch_bounds__(BAS_THREADS)
pw_basins_kernel(const BasJobDev* __restrict__ jobs, u64* __restrict__ ws, pw_basins_out* __restrict__ out, int* __restrict__ diag) {
    __shared__ BasShared S;
    __shared__ __attribute__((aligned(16))) uint64_t s_tab[256];
    const BasJobDev& D = jobs[blockIdx.x];
    const int nx = D.nx, ny = D.ny, nz = D.nz, rows = ny * nz, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = D.L;
    const long V = D.V;
    const u64 cap_key = D.cap_key;
    const u64* map = ws + D.map_first;
    u64* word = ws + D.word_first;
    u64* table = ws + D.table_first;
    u64* list = ws + D.list_first;
    int* face_edge = (int*)(ws + D.face_first);
    pw_basins_basin* basins = (pw_basins_basin*)(ws + D.basin_first);
    pw_basins_edge* edges = (pw_basins_edge*)(ws + D.edge_first);
    pw_basins_label* labels = D.label_first >= 0 ? (pw_basins_label*)(ws + D.label_first) : nullptr;

    for (int t = tid; t < 256; t += BAS_THREADS) s_tab[t] = POW_EXP_TAB[t];
    if (tid == 0) {
        S.n_edges = S.n_boundary = 0;
        S.list_fill = 0;
        S.flags = 0;
    }

    // (1) the scan and the parents
    u64 wk = PAS_KEY_NONE;
    long wr = BAS_NO_RANK, blocked = 0, allowed = 0;
    for (long v = tid; v < V; v += BAS_THREADS) {                        // (the voxels)
        const double U = pw_bits2d(map[v]);
        const u64 key = pas_key(U);
        blocked += key == PAS_KEY_INF;
        if (!bas_allowed(U, cap_key)) {
            word[v] = BAS_NONE;
            continue;
        }
        ++allowed;
        if (pas_before(key, v, wk, wr)) {
            wk = key;
            wr = v;
        }
        const long row = v / nx;
        int c[3];
        const long p = bas_parent((int)(v - row * nx), (int)(row % ny), (int)(row / ny), v, nx, ny, nz, cap_key,
                                  [&](long r) { return pw_bits2d(map[r]); }, c);
        word[v] = bas_pack(p, c[0], c[1], c[2]);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const u64 ok = __shfl_xor(wk, s);
        const long orank = __shfl_xor(wr, s);
        if (pas_before(ok, orank, wk, wr)) {
            wk = ok;
            wr = orank;
        }
        blocked += __shfl_xor(blocked, s);
        allowed += __shfl_xor(allowed, s);
    }
    if (lane == 0) {
        S.red_key[wave] = wk;
        S.red_rank[wave] = wr;
        S.red_blocked[wave] = blocked;
        S.red_allowed[wave] = allowed;
    }
    __syncthreads();
    wk = PAS_KEY_NONE;
    wr = BAS_NO_RANK;
    blocked = allowed = 0;
    for (int w = 0; w < BAS_WAVES; ++w) {
        if (pas_before(S.red_key[w], S.red_rank[w], wk, wr)) {
            wk = S.red_key[w];
            wr = S.red_rank[w];
        }
        blocked += S.red_blocked[w];
        allowed += S.red_allowed[w];
    }

    // (2) pointer jumping: a round that changes nothing ends it.  The distance to the root at least halves a round, so
    // at most ceil(log2 V) + 1 <= 19 rounds change a word (pw_basins.hpp, proof (2)); 64 is a bound, not a budget
    bool over = false;
    int rounds = 0;
    for (int round = 0; round < 64; ++round) {
        int changed = 0;
        for (long v = tid; v < V; v += BAS_THREADS) {                    // (the voxels)
            const u64 w = bas_load(word + v);
            if (w == BAS_NONE) continue;
            const long p = bas_low(w);
            if (p == v) continue;
            const u64 wp = bas_load(word + p);
            const long pp = bas_low(wp);
            if (pp == p) continue;
            bas_store(word + v, bas_pack(pp, bas_clamp(bas_o(w, 0) + bas_o(wp, 0), over), bas_clamp(bas_o(w, 1) + bas_o(wp, 1), over),
                                         bas_clamp(bas_o(w, 2) + bas_o(wp, 2), over)));
            changed = 1;
        }
        ++rounds;
        if (!__syncthreads_or(changed)) break;                       // (reduced over the workgroup: uniform)
    }

    // (3) the numbering: the roots of every row, the rows before a row, a root's number
    for (int r = wave; r < rows; r += BAS_WAVES) {                       // (the rows of the wave)
        const long v = (long)r * nx + lane;
        const bool root = lane < nx && word[v] != BAS_NONE && bas_low(word[v]) == v;
        const u64 m = __ballot(root);
        if (lane == 0) S.row_count[r] = cavity_popcount(m);
    }
    __syncthreads();
    if (wave == 0) {
        int mine = 0;
        for (int q = 0; q < 64; ++q) {                                   // (the 64 rows of the lane)
            const int r = lane * 64 + q;
            mine += r < rows ? S.row_count[r] : 0;
        }
        int incl = mine;
        for (int s = 1; s < 64; s <<= 1) {
            const int other = __shfl_up(incl, s);
            incl += lane >= s ? other : 0;
        }
        int before = incl - mine;
        for (int q = 0; q < 64; ++q) {
            const int r = lane * 64 + q;
            if (r >= rows) break;
            const int count = S.row_count[r];
            S.row_count[r] = before;
            before += count;
        }
        if (lane == 63) S.B = incl;
    }
    __syncthreads();
    const int B = S.B;
    const long b_cap = D.b_cap;
    for (int r = wave; r < rows; r += BAS_WAVES) {                       // (the rows of the wave)
        const long v = (long)r * nx + lane;
        const bool root = lane < nx && word[v] != BAS_NONE && bas_low(word[v]) == v;
        const u64 m = __ballot(root);
        if (!root) continue;
        const int id = S.row_count[r] + cavity_popcount(m & ((1ull << lane) - 1ull));
        word[v] = BAS_NUMBERED | bas_pack(id, 0, 0, 0);
        if (id < b_cap) {
            pw_basins_basin& R = basins[id];
            R.root = v;
            R.n_voxels = 1;
            R.u_min = pw_bits2d(map[v]);
            for (int b = 0; b < BAS_MAX_BETAS; ++b) R.z[b] = R.e[b] = 0.0;
        }
    }
    __syncthreads();
    for (long v = tid; v < V; v += BAS_THREADS) {                        // (the voxels: a root's word does not change here)
        const u64 w = word[v];
        if (w == BAS_NONE || (w & BAS_NUMBERED)) continue;
        const long id = bas_low(word[bas_low(w)]);
        word[v] = BAS_NUMBERED | (w & ~0xffffffffull) | (u64)id;
        int o[3] = {bas_o(w, 0), bas_o(w, 1), bas_o(w, 2)};
        over = over || !bas_in_range(o);
        if (id < b_cap) atomicAdd((unsigned long long*)&basins[id].n_voxels, 1ull);
    }
    if (over) atomicOr(&S.flags, BAS_RANGE);
    __syncthreads();
    bool range = (S.flags & BAS_RANGE) != 0;
    if (labels) {
        for (long v = tid; v < V; v += BAS_THREADS) {                    // (the voxels)
            const u64 w = word[v];
            pw_basins_label Q;
            Q.basin = w == BAS_NONE ? -1 : (int)bas_low(w);
            for (int k = 0; k < 3; ++k) Q.o[k] = w == BAS_NONE || range ? 0 : bas_o(w, k);
            labels[v] = Q;
        }
    }

    // (4) the basins' sums: wave s owns the sum s of every basin and takes the rows in order
    for (int s = wave; s < 2 * L; s += BAS_WAVES) {                      // (at most two sums a wave)
        const int b = s >> 1, kind = s & 1;
        const double beta = D.betas[b];
        bool clamped = false;
        for (int r = 0; r < rows; ++r) {                                 // (the rows in order)
            const long v = (long)r * nx + lane;
            const u64 w = lane < nx ? word[v] : BAS_NONE;
            const bool ok = w != BAS_NONE;
            if (!__ballot(ok)) continue;
            const double U = ok ? pw_bits2d(map[v]) : 0.0;
            bool hot = false;
            const double wt = aff_weight(beta, U, s_tab, hot);
            clamped = clamped || (ok && hot);
            const double term = kind ? wt * U : wt;
            const int id = ok ? (int)bas_low(w) : -1;
            u64 live = __ballot(ok && id < b_cap);
            while (live) {                                               // (at most 64 basins a row: a turn strikes one off)
                const int lid = __shfl(id, __ffsll((long long)live) - 1);
                const bool member = ok && id == lid;
                const double sum = bas_tree(member ? term : 0.0);
                if (lane == 0) {
                    double* total = kind ? &basins[lid].e[b] : &basins[lid].z[b];
                    *total = *total + sum;
                }
                live &= ~__ballot(member);
            }
        }
        if (__ballot(clamped) && lane == 0) atomicOr(&S.flags, BAS_CLAMPED);
    }

    // (5) the edges.  The table is cleared whatever follows, so that what is read was written
    for (long t = tid; t < D.table_slots; t += BAS_THREADS) table[t] = BAS_NONE;   // (the slots)
    __syncthreads();
    range = (S.flags & BAS_RANGE) != 0;
    long n_boundary = 0;
    if (!range) {                                                    // (read after a barrier: uniform)
        const int shift = 64 - (__ffsll((long long)D.table_slots) - 1);
        const u64 mask = (u64)D.table_slots - 1;
        unsigned long long fresh = 0;
        bool wide = false;
        for (long f = tid; f < 3 * V; f += BAS_THREADS) {                // (the faces: f = k V + v)
            const int k = (int)(f / V);
            u64 key;
            double term;
            bool in_range;
            if (!bas_face(map, word, f - k * V, k, nx, ny, nz, key, term, in_range)) continue;
            ++n_boundary;
            if (!in_range) {
                wide = true;
                continue;
            }
            u64 h = shift < 64 ? (key * 0x9E3779B97F4A7C15ull) >> shift : 0;
            for (long probe = 0; probe < D.table_slots; ++probe) {       // (the slots: more than the distinct keys)
                const u64 old = atomicCAS((unsigned long long*)&table[h], BAS_NONE, key);
                if (old == BAS_NONE) ++fresh;
                if (old == BAS_NONE || old == key) break;
                h = (h + 1) & mask;
            }
        }
        if (fresh) atomicAdd(&S.n_edges, fresh);
        if (n_boundary) atomicAdd(&S.n_boundary, (unsigned long long)n_boundary);
        if (wide) atomicOr(&S.flags, BAS_RANGE);
    }
    __syncthreads();
    range = (S.flags & BAS_RANGE) != 0;
    const long E = range ? 0 : (long)S.n_edges;
    const bool overflow = B > b_cap || E > D.e_cap;
    const bool write_edges = !range && !overflow && E > 0;
    if (write_edges) {                                               // (uniform)
        long slots = 1;
        while (slots < E) slots <<= 1;                               // (at most 20 doublings: E <= 3 V < 2^20)
        for (long t = tid; t < slots; t += BAS_THREADS) list[t] = BAS_NONE;
        __syncthreads();
        for (long t = tid; t < D.table_slots; t += BAS_THREADS) {        // (the slots)
            const u64 key = table[t];
            if (key != BAS_NONE) list[atomicAdd(&S.list_fill, 1u)] = key;
        }
        __syncthreads();
        // a bitonic network over `slots` keys, BAS_NONE behind the last: log2(slots) (log2(slots) + 1) / 2 <= 210 passes
        for (long size = 2; size <= slots; size <<= 1) {
            for (long stride = size >> 1; stride > 0; stride >>= 1) {
                for (long t = tid; t < slots / 2; t += BAS_THREADS) {
                    const long i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const u64 a = list[i], b = list[j];
                    if ((a > b) == ((i & size) == 0)) {
                        list[i] = b;
                        list[j] = a;
                    }
                }
                __syncthreads();
            }
        }
        for (long e = tid; e < E; e += BAS_THREADS) {                    // (the edges)
            pw_basins_edge& R = edges[e];
            bas_edge_unkey(list[e], R.a, R.b, R.d);
            R.saddle_k = 0;
            R.n_faces = 0;
            R.saddle_voxel = BAS_NO_RANK;                            // (first the lowest 4 v + k among the saddle's ties)
            *(u64*)&R.saddle = PAS_KEY_NONE;                         // (first the saddle's key)
            for (int b = 0; b < BAS_MAX_BETAS; ++b) R.s[b][0] = R.s[b][1] = R.s[b][2] = 0.0;
        }
        __syncthreads();
        for (long f = tid; f < 3 * V; f += BAS_THREADS) {                // (the faces)
            const int k = (int)(f / V);
            u64 key;
            double term;
            bool in_range;
            int e = -1;
            if (bas_face(map, word, f - k * V, k, nx, ny, nz, key, term, in_range)) {
                long lo = 0, hi = E;                                 // list[lo] <= key < list[hi]: at most 20 halvings
                while (hi - lo > 1) {
                    const long mid = (lo + hi) >> 1;
                    if (list[mid] <= key) lo = mid; else hi = mid;
                }
                e = (int)lo;
                atomicAdd((unsigned long long*)&edges[e].n_faces, 1ull);
                atomicMin((unsigned long long*)&edges[e].saddle, pas_key(term));
            }
            face_edge[f] = e;
        }
        __syncthreads();
        for (long f = tid; f < 3 * V; f += BAS_THREADS) {                // (the faces)
            const int e = face_edge[f];
            if (e < 0) continue;
            const int k = (int)(f / V);
            u64 key;
            double term;
            bool in_range;
            bas_face(map, word, f - k * V, k, nx, ny, nz, key, term, in_range);
            if (pas_key(term) == *(const u64*)&edges[e].saddle)
                atomicMin((unsigned long long*)&edges[e].saddle_voxel, (unsigned long long)(4 * (f - k * V) + k));
        }
        __syncthreads();
        for (long f = tid; f < 3 * V; f += BAS_THREADS) {                // (the faces: one of an edge's is its saddle's)
            const int e = face_edge[f];
            if (e < 0) continue;
            const int k = (int)(f / V);
            if (edges[e].saddle_voxel != 4 * (f - k * V) + k) continue;
            u64 key;
            double term;
            bool in_range;
            bas_face(map, word, f - k * V, k, nx, ny, nz, key, term, in_range);
            edges[e].saddle = term;
        }
        __syncthreads();
        for (long e = tid; e < E; e += BAS_THREADS) {                    // (the edges)
            const long vk = edges[e].saddle_voxel;
            edges[e].saddle_voxel = vk >> 2;
            edges[e].saddle_k = (int)(vk & 3);
        }
        // the edges' sums: wave s owns the sum s = 3 beta + k of every edge and takes the rows in order
        for (int s = wave; s < 3 * L; s += BAS_WAVES) {                  // (at most three sums a wave)
            const int b = s / 3, k = s - 3 * b;
            const double beta = D.betas[b];
            for (int r = 0; r < rows; ++r) {                             // (the rows in order)
                const long v = (long)r * nx + lane;
                const int e = lane < nx ? face_edge[k * V + v] : -1;
                u64 live = __ballot(e >= 0);
                if (!live) continue;
                double term = 0.0;
                if (e >= 0) {
                    u64 key;
                    bool in_range;
                    bas_face(map, word, v, k, nx, ny, nz, key, term, in_range);
                }
                bool hot = false;
                const double wt = aff_weight(beta, term, s_tab, hot);
                while (live) {                                           // (at most 64 edges a row: a turn strikes one off)
                    const int le = __shfl(e, __ffsll((long long)live) - 1);
                    const bool member = e == le;
                    const double sum = bas_tree(member ? wt : 0.0);
                    if (lane == 0) edges[le].s[b][k] = edges[le].s[b][k] + sum;
                    live &= ~__ballot(member);
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        pw_basins_out& O = out[blockIdx.x];
        O.n_basins = B;
        O.n_edges = E;
        O.n_basins_written = B < b_cap ? B : b_cap;
        O.n_edges_written = write_edges ? E : 0;
        O.n_blocked = blocked;
        O.n_allowed = allowed;
        const bool some = wr != BAS_NO_RANK;
        O.u_min = some ? pw_bits2d(map[wr]) : aff_inf();
        const long row = some ? wr / nx : 0;
        O.u_min_voxel[0] = some ? (int)(wr - row * nx) : -1;
        O.u_min_voxel[1] = some ? (int)(row % ny) : -1;
        O.u_min_voxel[2] = some ? (int)(row / ny) : -1;
        O.flags = (S.flags & (BAS_RANGE | BAS_CLAMPED)) | (overflow ? BAS_OVERFLOW : 0);
        diag[2 * blockIdx.x] = rounds;
        diag[2 * blockIdx.x + 1] = (int)S.n_boundary;
    }
}

const char* const ENTRY = "pw_basins";
int bas_bad(long k, const char* what) { return stat_bad(ENTRY, k, what); }

inline long bas_voxels(const pw_basins_job& J) { return (long)J.nx * J.ny * J.nz; }

// Everything is checked before anything is launched or written
int bas_check(const pw_basins_job* jobs, long n_jobs, const double* xyz, long n_points, const double* coef, long n_coef,
              const double* field, long n_field, const double* map, long n_map, const pw_basins_basin* basins, long n_basins,
              const pw_basins_edge* edges, long n_edges, const pw_basins_label* labels, long n_labels, long n_out) {
    for (long k = 0; k < n_jobs; ++k) {
        const pw_basins_job& J = jobs[k];
        GRID_CHECK(grid_dims_check(ENTRY, k, J.nx, J.ny, J.nz));
        const long V = bas_voxels(J);
        const bool lj = J.field_first == -1;
        if (J.n < 0) return bas_bad(k, "a negative count");
        if (lj && span_outside(J.atom_first, J.n, n_points)) return bas_bad(k, "atoms outside xyz");
        if (lj && span_outside(J.coef_first, J.n, n_coef)) return bas_bad(k, "coefficients outside coef");
        if (J.field_first < -1 || (!lj && span_outside(J.field_first, V, n_field))) return bas_bad(k, "the field is outside its array");
        if (J.map_first < -1 || (J.map_first >= 0 && span_outside(J.map_first, V, n_map))) return bas_bad(k, "the map is outside its array");
        if (J.b_cap < 0 || J.e_cap < 0) return bas_bad(k, "a negative capacity");
        if (span_outside(J.basin_first, J.b_cap, n_basins)) return bas_bad(k, "the rows are outside basins");
        if (span_outside(J.edge_first, J.e_cap, n_edges)) return bas_bad(k, "the rows are outside edges");
        if (J.label_first < -1 || (J.label_first >= 0 && span_outside(J.label_first, V, n_labels)))
            return bas_bad(k, "the labels are outside their array");
        if (span_outside(J.out, 1, n_out)) return bas_bad(k, "the row is outside out");
        if ((lj && J.n && (!xyz || !coef)) || (!lj && !field) || (J.map_first >= 0 && !map) || (J.b_cap && !basins) ||
            (J.e_cap && !edges) || (J.label_first >= 0 && !labels))
            return bas_bad(k, "null array");
        bool finite = true;
        for (int a = 0; a < 3; ++a) finite = finite && pw_finite(J.origin[a]);
        for (int a = 0; a < 6; ++a) finite = finite && pw_finite(J.step[a]);
        if (!finite) return bas_bad(k, "the origin or a step is not finite");
        if (!(J.step[0] > 0.0 && J.step[2] > 0.0 && J.step[5] > 0.0)) return bas_bad(k, "ax, by or cz <= 0");
        GRID_CHECK(grid_n_betas_check(ENTRY, k, J.n_betas));
        for (int b = 0; b < J.n_betas; ++b)
            if (!pw_finite(J.betas[b]) || !(J.betas[b] > 0.0)) return bas_bad(k, "a beta is not positive or not finite");
        if (!pas_value_ok(J.cap)) return bas_bad(k, "the cap is -inf or not a number");
        if (!lj) {
            GRID_CHECK(grid_field_check(ENTRY, k, field, J.field_first, V));
            continue;
        }
        GRID_CHECK(grid_core_check(ENTRY, k, J.core2, J.cutoff2));
        for (long a = 0; a < J.n; ++a) {                             // (atom by atom: its coordinates, then its row)
            GRID_CHECK(grid_xyz_check(ENTRY, k, xyz, J.atom_first + a, 1));
            GRID_CHECK(grid_coef_check(ENTRY, k, coef, J.coef_first + a, 1, 2, false));
        }
    }
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares its row of out with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].out, 1}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of basins with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].basin_first, (long)jobs[k].b_cap}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares rows of edges with an earlier job",
                             [&](long k) { return OutSpan{(long)jobs[k].edge_first, (long)jobs[k].e_cap}; }));
    GRID_CHECK(shared_output(ENTRY, n_jobs, "shares labels with an earlier job", [&](long k) {
        return OutSpan{(long)jobs[k].label_first, jobs[k].label_first >= 0 ? bas_voxels(jobs[k]) : 0};
    }));
    return shared_output(ENTRY, n_jobs, "shares entries of map with an earlier job", [&](long k) {
        return OutSpan{(long)jobs[k].map_first, jobs[k].map_first >= 0 ? bas_voxels(jobs[k]) : 0};
    });
}

// workspace_bytes: the budget of the workspaces of the jobs of one launch (0: BAS_WORKSPACE_BYTES; at 1 every job is a
// launch of its own); kernel_ms: when not null, the time of the device work of the call from the first launch to the last,
// the copies between them included, by HIP events on the context's stream; n_rounds, n_faces: when not null, n_jobs
// integers, job k's rounds of pointer jumping and boundary faces (diagnostic: the rounds differ between the paths)
int basins_call(pw_context* ctx, const pw_basins_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points, const double* coef,
                int64_t n_coef, const double* field, int64_t n_field, double* map, int64_t n_map, pw_basins_basin* basins,
                int64_t n_basins, pw_basins_edge* edges, int64_t n_edges, pw_basins_label* labels, int64_t n_labels,
                pw_basins_out* out, int64_t n_out, int64_t workspace_bytes, float* kernel_ms, int32_t* n_rounds, int32_t* n_faces) {
    if (!ctx || n_jobs < 0 || n_jobs > 0x7ffffff0 || (n_jobs && (!jobs || !out)) || n_points < 0 || n_coef < 0 || n_field < 0 ||
        n_map < 0 || n_basins < 0 || n_edges < 0 || n_labels < 0 || n_out < 0 || workspace_bytes < 0)
        return PW_E_BAD_ARG;
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n_jobs == 0) return PW_OK;
    PW_LOCK_CONTEXT(ctx);
    const long N = (long)n_jobs;
    const int rc = bas_check(jobs, N, xyz, (long)n_points, coef, (long)n_coef, field, (long)n_field, map, (long)n_map, basins,
                             (long)n_basins, edges, (long)n_edges, labels, (long)n_labels, (long)n_out);
    if (rc != PW_OK) return rc;
    if (pw_context_device(ctx) < 0)
        return pw_hostpath_basins(jobs, N, xyz, coef, field, map, basins, edges, labels, out, n_rounds, n_faces,
                                  pw_context_host_threads(ctx, 0));

    // the spans of the arrays that the jobs read, and the plan: jobs in order, gathered into launches while their
    // workspaces fit the budget
    const long budget_words = (workspace_bytes ? (long)workspace_bytes : BAS_WORKSPACE_BYTES) / 8;
    Span atoms, rows_ab;
    for (long k = 0; k < N; ++k) {
        if (jobs[k].field_first != -1) continue;
        atoms.widen((long)jobs[k].atom_first, (long)jobs[k].n);
        rows_ab.widen((long)jobs[k].coef_first, (long)jobs[k].n);
    }
    std::vector<BasJobDev> devs((size_t)N);
    std::vector<LaunchGroup> groups;
    LaunchGroup cur;
    for (long k = 0; k < N; ++k) {
        const pw_basins_job& J = jobs[k];
        const long V = bas_voxels(J);
        const bool lj = J.field_first == -1;
        BasJobDev& D = devs[k];
        D.b_cap = std::min((long)J.b_cap, V);                        // (B <= V and E <= 3 V: the same result)
        D.e_cap = std::min((long)J.e_cap, 3 * V);
        D.table_slots = 64;
        while (D.table_slots <= 3 * V) D.table_slots <<= 1;
        D.list_slots = 1;
        while (D.list_slots < D.e_cap) D.list_slots <<= 1;
        const long words = 2 * V + D.table_slots + D.list_slots + (3 * V + 1) / 2 + BAS_BASIN_WORDS * D.b_cap +
                           BAS_EDGE_WORDS * D.e_cap + (J.label_first >= 0 ? BAS_LABEL_WORDS * V : 0);
        place(groups, cur, budget_words, words);
        long at = cur.words;
        auto take = [&](long count) {
            const long first = at;
            at += count;
            return first;
        };
        D.n = lj ? (long)J.n : 0;
        D.atom_first = atoms.rel((long)J.atom_first, D.n);
        D.coef_first = rows_ab.rel((long)J.coef_first, D.n);
        D.map_first = take(V);
        D.word_first = take(V);
        D.table_first = take(D.table_slots);
        D.list_first = take(D.list_slots);
        D.face_first = take((3 * V + 1) / 2);
        D.basin_first = take(BAS_BASIN_WORDS * D.b_cap);
        D.edge_first = take(BAS_EDGE_WORDS * D.e_cap);
        D.label_first = J.label_first >= 0 ? take(BAS_LABEL_WORDS * V) : -1;
        D.item_first = cur.items;
        D.chunks = lj ? (V + AFF_CHUNK - 1) / AFF_CHUNK : 0;
        D.V = V;
        for (int a = 0; a < 3; ++a) D.o[a] = J.origin[a];
        for (int a = 0; a < 6; ++a) D.s[a] = J.step[a];
        for (int b = 0; b < BAS_MAX_BETAS; ++b) D.betas[b] = b < J.n_betas ? J.betas[b] : 0.0;
        D.core2 = J.core2; D.cutoff2 = J.cutoff2; D.cap_key = pas_key(J.cap);
        D.nx = J.nx; D.ny = J.ny; D.nz = J.nz; D.L = J.n_betas;
        cur.words = at; cur.cost += words; cur.items += D.chunks; cur.blocks += 1; cur.last += 1;
    }
    groups.push_back(cur);

    const size_t ws_bytes = sizeof(u64) * (size_t)most_words(groups), out_bytes = sizeof(pw_basins_out) * (size_t)N,
                 diag_bytes = sizeof(int) * 2 * (size_t)N;
    std::vector<pw_basins_out> res_out((size_t)N);
    std::vector<int> res_diag(2 * (size_t)N);

    DeviceScope dev_scope_;
    STAT_TRY(dev_scope_.enter(pw_context_device(ctx)));
    hipStream_t st = (hipStream_t)pw_context_stream(ctx);
    Events ev(kernel_ms);
    STAT_TRY(ev.create());
    {
        StreamBuffers buf(st);
        BasJobDev* d_jobs;
        double *d_xyz, *d_coef;
        u64* d_ws;
        pw_basins_out* d_out;
        int* d_diag;
        STAT_TRY(buf.alloc(&d_jobs, sizeof(BasJobDev) * (size_t)N));
        STAT_TRY(hipMemcpyAsync(d_jobs, devs.data(), sizeof(BasJobDev) * (size_t)N, hipMemcpyHostToDevice, st));
        STAT_TRY(atoms.upload(buf, &d_xyz, xyz, 3));
        STAT_TRY(rows_ab.upload(buf, &d_coef, coef, 2));
        STAT_TRY(buf.alloc(&d_ws, ws_bytes));
        STAT_TRY(buf.alloc(&d_out, out_bytes));
        STAT_TRY(buf.alloc(&d_diag, diag_bytes));
        const bool poison = scratch_poisoned();                      // (test hook, pw_stat_host.hpp)
        STAT_TRY(poison_scratch(poison, d_ws, ws_bytes, st));
        STAT_TRY(poison_scratch(poison, d_out, out_bytes, st));
        STAT_TRY(poison_scratch(poison, d_diag, diag_bytes, st));
        STAT_TRY(ev.start(st));
        // (a group's rows are read back before the next group takes the workspace over: what a job wrote is known only
        // from its row of out)
        for (const LaunchGroup& G : groups) {
            const unsigned n_group = (unsigned)(G.last - G.first);
            for (long k = G.first; k < G.last; ++k)
                if (jobs[k].field_first >= 0)
                    STAT_TRY(hipMemcpyAsync(d_ws + devs[k].map_first, field + jobs[k].field_first, sizeof(double) * (size_t)devs[k].V,
                                            hipMemcpyHostToDevice, st));
            if (G.items) {
                const long blocks = launch_blocks(G.items, 65536);
                hipLaunchKernelGGL(pw_basins_field_kernel, dim3((unsigned)blocks), dim3(AFF_CHUNK), 0, st, d_jobs + G.first,
                                   (int)n_group, G.items, d_xyz, d_coef, d_ws);
                STAT_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(pw_basins_kernel, dim3(n_group), dim3(BAS_THREADS), 0, st, d_jobs + G.first, d_ws, d_out + G.first,
                               d_diag + 2 * G.first);
            STAT_TRY(hipGetLastError());
            STAT_TRY(hipMemcpyAsync(res_out.data() + G.first, d_out + G.first, sizeof(pw_basins_out) * n_group, hipMemcpyDeviceToHost, st));
            STAT_TRY(hipStreamSynchronize(st));
            for (long k = G.first; k < G.last; ++k) {
                const pw_basins_job& J = jobs[k];
                const BasJobDev& D = devs[k];
                const pw_basins_out& O = res_out[(size_t)k];
                if (O.n_basins_written)
                    STAT_TRY(hipMemcpyAsync(basins + J.basin_first, d_ws + D.basin_first, sizeof(pw_basins_basin) * (size_t)O.n_basins_written,
                                            hipMemcpyDeviceToHost, st));
                if (O.n_edges_written)
                    STAT_TRY(hipMemcpyAsync(edges + J.edge_first, d_ws + D.edge_first, sizeof(pw_basins_edge) * (size_t)O.n_edges_written,
                                            hipMemcpyDeviceToHost, st));
                if (J.label_first >= 0)
                    STAT_TRY(hipMemcpyAsync(labels + J.label_first, d_ws + D.label_first, sizeof(pw_basins_label) * (size_t)D.V,
                                            hipMemcpyDeviceToHost, st));
                if (J.map_first >= 0)
                    STAT_TRY(hipMemcpyAsync(map + J.map_first, d_ws + D.map_first, sizeof(double) * (size_t)D.V, hipMemcpyDeviceToHost, st));
            }
        }
        STAT_TRY(ev.stop(st));
        STAT_TRY(hipMemcpyAsync(res_diag.data(), d_diag, diag_bytes, hipMemcpyDeviceToHost, st));
    }
    STAT_TRY(hipStreamSynchronize(st));
    STAT_TRY(ev.read());
    for (long k = 0; k < N; ++k) {
        out[jobs[k].out] = res_out[(size_t)k];
        if (n_rounds) n_rounds[k] = res_diag[2 * (size_t)k];
        if (n_faces) n_faces[k] = res_diag[2 * (size_t)k + 1];
    }
    return PW_OK;
}

}  // namespace

extern "C" int pw_basins(pw_context* ctx, const pw_basins_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                         const double* coef, int64_t n_coef, const double* field, int64_t n_field, double* map, int64_t n_map,
                         pw_basins_basin* basins, int64_t n_basins, pw_basins_edge* edges, int64_t n_edges, pw_basins_label* labels,
                         int64_t n_labels, pw_basins_out* out, int64_t n_out) {
    return basins_call(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, field, n_field, map, n_map, basins, n_basins, edges, n_edges,
                       labels, n_labels, out, n_out, 0, nullptr, nullptr, nullptr);
}

// measurement and test hook (not part of the header): pw_basins with the budget of the workspace of a launch given (0:
// the default; the result may not depend on it), the device work timed by HIP events when kernel_ms is not null, and per
// job the rounds of pointer jumping and the boundary faces in n_rounds[0 .. n_jobs) and n_faces[0 .. n_jobs) when those
// are not null -- diagnostic, not part of the defined bytes
extern "C" int pw_internal_basins(pw_context* ctx, const pw_basins_job* jobs, int64_t n_jobs, const double* xyz, int64_t n_points,
                                  const double* coef, int64_t n_coef, const double* field, int64_t n_field, double* map,
                                  int64_t n_map, pw_basins_basin* basins, int64_t n_basins, pw_basins_edge* edges, int64_t n_edges,
                                  pw_basins_label* labels, int64_t n_labels, pw_basins_out* out, int64_t n_out,
                                  int64_t workspace_bytes, float* kernel_ms, int32_t* n_rounds, int32_t* n_faces) {
    return basins_call(ctx, jobs, n_jobs, xyz, n_points, coef, n_coef, field, n_field, map, n_map, basins, n_basins, edges, n_edges,
                       labels, n_labels, out, n_out, workspace_bytes, kernel_ms, n_rounds, n_faces);
}
