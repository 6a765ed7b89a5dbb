// grid_plan_check.cpp -- the planner of the grid entries (pywindow_amd/csrc/pw_grid_host.hpp: LaunchGroup, place, Span,
// span_outside) in a stand-alone program on the CPU; in the library it runs only on the device path.  Built with the
// sanitizers and run without arguments, it prints one line and returns 0 when every check holds:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include tests/tools/grid_plan_check/grid_plan_check.cpp -o grid_plan_check && ./grid_plan_check
// (the HIP headers are only read for their types; nothing of HIP is called or linked.)
//
// The three ways the entries account for a job of `c` words, over costs 0 .. 5, three and four jobs and every budget
// from 1 to the total + 5:
//   A  pw_affinity, pw_rigid_affinity   charge c + 1, advance the words by c + 1
//   B  pw_cavity, pw_pore_sizes         charge c + 1, advance the words by c
//   C  pw_passage, pw_hop               charge c, advance the words by c
// Checked: the groups partition [0, N) in order and none is empty; a group of more than one job is within the budget;
// the offsets handed out inside a group follow one another without overlap and end at the group's words; the
// boundaries are those of the rule as each entry wrote it out before the header (restated below with plain integers);
// most_words is the largest group.  Span over every mix of up to three members (first 0 .. 3, count 0 .. 2) is the
// minimum and maximum of the members that have entries, or (0, 0); span_outside is its definition.
// launch_blocks (pw_stat_host.hpp, the grid of a capped launch) at 0, 1, cap - 1, cap and cap + 1 items for the caps of the
// launch sites (65536 and 2^20) and a small one: min(items, cap) with the test hook off, min(items, hook) with it at 1 and
// 3, the site's cap again after 0; the hook returns exactly the number of calls that got fewer workgroups than items
// since it was last called, and clears it.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../../pywindow_amd/csrc/pw_grid_host.hpp"

extern "C" char* pw_internal_error_buffer(void) {
    static char buffer[512];
    return buffer;
}

using namespace pw;

static long g_checks = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// the first job of every group by the rule as the entries had it: style A and C compared the words, style B a cost of
// its own
static std::vector<long> boundaries_before(char style, const std::vector<long>& c, long budget) {
    std::vector<long> firsts{0};
    long first = 0, used = 0;
    for (long k = 0; k < (long)c.size(); ++k) {
        const long charge = style == 'C' ? c[k] : c[k] + 1;
        if (k > first && used + charge > budget) {
            firsts.push_back(k);
            first = k;
            used = 0;
        }
        used += charge;
    }
    return firsts;
}

static void plan(char style, const std::vector<long>& c, long budget) {
    const long N = (long)c.size();
    std::vector<LaunchGroup> groups;
    std::vector<long> offset((size_t)N), advance((size_t)N);
    LaunchGroup cur;
    for (long k = 0; k < N; ++k) {
        const long charge = style == 'C' ? c[k] : c[k] + 1;
        place(groups, cur, budget, charge);
        offset[k] = cur.words;
        advance[k] = style == 'A' ? c[k] + 1 : c[k];
        cur.words += advance[k]; cur.cost += charge; cur.items += 1; cur.last += 1;
    }
    groups.push_back(cur);

    const std::vector<long> firsts = boundaries_before(style, c, budget);
    CHECK(groups.size() == firsts.size());
    long next = 0, most = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const LaunchGroup& G = groups[g];
        CHECK(G.first == next && G.first == firsts[g]);
        CHECK(G.last > G.first);
        CHECK(G.last - G.first == 1 || G.cost <= budget);
        CHECK(G.items == G.last - G.first && G.blocks == 0 && G.rows == 0);
        long at = 0;
        for (long k = G.first; k < G.last; ++k) {
            CHECK(offset[k] == at);
            at += advance[k];
        }
        CHECK(at == G.words);
        most = G.words > most ? G.words : most;
        next = G.last;
    }
    CHECK(next == N);
    CHECK(most_words(groups) == most);
}

static void plans() {
    for (int N = 3; N <= 4; ++N) {
        std::vector<long> c((size_t)N, 0);
        for (;;) {
            long total = 0;
            for (long v : c) total += v;
            for (const char style : {'A', 'B', 'C'})
                for (long budget = 1; budget <= total + 5; ++budget) plan(style, c, budget);
            int q = 0;
            while (q < N && ++c[q] > 5) c[q++] = 0;
            if (q == N) break;
        }
    }
}

static void spans() {
    for (int members = 1; members <= 3; ++members) {
        std::vector<long> m((size_t)members, 0);                     // a member is first * 3 + count
        for (;;) {
            Span s;
            long lo = LONG_MAX, hi = 0;
            for (long v : m) {
                const long first = v / 3, count = v % 3;
                s.widen(first, count);
                if (count) {
                    lo = first < lo ? first : lo;
                    hi = first + count > hi ? first + count : hi;
                }
            }
            if (lo == LONG_MAX) {
                CHECK(s.lo_or_zero() == 0 && s.count() == 0 && s.lo < 0);
            } else {
                CHECK(s.lo == lo && s.lo_or_zero() == lo && s.hi == hi && s.count() == hi - lo);
                for (long v : m) CHECK(s.rel(v / 3, v % 3) == (v % 3 ? v / 3 - lo : 0));
            }
            int q = 0;
            while (q < members && ++m[q] > 11) m[q++] = 0;
            if (q == members) break;
        }
    }
}

static void ranges() {
    for (long limit = 0; limit <= 5; ++limit)
        for (long first = -2; first <= 7; ++first)
            for (long count = 0; count <= 7; ++count)
                CHECK(span_outside(first, count, limit) == (first < 0 || first + count > limit));
    CHECK(span_outside(LONG_MAX - 1, 5, LONG_MAX) && !span_outside(LONG_MAX - 5, 5, LONG_MAX));   // (no overflow on the way)
}

static void launches() {
    CHECK(launch_cap_hook(0) == 0);                                  // (off at start, nothing counted)
    for (const long hook : {0l, 1l, 3l, 0l})
        for (const long cap : {7l, 65536l, 1l << 20}) {
            CHECK(launch_cap_hook(hook) == 0);
            long cut = 0;
            for (const long items : {0l, 1l, cap - 1, cap, cap + 1}) {
                const long limit = hook > 0 ? hook : cap, want = items < limit ? items : limit;
                CHECK(launch_blocks(items, cap) == want);
                cut += want < items;
            }
            CHECK(cut == (hook > 0 ? 3 : 1));                        // (cap - 1, cap, cap + 1 under the hook; cap + 1 without)
            CHECK(launch_cap_hook(hook) == cut);
            CHECK(launch_cap_hook(hook) == 0);                       // (the count was cleared)
        }
    CHECK(launch_cap_hook(-5) == 0 && launch_blocks(10, 4) == 4 && launch_cap_hook(0) == 1);   // (a negative value is 0)
}

int main() {
    plans();
    spans();
    ranges();
    launches();
    printf("grid_plan_check: %ld checks hold\n", g_checks);
    return 0;
}
