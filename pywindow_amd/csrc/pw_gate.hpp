// pw_gate.hpp -- gating statistics of a series against many thresholds (include/pywindow_amd.h: pw_gate_counts),
// single source for the gfx950 kernels (pw_gate.hip) and the host path (pw_hostpath.cpp).  The reference has no
// counterpart: it says whether a guest fits through a window of one structure, never how often or for how long.
//
// DEFINED RESULT.  For a series a[0..n) and a threshold d every entry has a state -- OPEN a[t] >= d, CLOSED a[t] < d,
// GAP a[t] a NaN (recognised on the bits) -- and the series falls into maximal runs of equal state.  A run of a
// state other than GAP is tallied when it ends: its length, whether its LEFT neighbour is a run of the opposite
// state (an opening / a closing) and whether both neighbours are (a COMPLETE run: its true length is known; a run
// that touches a gap or an end of the series is censored).  Twelve integers a threshold (GATE_FIELDS, the order of
// the header) and, for the complete runs, a histogram of their lengths.
//
// Every output is an integer and every sum is of integers, so the result is the definition itself whatever the
// order of the work: the device, the launch geometry, how the thresholds are cut into slabs to bound the workspace,
// the thread count of the host path, the run.  Both paths cut the time axis into chunks of GATE_CHUNK entries:
// gate_chunk walks one chunk for one threshold, tallies the runs that lie strictly inside it -- both neighbours
// are in sight -- and returns a SUMMARY of the chunk's first and last run; gate_merge takes the summaries of a
// threshold in chunk order and tallies the runs that touch or cross chunk boundaries.
#pragma once
#include "pw_common.hpp"

namespace pw {

constexpr int GATE_CHUNK = 512;          // entries of one chunk of the time axis (one summary a threshold)
constexpr int GATE_TILE = 256;           // thresholds of one workgroup, one a lane
constexpr int GATE_FIELDS = 12;
constexpr long GATE_WORKSPACE_BYTES = 64l << 20;   // summaries of one launch pair (pw_gate.hip: gate_plan)
constexpr long GATE_MAX = 1l << 31;      // largest n

// states: two bits each in a summary; x ^ y == 1 says "opposite" whenever one of the two is OPEN or CLOSED
constexpr unsigned GATE_CLOSED = 0, GATE_OPEN = 1, GATE_GAP = 2, GATE_NONE = 3;

// (an infinity never reaches this: the entry refuses it, so all ones in the exponent is a NaN)
PW_HD inline unsigned gate_state(double a, double d) {
    union { double d; unsigned long long u; } c;
    c.d = a;
    const bool gap = (c.u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
    return gap ? GATE_GAP : a >= d ? GATE_OPEN : GATE_CLOSED;
}

// the twelve counts of one threshold, in the order of the header; I: unsigned within a chunk, long beyond
template <class I>
struct GateTally {
    I n_open = 0, n_closed = 0, open_runs = 0, closed_runs = 0, longest_open = 0, longest_closed = 0;
    I openings = 0, closings = 0, complete_open_runs = 0, complete_closed_runs = 0;
    I complete_open_frames = 0, complete_closed_frames = 0;
};

// a run of `state` and `len` entries has ended; left / right: its neighbour there is a run of the opposite state.
// hist(s, len): one more complete run of that length, s = 0 open, 1 closed.  Selects, not indexed counters: the
// tally stays in registers.
template <class I, class Hist>
PW_HD inline void gate_close(GateTally<I>& T, unsigned state, I len, bool left, bool right, Hist&& hist) {
    if (state == GATE_GAP) return;
    const bool open = state == GATE_OPEN, both = left && right;
    const I o = open ? 1 : 0, c = open ? 0 : 1;
    T.n_open += open ? len : 0;
    T.n_closed += open ? 0 : len;
    T.open_runs += o;
    T.closed_runs += c;
    T.longest_open = open && len > T.longest_open ? len : T.longest_open;
    T.longest_closed = !open && len > T.longest_closed ? len : T.longest_closed;
    T.openings += left ? o : 0;
    T.closings += left ? c : 0;
    T.complete_open_runs += both ? o : 0;
    T.complete_closed_runs += both ? c : 0;
    T.complete_open_frames += both && open ? len : 0;
    T.complete_closed_frames += both && !open ? len : 0;
    if (both) hist(open ? 0 : 1, len);
}

// A chunk's summary, one 32-bit word: the state and length of its first and of its last run, the state of the run
// after the first (GATE_NONE: the chunk is a single run, first and last are the same) and of the run before the
// last (GATE_NONE likewise).  Neither run is tallied by gate_chunk: either may go on in the neighbouring chunk.
static_assert(GATE_CHUNK < 1024, "a run's length within a chunk takes ten bits");
PW_HD inline unsigned gate_pack(unsigned first, unsigned second, unsigned last, unsigned before, unsigned first_len,
                                unsigned last_len) {
    return first | second << 2 | last << 4 | before << 6 | first_len << 8 | last_len << 18;
}

// one chunk a[0..len), 1 <= len <= GATE_CHUNK, against d: the runs strictly inside go into T, the rest is the summary
template <class P, class I, class Hist>
PW_HD inline unsigned gate_chunk(P a, int len, double d, GateTally<I>& T, Hist&& hist) {
    unsigned cs = gate_state(a[0], d), prev = GATE_NONE;           // the current run and the one before it
    unsigned first = cs, second = GATE_NONE, first_len = 0, run = 1;
    for (int t = 1; t < len; ++t) {
        const unsigned s = gate_state(a[t], d);
        if (s != cs) {
            if (prev == GATE_NONE) {
                first_len = run;
                second = s;
            } else {
                gate_close(T, cs, (I)run, (prev ^ cs) == 1, (s ^ cs) == 1, hist);
            }
            prev = cs;
            cs = s;
            run = 0;
        }
        ++run;
    }
    if (prev == GATE_NONE) first_len = run;
    return gate_pack(first, second, cs, prev, first_len, run);
}

// the run that is open at the end of the chunks seen so far
struct GateWalk {
    unsigned state = GATE_NONE;
    long len = 0;
    bool left = false;
};

// the next chunk's summary: its first run continues the walk's run or ends it; when the chunk holds more than one
// run its first run ends inside it and its last run becomes the walk's.  On "x ^ y == 1": it is also true of
// GAP ^ NONE, so it says "opposite" only when one side is OPEN or CLOSED.  That holds wherever it is used here: as
// the `right` of a run it stands beside the run's own state, and gate_close drops a GAP run before it looks at
// left or right; as `left` it is kept for the run that `first` / `last` starts, which gate_close drops likewise
// when that state is a GAP, and `first`, `last` are never NONE (`before` is NONE only when `second` is, and is
// then not read).
template <class Hist>
PW_HD inline void gate_merge(GateWalk& W, unsigned summary, GateTally<long>& T, Hist&& hist) {
    const unsigned first = summary & 3, second = summary >> 2 & 3, last = summary >> 4 & 3, before = summary >> 6 & 3;
    const long first_len = summary >> 8 & 1023, last_len = summary >> 18 & 1023;
    if (W.state == first) {
        W.len += first_len;
    } else {
        if (W.state != GATE_NONE) gate_close(T, W.state, W.len, W.left, (first ^ W.state) == 1, hist);
        W.left = W.state != GATE_NONE && (W.state ^ first) == 1;
        W.state = first;
        W.len = first_len;
    }
    if (second != GATE_NONE) {
        gate_close(T, W.state, W.len, W.left, (second ^ W.state) == 1, hist);
        W.state = last;
        W.len = last_len;
        W.left = (before ^ last) == 1;
    }
}

// the end of the series: the walk's run is bounded by it on the right
template <class Hist>
PW_HD inline void gate_finish(GateWalk& W, GateTally<long>& T, Hist&& hist) {
    if (W.state != GATE_NONE) gate_close(T, W.state, W.len, W.left, false, hist);
    W = GateWalk{};
}

}  // namespace pw
