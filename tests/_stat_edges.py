"""Edge sweeps of the six statistical entries (pw_kde_sums, pw_kde2_sums, pw_kde_wsums, pw_corr_sums, pw_dft_sums,
pw_gate_counts), shared by tests/test_stat_edges.py (CPU: the coverage of every sweep is ASSERTED, and the host path
is held to exact references) and tests/test_gpu_stat_edges.py (device against host path and those references, with
the device scratch poisoned and after different work).

The device kernels of these entries are register tiles with no CPU twin: the host path is a plain loop over the same
pw_*.hpp definition and never runs a cut-short tile, an EDGE instantiation, a partial kernel's write guard or a
reduce kernel's chunk count.  So each entry gets ONE batch of the smallest jobs that reach every such path, and a
pure-Python restatement of the plan and of the kernels' branch conditions (`classes`) that says which paths a list
of shapes reaches; `all_classes` is the full set.  Both are computed from the constants of the sources (`constant`),
never from literals: a changed tile moves the sweep with it, or fails the comparison of the two sets."""
import contextlib
import ctypes
import functools
import re

import numpy as np

import _corr_cases as CO
import _dft_cases as DF
import _gate_cases as GA
import _kde2_cases as K2
import _kde_cases as K
import _kdew_cases as KW
from _util import ROOT

#: what the float outputs hold before a call where a test looks at entries nobody owns (gate: GA.SENTINEL)
SENTINEL = -77.0
#: integer-valued series stay within +-INT_RANGE: a lagged sum of 2000 products is below 2^32, a plain sum below 2^26
INT_RANGE = 1024


@functools.lru_cache(maxsize=None)
def constant(name: str, source: str) -> int:
    text = (ROOT / "pywindow_amd" / "csrc" / source).read_text()
    return int(re.search(rf"constexpr \w+ {name} = (\d+)", text).group(1))


def sizes(tile: int):
    """"The sizes for T": every size to 2 T + 1 for a small tile, both edges +-9 and 1, 2, 3 for a large one."""
    if tile <= 128:
        return list(range(1, 2 * tile + 2))
    near = [s for t in (tile, 2 * tile) for s in range(t - 9, t + 10)]
    return sorted(set([1, 2, 3] + near))


def tail(size: int, tile: int):
    """(tiles, entries of the last one) of `size` entries cut into tiles."""
    tiles = -(-size // tile)
    return tiles, size - (tiles - 1) * tile


def cross(dims, edge, interior):
    """Sparse crossing: every value of each dimension twice, with the others at their edge and at their interior
    value.  Shapes in a fixed order, without repeats."""
    out = []
    for d, values in enumerate(dims):
        for v in values:
            for other in (edge, interior):
                shape = tuple(v if i == d else other[i] for i in range(len(dims)))
                if shape not in out:
                    out.append(shape)
    return out


# ---- pw_corr_sums --------------------------------------------------------------------------------------------------
def corr_constants():
    c = lambda n: constant(n, "pw_corr.hpp")
    return c("CORR_CHUNK"), c("CORR_LANE_LAGS"), c("CORR_WAVE")


def corr_shapes():
    """(n, n_lags): every n to two chunks and three register steps with all its lags, and the lengths just above three
    chunks with all lags and with one lane beyond a tile."""
    C, R, W = corr_constants()
    shapes = [(n, n) for n in range(1, 2 * C + 3 * R + 1)]
    shapes += [(n, lags) for n in range(3 * C, 3 * C + R) for lags in (n, W * R + R)]
    return shapes


def corr_classes(shapes):
    """pw_corr_partial_kernel's paths at the default budget (one slab a job: lag_first = 0, m = n_lags)."""
    C, R, W = corr_constants()
    T = W * R
    lane = np.arange(W)
    got = set()
    for n, m in shapes:
        got.add(("n mod R", n % R))
        for tile in range(-(-m // T)):
            lag0 = tile * T
            if (m - lag0) % R and m - lag0 < T:
                got.add(("tile ends inside a lane", (m - lag0) % R))
            for chunk in range(-(-n // C)):
                t0 = chunk * C
                if t0 >= n - lag0:
                    got.add(("tile without a term", True))
                    continue
                edge = not t0 + C + lag0 + T - 1 <= n
                got.add(("EDGE", edge))
                if edge:
                    count = np.clip(n - (lag0 + lane * R) - t0, 0, C + R)
                    got.update(("count", int(c)) for c in np.unique(count))
    return got


def corr_all_classes():
    C, R, _ = corr_constants()
    return ({("n mod R", r) for r in range(R)} | {("tile ends inside a lane", r) for r in range(1, R)} |
            {("tile without a term", True), ("EDGE", True), ("EDGE", False)} | {("count", c) for c in range(C + R + 1)})


def _series(rng, n, kind, scale=1.0):
    if kind == "integer":
        return rng.integers(-INT_RANGE, INT_RANGE + 1, n).astype(np.float64)
    return rng.standard_normal(n) * scale


@functools.lru_cache(maxsize=None)
def corr_jobs(kind: str = "normal", seed: int = 0, reverse: bool = False):
    """_corr_cases jobs (a, b or None, n_lags) of corr_shapes(); every third one an autocorrelation."""
    rng = np.random.default_rng(1000 + seed)
    shapes = corr_shapes()[::-1][1:] if reverse else corr_shapes()
    jobs = []
    for k, (n, lags) in enumerate(shapes):
        a = _series(rng, n, kind, 1.0 + k % 7)
        jobs.append((a, None if k % 3 == 0 else _series(rng, n, kind), lags))
    return jobs


def corr_exact(jobs):
    """The lagged sums of integer-valued series in int64, one job after the other: exact, and far below 2^53."""
    out = []
    for a, b, lags in jobs:
        ai = a.astype(np.int64)
        bi = ai if b is None else b.astype(np.int64)
        assert (ai == a).all() and np.abs(ai).max() <= INT_RANGE and np.abs(bi).max() <= INT_RANGE
        n = len(ai)
        out.append(np.correlate(bi, ai, "full")[n - 1:n - 1 + lags])      # [n - 1 + k] = sum_t a[t] b[t + k]
    return np.concatenate(out)


# ---- pw_dft_sums ---------------------------------------------------------------------------------------------------
def dft_constants():
    c = lambda n: constant(n, "pw_dft.hpp")
    return {"C": c("DFT_CHUNK"), "W": c("DFT_WAVE"), "F": c("DFT_LANE_FREQS"), "WC": c("DFT_WAVE_CHUNKS"),
            "GW": c("DFT_GROUP_WAVES"), "RB": constant("DFT_RB", "pw_dft.hip"), "RED": constant("DFT_RED_CHUNKS", "pw_dft.hip")}


def dft_tile_freqs():
    k = dft_constants()
    T = k["W"] * k["F"]
    return (k["W"] - 1, k["W"], k["W"] + 1, T - 1, T, T + 1, 2 * T + 1)


def dft_last_lengths():
    k = dft_constants()
    return (1, 3, 6, k["C"] - 3, k["C"])


def dft_shapes():
    """(n, n_freq): every n to two chunks and two staged blocks with 3 frequencies; the tile edges of the frequencies
    on a handful of n; every chunk count to a workgroup's chunks and one more register tile, each with five lengths of
    the last chunk."""
    k = dft_constants()
    C = k["C"]
    shapes = [(n, 3) for n in range(1, 2 * C + 2 * k["RB"] + 1)]
    ns = (1, C - 1, C, C + 1, 2 * C + k["RB"] - 1)
    shapes += [(n, nf) for i, nf in enumerate(dft_tile_freqs()) for n in (ns[i % 5], ns[(i + 2) % 5])]
    most = k["GW"] * k["WC"] + k["WC"]
    shapes += [((chunks - 1) * C + last, 3) for chunks in range(1, most + 1) for last in dft_last_lengths()]
    return list(dict.fromkeys(shapes))                           # (the first chunk counts are among the first n)


def dft_reduce_edges():
    red = dft_constants()["RED"]
    return {red - 1, red, red + 1, 2 * red - 1, 2 * red, 2 * red + 1}


def dft_classes(shapes):
    """pw_dft_partial_kernel's and pw_dft_reduce_kernel's paths at the default budget (one slab a job)."""
    k = dft_constants()
    C, WC, RB, RED = k["C"], k["WC"], k["RB"], k["RED"]
    T = k["W"] * k["F"]
    got = set()
    for n, nf in shapes:
        chunks, last = tail(n, C)
        got.add(("len mod RB", last % RB))
        got.add(("chunks mod WC", chunks % WC))
        got.add(("reduce: chunks of the last round", chunks % RED))
        if chunks in dft_reduce_edges():
            got.add(("reduce: chunks", chunks))
        got.add(("frequencies: tiles, last tile",) + tail(nf, T))
        for ch0 in range(0, -(-chunks // (k["GW"] * WC)) * k["GW"] * WC, WC):       # every wave of every workgroup
            lens = [min(max(n - (ch0 + c) * C, 0), C) for c in range(WC)]
            if lens[-1] == C:
                got.add(("wave", "whole"))
            elif lens[0] == 0:
                got.add(("wave", "skipped"))
            else:
                got.add(("wave", "EDGE"))
                got.add(("EDGE: chunks with a term", sum(v > 0 for v in lens)))
                if lens[0] < C:
                    got.add(("EDGE: skipped block", True))
                got.update(("EDGE: chunk ends inside a block", v % RB) for v in lens if 0 < v < C)
    return got


def dft_all_classes():
    k = dft_constants()
    T = k["W"] * k["F"]
    return ({("len mod RB", r) for r in range(k["RB"])} | {("chunks mod WC", r) for r in range(k["WC"])} |
            {("reduce: chunks of the last round", r) for r in range(k["RED"])} |
            {("reduce: chunks", c) for c in dft_reduce_edges()} |
            {("frequencies: tiles, last tile",) + tail(nf, T) for nf in (3,) + dft_tile_freqs()} |
            {("wave", "whole"), ("wave", "skipped"), ("wave", "EDGE"), ("EDGE: skipped block", True)} |
            {("EDGE: chunks with a term", c) for c in range(1, k["WC"] + 1)} |
            {("EDGE: chunk ends inside a block", r) for r in range(k["RB"])})


@functools.lru_cache(maxsize=None)
def dft_jobs(kind: str = "normal", seed: int = 0, reverse: bool = False):
    """_dft_cases jobs (a, period, j_first, j_step, n_freq) of dft_shapes(): j = 0, 1, 2, ... of a period 4 n + 1."""
    rng = np.random.default_rng(2000 + seed)
    shapes = dft_shapes()[::-1][1:] if reverse else dft_shapes()
    return [(_series(rng, n, kind, 1.0 + k % 5), 4 * max(n, nf) + 1, 0, 1, nf) for k, (n, nf) in enumerate(shapes)]


def dft_exact_j0(jobs):
    """(index of every job's j = 0 in the packed result, the integer sum of its series): there re is the sum, im 0."""
    at, where, sums = 0, [], []
    for a, _, j_first, _, nf in jobs:
        assert j_first == 0 and (a == np.rint(a)).all() and np.abs(a).max() <= INT_RANGE
        where.append(at)
        sums.append(int(a.astype(np.int64).sum()))
        at += nf
    return np.array(where), np.array(sums, dtype=np.float64)


# ---- pw_kde_sums, pw_kde2_sums, pw_kde_wsums ---------------------------------------------------------------------------
def kde_constants():
    c = lambda n: constant(n, "pw_kde.hpp")
    W = c("KDE_WAVE")
    return {"C": c("KDE_CHUNK"), "T": W * c("KDE_LANE_POINTS"), "T2": W * c("KDE2_LANE_POINTS"), "STAGE": c("KDE2_STAGE"),
            "TW": W * c("KDEW_LANE_POINTS"), "RT": c("KDEW_REPLICAS"), "G": c("KDEW_GROUP")}


def kde_shapes():
    """(n_samples, n_points), and one job without samples."""
    k = kde_constants()
    C, T = k["C"], k["T"]
    return cross([sizes(C), sizes(T)], (C + 1, T + 1), (C // 5, T // 3)) + [(0, T + 1)]


def _sample_classes(n, chunk):
    return {("no samples", True)} if n == 0 else {("samples: chunks, last chunk",) + tail(n, chunk)}


def kde_classes(shapes):
    k = kde_constants()
    got = set()
    for n, m in shapes:
        got |= _sample_classes(n, k["C"])
        got.add(("points: tiles, last tile",) + tail(m, k["T"]))
    return got


def kde_all_classes():
    k = kde_constants()
    return ({("no samples", True)} | {("samples: chunks, last chunk",) + tail(n, k["C"]) for n in sizes(k["C"]) + [k["C"] // 5]} |
            {("points: tiles, last tile",) + tail(m, k["T"]) for m in sizes(k["T"])})


@functools.lru_cache(maxsize=None)
def kde_jobs(seed: int = 0, reverse: bool = False):
    rng = np.random.default_rng(3000 + seed)
    shapes = kde_shapes()[::-1][1:] if reverse else kde_shapes()
    return [(rng.normal(5.0, 0.6, n), np.linspace(2.5, 7.5, m) if m > 1 else np.array([5.1]), 1.0 / (0.08 + 0.001 * (k % 90)))
            for k, (n, m) in enumerate(shapes)]


def kde2_sample_sizes():
    k = kde_constants()
    return sorted(set(sizes(k["C"])) | set(sizes(k["STAGE"])))


def kde2_shapes():
    """(n_samples, nx, ny): the points are the mesh nx x ny.  Each axis takes the sizes for the point tile with the
    other axis at 1 (so the number of points takes them too) and at 3; the samples take the sizes for the chunk and
    for the staged part of one."""
    k = kde_constants()
    C, T = k["C"], k["T2"]
    shapes = []
    for n in kde2_sample_sizes():
        shapes += [(n, T + 1, 1), (n, T // 9, 3)]
    for v in sizes(T):
        shapes += [(C + 1, v, 1), (C // 5, v, 3), (C + 1, 1, v), (C // 5, 3, v)]
    out = []
    for s in shapes + [(0, T + 1, 1)]:
        if s not in out:
            out.append(s)
    return out


def kde2_classes(shapes):
    k = kde_constants()
    got = set()
    for n, nx, ny in shapes:
        got |= _sample_classes(n, k["C"])
        if n:
            got.add(("samples: staged parts of the last chunk, last part",) + tail(tail(n, k["C"])[1], k["STAGE"]))
        got.add(("points: tiles, last tile",) + tail(nx * ny, k["T2"]))
        got.add(("axis x", nx))
        got.add(("axis y", ny))
    return got


def kde2_all_classes():
    k = kde_constants()
    C, T = k["C"], k["T2"]
    points = set(sizes(T)) | {3 * v for v in sizes(T)} | {T + 1, 3 * (T // 9)}
    return ({("no samples", True)} | {("samples: chunks, last chunk",) + tail(n, C) for n in kde2_sample_sizes() + [C + 1, C // 5]} |
            {("samples: staged parts of the last chunk, last part",) + tail(tail(n, C)[1], k["STAGE"])
             for n in kde2_sample_sizes() + [C + 1, C // 5]} |
            {("points: tiles, last tile",) + tail(m, T) for m in points} |
            {("axis x", v) for v in sizes(T) + [T + 1, T // 9]} | {("axis y", v) for v in sizes(T)})


@functools.lru_cache(maxsize=None)
def kde2_jobs(seed: int = 0, reverse: bool = False):
    rng = np.random.default_rng(4000 + seed)
    shapes = kde2_shapes()[::-1][1:] if reverse else kde2_shapes()
    jobs = []
    for k, (n, nx, ny) in enumerate(shapes):
        xy = rng.normal((5.0, -2.0), (0.6, 0.3), (n, 2))
        ax = np.linspace(3.0, 7.0, nx) if nx > 1 else np.array([5.2])
        ay = np.linspace(-3.0, -1.0, ny) if ny > 1 else np.array([-2.1])
        jobs.append((xy, K2.mesh_points(ax, ay), (1.0 / (0.2 + 0.001 * (k % 50)), rng.uniform(-2.0, 2.0), 1.0 / 0.15)))
    return jobs


def kdew_replica_sizes():
    k = kde_constants()
    return sorted(set(sizes(k["RT"])) | set(sizes(k["G"])))


def kdew_shapes():
    """(n_samples, n_points, n_replicas), and one job without samples."""
    k = kde_constants()
    C, T, RT, G = k["C"], k["TW"], k["RT"], k["G"]
    return cross([sizes(C), sizes(T), kdew_replica_sizes()], (C + 1, T + 1, RT + 1), (C // 5, T // 3, G // 2 + 1)) + [(0, T + 1, RT + 1)]


def kdew_classes(shapes):
    """pw_kdew_partial_kernel's paths at the default budget (one slab a job)."""
    k = kde_constants()
    RT, G = k["RT"], k["G"]
    got = set()
    for n, m, r in shapes:
        got |= _sample_classes(n, k["C"])
        got.add(("points: tiles, last tile",) + tail(m, k["TW"]))
        got.add(("replicas: tiles, last tile",) + tail(r, RT))
        if n:
            for b0 in range(0, r, RT):
                nb = min(r - b0, RT)
                got.add(("WHOLE", nb == RT))
                if nb < RT:
                    got.add(("cut short: groups, replicas of the last group",) + tail(nb, G))
    return got


def kdew_all_classes():
    k = kde_constants()
    return ({("no samples", True), ("WHOLE", True), ("WHOLE", False)} |
            {("samples: chunks, last chunk",) + tail(n, k["C"]) for n in sizes(k["C"]) + [k["C"] // 5]} |
            {("points: tiles, last tile",) + tail(m, k["TW"]) for m in sizes(k["TW"])} |
            {("replicas: tiles, last tile",) + tail(r, k["RT"]) for r in kdew_replica_sizes()} |
            {("cut short: groups, replicas of the last group",) + tail(nb, k["G"]) for nb in range(1, k["RT"])})


@functools.lru_cache(maxsize=None)
def kdew_jobs(seed: int = 0, reverse: bool = False, ones: bool = False):
    """_kdew_cases jobs (samples, points, weights (R, n), inv_bandwidth) of kdew_shapes(); `ones`: every weight 1.0."""
    rng = np.random.default_rng(5000 + seed)
    shapes = kdew_shapes()[::-1][1:] if reverse else kdew_shapes()
    jobs = []
    for k, (n, m, r) in enumerate(shapes):
        x = rng.normal(5.0, 0.6, n)
        g = np.linspace(2.5, 7.5, m) if m > 1 else np.array([5.1])
        jobs.append((x, g, np.ones((r, n)) if ones else KW.edge_weights(rng, n, r), 1.0 / (0.08 + 0.001 * (k % 90))))
    return jobs


# ---- pw_gate_counts ------------------------------------------------------------------------------------------------
GATE_BINS = (0, 5)
GATE_SUBSET = 13        # every 13th job goes through the definition in Python (13 and the four n_thr are coprime)


def gate_thresholds():
    T = GA.TILE
    return (1, T - 1, T, T + 1)


def gate_shapes():
    """(n, n_thr): every n to two chunks and 16 entries, the thresholds around the tile dealt round-robin."""
    thr = gate_thresholds()
    return [(n, thr[(n - 1) % len(thr)]) for n in range(1, 2 * GA.CHUNK + 16 + 1)]


def gate_classes(shapes):
    got = set()
    series = {len(a): a for a, _ in gate_jobs()}
    gaps, entries = 0, 0
    for n, m in shapes:
        got.add(("entries: chunks, last chunk",) + tail(n, GA.CHUNK))
        got.add(("thresholds: tiles, last tile",) + tail(m, GA.TILE))
        gaps, entries = gaps + int(np.isnan(series[n]).sum()), entries + n
    got.add(("about a tenth gaps", bool(0.05 * entries < gaps < 0.15 * entries)))
    return got


def gate_all_classes():
    return ({("entries: chunks, last chunk",) + tail(n, GA.CHUNK) for n in range(1, 2 * GA.CHUNK + 16 + 1)} |
            {("thresholds: tiles, last tile",) + tail(m, GA.TILE) for m in gate_thresholds()} | {("about a tenth gaps", True)})


@functools.lru_cache(maxsize=None)
def gate_jobs(seed: int = 0, reverse: bool = False):
    """_gate_cases jobs (a, thresholds): the first n_thr of one unsorted list, about 10 % gaps."""
    rng = np.random.default_rng(6000 + seed)
    every = rng.uniform(-1.5, 1.5, max(gate_thresholds()))
    shapes = gate_shapes()[::-1][1:] if reverse else gate_shapes()
    return [(GA.smooth_noise(n, 7000 + 2000 * seed + n, gaps=0.1), every[:m]) for n, m in shapes]


# ---- the six entries behind one face -------------------------------------------------------------------------------
def _library():
    from pywindow_amd import _lib

    return _lib.load()


def set_poison(on: bool) -> None:
    """The library's test hook pw_internal_poison_scratch (csrc/pw_kde.hip)."""
    L = _library()
    L.pw_internal_poison_scratch.argtypes = [ctypes.c_int]
    L.pw_internal_poison_scratch.restype = None
    L.pw_internal_poison_scratch(1 if on else 0)


def set_launch_cap(blocks: int) -> int:
    """The library's test hook pw_internal_launch_cap (csrc/pw_kde.hip): while blocks > 0 every capped launch gets
    min(items, blocks) workgroups, 0 gives each launch site its own cap back.  Returns how many launches were given
    fewer workgroups than items since the last call, and clears that count."""
    L = _library()
    L.pw_internal_launch_cap.argtypes = [ctypes.c_int]
    L.pw_internal_launch_cap.restype = ctypes.c_long
    return int(L.pw_internal_launch_cap(int(blocks)))


@contextlib.contextmanager
def poisoned():
    set_poison(True)
    try:
        yield
    finally:
        set_poison(False)


def _spans(size, firsts, counts):
    owned = np.zeros(size, dtype=bool)
    for f, c in zip(firsts.tolist(), counts.tolist()):
        owned[f:f + c] = True
    return owned


class Entry:
    """One statistical entry: `jobs(...)` the sweep (reverse=True, seed=1: the same shapes in the opposite order with
    other values, less one -- "different work"), `mixed()` the existing mixed batch, `pack`, `run` (the result as a
    tuple of arrays, through the budget hook where the entry has one, outputs prefilled with `fill`), `owned` (which
    entries of each array of the result some job owns), `holes` (a packed batch whose result has entries nobody owns)."""
    budgets = (1, 100_000, 0)
    vp, i64, pf = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_float)

    def call(self, ctx, name, argtypes, *args):
        L = _library()
        f = getattr(L, name)
        f.argtypes = argtypes
        rc = f(ctx._h, *args)
        assert rc == 0, L.pw_last_error()

    def holes(self, packed):
        rec = packed[0].copy()
        rec["out_first"] += 2 * (np.arange(len(rec)) + 1)
        return (rec,) + tuple(packed[1:])


class Kde(Entry):
    name, budgets = "kde", (0,)
    jobs, shapes, classes, all_classes = staticmethod(kde_jobs), staticmethod(kde_shapes), staticmethod(kde_classes), staticmethod(kde_all_classes)
    mixed, pack = staticmethod(K.mixed_batch), staticmethod(K.pack)

    def run(self, ctx, packed, budget=0, fill=0.0):
        rec, x, g = (np.ascontiguousarray(a) for a in packed)
        sums = np.full(len(g), fill)
        self.call(ctx, "pw_kde_sums", [self.vp, self.vp, self.i64, self.vp, self.vp, self.vp], rec.ctypes.data, len(rec),
                  x.ctypes.data, g.ctypes.data, sums.ctypes.data)
        return (sums,)

    def owned(self, packed):
        rec = packed[0]
        return (_spans(len(packed[2]), rec["point_first"], rec["n_points"]),)

    def holes(self, packed):                                     # (the sums lie like the points: jobs taken out)
        return (np.delete(packed[0], np.arange(2, len(packed[0]), 5)),) + tuple(packed[1:])


class Kde2(Kde):
    name, budgets = "kde2", Entry.budgets
    jobs, shapes, classes, all_classes = staticmethod(kde2_jobs), staticmethod(kde2_shapes), staticmethod(kde2_classes), staticmethod(kde2_all_classes)
    mixed, pack = staticmethod(K2.mixed_batch), staticmethod(K2.pack)

    def run(self, ctx, packed, budget=0, fill=0.0):
        rec, x, g = (np.ascontiguousarray(a) for a in packed)
        sums = np.full(len(g), fill)
        self.call(ctx, "pw_internal_kde2_sums", [self.vp, self.vp, self.i64, self.vp, self.vp, self.vp, self.i64, self.pf],
                  rec.ctypes.data, len(rec), x.ctypes.data, g.ctypes.data, sums.ctypes.data, int(budget), None)
        return (sums,)


class Kdew(Entry):
    name = "kdew"
    jobs, shapes, classes, all_classes = staticmethod(kdew_jobs), staticmethod(kdew_shapes), staticmethod(kdew_classes), staticmethod(kdew_all_classes)
    mixed, pack = staticmethod(KW.edge_jobs), staticmethod(KW.pack)

    def size(self, rec):
        return int((rec["out_first"] + rec["n_replicas"] * rec["n_points"]).max())

    def run(self, ctx, packed, budget=0, fill=0.0):
        rec, x, g, w = (np.ascontiguousarray(a) for a in packed)
        sums = np.full(self.size(rec), fill)
        self.call(ctx, "pw_internal_kde_wsums", [self.vp, self.vp, self.i64, self.vp, self.vp, self.vp, self.vp, self.i64, self.pf],
                  rec.ctypes.data, len(rec), x.ctypes.data, g.ctypes.data, w.ctypes.data, sums.ctypes.data, int(budget), None)
        return (sums,)

    def owned(self, packed):
        rec = packed[0]
        return (_spans(self.size(rec), rec["out_first"], rec["n_replicas"] * rec["n_points"]),)


class Corr(Entry):
    name = "corr"
    jobs, shapes, classes, all_classes = staticmethod(corr_jobs), staticmethod(corr_shapes), staticmethod(corr_classes), staticmethod(corr_all_classes)
    mixed, pack = staticmethod(CO.mixed_batch), staticmethod(CO.pack)

    def size(self, rec):
        live = rec[rec["n"] > 0]
        return int((live["out_first"] + live["n_lags"]).max())

    def run(self, ctx, packed, budget=0, fill=0.0):
        rec, x = (np.ascontiguousarray(a) for a in packed)
        sums = np.full(self.size(rec), fill)
        self.call(ctx, "pw_internal_corr_sums", [self.vp, self.vp, self.i64, self.vp, self.vp, self.i64, self.pf],
                  rec.ctypes.data, len(rec), x.ctypes.data, sums.ctypes.data, int(budget), None)
        return (sums,)

    def owned(self, packed):
        rec = packed[0]
        live = rec[rec["n"] > 0]
        return (_spans(self.size(rec), live["out_first"], live["n_lags"]),)


class Dft(Entry):
    name = "dft"
    jobs, shapes, classes, all_classes = staticmethod(dft_jobs), staticmethod(dft_shapes), staticmethod(dft_classes), staticmethod(dft_all_classes)
    mixed, pack = staticmethod(DF.mixed_batch), staticmethod(DF.pack)

    def live(self, rec):
        return rec[(rec["n"] > 0) & (rec["n_freq"] > 0)]

    def size(self, rec):
        live = self.live(rec)
        return int((live["out_first"] + live["n_freq"]).max())

    def run(self, ctx, packed, budget=0, fill=0.0):
        rec, x = (np.ascontiguousarray(a) for a in packed)
        re, im = np.full(self.size(rec), fill), np.full(self.size(rec), fill)
        self.call(ctx, "pw_internal_dft_sums", [self.vp, self.vp, self.i64, self.vp, self.vp, self.vp, self.i64, self.pf],
                  rec.ctypes.data, len(rec), x.ctypes.data, re.ctypes.data, im.ctypes.data, int(budget), None)
        return re, im

    def owned(self, packed):
        live = self.live(packed[0])
        mask = _spans(self.size(packed[0]), live["out_first"], live["n_freq"])
        return mask, mask


class Gate(Entry):
    name = "gate"
    jobs, shapes, classes, all_classes = staticmethod(gate_jobs), staticmethod(gate_shapes), staticmethod(gate_classes), staticmethod(gate_all_classes)
    mixed, pack = staticmethod(GA.mixed_batch), staticmethod(GA.pack)

    def __init__(self, n_bins):
        self.n_bins = n_bins
        self.name = f"gate-{n_bins}-bins"

    def run(self, ctx, packed, budget=0, fill=0):
        rows = len(self.owned(packed)[0])
        counts = np.full((rows, GA.FIELDS), fill, dtype=np.int64)
        hist = np.full((rows, 2, self.n_bins), fill, dtype=np.int64)
        rc, counts, hist = GA.raw_counts(ctx, *packed, self.n_bins, counts, hist, workspace_bytes=budget)
        assert rc == 0, _library().pw_last_error()
        return counts, hist

    def owned(self, packed):
        rec = packed[0]
        live = rec[(rec["n"] > 0) & (rec["n_thr"] > 0)]
        mask = _spans(int((live["out_first"] + live["n_thr"]).max()), live["out_first"], live["n_thr"])
        return mask, mask

    def holes(self, packed):
        raise NotImplementedError("use pack_with_holes: the rows are dealt when the jobs are packed")


def pack_with_holes(entry, jobs):
    """The batch with entries of the result that no job owns, and the batch as `pack` lays it out."""
    if isinstance(entry, Gate):
        return GA.pack(jobs, hole=2)
    return entry.holes(entry.pack(jobs))


ENTRIES = (Kde(), Kde2(), Kdew(), Corr(), Dft()) + tuple(Gate(b) for b in GATE_BINS)


def same(got, want):
    """Bit for bit, array by array (for gate's int64 that is np.array_equal)."""
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))
