"""Inputs shared by tests/test_pores.py (host path against the definition) and tests/test_gpu_pores.py (device against
the host path and against the definition): the probe-swept cavity for a ladder of probes (pw_pore_sizes).  Every output
is an integer: every comparison is of bytes.  numpy only and seeded; nothing here is taken from
pywindow_amd/csrc/pw_pores.hpp -- `reference` is the definition of include/pywindow_amd.h written directly: a level's
open voxels and their component by tests/_cavity_cases.py, K by the written rule in float64, the sweep as a brute-force
OR over the integer offsets with di^2 + dj^2 + dl^2 <= K (or, where the reach has fewer voxels than the ball has
offsets, over the voxels of the reach: the same set), the attribution as a per-voxel maximum over the levels."""
import ctypes
import functools
import math

import numpy as np

import _cavity_cases as C

SENTINEL = C.SENTINEL
MAX_K2 = 3 * 63 * 63
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


class Case:
    """One job: the grid (dims (nx, ny, nz), origin, spacing h), the seed voxel, the ladder `probes` (L,), and either
    atoms (n, 3) with radii (n,) and planes (m, 4), or ready-made open words (L, ny * nz) uint64 (word l * ny + j)."""

    def __init__(self, name, dims, seed, probes, h=1.0, origin=(0.0, 0.0, 0.0), xyz=None, radii=None, planes=None, words=None):
        self.name, self.dims, self.seed = name, tuple(int(d) for d in dims), tuple(int(s) for s in seed)
        self.probes = np.ascontiguousarray(probes, dtype=np.float64).reshape(-1)
        self.h, self.origin = float(h), np.asarray(origin, dtype=np.float64)
        self.xyz = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.radii = np.zeros(0) if radii is None else np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
        self.planes = np.zeros((0, 4)) if planes is None else np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        self.words = None if words is None else np.ascontiguousarray(words, dtype=np.uint64).reshape(len(self.probes), -1)
        assert len(self.xyz) == len(self.radii)
        assert self.words is None or self.words.shape[1] == self.dims[1] * self.dims[2]

    @property
    def L(self):
        return len(self.probes)

    def level(self, l) -> C.Case:
        """Level l as a pw_cavity job."""
        return C.Case(f"{self.name}[{l}]", self.dims, self.seed, self.xyz, self.radii, float(self.probes[l]), self.origin,
                      self.h, self.planes, None if self.words is None else self.words[l])


def k2_rule(p, h) -> int:
    """The largest integer k in [0, MAX_K2] with (double)k * (h * h) <= p * p, each product rounded once."""
    h2, p2 = np.float64(h) * np.float64(h), np.float64(p) * np.float64(p)
    return int(np.flatnonzero(np.arange(MAX_K2 + 1).astype(np.float64) * h2 <= p2)[-1])


def probe_for(k2: int) -> float:
    """A probe that has K = k2 at h = 1 (MAX_K2 + 1 and beyond: the clamp)."""
    return math.sqrt(k2 + 0.5)


def ball_offsets(K: int, shape):
    """The integer offsets (dl, dj, di) with di^2 + dj^2 + dl^2 <= K that can join two voxels of the grid."""
    R = math.isqrt(K)
    span = [range(-min(R, n - 1), min(R, n - 1) + 1) for n in shape]
    return [(dl, dj, di) for dl in span[0] for dj in span[1] for di in span[2] if di * di + dj * dj + dl * dl <= K]


def sweep(reach: np.ndarray, K: int) -> np.ndarray:
    """The voxels [l, j, i] of the grid within squared distance K, in integers, of a voxel of `reach`."""
    out = np.zeros_like(reach)
    centres = np.argwhere(reach)
    offsets = ball_offsets(K, reach.shape)
    if len(centres) <= len(offsets):
        l, j, i = np.ogrid[:reach.shape[0], :reach.shape[1], :reach.shape[2]]
        for cl, cj, ci in centres:
            out |= (i - ci) ** 2 + (j - cj) ** 2 + (l - cl) ** 2 <= K
        return out
    for off in offsets:
        dst = tuple(slice(max(0, d), n + min(0, d)) for d, n in zip(off, reach.shape))
        src = tuple(slice(max(0, -d), n + min(0, -d)) for d, n in zip(off, reach.shape))
        out[dst] |= reach[src]
    return out


def reference(c: Case):
    """(the L PORES_LEVEL_DTYPE rows, the PORES_OUT_DTYPE row, the L * ny * nz mask words) of the definition."""
    from pywindow_amd import _lib

    nx, ny, nz = c.dims
    i, j, l = c.seed
    levels = np.zeros(c.L, dtype=_lib.PORES_LEVEL_DTYPE)
    swept, domain = [], None
    for q in range(c.L):
        ok = C.open_voxels(c.level(q))
        reach = C.component(ok, c.seed)
        if q == 0:
            domain = reach
        K = k2_rule(c.probes[q], c.h)
        ll, jj, ii = np.nonzero(reach)
        levels["n_reach"][q] = reach.sum()
        levels["n_face"][q] = ((ii == 0) | (ii == nx - 1) | (jj == 0) | (jj == ny - 1) | (ll == 0) | (ll == nz - 1)).sum()
        levels["k2"][q] = K
        levels["flags"][q] = 0 if ok[l, j, i] else _lib.CAV_SEED_CLOSED
        swept.append(sweep(reach, K) & domain)
        levels["n_swept"][q] = swept[q].sum()
    cover = np.full((nz, ny, nx), -1)
    for q in range(c.L):
        cover[swept[q]] = q                                          # (ascending: the largest level stays)
    for q in range(c.L):
        levels["n_largest"][q] = (cover == q).sum()
    out = np.zeros((), dtype=_lib.PORES_OUT_DTYPE)
    out["n_domain"], out["n_none"], out["n_levels"] = domain.sum(), (domain & (cover < 0)).sum(), c.L
    return levels, out, np.concatenate([C.pack_words(s) for s in swept])


_cache = {}


def reference_cached(c: Case):
    """`reference`, computed once a case object and shared; the results are read-only."""
    if id(c) not in _cache:
        got = reference(c)
        for a in got:
            a.setflags(write=False)
        _cache[id(c)] = (c, got)                                     # (the case is kept: its id stays its own)
    return _cache[id(c)][1]


def words_of(dims, voxels=None, full=False, beyond=False):
    """The ny * nz words of a grid with the voxels (i, j, l) set, or all of them; `beyond`: with the bits >= nx set too."""
    nx, ny, nz = dims
    ok = np.full((nz, ny, nx), full, dtype=bool)
    for i, j, l in voxels or ():
        ok[l, j, i] = True
    w = C.pack_words(ok)
    return w | (ALL << np.uint64(nx)) if beyond and nx < 64 else w


def centre_case(name, dims, centre, k2s, beyond=False, extra=()):
    """Ready-made levels: level 0 has every voxel open and probe 0 -- the domain is the grid --, the levels after it only
    `centre` (and the voxels `extra`, which the fill does not reach unless they touch it), with the probes of k2s at h = 1."""
    full = words_of(dims, full=True, beyond=beyond)
    one = words_of(dims, [centre, *extra], beyond=beyond)
    return Case(name, dims, centre, [0.0] + [probe_for(k) for k in k2s], words=np.stack([full] + [one] * len(k2s)))


def lattice_case(name, dims, n_atoms, seed, probes, h=0.5, planes=None):
    """Random atoms around a hollow middle in which the seed voxel lies (tests/_cavity_cases.py: lattice_job)."""
    xyz, radii = C.random_atoms(n_atoms, dims, seed, h, hollow=2.5)
    return Case(name, dims, tuple((d - 1) // 2 for d in dims), probes, h, xyz=xyz, radii=radii, planes=planes)


BALL_K2 = (0, 1, 2, 3, 4, 5, 6, 8, 9)
ROW_GRIDS = ((1, 1), (63, 1), (8, 8), (5, 13), (6, 43), (7, 37), (19, 27))    # ny * nz = 1, 63, 64, 65, 258, 259, 513


@functools.lru_cache(maxsize=None)
def cases():
    """The smallest shapes at which the kernel and the host path can go wrong."""
    out = []
    # the ball: one centre in 9 x 9 x 9 at every K below 10 that is a sum of three squares; 6 and 7 give the same ball
    out.append(centre_case("ball", (9, 9, 9), (4, 4, 4), BALL_K2))
    out.append(centre_case("ball-6-and-7", (9, 9, 9), (4, 4, 4), (6, 7)))
    # the farthest two voxels of the largest grid: (63, 63, 63) is at exactly MAX_K2 from (0, 0, 0)
    out.append(centre_case("corner", (64, 64, 64), (0, 0, 0), (MAX_K2 - 1, MAX_K2)))
    # word edges: a centre at bit 0 and at bit 63 of nx = 64; nx = 63, 5, 1 with the bits beyond nx set in the words
    for nx, bit in ((64, 0), (64, 63), (63, 62), (63, 0), (5, 4), (5, 0), (1, 0)):
        out.append(centre_case(f"word-edge-nx={nx}-bit={bit}", (nx, 4, 3), (bit, 1, 1), (1, 5, 70), beyond=True))
    # rows: fewer than threads, around the wave and the workgroup, centres in the first and in the last row
    for ny, nz in ROW_GRIDS:
        out.append(centre_case(f"rows={ny}x{nz}-first", (9, ny, nz), (4, 0, 0), (5, 27)))
        out.append(centre_case(f"rows={ny}x{nz}-last", (9, ny, nz), (4, ny - 1, nz - 1), (5, 27)))
    for dims in ((64, 1, 1), (1, 64, 1), (1, 1, 64), (1, 1, 1)):
        mid = tuple((d - 1) // 3 for d in dims)
        out.append(centre_case(f"line-{dims}", dims, mid, (0, 9, 500, MAX_K2 + 5)))
    # the sweep is of the cavity: a second open component is not swept from (and the domain's voxels that are not
    # open at the level are swept into); a serpentine one voxel wide at K = 1
    out.append(centre_case("second-component", (12, 9, 7), (2, 4, 3), (2, 4), extra=[(9, 4, 3), (9, 5, 3), (6, 0, 0)]))
    for dims in ((8, 8, 8), (64, 5, 3)):
        ok, _, _ = C.serpentine(*dims)
        out.append(Case(f"serpentine-{dims}", dims, (0, 0, 0), [0.0, 1.0], words=np.stack([C.pack_words(ok)] * 2)))
    # attribution, with levels that are not nested: level 1 a line along x (K = 1: a tube), level 2 the seed alone
    # (K = 2: a ball that has (0, 1, 1), which the tube has not, and has not the ends of the tube)
    dims = (11, 7, 7)
    line = words_of(dims, [(i, 3, 3) for i in range(11)])
    out.append(Case("not-nested", dims, (5, 3, 3), [0.0, 1.0, probe_for(2)],
                    words=np.stack([words_of(dims, full=True), line, words_of(dims, [(5, 3, 3)])])))
    # a level with a closed seed between two open ones; the seed closed at level 0 (no domain) with open levels after it
    shut = words_of(dims, [(i, 3, 3) for i in range(11) if i != 5])
    out.append(Case("closed-between", dims, (5, 3, 3), [0.0, 1.0, 2.0, 3.0],
                    words=np.stack([words_of(dims, full=True), line, shut, words_of(dims, [(5, 3, 3), (5, 4, 3)])])))
    out.append(Case("no-domain-words", dims, (5, 3, 3), [0.0, 1.0], words=np.stack([shut, line])))
    # the classification path: n = 0, 1, 5, 200 atoms with planes and 5 levels; the tie of pw_cavity at two probes; a
    # seed inside an atom; ladders of L = 1, 2, 63, 64 whose last levels have closed seeds
    planes = [[1.0, 0.2, 0.0, 5.0], [-1.0, 0.0, 0.3, -1.5], [0.0, 0.0, 1.0, 3.75]]
    wider = [[1.0, 0.2, 0.0, 7.0], [-1.0, 0.0, 0.3, -1.5], [0.0, 0.0, 1.0, 5.25]]
    five = [0.0, 0.25, 0.5, 0.9, 1.3]
    out.append(Case("atoms-0", (15, 13, 11), (7, 6, 5), five, 0.5, planes=planes))
    out.append(Case("atoms-1", (15, 13, 11), (7, 6, 5), five, 0.5, xyz=[[1.0, 1.2, 0.9]], radii=[1.1], planes=planes))
    for n in (5, 200):
        out.append(lattice_case(f"atoms-{n}", (21, 19, 17), n, 100 + n, five, planes=wider))
    out.append(Case("tie", (13, 13, 13), (0, 0, 0), [0.0, 1.25], 1.0, (-6.0, -6.0, -6.0), xyz=[[0.0, 0.0, 0.0]], radii=[3.75]))
    out.append(Case("no-domain", (13, 13, 13), (6, 6, 6), [0.0, 1.0, 2.0], 1.0, (-6.0, -6.0, -6.0), xyz=[[0.0, 0.0, 0.0]], radii=[5.0]))
    for L in (1, 2, 63, 64):
        out.append(lattice_case(f"ladder-{L}", (13, 12, 11), 30, 300 + L, 0.07 * np.arange(L), 0.5))
    return out


def mixed_batch():
    """64 jobs of mixed grids and numbers of levels."""
    small = [c for c in cases() if c.dims != (64, 64, 64)]
    jobs = [small[(5 * k) % len(small)] for k in range(64)]
    assert len({c.dims for c in jobs}) > 10 and len({c.L for c in jobs}) > 5
    return jobs


def other_shapes():
    """Jobs of other shapes and values: what a context did before."""
    return [lattice_case("before-a", (50, 3, 40), 25, 31, [0.0, 0.6]), lattice_case("before-b", (9, 33, 2), 10, 32, [0.3])]


class Packed:
    """The arguments of a call for a list of cases.  A job's row of out, its rows of levels and its mask words come one
    job after the other, `hole` entries that nobody owns in front of each; atoms, planes and probes that several jobs
    hold (the same case object) are stored once.  `masks`: which jobs get a mask (True: all)."""

    def __init__(self, jobs, hole=0, masks=True):
        from pywindow_amd import _lib

        self.jobs = list(jobs)
        self.with_mask = [bool(masks)] * len(self.jobs) if isinstance(masks, bool) else [bool(m) for m in masks]
        self.rec = np.zeros(len(self.jobs), dtype=_lib.PORES_JOB_DTYPE)
        self.open_first = np.full(len(self.jobs), -1, dtype=np.int64)
        xyz, radii, planes, probes, words, where = [np.zeros((0, 3))], [np.zeros(0)], [np.zeros((0, 4))], [np.zeros(0)], [np.zeros(0, dtype=np.uint64)], {}
        atoms = cuts = ladder = row = level = at = n_words = 0
        for k, c in enumerate(self.jobs):
            if id(c) not in where:
                where[id(c)] = (atoms, cuts, ladder)
                xyz.append(c.xyz); radii.append(c.radii); planes.append(c.planes); probes.append(c.probes)
                atoms += len(c.xyz); cuts += len(c.planes); ladder += c.L
            a, p, q = where[id(c)]
            size = c.L * c.dims[1] * c.dims[2]
            row += hole
            level += hole
            at += hole if self.with_mask[k] else 0
            self.rec[k] = (a, len(c.xyz), a, p, len(c.planes), q, c.L, level, at if self.with_mask[k] else -1, row, c.origin,
                           c.h, *c.dims, c.seed)
            if c.words is not None:
                self.open_first[k] = n_words
                words.append(c.words.reshape(-1))
                n_words += size
            row += 1
            level += c.L
            at += size if self.with_mask[k] else 0
        self.xyz, self.radii, self.planes = np.concatenate(xyz), np.concatenate(radii), np.concatenate(planes)
        self.probes, self.words = np.concatenate(probes), np.concatenate(words)
        self.n_levels, self.n_out, self.n_mask = level, row, at

    def blank(self):
        """(levels, out, mask) with every byte SENTINEL."""
        from pywindow_amd import _lib

        def filled(dtype, n):
            return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dtype).itemsize * n), dtype=dtype).copy()

        return filled(_lib.PORES_LEVEL_DTYPE, self.n_levels), filled(_lib.PORES_OUT_DTYPE, self.n_out), filled(np.uint64, self.n_mask)

    def expected(self):
        """(levels, out, mask) of the definition in this layout, SENTINEL bytes where nobody writes."""
        levels, out, mask = self.blank()
        for k, c in enumerate(self.jobs):
            lv, o, w = reference_cached(c)
            J = self.rec[k]
            levels[int(J["level_first"]):int(J["level_first"]) + c.L] = lv
            out[int(J["out"])] = o
            if self.with_mask[k]:
                mask[int(J["mask_first"]):int(J["mask_first"]) + len(w)] = w
        return levels, out, mask


def raw(ctx, P: Packed, workspace_bytes=None, timed=False, sizes=None):
    """pw_pore_sizes through ctypes into SENTINEL-filled arrays -- through the library's test entry when the jobs carry
    ready-made open words or `workspace_bytes` is given (0: the default budget).  `sizes`: other numbers of rows and
    entries of (xyz, radii, planes, probes, levels, out, mask) to tell the entry, None for the true ones.  Returns
    (rc, (levels, out, mask)[, ms])."""
    from pywindow_amd import _lib

    L = _lib.load()
    rec = np.ascontiguousarray(P.rec, dtype=_lib.PORES_JOB_DTYPE)
    levels, out, mask = P.blank()
    told = [len(P.xyz), len(P.radii), len(P.planes), len(P.probes), P.n_levels, P.n_out, P.n_mask]
    for q, v in enumerate(sizes or ()):
        told[q] = told[q] if v is None else v
    args = [ctx._h, rec.ctypes.data, len(rec), P.xyz.ctypes.data, told[0], P.radii.ctypes.data, told[1], P.planes.ctypes.data,
            told[2], P.probes.ctypes.data, told[3], levels.ctypes.data, told[4], out.ctypes.data, told[5], mask.ctypes.data, told[6]]
    ms = ctypes.c_float(0.0)
    if workspace_bytes is None and not (P.open_first >= 0).any() and not timed:
        rc = L.pw_pore_sizes(*args)
    else:
        rc = L.pw_internal_pore_sizes(*args, P.words.ctypes.data, P.open_first.ctypes.data, len(P.words),
                                      int(workspace_bytes or 0), ctypes.byref(ms) if timed else None)
    return (rc, (levels, out, mask), ms.value) if timed else (rc, (levels, out, mask))


same = C.same


def first_difference(got, want):
    """For an assertion's message: the first entry that differs."""
    for name, g, w in zip(("levels", "out", "mask"), got, want):
        for k in range(len(w)):
            if g[k].tobytes() != w[k].tobytes():
                return name, k, g[k], w[k]
    return None


def bad_batches():
    """[(Packed, sizes, reason)]: two jobs of which job 1 is refused."""
    good = next(c for c in cases() if c.name == "tie")
    other = lattice_case("other", (9, 8, 7), 6, 41, [0.0, 0.5, 1.0])
    with_planes = lattice_case("with-planes", (9, 8, 7), 6, 42, [0.0, 0.5, 1.0], planes=[[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0]])
    out = []

    def edit(fn, reason, second=other, sizes=None):
        P = Packed([good, second])
        fn(P)
        out.append((P, sizes, reason))

    def field(name, value):
        def fn(P):
            P.rec[name][1] = value
        return fn

    def entry(array, at, value):
        def fn(P):
            a = getattr(P, array).copy()
            a.reshape(-1)[at(P)] = value
            setattr(P, array, a)
        return fn

    def ladder(values):
        def fn(P):
            P.probes = P.probes.copy()
            P.probes[int(P.rec["probe_first"][1]):int(P.rec["probe_first"][1]) + 3] = values
        return fn

    n = len(good.xyz) + len(other.xyz)
    edit(field("n_levels", 0), "n_levels outside 1 .. PW_PORES_MAX_LEVELS")
    edit(field("n_levels", 65), "n_levels outside 1 .. PW_PORES_MAX_LEVELS")
    edit(ladder([0.0, 0.5, 0.5]), "the probes are not strictly ascending")
    edit(ladder([0.0, 1.0, 0.5]), "the probes are not strictly ascending")
    edit(ladder([-0.25, 0.5, 1.0]), "a negative probe")
    edit(ladder([0.0, np.nan, 1.0]), "a probe is not finite")
    edit(ladder([0.0, 0.5, np.inf]), "a probe is not finite")
    edit(field("probe_first", -1), "probes outside the array")
    edit(lambda P: None, "probes outside the array", sizes=(None, None, None, 4, None, None, None))
    edit(lambda P: None, "atoms outside xyz", sizes=(n - 1, None, None, None, None, None, None))
    edit(field("atom_first", -1), "atoms outside xyz")
    edit(lambda P: None, "radii outside the array", sizes=(None, n - 1, None, None, None, None, None))
    edit(lambda P: None, "planes outside the array", second=with_planes, sizes=(None, None, 1, None, None, None, None))
    edit(lambda P: None, "the rows are outside levels", sizes=(None, None, None, None, 4, None, None))
    edit(field("level_first", -1), "the rows are outside levels")
    edit(lambda P: None, "the row is outside out", sizes=(None, None, None, None, None, 1, None))
    edit(field("out", -1), "the row is outside out")
    edit(lambda P: None, "the words are outside mask", sizes=(None, None, None, None, None, None, 2 * 169 + 3 * 56 - 1))
    edit(field("mask_first", -2), "the words are outside mask")
    edit(field("out", 0), "shares its row of out with an earlier job")
    edit(field("level_first", 1), "shares rows of levels with an earlier job")
    edit(field("level_first", 0), "shares rows of levels with an earlier job")
    edit(field("mask_first", 2 * 169 - 1), "shares words of mask with an earlier job")
    edit(field("mask_first", 0), "shares words of mask with an earlier job")
    # pw_cavity's own refusals for the grid, the seed and the values
    for name in ("nx", "ny", "nz"):
        edit(field(name, 0), "a dimension outside 1 .. PW_CAVITY_MAX_G")
        edit(field(name, 65), "a dimension outside 1 .. PW_CAVITY_MAX_G")
    edit(field("seed", [9, 0, 0]), "the seed is outside the grid")
    edit(field("seed", [0, -1, 0]), "the seed is outside the grid")
    edit(field("seed", [0, 0, 7]), "the seed is outside the grid")
    edit(field("spacing", 0.0), "spacing <= 0")
    edit(field("spacing", np.nan), "the origin or the spacing is not finite")
    edit(field("origin", [0.0, np.inf, 0.0]), "the origin or the spacing is not finite")
    edit(field("n", -1), "a negative count")
    edit(entry("xyz", lambda P: 3 * int(P.rec["atom_first"][1]) + 4, np.nan), "a coordinate is not finite")
    edit(entry("radii", lambda P: int(P.rec["radius_first"][1]) + 1, -0.5), "a negative radius")
    edit(entry("radii", lambda P: int(P.rec["radius_first"][1]) + 1, np.inf), "a radius is not finite")
    edit(entry("planes", lambda P: 4 * int(P.rec["plane_first"][1]) + 5, np.inf), "a plane is not finite", second=with_planes)
    return out
