"""Constructed molecules that take the optimiser chains (pw_unit.hpp: NearGap4 / NearGap1 and the L-BFGS-B and
Nelder-Mead searches that evaluate through them) to the edges of their candidate lists, the numpy bookkeeping that
proves what each case reaches, and the reference runner: live ``scipy.optimize.minimize`` on the oracle's objective
for the pore centre, the oracle's ``find_windows(detail=)`` for a window.  Shared by tests/test_opt_edges.py (host
context against SciPy, and the conditions) and tests/test_gpu_opt_edges.py (device against host context and SciPy).

The lists: a rebuild at a reference point R keeps the atoms whose gap at R is within 2 * DELTA + MARGIN = 0.600001
of the minimum there -- at most 32 for the four-point objective (pore centre, window neck), at most 64 for the
one-point objective of the in-plane simplex; more: no list, every atom.  A lane's candidates are list positions
l and l + 16 (four-point), or its own lane number (one-point); the list is filled in STORED order, ballot block by
ballot block of 64 atoms."""
import contextlib
import functools

import numpy as np

from pywindow_amd import _lib
from pywindow_amd import element_data as E
from pywindow_amd import synth

DELTA = 0.3                 # NearGap4 / NearGap1: how far (1-norm) a point may lie from the list's reference point
SLACK = 0.600001            # ... and 2.0 * DELTA + MARGIN: the gaps above the minimum there that are listed
BAND = 1e-9                 # no count may depend on a slack moved by this much
LIST4, LIST1 = 32, 64       # capacities of the two lists
PORE_STAGES = _lib.STAGE_BASIC | _lib.STAGE_OPT
WINDOW_STAGES = _lib.STAGE_BASIC | _lib.STAGE_OPT | _lib.STAGE_WINDOWS

#: SciPy's message -> (opt_task, opt_msg) of the record (pw_lbfgsb.hpp: LbTask / LbMsg), and its status
TASKS = {
    "CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL": (4, 401, 0),
    "CONVERGENCE: RELATIVE REDUCTION OF F <= FACTR*EPSMCH": (4, 402, 0),
    "ABNORMAL: ": (8, 0, 2),
}


class CaseRejected(AssertionError):
    """A count sits within BAND of the slack: rounding would decide membership.  Change the seed."""


# ---- bookkeeping (numpy, float64) ----------------------------------------------------------------------------------
def gaps(xyz, vdw, p):
    return np.sqrt(((xyz - np.asarray(p, float)) ** 2).sum(axis=1)) - vdw


def listed(xyz, vdw, p):
    """Mask of the atoms a rebuild at ``p`` lists; raises where the slack moved by +-BAND changes it."""
    g = gaps(xyz, vdw, p)
    m = g.min()
    mask = g <= m + SLACK
    if (g <= m + SLACK - BAND).sum() != mask.sum() or (g <= m + SLACK + BAND).sum() != mask.sum():
        raise CaseRejected(f"an atom within {BAND:g} of the slack at {p}")
    return mask


def candidates(xyz, vdw, p):
    return int(listed(xyz, vdw, p).sum())


def stored_order(vdw):
    """Input indices in stored order: grouped by radius, groups by first appearance, stable inside a group
    (pw_unit.hpp: template_groups_build).  One radius: the input order."""
    vdw = np.asarray(vdw)
    first = {}
    for i, v in enumerate(vdw):
        first.setdefault(float(v), i)
    return np.array(sorted(range(len(vdw)), key=lambda i: (first[float(vdw[i])], i)), dtype=np.int64)


def stored_index(vdw, atom):
    return int(np.nonzero(stored_order(vdw) == atom)[0][0])


def holder(xyz, vdw, p):
    return int(np.argmin(gaps(xyz, vdw, p)))


def list_position(xyz, vdw, p, atom):
    """Rank of ``atom`` among the atoms listed at ``p``, in stored order."""
    mask = listed(xyz, vdw, p)
    assert mask[atom]
    order = stored_order(vdw)
    return int(mask[order][: int(np.nonzero(order == atom)[0][0])].sum())


def fibonacci(n):
    """n unit vectors on the golden spiral."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    t = np.pi * (3.0 - np.sqrt(5.0)) * np.arange(n)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(t), r * np.sin(t), z], axis=1)


# ---- pore cases ----------------------------------------------------------------------------------------------------
class PoreCase:
    def __init__(self, name, xyz, vdw, mass, start, box):
        self.name, self.start = name, np.asarray(start, float)
        self.xyz, self.vdw, self.mass = np.ascontiguousarray(xyz, float), np.ascontiguousarray(vdw, float), np.ascontiguousarray(mass, float)
        self.box = tuple((None if a is None else float(a), None if b is None else float(b)) for a, b in box)

    def __repr__(self):
        return self.name

    @property
    def params(self):
        return _lib.Params(opt_start=self.start, opt_bounds=self.box)

    def batch(self):
        return _lib.Batch(np.array([0, len(self.xyz)], np.int64), self.xyz, self.vdw, self.mass)

    @functools.cached_property
    def ref(self):
        """Live SciPy on the oracle's objective, every point recorded."""
        from scipy.optimize import minimize

        from oracle import pw_oracle as O

        cage = O.Cage(self.xyz, self.vdw)
        points = []

        def f(p):
            points.append(np.array(p, float))
            return -(cage.gap(p)[0] * 2)

        res = minimize(f, x0=self.start, bounds=self.box)
        d, atom = O.pore_diameter(cage, res.x)
        return {"res": res, "points": np.array(points), "d": d, "atom": atom}

    @functools.cached_property
    def counts(self):
        return np.array([candidates(self.xyz, self.vdw, p) for p in self.ref["points"]])

    @property
    def nbd(self):
        """L-BFGS-B's kind of each variable's bounds: 0 none, 1 lower only, 2 both, 3 upper only."""
        return tuple((0 if b is None else 3) if a is None else (1 if b is None else 2) for a, b in self.box)


def check_pore_record(case, rec, where):
    """One record against the case's live SciPy run: bit for bit, count for count."""
    ref = case.ref
    res = ref["res"]
    tag = f"{where} {case.name}"
    assert np.asarray(rec["pore_opt_c"]).tobytes() == np.asarray(res.x, float).tobytes(), (tag, rec["pore_opt_c"], res.x)
    assert float(rec["pore_opt_d"]) == ref["d"] and int(rec["pore_opt_atom"]) == ref["atom"], (tag, rec["pore_opt_d"], ref["d"],
                                                                                            rec["pore_opt_atom"], ref["atom"])
    assert (int(rec["opt_nit"]), int(rec["opt_nfev"])) == (int(res.nit), int(res.nfev)), (tag, rec["opt_nit"], res.nit,
                                                                                          rec["opt_nfev"], res.nfev)
    task, msg, status = TASKS[str(res.message)]
    assert int(res.status) == status, (tag, res.status, res.message)
    assert (int(rec["opt_task"]), int(rec["opt_msg"])) == (task, msg), (tag, rec["opt_task"], rec["opt_msg"], res.message)


def _shell(n_shell, n_far, seed, radii=(1.7,), centre=(3.1, -2.2, 1.4)):
    """``n_shell`` atoms whose gap at ``centre`` is 4.3 +- 0.02 (a Fibonacci sphere of radius 6 for the radius 1.7),
    ``n_far`` atoms 3 A further out, radii drawn from ``radii``; not yet permuted."""
    rng = np.random.default_rng(seed)
    centre = np.array(centre)
    vdw = np.array(radii)[rng.integers(0, len(radii), size=n_shell + n_far)] if len(radii) > 1 else np.full(n_shell + n_far, radii[0])
    gap = np.concatenate([4.3 + rng.uniform(-0.02, 0.02, size=n_shell), np.full(n_far, 7.3)])
    dirs = np.concatenate([fibonacci(n_shell), fibonacci(n_far)[:, [2, 0, 1]]])
    return centre, centre + dirs * (gap + vdw)[:, None], vdw


def shell_case(n, box, start, seed=0):
    centre, xyz, vdw = _shell(n, 40, seed)
    perm = np.random.default_rng(seed + 1000).permutation(len(xyz))
    half = float(box)
    return PoreCase(f"shell{n}/box{box:g}", xyz[perm], vdw[perm], np.full(len(xyz), 12.0), centre + np.array(start),
                    [(c - half, c + half) for c in centre])


def tilted_case(seed=0):
    """32 atoms whose gaps at the centre grow from 4.3 on the -x side to 4.75 on the +x side, in a box that lets the
    centre move 0.25 along x and 0.02 along y and z: the run stays within DELTA (1-norm) of its start, so ONE list, built
    at the start, serves it to the end -- and the optimum, 0.225 along x where every gap is 4.525, is held by atoms whose
    gap at the start exceeded the minimum there by more than DELTA.  A slack of 2 DELTA lists them; less does not."""
    rng = np.random.default_rng(seed + 77)
    centre = np.array((3.1, -2.2, 1.4))
    dirs = np.concatenate([fibonacci(LIST4), fibonacci(40)[:, [2, 0, 1]]])
    gap = np.concatenate([4.3 + 0.225 * (1.0 + dirs[:LIST4, 0]) + rng.uniform(-0.005, 0.005, size=LIST4), np.full(40, 7.3)])
    xyz = centre + dirs * (gap + 1.7)[:, None]
    perm = rng.permutation(len(xyz))
    half = (0.25, 0.02, 0.02)
    return PoreCase("tilted32/thin box", xyz[perm], np.full(len(xyz), 1.7), np.full(len(xyz), 12.0), centre,
                    [(c - h, c + h) for c, h in zip(centre, half)])


def references(case):
    """The reference point of the list at every recorded point, as the device moves it: the points come in fours (f
    and the three forward-difference points of one gradient); when one of a four lies more than DELTA (1-norm) from
    the reference, the list is rebuilt around the first of them."""
    pts = case.ref["points"]
    assert len(pts) % 4 == 0
    ref, out = None, []
    for k in range(0, len(pts), 4):
        if ref is not None:
            far = np.abs(pts[k:k + 4] - ref).sum(axis=1)
            if (np.abs(far - DELTA) < BAND).any():
                raise CaseRejected(f"a point within {BAND:g} of DELTA from its reference")
        if ref is None or (far > DELTA).any():
            ref = pts[k]
        out += [ref] * 4
    return np.array(out)


def beyond_delta(case):
    """Recorded points whose holder's gap at the list's reference point exceeds the minimum there by more than
    DELTA + MARGIN: a list built with a slack of DELTA would not hold it."""
    n = 0
    for p, r in zip(case.ref["points"], references(case)):
        g = gaps(case.xyz, case.vdw, r)
        over = g[holder(case.xyz, case.vdw, p)] - g.min() - (DELTA + 1e-6)
        if abs(over) < BAND:
            raise CaseRejected("a holder within 1e-9 of the smaller slack")
        n += over > 0
    return n


SMALL = dict(box=0.1, start=(0.03, -0.02, 0.05))
WIDE = dict(box=1.0, start=(0.3, -0.2, 0.5))


@functools.lru_cache(maxsize=None)
def shell_small():
    return [shell_case(n, **SMALL) for n in (31, 32, 33)]


@functools.lru_cache(maxsize=None)
def shell_wide():
    return [shell_case(n, **WIDE) for n in (32, 33, 65)]


def _placed(two_radii, seed):
    """The full list of 32 in a small box with the atoms ordered from the recorded points: the holder of the final
    minimum at list position 31, holders of other recorded points at positions 16 and 0, their stored indices at
    >= 128, in 64..127 and below 64."""
    radii = (1.7, 1.2) if two_radii else (1.7,)
    centre, xyz, vdw = _shell(LIST4, 140, seed, radii)
    shell = np.arange(LIST4)
    far = list(range(LIST4, len(xyz)))
    probe = PoreCase("probe", xyz, vdw, np.full(len(xyz), 12.0), centre + np.array(SMALL["start"]),
                     [(c - SMALL["box"], c + SMALL["box"]) for c in centre])
    pts = probe.ref["points"]
    holders = [holder(xyz, vdw, p) for p in pts]
    last = holder(xyz, vdw, probe.ref["res"].x)
    others = [h for h in dict.fromkeys(holders) if h != last]
    g1 = None
    for a in others:                              # position 0 and position 31: the first and the last radius group
        if not two_radii or vdw[a] != vdw[last]:
            g1 = vdw[a]
            first = a
            break
    assert g1 is not None, "no holder of the other radius: change the seed"
    s1 = int((vdw[shell] == g1).sum())
    mid = None
    for b in others:
        if b != first and ((vdw[b] == g1) == (s1 > 16)):
            mid = b
            break
    assert mid is not None, "no third holder in the group that position 16 falls into: change the seed"
    grp = lambda i: 0 if vdw[i] == g1 else 1  # noqa: E731
    rest = [i for i in shell if i not in (first, mid, last)]
    seq = [first] + [i for i in rest if grp(i) == 0] + [i for i in rest if grp(i) == 1]
    seq.insert(16, mid)
    seq.append(last)
    assert [grp(i) for i in seq] == sorted(grp(i) for i in seq) and len(seq) == LIST4
    target = {0: 5, 16: 70, 31: 135}              # stored index of the three holders
    stored = []
    pool = {0: [i for i in far if grp(i) == 0], 1: [i for i in far if grp(i) == 1]}
    for pos, atom in enumerate(seq):
        if pos and grp(atom) != grp(seq[pos - 1]):
            stored += pool[0]                     # the first group ends: the rest of its far atoms
            pool[0] = []
        while pos in target and len(stored) < target[pos]:
            stored.append(pool[grp(atom)].pop())
        stored.append(atom)
    stored += pool[0] + pool[1] if grp(seq[-1]) == 0 else pool[1]
    assert len(stored) == len(xyz) and (not pool[0] or grp(seq[-1]) == 0)
    # an input order with this stored order: the groups interleaved at random, an atom of the first group first
    rng = np.random.default_rng(seed + 2000)
    a, b = [i for i in stored if grp(i) == 0], [i for i in stored if grp(i) == 1]
    order = [a.pop(0)]
    while a or b:
        take_a = bool(a) and (not b or rng.random() < len(a) / (len(a) + len(b)))
        order.append(a.pop(0) if take_a else b.pop(0))
    order = np.array(order)
    case = PoreCase(f"placed/{'two radii' if two_radii else 'one radius'}", xyz[order], vdw[order], np.full(len(xyz), 12.0),
                    probe.start, probe.box)
    assert np.array_equal(order[stored_order(case.vdw)], stored)
    return case


@functools.lru_cache(maxsize=None)
def shell_placed():
    return [_placed(False, 0), _placed(True, 0)]


def placed_facts(case):
    """(list position, stored index) of the holder at every recorded point, and of the final one."""
    pts = list(case.ref["points"]) + [case.ref["res"].x]
    out = []
    for p in pts:
        h = holder(case.xyz, case.vdw, p)
        out.append((list_position(case.xyz, case.vdw, p, h), stored_index(case.vdw, h)))
    return out[:-1], out[-1]


# the first frame of the synthetic trajectory whose run to two bounds stops on the projected gradient and whose run with
# mixed bound kinds ends ABNORMAL (cc3_boxes): with the other boxes, every ending SciPy has
CC3_FRAME = 171


@functools.lru_cache(maxsize=None)
def cc3():
    """(coordinates, radii, masses) of one noisy CC3 frame, its centre of mass and the pore radius there."""
    from oracle import pw_oracle as O

    elements, base = synth.load_cc3_base()
    ids = E.element_ids(elements)
    xyz = synth.noisy_frame(base, synth.SEED_BASE + CC3_FRAME)
    cage = O.Cage(xyz, E.VDW[ids], E.MASS[ids])
    com = O.centre_of_mass(cage)
    return xyz, E.VDW[ids], E.MASS[ids], com, O.pore_diameter(cage, com)[0] / 2


@functools.lru_cache(maxsize=None)
def cc3_boxes():
    xyz, vdw, mass, com, r = cc3()
    t = r / 10
    rel = lambda name, start, box: PoreCase(  # noqa: E731
        f"cc3/{name}", xyz, vdw, mass, com + np.array(start),
        [(None if a is None else c + a, None if b is None else c + b) for c, (a, b) in zip(com, box)])
    return [
        rel("tenth", (0.0, 0.0, 0.0), [(-t, t)] * 3),
        rel("start on an upper bound", (0.0, t, 0.0), [(-t, t)] * 3),
        rel("start in a corner", (-t, t, -t), [(-t, t)] * 3),
        rel("ends on two bounds", (2.0, -1.5, 1.0), [(-3.0, 3.0)] * 3),
        rel("thin axis", (0.1, 0.0, -0.1), [(-t, t), (-4e-9, 4e-9), (-t, t)]),
        rel("open", (0.2, 0.1, -0.3), [(None, None)] * 3),
        rel("mixed kinds", (0.2, 0.1, -0.3), ((None, None), (-0.4, None), (None, 0.2))),
    ]


FAR_SHIFTS = (18250.0, 18265.0)          # 3 s^2 either side of the 1e9 at which a rebuild stops listing


@functools.lru_cache(maxsize=None)
def cc3_far():
    xyz, vdw, mass, com, r = cc3()
    # (the centre of mass goes to (s, s, s); start and box as opt_pore_diameter builds them)
    return [PoreCase(f"cc3/far {s:g}", xyz + (s - com), vdw, mass, np.full(3, s), [(s - r, s + r)] * 3) for s in FAR_SHIFTS]


@functools.lru_cache(maxsize=None)
def pore_cases():
    return shell_small() + shell_placed() + shell_wide() + cc3_boxes() + cc3_far() + [tilted_case()]


#: the names of pore_cases(), for parametrising without building a case at collection
PORE_NAMES = ("shell31/box0.1", "shell32/box0.1", "shell33/box0.1", "placed/one radius", "placed/two radii", "shell32/box1",
              "shell33/box1", "shell65/box1", "cc3/tenth", "cc3/start on an upper bound", "cc3/start in a corner",
              "cc3/ends on two bounds", "cc3/thin axis", "cc3/open", "cc3/mixed kinds", "cc3/far 18250", "cc3/far 18265", "tilted32/thin box")


def pore_case(name):
    cases = pore_cases()
    assert tuple(c.name for c in cases) == PORE_NAMES
    return cases[PORE_NAMES.index(name)]


def neighbours():
    """Two ordinary CC3 frames of other sizes (atoms dropped from the end: hydrogens), ragged company in a launch."""
    elements, base = synth.load_cc3_base()
    ids = E.element_ids(elements)
    out = []
    for seed, n in ((11, len(base) - 5), (12, len(base) - 17)):
        out.append((synth.noisy_frame(base, synth.SEED_BASE + seed)[:n], E.VDW[ids][:n], E.MASS[ids][:n]))
    return out


def mixed_batch(case):
    """[CC3 frame, the case, CC3 frame] as one batch; the case is unit 1."""
    (x0, v0, m0), (x2, v2, m2) = neighbours()
    parts = [(x0, v0, m0), (case.xyz, case.vdw, case.mass), (x2, v2, m2)]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    return _lib.Batch(off, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                      np.concatenate([p[2] for p in parts]))


# ---- window cases --------------------------------------------------------------------------------------------------
RIMS = (20, 32, 33, 63, 64, 65)
LAST_HOLDER = {64: 63, 65: 64}       # rim size -> list position the holder of the final minimum is put at


@contextlib.contextmanager
def counted_window_fits():
    """Counts the objective evaluations of each ``window_fit`` call of the oracle (the capture's n_eval column)."""
    from oracle import pw_oracle as O

    calls = [0]
    per_fit = []
    gap, fit = O.Cage.gap, O.window_fit

    def counting_gap(self, point):
        calls[0] += 1
        return gap(self, point)

    def counting_fit(*a, **kw):
        before = calls[0]
        out = fit(*a, **kw)
        per_fit.append(calls[0] - before)
        return out

    O.Cage.gap, O.window_fit = counting_gap, counting_fit
    try:
        yield per_fit
    finally:
        O.Cage.gap, O.window_fit = gap, fit


class WindowCase:
    def __init__(self, m, xyz, vdw, name=None, **options):
        """``options``: window_analysis's keywords (z_bounds, lb_z), for the oracle and as the context's params."""
        self.name, self.m, self.options = name or f"rim{m}", m, options
        self.xyz, self.vdw, self.mass = np.ascontiguousarray(xyz), np.ascontiguousarray(vdw), np.full(len(xyz), 12.0)

    def __repr__(self):
        return self.name

    def batch(self):
        return _lib.Batch(np.array([0, len(self.xyz)], np.int64), self.xyz, self.vdw, self.mass)

    @functools.cached_property
    def ref(self):
        from oracle import pw_oracle as O

        detail = {}
        with counted_window_fits() as evals:
            win = O.find_windows(O.Cage(self.xyz, self.vdw, self.mass), detail, **self.options)
        return {"win": win, "detail": detail, "evals": evals}

    def analyse_debug(self, ctx):
        """(records, stage captures) of the case on ``ctx``, under the case's options."""
        with ctx.lock:
            if self.options:
                ctx.set_params(_lib.Params(**self.options))
            try:
                return ctx.analyse_debug(self.batch(), WINDOW_STAGES)
            finally:
                if self.options:
                    ctx.set_params(None)

    def final_point(self):
        w = self.ref["detail"]["windows"][0]
        return np.array([w["xy"][0], w["xy"][1], w["z"].x[0]])


def _rim_molecule(m, seed=0, hole=3.5, shell_r=8.0, vdw=1.2):
    rng = np.random.default_rng(seed + m)
    s = fibonacci(300) * shell_r
    axis = np.hypot(s[:, 0], s[:, 1])
    s = s[~((s[:, 2] > 0) & (axis < hole + 0.9))]
    t = 2 * np.pi * (np.arange(m) + rng.uniform(0, 1)) / m
    rr = hole + rng.uniform(-0.003, 0.003, size=m)
    rim = np.stack([rr * np.cos(t), rr * np.sin(t), np.full(m, np.sqrt(shell_r ** 2 - hole ** 2))], axis=1)
    xyz = np.concatenate([s, rim])
    is_rim = np.arange(len(xyz)) >= len(s)
    perm = rng.permutation(len(xyz))
    return xyz[perm] + np.array([1.5, -0.7, 0.9]), is_rim[perm]


@functools.lru_cache(maxsize=None)
def window_case(m):
    xyz, is_rim = _rim_molecule(m)
    vdw = np.full(len(xyz), 1.2)
    case = WindowCase(m, xyz, vdw)
    case.is_rim = is_rim
    want = LAST_HOLDER.get(m)
    for _ in range(4):
        if want is None:
            break
        w = case.ref["detail"]["windows"][0]
        h = holder(w["rot"], case.vdw, case.final_point())
        if list_position(w["rot"], case.vdw, case.final_point(), h) == want:
            break
        # one radius: stored order = input order; the holder goes behind every other rim atom
        order = np.array([i for i in range(len(xyz)) if i != h] + [h])
        xyz, is_rim = case.xyz[order], case.is_rim[order]
        case = WindowCase(m, xyz, vdw)
        case.is_rim = is_rim
    return case


FAR_Z = 31700.0          # FAR_Z^2 is just above the 1e9 at which a rebuild stops listing


@functools.lru_cache(maxsize=None)
def window_far_z():
    """The rim of 20 with the neck search held at z >= FAR_Z (z_bounds, lb_z=False): it ends on that bound, and the
    in-plane search starts |p|^2 >= 1e9 from the origin of its frame -- no list, whatever the count -- and, the
    objective having no minimum out there, walks away until Nelder-Mead's tolerances stop it."""
    base = window_case(20)
    case = WindowCase(20, base.xyz, base.vdw, "rim20/far z", z_bounds=(FAR_Z, None), lb_z=False)
    case.is_rim = base.is_rim
    return case


def window_cases():
    return [window_case(m) for m in RIMS]


def check_window_capture(case, rec, dbg, where):
    """Record and stage capture of one unit against the oracle's find_windows(detail): everything bit for bit."""
    ref = case.ref
    tag = f"{where} {case.name}"
    assert int(rec["status"]) == 0 and int(rec["n_windows"]) == len(ref["win"][0]) == 1, (tag, rec["status"], rec["n_windows"])
    d = ref["detail"]
    ns = len(d["kept"])
    assert int(dbg["n_survivors"]) == ns and np.array_equal(dbg["pass_idx"][:ns], d["kept"]), tag
    assert np.array_equal(dbg["labels"][:ns], d["labels"]), tag
    w, o = dbg["win"][0], d["windows"][0]
    assert np.array_equal(w[0:3], o["vector"]), (tag, "vector")
    a1, a2 = _raw_angles(o["vector"])
    assert w[3] == a1 and w[4] == a2, (tag, "angles", w[3], a1, w[4], a2)
    assert w[5] == o["fine"][0], (tag, "neck position")
    assert w[7] == o["z"].x[0], (tag, "z optimum", w[7], o["z"].x[0])
    assert w[8] == o["xy"][0] and w[9] == o["xy"][1], (tag, "in-plane optimum", w[8:10], o["xy"])
    assert w[10] == ref["win"][0][0], (tag, "diameter", w[10], ref["win"][0][0])
    assert int(w[11]) == ref["evals"][0], (tag, "evaluations", w[11], ref["evals"][0])
    assert np.array_equal(rec["win_d"][:1], ref["win"][0]), (tag, "win_d")
    assert np.array_equal(np.asarray(rec["win_c"])[:1], ref["win"][1]), (tag, "win_c", rec["win_c"][0], ref["win"][1])


def _raw_angles(v):
    """What angle_between_vectors returned for the chosen vector (the capture's angle columns)."""
    from oracle import pw_oracle as O

    return O._angle(np.array([v[0], v[1], 0]), np.array([1, 0, 0])), O._angle(v, np.array([0, 0, 1]))


def diff_fields(a, b):
    """Names of the fields in which two records (or captures) differ, for a message."""
    return [k for k in a.dtype.names if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
