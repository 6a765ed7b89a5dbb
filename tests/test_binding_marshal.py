"""The Python binding of the grid, charge and crystal entries (pywindow_amd/_lib.py, Context.cavity ... Context.hop): what
each wrapper hands the library and what it hands back, as BYTES against the `raw` helpers of the case files, which build
their ctypes calls themselves.  Tiny jobs on the host context (device = -1); the tests marked `gpu` run the same jobs on
the device and want the bytes of the host context, to show that the order of pointers and lengths reaches the device
entries as well.  No test here says what an entry computes: tests/test_<entry>.py do."""
import re

import numpy as np
import pytest

import _affinity_cases as AF
import _basins_cases as BA
import _cavity_cases as CV
import _channels_cases as CH
import _charges_cases as Q
import _charges_cell_cases as QC
import _ewald_cases as EW
import _hop_cases as HO
import _passage_cases as PA
import _percolation_cases as PC
import _pores_cases as PO
import _rigid_cases as RI
import _rigid_cell_cases as RC
import _sasa_cases as SA
from pywindow_amd import _lib


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=2)


@pytest.fixture(params=["host", pytest.param("device", marks=pytest.mark.gpu)])
def ctx(request, host):
    return host if request.param == "host" else request.getfixturevalue("hip_ctx")


def named(cases, *names):
    by_name = {c.name: c for c in cases}
    return [by_name[n] for n in names]


class Entry:
    """One wrapper and how the case file of its entry packs, blanks and calls.  `names`: the result keywords of the
    wrapper in the order of `raw`'s tuple; `returns`: the same names in the order of the wrapper's tuple; `given`: the
    names the wrapper takes; `none`: the names it returns as None when no job has one; `jobs` / `bare` / `opened`:
    lists of cases -- every result owned, no optional result owned, ready-made open words; `optional`: [(cases,
    input keywords that are empty for them)]; `routes`: keyword sets of the measurement route that change no byte."""

    def __init__(self, method, module, jobs, pack, inputs, names, blank, returns=None, given=None, none=(), bare=None,
                 opened=None, optional=(), routes=(), timer=("workspace_bytes", "kernel_ms"), times=1, raw=None,
                 allocating=None, bad=None, diagnostics=None):
        self.method, self.module, self.jobs, self.pack, self.inputs = method, module, jobs, pack, inputs
        self.names, self.blank = names, blank
        self.returns, self.given, self.none = returns or names, given or names, none
        self.bare, self.opened, self.optional, self.routes, self.timer, self.times = bare, opened, optional, routes, timer, times
        self.raw_call = raw or (lambda ctx, packed: module.raw(ctx, packed))
        self.allocating = allocating or (lambda: pack(jobs(), 1))
        self.bad = bad or (lambda: next((b[0], b[-1]) for b in module.bad_batches() if all(v is None or v == () for v in b[1:-1])))
        self.diagnostics = diagnostics

    def __repr__(self):
        return self.method

    def raw(self, ctx, packed):
        rc, got = self.raw_call(ctx, packed)
        assert rc == 0, (self.method, _lib.load().pw_last_error().decode())
        return got if isinstance(got, tuple) else (got,)

    def call(self, ctx, packed, given=None, without=(), **kw):
        """The wrapper on the packed arrays, its results in the order of `raw`'s."""
        args, keywords = self.inputs(packed)
        keywords = {k: v for k, v in keywords.items() if k not in without}
        if given is not None:
            keywords.update((n, a) for n, a in zip(self.names, given) if n in self.given)
        got = getattr(ctx, self.method)(*args, **keywords, **kw)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(self.returns)
        return tuple(got[self.returns.index(n)] for n in self.names)


def same(got, want):
    return all(g is not None and g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def zeros_of(blank):
    return tuple(np.zeros(len(a), dtype=a.dtype) for a in blank)


# ---- the fourteen entries ------------------------------------------------------------------------------------------
def _cavity_with_planes():
    return CV.lattice_job("with-planes", (9, 8, 7), 6, 42, planes=[[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0]])


cavity = Entry(
    "cavity", CV, lambda: named(CV.cases(), "cut-in-two-(3, 3, 3)") + [_cavity_with_planes()],
    lambda jobs, hole, **kw: CV.pack(jobs, hole, **kw), lambda p: (p[:3], dict(planes=p[3])), ("out", "mask"),
    lambda p: CV.blank(p[4], p[5]), none=("mask",), bare=lambda: CV.pack(named(CV.cases(), "no-atoms-(2, 2, 2)"), 0, mask=False),
    opened=lambda: named(CV.cases(), "word-edge-nx=5-bit=4", "cut-in-two-(3, 3, 3)", "word-edge-nx=63-bit=0"),
    optional=[(lambda: named(CV.cases(), "no-atoms-(2, 2, 2)", "cut-in-two-(3, 3, 3)"), ("planes",))])
cavity.open = lambda p: dict(open_words=p[6], open_first=p[7])


def _sasa_jobs(grid=True):
    xyz, radii = SA.random_atoms(6, 3.0, 41)
    u = SA.spiral(64)
    jobs = [SA.Case("good", xyz, radii, u), SA.Case("other", xyz[:5] + 0.5, radii[:5], u, probe=0.5)]
    if grid:
        jobs.append(SA.Case("gridded", xyz[:4] - 0.5, radii[:4], u, dims=(9, 8, 7), h=0.5, words=np.arange(56, dtype=np.uint64)))
    return jobs


sasa = Entry(
    "sasa", SA, _sasa_jobs, lambda jobs, hole: SA.pack(jobs, hole), lambda p: (p[:4], dict(words=p[4])), ("out", "exposed", "inside"),
    lambda p: SA.blank(p[6], p[5]), optional=[(lambda: _sasa_jobs(grid=False), ("words",))], timer=("kernel_ms",),
    routes=[lambda p: dict(block_atoms=2), lambda p: dict(list_capacity=-1, lds_words=-1, block_atoms=7)])


def _pores_jobs():
    return [PO.lattice_case("other", (9, 8, 7), 6, 41, [0.0, 0.5, 1.0]),
            PO.lattice_case("with-planes", (9, 8, 7), 6, 42, [0.0, 0.5], planes=[[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, 2.0]])]


pores = Entry(
    "pore_sizes", PO, _pores_jobs, lambda jobs, hole, **kw: PO.Packed(jobs, hole, **kw),
    lambda P: ((P.rec, P.xyz, P.radii, P.probes), dict(planes=P.planes)), ("levels", "out", "mask"), lambda P: P.blank(), none=("mask",),
    bare=lambda: PO.Packed(_pores_jobs()[:1], 0, masks=False),
    opened=lambda: named(PO.cases(), "word-edge-nx=5-bit=4", "word-edge-nx=1-bit=0") + _pores_jobs()[:1],
    optional=[(lambda: _pores_jobs()[:1], ("planes",))])
pores.open = lambda P: dict(open_words=P.words, open_first=P.open_first)

affinity = Entry(
    "affinity", AF, lambda: named(AF.cases(), "V=1", "no-mask-3x2x2"), lambda jobs, hole, **kw: AF.pack(jobs, hole, **kw),
    lambda p: ((p[0], p[1], p[2], p[4]), dict(words=p[3], edges=p[5])), ("out", "levels", "hist", "energies"), AF.blank_of,
    allocating=lambda: AF.pack(named(AF.cases(), "V=1", "no-mask-3x2x2"), 1, energies=False),
    optional=[(lambda: named(AF.cases(), "no-mask-64x1x1"), ("words", "edges"))])

rigid = Entry(
    "rigid_affinity", RI, lambda: named(RI.cases(), "V=1", "no-mask-3x2x2"), lambda jobs, hole, **kw: RI.pack(jobs, hole, **kw),
    lambda p: ((p[0], p[1], p[2], p[3], p[4], p[6]), dict(words=p[5])), ("out", "levels", "maps"), RI.blank_of,
    allocating=lambda: RI.pack(named(RI.cases(), "V=1", "no-mask-3x2x2"), 1, maps=False),
    optional=[(lambda: named(RI.cases(), "no-mask-3x2x2"), ("words",))])


def _pairs_and_instances(jobs, item):
    n_pairs, instances = item
    return n_pairs.dtype == np.int64 and n_pairs.shape == (len(jobs),) and type(instances) is int


def _two_counts(jobs, item):
    return len(item) == 2 and all(a.dtype == np.int32 and a.shape == (len(jobs),) for a in item)


rigid_cell = Entry(
    "rigid_cell", RC, lambda: named(RC.cases(), "n=1", "M=2"), lambda jobs, hole: RC.pack(jobs, hole), lambda p: (p[:6], {}),
    ("out", "levels", "maps"), lambda p: RC.blank(p[8], p[7], p[6]), none=("maps",),
    bare=lambda: RC.pack(named(RC.cases(), "no-map"), 0), routes=[lambda p: dict(skip=False)], diagnostics=_pairs_and_instances)


def _ewald_raw(ctx, packed):
    """pw_rigid_cell_ewald through ctypes into SENTINEL-filled arrays (the case file has no `raw`: its tests call the
    wrapper)."""
    rec = np.ascontiguousarray(packed[0], dtype=_lib.RIGID_CELL_EWALD_JOB_DTYPE)
    out, levels, maps = RC.blank(packed[11], packed[10], packed[9])
    args = [ctx._h, rec.ctypes.data, len(rec)]
    for a in packed[1:9] + (maps, levels, out):
        args += [a.ctypes.data, len(a)]
    return _lib.load().pw_rigid_cell_ewald(*args), (out, levels, maps)


def _ewald_bad():
    packed = list(EW.pack(EW.shared_jobs()[4:6]))
    packed[0] = packed[0].copy()
    packed[0]["alpha"][1] = np.nan
    return tuple(packed), "alpha is not finite"


ewald = Entry(
    "rigid_cell_ewald", EW, lambda: [EW.shared_jobs()[q] for q in (1, 2, 5)], lambda jobs, hole: EW.pack(jobs, hole),
    lambda p: (p[:9], {}), ("out", "levels", "maps"), lambda p: RC.blank(p[11], p[10], p[9]), none=("maps",),
    bare=lambda: EW.pack(EW.shared_jobs()[1:2], 0), routes=[lambda p: dict(skip=False)], raw=_ewald_raw, bad=_ewald_bad,
    diagnostics=_pairs_and_instances)


def _charges_raw(module):
    def raw(ctx, packed):
        """The case file's `raw` with the charges as the wrapper returns them: up to the furthest entry of a job, zero
        where no job writes (the wrapper takes no charges of the caller's)."""
        rc, (q, rows) = module.raw(ctx, packed)
        charges = np.zeros(packed[-1])
        for r in packed[0]:
            charges[r["charge_first"]:r["charge_first"] + r["n"]] = q[r["charge_first"]:r["charge_first"] + r["n"]]
        return rc, (charges, rows)
    return raw


def _charges_blank(module):
    return lambda p: (np.zeros(p[-1]), module.blank(p)[1])


charges = Entry(
    "charges", Q, lambda: [Q.Case("good 0", *Q.cluster(5, 61)), Q.Case("good 1", *Q.cluster(7, 62))],
    lambda jobs, hole: Q.pack(jobs, hole), lambda p: (p[:3], {}), ("charges", "out"), _charges_blank(Q), given=("out",),
    raw=_charges_raw(Q))

charges_cell = Entry(
    "charges_cell", QC, lambda: [QC.gas_case(5, 61, QC.ORTHO, converges=False), QC.gas_case(7, 62, QC.SKEWED, converges=False)],
    lambda jobs, hole: QC.pack(jobs, hole), lambda p: (p[:4], {}), ("charges", "out"), _charges_blank(QC), given=("out",),
    raw=_charges_raw(QC), times=3)


def _channels_jobs(**kw):
    return [CH.lattice_job("other", (9, 8, 7), 6, 41, c_max=4, **kw), CH.lattice_job("small", (5, 4, 3), 4, 42, c_max=3, **kw)]


channels = Entry(
    "channels", CH, _channels_jobs, lambda jobs, hole: CH.pack(jobs, hole), lambda p: (p[:3], {}), ("out", "comps", "mask", "labels"),
    lambda p: CH.blank(*p[3:7]), none=("comps", "mask", "labels"),
    bare=lambda: CH.pack([CH.lattice_job("bare", (5, 4, 3), 4, 42, c_max=0, mask=False, labels=False)], 0),
    opened=lambda: named(CH.cases(), "channel-along-a", "slab") + _channels_jobs()[1:])
channels.open = lambda p: dict(open_words=p[7], open_first=p[8])


def _percolation_jobs():
    return [PC.Case("field-with-map", named(PC.cases(), "ties-(3, 4, 5)")[0].field, map=True)] + named(PC.atom_cases(), "orthorhombic-n=1")


_lattice = [(lambda: named(PC.cases(), "ties-(3, 4, 5)", "normal-(1, 5, 6)"), ("xyz", "coef")),
            (lambda: named(PC.atom_cases(), "orthorhombic-n=1"), ("field",))]

percolation = Entry(
    "percolation", PC, _percolation_jobs, lambda jobs, hole: PC.pack(jobs, hole), lambda p: (p[:1], dict(xyz=p[1], coef=p[2], field=p[3])),
    ("levels", "out", "maps"), lambda p: PC.blank(*p[4:7]), none=("maps",), bare=lambda: PC.pack(named(PC.cases(), "ties-(3, 4, 5)"), 0),
    optional=_lattice, diagnostics=_two_counts)

basins = Entry(
    "basins", BA,
    lambda: named(BA.cases(), "ties-(3, 4, 5)") + named(BA.atom_cases(), "orthorhombic-n=1") + named(BA.cases(), "ties-blocked-(3, 4, 5)"),
    lambda jobs, hole: BA.pack(jobs, hole), lambda p: (p[:1], dict(xyz=p[1], coef=p[2], field=p[3])),
    ("out", "basins", "edges", "labels", "maps"), lambda p: BA.blank(*p[4:9]), returns=("out", "basins", "edges", "maps", "labels"),
    none=("maps", "labels"), bare=lambda: BA.pack(named(BA.cases(), "normal-(3, 4, 5)"), 0),
    optional=[(lambda: named(BA.cases(), "ties-(3, 4, 5)", "normal-(3, 4, 5)"), ("xyz", "coef")),
              (lambda: named(BA.atom_cases(), "orthorhombic-n=1"), ("field",))], diagnostics=_two_counts)


def _two_planes():
    return [[1, 0, 0, 3.0], [0, 1, 0, 3.0]]


def _passage_jobs(planes=True):
    xyz, coef = AF.shell_atoms(6, (9, 8, 7), 0.5, 60)
    cuts = _two_planes() if planes else None
    return [PA.Case("atoms", (9, 8, 7), (4, 4, 3), xyz=xyz, coef=coef, planes=cuts, h=0.5),
            PA.Case("field", (5, 4, 3), (2, 2, 1), field=PA.random_field((5, 4, 3), 61), planes=cuts)]


passage = Entry(
    "passage", PA, _passage_jobs, lambda jobs, hole: PA.pack(jobs, hole),
    lambda p: (p[:1], dict(xyz=p[1], coef=p[2], planes=p[3], field=p[4])), ("out",), lambda p: (PA.blank(p[5]),),
    optional=[(lambda: _passage_jobs(planes=False)[1:], ("xyz", "coef", "planes")),
              (lambda: _passage_jobs(planes=False)[:1], ("field", "planes"))],
    routes=[lambda p: dict(grids=3), lambda p: dict(fills=np.zeros(p[5], dtype=np.int32))])


def _hop_jobs(planes=True, **kw):
    xyz, coef = AF.shell_atoms(6, (9, 8, 7), 0.5, 60)
    cuts = _two_planes() if planes else None
    return [HO.Case("atoms", (9, 8, 7), (4, 4), None, xyz, coef, planes=cuts, h=0.5, betas=(0.4, 0.9), **kw),
            HO.Case("field", (5, 4, 3), (2, 2), HO.random_field((5, 4, 3), 61), planes=cuts, betas=(0.4, 0.9), **kw)]


hop = Entry(
    "hop", HO, _hop_jobs, lambda jobs, hole: HO.pack(jobs, hole),
    lambda p: ((p[0], p[5]), dict(xyz=p[1], coef=p[2], planes=p[3], field=p[4])),
    ("slabs", "sums", "out", "words"), lambda p: HO.blank(p[6]), none=("words",), bare=lambda: HO.pack(_hop_jobs(words=False), 0),
    optional=[(lambda: _hop_jobs(planes=False)[1:], ("xyz", "coef", "planes")), (lambda: _hop_jobs(planes=False)[:1], ("field", "planes"))],
    times=3)

ENTRIES = [cavity, sasa, pores, affinity, rigid, rigid_cell, ewald, charges, charges_cell, channels, percolation, basins, passage, hop]
every_entry = pytest.mark.parametrize("e", ENTRIES, ids=repr)


# ---- results ---------------------------------------------------------------------------------------------------------
@every_entry
def test_given_results(ctx, host, e):
    """SENTINEL-filled arrays go in by keyword and come back as the same objects with the bytes of `raw` on the host
    context: entries no job owns keep the SENTINEL."""
    packed = e.pack(e.jobs(), 1)
    want = e.raw(host, packed)
    blank = e.blank(packed)
    got = e.call(ctx, packed, given=blank)
    assert all(g is b for n, g, b in zip(e.names, got, blank) if n in e.given)
    assert same(got, want), e
    assert any(w.tobytes() != b.tobytes() for w, b in zip(want, e.blank(packed)))        # (something was written)
    for n, w in zip(e.names, want):
        if n in e.given:                                                                  # (a hole in front of every job)
            assert bytes([e.module.SENTINEL]) * w.dtype.itemsize == w[0].tobytes(), (e, n)


@pytest.mark.parametrize("e", [cavity, pores, channels], ids=repr)
def test_open_words(ctx, host, e):
    """`open_words` / `open_first` reach the measurement entry as `raw` hands them over."""
    packed = e.pack(e.opened(), 1)
    assert same(e.call(ctx, packed, given=e.blank(packed), **e.open(packed)), e.raw(host, packed)), e
    assert not same(e.call(ctx, packed, given=e.blank(packed)), e.raw(host, packed))     # (the words decide)


@every_entry
def test_allocated_results(host, e):
    """Without the result keywords every array is made here: zeros of the dtype up to the furthest entry a job owns (the
    sizes of `pack`), filled like zeros of the caller's; None where no job has such a result."""
    for packed in (e.allocating(),) + ((e.bare(),) if e.bare else ()):
        want = e.call(host, packed, given=zeros_of(e.blank(packed)))
        got = e.call(host, packed)
        for n, g, w in zip(e.names, got, want):
            if n in e.none and len(w) == 0:
                assert g is None, (e, n)
            else:
                assert same([g], [w]), (e, n)
    if e.bare:
        assert all(len(a) == 0 for n, a in zip(e.names, e.blank(e.bare())) if n in e.none)
    if e is affinity:
        assert len(got[3]) == 0
    if e is rigid:
        assert len(got[2]) == 0


@every_entry
def test_an_empty_batch(host, e):
    packed = e.pack([], 1)
    got = e.call(host, packed)
    for n, g, b in zip(e.names, got, e.blank(packed)):
        assert len(b) == 0
        assert g is None if n in e.none else (g.dtype == b.dtype and g.shape == (0,)), (e, n)
    assert same(e.call(host, packed, given=e.blank(packed)), e.blank(packed))


@pytest.mark.parametrize("e", [e for e in ENTRIES if e.optional], ids=repr)
def test_optional_inputs(host, e):
    """An input left out gives the bytes of the explicit empty array."""
    for jobs, names in e.optional:
        packed = e.pack(jobs(), 1)
        assert all(len(e.inputs(packed)[1][n]) == 0 for n in names)
        assert same(e.call(host, packed, given=e.blank(packed), without=names), e.raw(host, packed)), (e, names)


# ---- the measurement route ---------------------------------------------------------------------------------------
@every_entry
def test_measurement_route(ctx, host, e):
    """The measurement keywords change no byte; `kernel_ms` and `diagnostics` receive one item a call."""
    jobs = e.jobs()
    packed = e.pack(jobs, 1)
    want = e.raw(host, packed)
    times = []
    keywords = {"workspace_bytes": 0, "kernel_ms": times}
    assert same(e.call(ctx, packed, given=e.blank(packed), **{k: keywords[k] for k in e.timer}), want), e
    assert len(times) == 1
    if e.times == 1:
        assert type(times[0]) is float
    else:
        assert type(times[0]) is tuple and len(times[0]) == e.times and all(type(t) is float for t in times[0])
    for route in e.routes:
        assert same(e.call(ctx, packed, given=e.blank(packed), **route(packed)), want), (e, route(packed).keys())
    if e.diagnostics:
        items = []
        assert same(e.call(ctx, packed, given=e.blank(packed), diagnostics=items), want), e
        assert len(items) == 1 and type(items[0]) is tuple and e.diagnostics(jobs, items[0])
    if e is passage:
        fills = np.full(packed[5], -1, dtype=np.int32)
        e.call(ctx, packed, given=e.blank(packed), fills=fills)
        assert (fills >= 0).sum() == sum(c.rows for c in jobs)


# ---- refusals ----------------------------------------------------------------------------------------------------
@every_entry
def test_results_the_binding_refuses(host, e):
    packed = e.pack(e.jobs(), 1)
    for q, name in enumerate(e.names):
        if name not in e.given:
            continue
        good = e.blank(packed)[q]
        wrong = np.int8 if good.dtype != np.int8 else np.uint8
        for bad in (np.zeros(len(good), dtype=wrong), np.zeros(2 * len(good) + 4, dtype=good.dtype)[::2],
                    np.zeros((2, len(good)), dtype=good.dtype)):
            given = list(e.blank(packed))
            given[q] = bad
            with pytest.raises(ValueError):
                e.call(host, packed, given=given)


@pytest.mark.parametrize("e", [cavity, pores, channels], ids=repr)
def test_open_words_the_binding_refuses(host, e):
    packed = e.pack(e.opened(), 1)
    opened = e.open(packed)
    with pytest.raises(ValueError):
        e.call(host, packed, open_words=opened["open_words"])
    with pytest.raises(ValueError):
        e.call(host, packed, open_first=opened["open_first"], kernel_ms=[])
    with pytest.raises(ValueError):
        e.call(host, packed, open_words=opened["open_words"], open_first=opened["open_first"][:-1])


def test_other_arguments_the_binding_refuses(host):
    packed = passage.pack(passage.jobs(), 1)
    for fills in (np.zeros(packed[5] + 1, dtype=np.int32), np.zeros(packed[5], dtype=np.int64), np.zeros((packed[5], 1), dtype=np.int32)):
        with pytest.raises(ValueError):
            passage.call(host, packed, fills=fills)
    packed = sasa.pack(sasa.jobs(), 1)
    out, exposed, inside = sasa.blank(packed)
    with pytest.raises(ValueError):
        sasa.call(host, packed, given=(out, exposed, np.concatenate([inside, inside])))
    for e in (charges, charges_cell):
        packed = e.pack(e.jobs(), 1)
        with pytest.raises(ValueError):
            e.call(host, packed, given=(None, e.blank(packed)[1][:-1]))


@every_entry
def test_what_the_library_refuses(host, e):
    """A refusal of the library's comes out as ValueError with its text."""
    packed, reason = e.bad()
    with pytest.raises(ValueError, match=re.escape(f"pw_{e.method}: job 1: ")) as raised:
        e.call(host, packed, given=e.blank(packed))
    assert reason in str(raised.value)
