"""Batches for the launch-cap hook (pw_stat_host.hpp: launch_blocks; pw_internal_launch_cap), shared by
tests/test_launch_cap.py (CPU: what every batch puts next to what is ASSERTED from its packed records, and the host
path is shown to ignore the hook) and tests/test_gpu_launch_cap.py (device at 1, 2, 3 and 5 workgroups a launch against
the host path on the same packed arrays).

The kernels reached are those whose workgroups walk the work items of a launch with
`for (item = blockIdx.x; item < total; item += gridDim.x)`.  Without the hook a workgroup takes a second item only
beyond 65536 items; with it a batch of a dozen items sends every workgroup round the loop, at cap 1 one workgroup
through the whole batch in order.  So the batches are tiny and ORDERED: each thing that must be right only on a second
turn -- LDS left by the item before, per-item state, a table refilled for a job of other sizes, an item skipped ahead of
a barrier -- follows its opposite at least once.  Every entry is built from its own case module (C.pack, C.raw, C.same,
C.first_difference); tile sizes come from the sources (`_stat_edges.constant`).

`Entry.kernels` lists the capped kernels the batch launches, one name a launch of its one launch group: the hook's
counter must reach their number at every cap, since every one of them has at least 2 x 5 items."""
import functools

import numpy as np

import _affinity_cases as A
import _basins_cases as BA
import _hop_cases as HO
import _passage_cases as PA
import _percolation_cases as PC
import _rigid_cases as R
import _stat_edges as S

CAPS = (1, 2, 3, 5)
STAT_CAPS = (1, 3)
MIN_ITEMS = 2 * max(CAPS)
REAL_CAP = 65536                                                     # (checked against the sources by test_launch_cap.py)


def chunk():
    return S.constant("AFF_CHUNK", "pw_affinity.hpp")


def chunks_of(voxels):
    return -(-int(voxels) // chunk())


def follows(values, earlier, later):
    """Whether some job for which `later` holds comes right after one for which `earlier` holds."""
    return any(earlier(a) and later(b) for a, b in zip(values[:-1], values[1:]))


def last_chunks(voxels):
    """The voxels of the last chunk of every job that has one."""
    return {int(v) - (chunks_of(v) - 1) * chunk() for v in voxels if v}


# ---- the field body (pw_field_dev.hpp, pw_field_cell_dev.hpp) and pw_affinity ----------------------------------------
def field_shapes(tile):
    """(dims, atoms) of the jobs of a field batch, in order: 65 voxels (a last chunk of 1) with a few atoms; more than a
    tile of atoms right after it, the last chunk full; no atom right after that (no barrier is taken and no LDS written:
    the item must not inherit U or the LDS of the job before); one chunk exactly; more than two tiles on three chunks;
    no atom again on a grid of 12 voxels; one tile exactly."""
    return [((5, 13, 1), 5), ((8, 8, 2), tile + 2), ((7, 5, 2), 0), ((4, 4, 4), 3), ((43, 3, 1), 2 * tile + 1), ((3, 2, 2), 0),
            ((6, 5, 2), tile)]


def field_properties(n, voxels, tile):
    n = [int(v) for v in n]
    return {
        "a job without atoms follows one with atoms": follows(n, lambda a: a > 0, lambda b: b == 0),
        "a job with atoms follows one without": follows(n, lambda a: a == 0, lambda b: b > 0),
        "more than a tile of atoms follows less than a tile": follows(n, lambda a: 0 < a < tile, lambda b: b > tile),
        "less than a tile follows more than two tiles": follows(n, lambda a: a > 2 * tile, lambda b: b < tile),
        "a last chunk of 1 voxel": 1 in last_chunks(voxels),
        "a last chunk of 64 voxels": chunk() in last_chunks(voxels),
    }


class Entry:
    """One entry under the hook.  `jobs()` the batch, `packed()` its arrays with one entry nobody owns in front of every
    job's outputs, `run(ctx, packed)` -> (rc, result), `items(packed)` -> {kernel: work items}, `properties(packed)` ->
    {what the batch puts next to what: bool}."""
    caps = CAPS
    hole = 1
    out_index = 0

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return self.C.pack(self.jobs(), hole=self.hole)

    def run(self, ctx, packed):
        return self.C.raw(ctx, packed)

    def same(self, got, want):
        return self.C.same(got, want)

    def out_rows(self, got):
        """The rows of `out` of a result: one a job and `hole` nobody owns in front of each."""
        return got[self.out_index]

    def first_difference(self, got, want):
        return self.C.first_difference(got, want)


class Affinity(Entry):
    name, C = "pw_affinity", A
    kernels = ("pw_affinity_kernel",)

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        tile = S.constant("AFF_TILE", "pw_affinity.hpp")
        # (count of the mask or None, betas, edges): a masked job after an unmasked one and back, L and E of every kind
        extra = [(None, (0.4,), ()), (128, (0.4, 1.0), (-1.0, 0.0, 5.0)), (None, (0.0, 0.3, 0.7), (0.0,)), (64, (0.4,), ()),
                 (None, np.linspace(0.0, 2.0, 8), np.linspace(-3.0, 3.0, 16)), (1, (0.2, 0.9), (-0.5, 0.5)), (None, (0.4,), (0.0,))]
        shapes = field_shapes(tile)
        shapes[1] = ((8, 8, 4), shapes[1][1])                        # (room for a mask of 128 voxels)
        out = []
        for k, ((dims, n), (count, betas, edges)) in enumerate(zip(shapes, extra)):
            words = None if count is None else A.words_with(dims, count, 900 + k)
            out.append(A.Case(f"cap-{k}", dims, *A.shell_atoms(n, dims, 0.7, 910 + k), words=words, h=0.7,
                              cutoff2=(0.0, 16.0)[k % 2], betas=betas, edges=edges))
        return out

    def items(self, packed):
        return {"pw_affinity_kernel": sum(chunks_of(v) for v in packed[10])}

    def properties(self, packed):
        rec, tile = packed[0], S.constant("AFF_TILE", "pw_affinity.hpp")
        masked = [int(w) >= 0 for w in rec["word_first"]]
        out = field_properties(rec["n"], packed[10], tile)
        out["a masked job follows an unmasked one"] = follows(masked, lambda a: not a, lambda b: b)
        out["an unmasked job follows a masked one"] = follows(masked, lambda a: a, lambda b: not b)
        out["n_betas of 1, 2, 3 and 8"] = {1, 2, 3, 8} <= set(rec["n_betas"].tolist())
        out["n_edges of 0, 1, 3 and 16"] = {0, 1, 3, 16} <= set(rec["n_edges"].tolist())
        out["fewer betas and edges follow more"] = follows(list(zip(rec["n_betas"].tolist(), rec["n_edges"].tolist())),
                                                           lambda a: a == (8, 16), lambda b: b[0] < 8 and b[1] < 16)
        return out


class FieldEntry(Entry):
    """An entry whose field kernel is the shared body: every job of the batch has atoms or none, never a caller's field."""

    def items(self, packed):
        rec = packed[0]
        assert (rec["field_first"] < 0).all()
        return {self.kernels[0]: sum(chunks_of(int(a) * int(b) * int(c)) for a, b, c in zip(rec["nx"], rec["ny"], rec["nz"]))}

    def properties(self, packed):
        rec = packed[0]
        voxels = [int(a) * int(b) * int(c) for a, b, c in zip(rec["nx"], rec["ny"], rec["nz"])]
        return field_properties(rec["n"], voxels, S.constant("PAS_FIELD_TILE", "pw_passage.hpp"))


def _box_shapes():
    return field_shapes(S.constant("PAS_FIELD_TILE", "pw_passage.hpp"))


class Passage(FieldEntry):
    name, C = "pw_passage", PA
    kernels = ("pw_passage_field_kernel",)

    def out_rows(self, got):
        return got

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        out = []
        for k, (dims, n) in enumerate(_box_shapes()):
            atoms = A.shell_atoms(n, dims, 0.7, 920 + k)
            probe = PA.Case(f"cap-{k}", dims, (0, 0, 0), xyz=atoms[0], coef=atoms[1], h=0.7, cutoff2=(0.0, 16.0)[k % 2])
            U = PA.field_of(probe)
            l, j, i = np.unravel_index(int(np.argmin(U)), U.shape)   # (the seed where the field is lowest: the result shows it)
            planes = [[1.0, 0.0, 0.0, 0.7 * (dims[0] - 1.5)], [0.0, 1.0, 0.2, 100.0]] if k % 3 == 1 else None
            out.append(PA.Case(f"cap-{k}", dims, (int(i), int(j), int(l)), xyz=atoms[0], coef=atoms[1], planes=planes, h=0.7,
                               cutoff2=(0.0, 16.0)[k % 2]))
        return out


class Hop(FieldEntry):
    name, C = "pw_hop", HO
    kernels = ("pw_hop_field_kernel",)
    out_index = 2

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        return [HO.seeded(f"cap-{k}", dims, None, *A.shell_atoms(n, dims, 0.7, 930 + k), h=0.7, cutoff2=(0.0, 16.0)[k % 2],
                          cap=50.0, betas=((0.4,), (0.2, 0.9))[k % 2], words=k % 2 == 0)
                for k, (dims, n) in enumerate(_box_shapes())]


class Percolation(FieldEntry):
    name, C = "pw_percolation", PC
    kernels = ("pw_percolation_field_kernel",)
    out_index = 1

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        out = []
        for k, (dims, n) in enumerate(_box_shapes()):
            step = PC.SKEW if k % 2 else (0.5, 0.0, 0.5, 0.0, 0.0, 0.5)
            xyz, coef = PC._atoms(n, dims, step, 940 + k)
            out.append(PC.Case(f"cap-{k}", dims=dims, xyz=xyz, coef=coef, core2=0.09, cutoff2=(0.0, 6.25)[k % 2], origin=(0.1, -0.2, 0.3),
                               step=step, map=k != 3, brute=False))
        return out


class Basins(FieldEntry):
    name, C = "pw_basins", BA
    kernels = ("pw_basins_field_kernel",)

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        return [BA.Case(c.name, dims=c.dims, xyz=c.xyz, coef=c.coef, core2=c.core2, cutoff2=c.cutoff2, origin=c.origin, step=c.step,
                        map=c.map, brute=False, labels=k % 2 == 0, cap=BA.INF if k % 3 else 50.0, b_cap=160, e_cap=640,
                        betas=(0.4,) if k % 2 else (0.1, 0.5, 0.9))
                for k, c in enumerate(Percolation().jobs())]


# ---- pw_rigid_affinity -----------------------------------------------------------------------------------------------
def rigid_class(S_, charged):
    """pw_rigid.hip: rigid_class."""
    return (S_ - 1 if S_ <= 3 else 3) * 2 + (1 if charged else 0)


def rigid_shapes(tile):
    """(dims, atoms, S, M, charged) of a rigid batch, in order: seven jobs of seven instance classes, charged and not in
    turn; S = 1, 3 and above 3 (the guarded instance); M = 1 first, 9 second and 5 third, so the directions are refilled
    with fewer after more and the largest M is not the first; more than a tile of atoms first and again in the fifth job,
    each followed by a job that stages its atoms once."""
    return [((5, 13, 1), tile + 2, 1, 1, 0), ((8, 8, 1), 4, 3, 9, 1), ((7, 5, 2), 7, 5, 5, 0), ((4, 4, 4), 3, 1, 5, 1),
            ((43, 3, 1), tile + 1, 3, 1, 0), ((3, 2, 2), 5, 4, 9, 1), ((6, 5, 2), 6, 2, 5, 0)]


def rigid_properties(n, S_, M, charged, voxels, tile):
    n, S_, M, charged = ([int(v) for v in a] for a in (n, S_, M, charged))
    classes = [rigid_class(s, c) for s, c in zip(S_, charged)]
    return {
        "at least three instance classes, each next to another": len(set(classes)) >= 3 and all(a != b for a, b in zip(classes[:-1], classes[1:])),
        "a charged job follows an uncharged one": follows(charged, lambda a: not a, lambda b: b),
        "an uncharged job follows a charged one": follows(charged, lambda a: a, lambda b: not b),
        "S of 1, 3 and above 3": {1, 3} <= set(S_) and max(S_) > 3,
        "fewer sites follow more": follows(S_, lambda a: a > 3, lambda b: b <= 3),
        "M of 1, 5 and 9": {1, 5, 9} <= set(M),
        "the largest M is not the first job's": M[0] < max(M),
        "fewer directions follow more": follows(M, lambda a: a == 9, lambda b: b == 5),
        "atoms staged once follow atoms staged tile by tile": follows(n, lambda a: a > tile, lambda b: b <= tile),
        "atoms staged tile by tile follow atoms staged once": follows(n, lambda a: a <= tile, lambda b: b > tile),
        "a last chunk of 1 voxel": 1 in last_chunks(voxels),
        "a last chunk of 64 voxels": chunk() in last_chunks(voxels),
    }


class Rigid(Entry):
    name, C = "pw_rigid_affinity", R

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        out = []
        for k, (dims, n, S_, M, charged) in enumerate(rigid_shapes(S.constant("AFF_TILE", "pw_affinity.hpp"))):
            words = R.words_with(dims, 40, 950 + k) if k == 2 else None   # (70 voxels of which 40: one masked job)
            out.append(R.Case(f"cap-{k}", dims, *R.guest_atoms(n, S_, dims, 0.7, 960 + k), offsets=R.line(S_, 0.4),
                              dirs=R.unit_dirs(M, 970 + k), words=words, h=0.7, cutoff2=(0.0, 16.0)[k % 2],
                              betas=((0.4,), (0.0, 0.8), (0.1, 0.5, 0.9))[k % 3], charged=charged, map_level=(k % 3) - 1 if k % 3 else -1))
        return out

    @property
    def kernels(self):
        rec = self.packed()[0]
        return tuple(f"pw_rigid_kernel<class {c}>" for c in sorted({rigid_class(int(s), int(q)) for s, q in zip(rec["n_sites"], rec["charged"])}))

    def items(self, packed):
        total = sum(chunks_of(v) for v in packed[10])
        return {k: total for k in self.kernels}                      # (every instance walks every item of the launch)

    def properties(self, packed):
        rec = packed[0]
        return rigid_properties(rec["n"], rec["n_sites"], rec["n_dirs"], rec["charged"], packed[10], S.constant("AFF_TILE", "pw_affinity.hpp"))


# ---- pw_rigid_cell and pw_rigid_cell_ewald -----------------------------------------------------------------------------
def cell_shapes(tile, near_cap):
    """(dims, listed atoms, S, M, charged, rows K, cell atoms) of a batch on the crystal cell, in order.
    0: a (5, 6, 7) grid (every group cut at an edge), more than a tile of atoms that all survive: staged tile by tile.
    1: a (9, 2, 3) grid right after it -- the longer x axis and the shorter y and z axes refill s_axis -- six atoms staged
       once, S = 3, M = 9 (orientation tiles of 4, 4 and 1).
    2: uncharged between two charged ones; more survivors than the near list holds: the list is built in segments.
    3: charged without a row (K = 0), S above 3, M = 5 (4 and 1); its near list is `single` after the segments.
    4: uncharged, S = 2, M = 6 (4 and 2).
    5: charged, S = 3, M = 7 (4 and 3): its row 0 of the tables kernel is a workgroup's second item at every cap.
    6: charged, S = 1, M = 66 (tiles of 4 and a last one of 2): more orientations than lanes in the tables kernel, and
       the largest M is the last job's."""
    return [((5, 6, 7), tile + 20, 1, 1, 1, 7, 5), ((9, 2, 3), 6, 3, 9, 1, 5, 67), ((4, 4, 4), near_cap + 150, 1, 1, 0, 4, 3),
            ((3, 3, 2), 10, 5, 5, 1, 0, 4), ((6, 5, 2), 8, 2, 6, 0, 6, 3), ((2, 3, 5), 12, 3, 7, 1, 9, 9), ((3, 2, 1), 4, 1, 66, 1, 3, 2)]


def groups_of(n):
    return -(-int(n) // S.constant("RCELL_G", "pw_rigid_cell.hpp"))


@functools.lru_cache(maxsize=None)
def ewald_jobs():
    import _ewald_cases as E

    out = []
    tile, near_cap = S.constant("AFF_TILE", "pw_affinity.hpp"), S.constant("RCELL_NEAR_CAP", "pw_rigid_cell.hpp")
    for k, (dims, n, S_, M, charged, K, n_cell) in enumerate(cell_shapes(tile, near_cap)):
        step = E.SKEW if k in (1, 5) else E.C.ortho(0.5)
        # (jobs 0 and 2: every listed atom within the cutoff of every voxel, so the survivors are the atoms)
        inputs = E.make_inputs(n, S_, M, dims, step, 800 + 10 * k, n_cell=n_cell, K=K, pad=1.0 if k in (0, 2) else 2.0, top=3)
        out.append(E.Job(f"cap-{k}", inputs, dims, step=step, core2=0.0025 if k in (0, 2) else 0.04, cutoff2=100.0 if k in (0, 2) else 6.25,
                         betas=((0.4,), (0.3, 0.9), (0.0, 0.5, 1.0))[k % 3], alpha=0.2 if k in (0, 2) else 0.5, charged=charged, map=k != 4))
    return out


def cell_properties(rec, n_pairs, charged=None, K=None, kvecs=None):
    """`rec`: the RIGID_CELL_JOB_DTYPE records; n_pairs: the host path's count of (atom, orientation, site, voxel) tuples
    behind the skip, which for the jobs whose atoms all survive tells the length of the near list."""
    tile, near_cap = S.constant("AFF_TILE", "pw_affinity.hpp"), S.constant("RCELL_NEAR_CAP", "pw_rigid_cell.hpp")
    n, S_, M = ([int(v) for v in rec[f]] for f in ("n", "n_sites", "n_dirs"))
    dims = [(int(a), int(b), int(c)) for a, b, c in zip(rec["nx"], rec["ny"], rec["nz"])]
    voxels = [a * b * c for a, b, c in dims]
    all_survive = [int(p) == a * b * c * v and a > 0 for p, a, b, c, v in zip(n_pairs, n, M, S_, voxels)]
    # the near list: in segments when more atoms survive than it holds; single (and staged once) when the job has at
    # most a tile of atoms at all
    segments = [ok and a > near_cap for ok, a in zip(all_survive, n)]
    tiled = [ok and tile < a <= near_cap for ok, a in zip(all_survive, n)]
    once = [a <= tile for a in n]
    classes = [s - 1 if s <= 3 else 3 for s in S_]
    ot = S.constant("EWALD_OT", "pw_ewald.hpp")
    out = {
        "at least three instance classes, each next to another": len(set(classes)) >= 3 and all(a != b for a, b in zip(classes[:-1], classes[1:])),
        "S of 1, 3 and above 3": {1, 3} <= set(S_) and max(S_) > 3,
        "fewer sites follow more": follows(S_, lambda a: a > 3, lambda b: b <= 3),
        "M of 1, 5 and 9": {1, 5, 9} <= set(M),
        "the largest M is not the first job's": M[0] < max(M),
        "fewer directions follow more": follows(M, lambda a: a == 9, lambda b: b < 9),
        "atoms staged once follow atoms staged tile by tile": follows(list(zip(tiled, once)), lambda a: a[0], lambda b: b[1]),
        "a single near list follows one built in segments": follows(list(zip(segments, once)), lambda a: a[0], lambda b: b[1]),
        "segments follow a single list": follows(list(zip(segments, once)), lambda a: a[1], lambda b: b[0]),
        "(5, 6, 7) then (9, 2, 3): a longer axis and shorter ones": follows(dims, lambda a: a == (5, 6, 7), lambda b: b == (9, 2, 3)),
        "the grids of neighbouring jobs differ": all(a != b for a, b in zip(dims[:-1], dims[1:])),
        "a shorter axis follows a longer one along x, y and z": all(follows([d[q] for d in dims], lambda a: a > 4, lambda b: b < 4) for q in range(3)),
        "a grid cut by its groups and one that is not": any(all(d % 4 for d in a) for a in dims) and any(not any(d % 4 for d in a) for a in dims),
    }
    if charged is not None:
        charged, K = [int(v) for v in charged], [int(c) and int(v) for c, v in zip(charged, K)]
        live = {m - (-(-m // ot) - 1) * ot for m, c, rows in zip(M, charged, K) if rows} | {ot for m, rows in zip(M, K) if rows and m > ot}
        out.update({
            "a charged job follows an uncharged one": follows(charged, lambda a: not a, lambda b: b),
            "an uncharged job between two charged ones": any(a and not b and c for a, b, c in zip(charged[:-2], charged[1:-1], charged[2:])),
            "a charged job without a row": any(c and not rows for c, rows in zip(charged, K)),
            "orientation tiles with 1, 2, 3 and 4 live orientations": live >= set(range(1, ot + 1)),
            "indices of both signs": bool((kvecs[:, :3] < 0).any() and (kvecs[:, :3] > 0).any()),
            "a job's row 0 is beyond the largest cap": sum(1 for rows, first in zip(K, np.cumsum([0] + K[:-1])) if rows and first >= max(CAPS)) >= 2,
            "M above 64 once": sum(m > 64 for m, rows in zip(M, K) if rows) == 1,
        })
    return out


class RigidCell(Entry):
    name = "pw_rigid_cell"

    @property
    def C(self):
        import _rigid_cell_cases as RC

        return RC

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        return [j.uncharged_case() for j in ewald_jobs()]

    @property
    def kernels(self):
        rec = self.cell_records(self.packed())
        return tuple(f"pw_rigid_cell_kernel<class {c}>" for c in sorted({min(int(s), 4) - 1 for s in rec["n_sites"]})) + ("pw_rigid_cell_sums_kernel",)

    def cell_records(self, packed):
        return packed[0]

    def items(self, packed):
        rec = self.cell_records(packed)
        groups = sum(groups_of(a) * groups_of(b) * groups_of(c) for a, b, c in zip(rec["nx"], rec["ny"], rec["nz"]))
        chunks = sum(chunks_of(int(a) * int(b) * int(c)) for a, b, c in zip(rec["nx"], rec["ny"], rec["nz"]))
        return {k: chunks if k == "pw_rigid_cell_sums_kernel" else groups for k in self.kernels if k.startswith("pw_rigid_cell")}

    def pairs(self, packed):
        from pywindow_amd import _lib

        got = []
        rc, _ = self.C.raw(_lib.Context(-1, host_threads=4), packed, diagnostics=got)
        assert rc == 0
        return got[0][0]

    def properties(self, packed):
        return cell_properties(packed[0], self.pairs(packed))


class RigidCellEwald(RigidCell):
    name = "pw_rigid_cell_ewald"

    @property
    def C(self):
        import _ewald_cases as E

        return E

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        return ewald_jobs()

    @property
    def kernels(self):
        return RigidCell.kernels.fget(self) + ("pw_ewald_tables_kernel", "pw_ewald_urec_kernel")

    def cell_records(self, packed):
        return packed[0]["cell"]

    def run(self, ctx, packed):
        return 0, self.C.run(ctx, packed)                            # (a failure raises)

    def first_difference(self, got, want):
        return self.C.C.first_difference(got, want)

    def items(self, packed):
        rec, cell = packed[0], packed[0]["cell"]
        ot = S.constant("EWALD_OT", "pw_ewald.hpp")
        out = RigidCell.items(self, packed)
        K = [int(c) and int(v) for c, v in zip(rec["charged"], rec["n_k"])]
        out["pw_ewald_tables_kernel"] = sum(K)
        out["pw_ewald_urec_kernel"] = sum(groups_of(a) * groups_of(b) * groups_of(c) * -(-int(m) // ot)
                                          for rows, a, b, c, m in zip(K, cell["nx"], cell["ny"], cell["nz"], cell["n_dirs"]) if rows)
        return out

    def pairs(self, packed):
        from pywindow_amd import _lib

        got = []
        self.C.run(_lib.Context(-1, host_threads=4), packed, diagnostics=got)
        return got[0][0]

    def properties(self, packed):
        rec = packed[0]
        return cell_properties(rec["cell"], self.pairs(packed), rec["charged"], rec["n_k"], packed[8])


# ---- pw_charges and pw_charges_cell ------------------------------------------------------------------------------------
def solver_sizes(lds_atoms):
    """The atoms of the jobs of a solver batch, in order (0: the breakdown case of the entry): LDS jobs of falling sizes, a
    job beyond the LDS capacity -- the LDS instance skips it ahead of its barrier, the other instance skips all the rest
    -- , LDS jobs of rising sizes, then breakdown, converging, breakdown and a last larger job.  The dynamic LDS is sized
    for the largest LDS job, which is neither the first nor the last."""
    return [65, 129, 64, 3, lds_atoms + 1, 1, 2, 63, 0, 3, 0, 66]


def solver_properties(n, flags, lds_atoms, breakdown):
    n, flags = [int(v) for v in n], [int(v) for v in flags]
    lds = [v <= lds_atoms for v in n]
    broke = [bool(f & breakdown) for f in flags]
    clean = [f == 0 for f in flags]
    return {
        "LDS jobs of falling sizes": any(a > b > c and all(lds[k:k + 3]) for k, (a, b, c) in enumerate(zip(n[:-2], n[1:-1], n[2:]))),
        "LDS jobs of rising sizes": any(a < b < c and all(lds[k:k + 3]) for k, (a, b, c) in enumerate(zip(n[:-2], n[1:-1], n[2:]))),
        "one job beyond the LDS capacity between LDS jobs": lds.count(False) == 1 and 0 < lds.index(False) < len(n) - 1,
        "a smaller LDS job follows the largest": follows([v if ok else 0 for v, ok in zip(n, lds)], lambda a: a == max(v for v, ok in zip(n, lds) if ok),
                                                        lambda b: 0 < b),
        "the largest LDS job is not the first": n[0] < max(v for v, ok in zip(n, lds) if ok),
        "a converging job follows the breakdown": follows(list(zip(broke, clean)), lambda a: a[0], lambda b: b[1]),
        "the breakdown follows a converging job": follows(list(zip(broke, clean)), lambda a: a[1], lambda b: b[0]),
    }


class Charges(Entry):
    name, out_index = "pw_charges", 1
    kernels = ("pw_charges_kernel<true>", "pw_charges_kernel<false>")
    lds = ("CHG_LDS_ATOMS", "pw_charges.hpp")

    @property
    def C(self):
        import _charges_cases as Q

        return Q

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        Q = self.C
        out = []
        for k, n in enumerate(solver_sizes(S.constant(*self.lds))):
            if n == 0:
                out.append(Q.breakdown_case())
            elif n == 3:
                out.append(Q.converging_cluster(3, 1700 + k))
            else:                                                    # (a 30 Angstrom box: positive definite; a few steps are enough)
                x, p = Q.cluster(n, 1700 + k)
                out.append(Q.Case(f"cap-{k}", 2.5 * x, p, tol=1e-4, max_iter=12, converges=False))
        return out

    def items(self, packed):
        return {k: len(packed[0]) for k in self.kernels}             # (a job is an item of both instances: one of them skips it)

    def host_flags(self, packed):
        from pywindow_amd import _lib

        rc, (_, rows) = self.C.raw(_lib.Context(-1, host_threads=4), packed)
        assert rc == 0
        return rows["flags"][packed[0]["out"]]

    def properties(self, packed):
        return solver_properties(packed[0]["n"], self.host_flags(packed), S.constant(*self.lds), 2)


class ChargesCell(Charges):
    name = "pw_charges_cell"
    kernels = ("chc_solve_kernel<true>", "chc_solve_kernel<false>")
    lds = ("CHC_LDS_ATOMS", "pw_charges_cell.hpp")

    @property
    def C(self):
        import _charges_cell_cases as QC

        return QC

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        QC = self.C
        out = []
        for k, n in enumerate(solver_sizes(S.constant(*self.lds))):
            if n == 0:
                out.append(QC.breakdown_case())
            elif n == 3:
                out.append(QC.gas_case(3, 1800 + k, QC.ORTHO))
            else:                                                    # (short rows, as the capacity jobs of tests/test_gpu_charges_cell.py)
                c = QC.gas_case(n, 1800 + k, QC.SKEWED if k % 2 else QC.ORTHO, cutoff=6.0, tolerance=1e-3, tol=1e-4, max_iter=12, converges=False)
                # no row next to 65 rows: jobs 0 and 1
                out.append(c.but(f"cap-{k}", alpha=0.0, kvecs=np.zeros((0, 4))) if k == 0 else c.but(f"cap-{k}", kvecs=c.kvecs[:65].copy()) if k == 1 else c)
        return out

    def properties(self, packed):
        out = Charges.properties(self, packed)
        nk = packed[0]["n_k"].tolist()
        out["n_k == 0 next to n_k == 65"] = follows(nk, lambda a: a == 0, lambda b: b == 65)
        return out


# ---- the statistical entries that clamp a grid: the edge batch of tests/test_gpu_stat_edges.py ----------------------------
STAT_ENTRIES = tuple(e for e in S.ENTRIES if e.name in ("kde", "kde2", "kdew", "corr"))
#: the capped kernels of one launch of each (partial, reduce)
STAT_KERNELS = {"kde": ("pw_kde_partial_kernel", "pw_kde_reduce_kernel"), "kde2": ("pw_kde2_partial_kernel", "pw_kde2_reduce_kernel"),
                "kdew": ("pw_kdew_partial_kernel", "pw_kdew_reduce_kernel"), "corr": ("pw_corr_partial_kernel", "pw_corr_reduce_kernel")}


GRID_ENTRIES = (Affinity(), Passage(), Hop(), Percolation(), Basins(), Rigid(), RigidCell(), RigidCellEwald(), Charges(), ChargesCell())


# ---- one launch past the real cap (pw_affinity, hook off) -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def past_the_cap_jobs():
    """Sixteen unmasked 64^3 jobs of one atom and one beta (4096 items each: 65536), then a masked (3, 2, 2) grid with
    five atoms, two betas and two edges: item 65536, workgroup 0's second."""
    big = (64, 64, 64)
    jobs = [A.Case(f"big-{k}", big, *A.shell_atoms(1, big, 0.25, 980 + k), h=0.25, betas=(0.3 + 0.05 * k,)) for k in range(16)]
    d = (3, 2, 2)
    jobs.append(A.Case("the-17th", d, *A.shell_atoms(5, d, 1.0, 999), words=A.words_with(d, 7, 998), betas=(0.4, 1.0), edges=(-0.5, 0.5)))
    return jobs
