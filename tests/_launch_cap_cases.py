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
counter must reach their number at every cap, since every one of them has at least 2 x 5 items.

The second half of the file has the trajectory entries (`TrajEntry`: pw_trans_counts, pw_superpose, pw_cluster_gromos,
pw_covariance, pw_project; `Shape`; the sweeps of pw_dft_sums and pw_gate_counts through `STAT_ENTRIES`), whose kernels
stride by workgroup, by wave or by thread behind caps of their own, and the two batches that pass a real cap with the
hook off (8200 frames, 4 x 65536 + 5 projected rows)."""
import functools
import itertools

import numpy as np

import _affinity_cases as A
import _basins_cases as BA
import _cluster_cases as CL
import _cov_cases as CV
import _dft_cases as DF
import _gate_cases as GA
import _hop_cases as HO
import _passage_cases as PA
import _percolation_cases as PC
import _rigid_cases as R
import _shape_cases as SH
import _stat_edges as S
import _superpose_cases as SU
import _trans_cases as TR

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
STAT_ENTRIES = S.ENTRIES                                             # (kde, kde2, kdew, corr, dft and gate with 0 and 5 bins)
#: the capped kernels of one launch of each (partial, reduce; dft: twiddle, partial, reduce; gate: chunk, merge)
STAT_KERNELS = {"kde": ("pw_kde_partial_kernel", "pw_kde_reduce_kernel"), "kde2": ("pw_kde2_partial_kernel", "pw_kde2_reduce_kernel"),
                "kdew": ("pw_kdew_partial_kernel", "pw_kdew_reduce_kernel"), "corr": ("pw_corr_partial_kernel", "pw_corr_reduce_kernel"),
                "dft": ("pw_dft_twiddle_kernel", "pw_dft_partial_kernel", "pw_dft_reduce_kernel")}
STAT_KERNELS.update({e.name: ("pw_gate_chunk_kernel", "pw_gate_merge_kernel") for e in S.ENTRIES if e.name.startswith("gate")})


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


# ---- the trajectory entries: pw_dft_sums, pw_gate_counts, pw_trans_counts, pw_superpose, pw_cluster_gromos,
# ---- pw_covariance, pw_project, pw_shape_batch ------------------------------------------------------------------------------
# Their kernels stride by workgroup, by wave or by thread; `items` is what the launch site hands to launch_blocks: the
# workgroups that would take one turn each.  Where an entry makes several launches of a kernel, `items` is the LARGEST of
# them -- the launch the batch is built for -- and `properties` says what lies next to what inside it.
def budget_constant(name: str, source: str) -> int:
    """A workspace budget written as `<a>l << <b>` in the sources."""
    import re

    from _util import ROOT

    m = re.search(rf"constexpr long {name} = (\d+)l? << (\d+)", (ROOT / "pywindow_amd" / "csrc" / source).read_text())
    return int(m.group(1)) << int(m.group(2))


def ceil_div(a, b):
    return -(-int(a) // int(b))


def dft_launches(rec):
    """pw_dft.hip: dft_plan at the default budget -- [(workgroups of the twiddle kernel, items of the partial kernel, items
    of the reduce kernel)] a launch."""
    k = S.dft_constants()
    C, T, GC = k["C"], k["W"] * k["F"], k["GW"] * k["WC"]
    RF = S.constant("DFT_RED_FREQS", "pw_dft.hip")
    budget = budget_constant("DFT_WORKSPACE_BYTES", "pw_dft.hpp") // 16
    launches, cur = [], None
    for J in rec:
        n, nf = int(J["n"]), int(J["n_freq"])
        if n == 0 or nf == 0:
            continue
        chunks = ceil_div(n, C)
        each = C + chunks
        slab = nf if each <= budget // nf else max(budget // each // T * T, T)
        for q0 in range(0, nf, slab):
            m = min(nf - q0, slab)
            if cur is not None and cur[0] + each * m > budget:
                launches.append(cur)
                cur = None
            cur = cur or [0, 0, 0, 0]
            cur[0] += each * m
            cur[1] += C * m
            cur[2] += ceil_div(m, T) * ceil_div(chunks, GC)
            cur[3] += ceil_div(m, RF)
    if cur is not None:
        launches.append(cur)
    return [(ceil_div(tw, 256), items, red) for _, tw, items, red in launches]


def gate_launches(rec):
    """pw_gate.hip: gate_plan at the default budget -- [(items of the chunk kernel, workgroups of the merge kernel)]."""
    C, T = GA.CHUNK, GA.TILE
    budget = budget_constant("GATE_WORKSPACE_BYTES", "pw_gate.hpp") // 4
    launches, cur = [], None
    for J in rec:
        n, nt = int(J["n"]), int(J["n_thr"])
        if n == 0 or nt == 0:
            continue
        chunks = ceil_div(n, C)
        slab = nt if chunks <= budget // nt else max(budget // chunks // T * T, T)
        for q0 in range(0, nt, slab):
            m = min(nt - q0, slab)
            if cur is not None and cur[0] + chunks * m > budget:
                launches.append(cur)
                cur = None
            cur = cur or [0, 0, 0]
            cur[0] += chunks * m
            cur[1] += ceil_div(m, T) * chunks
            cur[2] += m
    if cur is not None:
        launches.append(cur)
    return [(items, ceil_div(lanes, 256)) for _, items, lanes in launches]


def stat_items(entry, packed):
    """{kernel: the fewest work items of a launch of it} for the sweeps of pw_dft_sums and pw_gate_counts, which are one
    launch each at the default budget (asserted by tests/test_launch_cap.py)."""
    launches = dft_launches(packed[0]) if entry.name == "dft" else gate_launches(packed[0])
    return len(launches), {k: min(l[i] for l in launches) for i, k in enumerate(STAT_KERNELS[entry.name])}


#: the arguments of the twiddle hook (pw_dft_phase_kernel, thread-strided, 256 a workgroup): more than 2 x 256 x 5, not a
#: multiple of 256, with the edge arguments of _dft_cases.twiddle_cases among them
def twiddle_batch():
    rng = np.random.default_rng(41)
    j, period, k = DF.twiddle_cases()[-3]
    count = 2 * 256 * max(CAPS) + 77
    return j, period, np.concatenate([k, rng.integers(0, 1 << 32, count - len(k))]).astype(np.int64)


class TrajEntry:
    """One trajectory entry under the hook.  `packed()` the batch with rows nobody owns; `run(ctx, packed, budget)` -> a
    tuple of arrays (a failure raises); `untouched(got)` whether the rows nobody owns still hold the sentinel;
    `exact(got)` whether the independent exact reference holds (None: the entry has none); `items`, `properties` as for
    the grid entries.  `budgets`: the workspace budgets the batch runs at (None: the entry's default), the first with every
    kernel of `kernels` cut, the others with at least `cut_small` launches cut."""
    caps = CAPS
    budgets = (None,)
    cut_small = 1

    def same(self, got, want):
        return S.same(got, want)

    def exact(self, got):
        return None


def host_context():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=4)


# ---- pw_trans_counts ------------------------------------------------------------------------------------------------------
def trans_instance(n_states):
    """pw_trans.hpp: trans_padded and pw_trans.hip: trans_block -- (P, BI) of the instance a call of n_states runs."""
    P = 2 if n_states <= 2 else 4 if n_states <= 4 else 8 if n_states <= 8 else 16
    return P, (4 if P == 16 else P)


def trans_work(rec, n_states):
    """pw_trans_count_kernel's work items of one launch in order, as (job, chunk, tile, block of origin states, skipped,
    in_lds, wn, lanes): the restatement of the kernel's own arithmetic."""
    CW, WINW, TILE = TR.CHUNK // 32, TR.WINDOW // 32, TR.TILE
    _, BI = trans_instance(n_states)
    nob = ceil_div(n_states, BI)
    out = []
    for q, J in enumerate(rec):
        n, nl, first, step = int(J["n"]), int(J["n_lags"]), int(J["lag_first"]), int(J["lag_step"])
        if n == 0 or nl == 0:
            continue
        nw = ceil_div(n, 32)
        for ch in range(ceil_div(nw, CW)):
            for tile in range(ceil_div(nl, TILE)):
                for b in range(nob):
                    wn = min(nw - ch * CW, CW)
                    lanes = min(nl - tile * TILE, TILE)
                    k_lo = first + tile * TILE * step
                    k_hi = min(first + (tile * TILE + lanes - 1) * step, n)
                    skipped = k_lo >= n
                    out.append((q, ch, tile, b, skipped, (not skipped) and wn + (k_hi >> 5) - (k_lo >> 5) + 1 <= WINW, wn, lanes))
    return out


class Trans(TrajEntry):
    """One call of pw_trans_counts at one n_states: A, a chunk and a word with 40 lags (idle lanes, the window in LDS);
    B, two chunks and a word with TILE lags FAR_STEP apart -- the window does not fit LDS in the two full chunks and does
    in the short last one --; B2, the same series with fewer edges and one lag more: its tile 1 is skipped (every lag
    >= n) between worked items; D, a chunk and a word with TILE + 3 lags (a full tile, then idle lanes; a full chunk after
    B2's short one); E, 40 entries (less than a wave of the pack kernel after jobs of many)."""
    def __init__(self, n_states):
        self.n_states = n_states
        self.name = f"pw_trans_counts-{n_states}-states"
        P, BI = trans_instance(n_states)
        self.kernels = (f"pw_trans_pack_kernel<{P}>", f"pw_trans_count_kernel<{P}, {BI}>")

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        S_ = self.n_states
        mid, long, short = TR.noise(TR.CHUNK + 1, 8), TR.noise(2 * TR.CHUNK + 1, 7), TR.noise(40, 9)
        full, fewer = TR.edges_for(S_ - 1), TR.edges_for(max(S_ - 2, 0))
        return [(mid, full, (0, 1, 40)), (long, full, (3, TR.FAR_STEP, TR.TILE)), (long, fewer, (3, TR.FAR_STEP, TR.TILE + 1)),
                (mid, full, (0, 1, TR.TILE + 3)), (short, full, (2, 3, 5))]

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return TR.pack(self.jobs(), hole=1)

    def run(self, ctx, packed, budget=None):
        rc, counts = TR.raw_counts(ctx, *packed, self.n_states, workspace_bytes=budget)
        assert rc == 0
        return (counts,)

    def owned(self, packed):
        rec = packed[0]
        return S._spans(int((rec["out_first"] + rec["n_lags"]).max()), rec["out_first"], rec["n_lags"])

    def untouched(self, got):
        return bool((got[0][~self.owned(self.packed())] == TR.SENTINEL).all())

    def exact(self, got):
        return bool(np.array_equal(got[0][self.owned(self.packed())], TR.reference_rows(self.jobs(), self.n_states)))

    def items(self, packed):
        rec = packed[0]
        waves = sum(ceil_div(int(n), 32) // 2 + 1 for n in rec["n"])
        return {self.kernels[0]: ceil_div(waves, 4), self.kernels[1]: len(trans_work(rec, self.n_states))}

    def properties(self, packed):
        rec = packed[0]
        work = trans_work(rec, self.n_states)
        CW, TILE = TR.CHUNK // 32, TR.TILE
        lds = [(w[5], not w[4] and not w[5]) for w in work]          # (in LDS, worked from global memory)
        skip = [w[4] for w in work]
        wn = [None if w[4] else w[6] for w in work]
        lanes = [None if w[4] else w[7] for w in work]
        return {
            "a window that does not fit LDS follows one that does": follows(lds, lambda a: a[0], lambda b: b[1]),
            "a window in LDS follows one that does not fit": follows(lds, lambda a: a[1], lambda b: b[0]),
            "a skipped tile between two worked ones": "wsw" in "".join(k for k, _ in itertools.groupby("s" if v else "w" for v in skip)),
            "a short last chunk follows a full one": follows([v for v in wn if v], lambda a: a == CW, lambda b: b < CW),
            "a full chunk follows a short one": follows([v for v in wn if v], lambda a: a < CW, lambda b: b == CW),
            "a tile with idle lanes follows a full tile": follows([v for v in lanes if v], lambda a: a == TILE, lambda b: b < TILE),
            "jobs of other n_edges follow each other": any(a != b for a, b in zip(rec["n_edges"][:-1], rec["n_edges"][1:])),
            "the pack kernel: n < 64 after a job of several waves": follows(rec["n"].tolist(), lambda a: a > 4 * 64, lambda b: b < 64),
        }


TRANS_STATES = (2, 4, 5, 16)                                         # P = 2, 4, 8, 16


# ---- pw_superpose -----------------------------------------------------------------------------------------------------------
class Superpose(TrajEntry):
    """391 jobs (6 x 64 + 7: no multiple of SUP_WAVES or of 64) that cycle through the case list of _superpose_cases --
    every size of SIZES, unsorted, weighted next to unweighted, the degenerate cases (identical, mirror image, collinear,
    planar, by 180 degrees) beside the random ones in every 64 consecutive jobs -- with `random n=1` moved behind
    `random n=4097`.  Caps 1 and 3: the solve kernel takes 64 jobs a workgroup, so that 2 x 5 workgroups of it would be
    more than 576 jobs where seven workgroups show the same second turn.  Runs again with a workspace of 100 jobs: four
    launches of each kernel."""
    name = "pw_superpose"
    caps = STAT_CAPS
    kernels = ("pw_superpose_moments_kernel", "pw_superpose_solve_kernel", "pw_superpose_residual_kernel")
    COUNT = 391

    @property
    def budgets(self):
        return (0, 100 * S.constant("SUP_MOMENT_FIELDS", "pw_superpose.hpp") * 8 + 100 * S.constant("SUP_SOLVE_FIELDS", "pw_superpose.hpp") * 8)

    cut_small = 2 * 4                                                # (four launches of the two wave-a-job kernels; the solve kernel's have two workgroups' worth)

    @functools.lru_cache(maxsize=None)
    def names(self):
        names = [c[0] for c in SU.cases()]
        names.remove("random n=1")
        names.insert(names.index(f"random n={max(SU.SIZES)}") + 1, "random n=1")
        return [names[k % len(names)] for k in range(self.COUNT)]

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        by_name = {c[0]: c[1:] for c in SU.cases()}
        return [by_name[n] for n in self.names()]

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return SU.pack(self.jobs(), hole=1)

    def run(self, ctx, packed, budget=None):
        rc, rows = SU.raw(ctx, *packed, workspace_bytes=budget)
        assert rc == 0
        return (rows,)

    def same(self, got, want):
        return SU.same_bytes(got[0], want[0])

    def untouched(self, got):
        rec = self.packed()[0]
        mask = np.ones(len(got[0]), dtype=bool)
        mask[rec["out"]] = False
        return bool(SU.untouched(got[0][mask]).all()) and int(mask.sum()) == len(rec)

    def items(self, packed):
        count = len(packed[0])
        waves = S.constant("SUP_WAVES", "pw_superpose.hip")
        return {self.kernels[0]: ceil_div(count, waves), self.kernels[1]: ceil_div(count, 64), self.kernels[2]: ceil_div(count, waves)}

    def properties(self, packed):
        rec = packed[0]
        n, weighted = rec["n"].tolist(), (rec["weight_first"] >= 0).tolist()
        sweeps = self.run(host_context(), packed)[0]["sweeps"][rec["out"]]
        degenerate = [any(w in name for w in ("identical", "mirror", "collinear", "planar", "180 degrees")) for name in self.names()]
        groups = [slice(g, g + 64) for g in range(0, len(rec), 64)]
        return {
            "no multiple of SUP_WAVES or of 64": len(rec) % S.constant("SUP_WAVES", "pw_superpose.hip") != 0 and len(rec) % 64 != 0,
            "a weighted job follows an unweighted one": follows(weighted, lambda a: not a, lambda b: b),
            "an unweighted job follows a weighted one": follows(weighted, lambda a: a, lambda b: not b),
            "n = 1 follows the largest": follows(n, lambda a: a == max(SU.SIZES), lambda b: b == 1),
            "every size, unsorted": set(SU.SIZES) <= set(n) and n != sorted(n) and n != sorted(n, reverse=True),
            "a degenerate job beside others in every workgroup of the solve kernel": all(any(degenerate[g]) and not all(degenerate[g]) for g in groups),
            "sweeps differ within every workgroup of the solve kernel": all(int(sweeps[g].max()) > int(sweeps[g].min()) for g in groups),
        }


# ---- pw_cluster_gromos ----------------------------------------------------------------------------------------------------------
class Cluster(TrajEntry):
    """Seven jobs in one launch group (jobs lie on blockIdx.y, the x grid is sized by the largest): n = 65; a 257-frame
    matrix at a middling cutoff; n = 1025, the largest, neither first nor last; the 257-frame matrix again at the cutoff
    that makes one cluster (done after one round; the pack kernel returns for it when the other matrices are packed);
    n = 129 with every frame a cluster of its own (130 rounds while the others return on done[]; four words a row for
    three that hold frames); n = 3; n = 64.  The number handed to launch_blocks is that of the launch for the largest job."""
    name = "pw_cluster_gromos"
    kernels = ("pw_cluster_pack_kernel", "pw_cluster_mirror_kernel", "pw_cluster_count_kernel")

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        by_name = {c[0]: c[1:] for c in CL.cases()}
        shared = by_name["n=257-middling"][0]
        return [by_name["n=65-middling"], (shared, by_name["n=257-middling"][1]), by_name["n=1025-middling"],
                (shared, by_name["n=257-one-cluster"][1]), by_name["n=129-all-singletons"], by_name["n=3-middling"], by_name["n=64-middling"]]

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return CL.pack(self.jobs(), hole=1)

    def run(self, ctx, packed, budget=None):
        rc, out = CL.raw(ctx, *packed, workspace_bytes=budget)
        assert rc == 0
        return out

    def same(self, got, want):
        return CL.same(got, want)

    def untouched(self, got):
        rec = self.packed()[0]
        mask = ~S._spans(len(got[0]), rec["out_first"], rec["n"])
        return int(mask.sum()) == len(rec) and all(bool((a[mask] == CL.SENTINEL).all()) for a in got[:3])

    def exact(self, got):
        return CL.same(got, CL.expected(self.jobs(), hole=1))

    def items(self, packed):
        n = int(packed[0]["n"].max())
        words = ceil_div(n, 64)
        stride = (words + 1) & ~1
        assert 8 * n * n <= budget_constant("CLUSTER_SLAB_BYTES", "pw_cluster.hpp")   # (the largest matrix is one slab)
        return {self.kernels[0]: ceil_div(n * stride, 4), self.kernels[1]: ceil_div(words * words, 4), self.kernels[2]: ceil_div(n, 4)}

    def properties(self, packed):
        rec = packed[0]
        n, first = rec["n"].tolist(), rec["d_first"].tolist()
        found = CL.expected(self.jobs(), hole=1)[3].tolist()
        words = sum(v * ((ceil_div(v, 64) + 1) & ~1) for v in n)
        return {
            "one launch group": 8 * words <= budget_constant("CLUSTER_BITS_BYTES", "pw_cluster.hpp"),
            "jobs of different n, the largest neither first nor last": len(set(n)) >= 5 and 0 < n.index(max(n)) < len(n) - 1,
            "sizes from NS up to 1025": set(n) <= set(CL.NS) and max(n) == 1025,
            "two jobs share a matrix at different cutoffs beside a job on another": any(
                first[a] == first[c] and first[b] != first[a] and rec["cutoff"][a] != rec["cutoff"][c]
                for a, b, c in zip(range(len(n) - 2), range(1, len(n) - 1), range(2, len(n)))),
            "a job done after one round beside the all-singletons job": follows(list(zip(n, found)), lambda a: a[1] == 1 and a[0] > 1,
                                                                                lambda b: b[1] == b[0] and b[0] > 64),
            "a row padded by a word": any(((ceil_div(v, 64) + 1) & ~1) > ceil_div(v, 64) for v in n),
            "every job but the smallest has frames for a second turn of a wave at cap 1": sum(v > 4 for v in n) >= len(n) - 1,
        }


PAST_THE_CAP_FRAMES = 8200
PAST_THE_CAP_CENTRE = 8195


def past_the_cap_cluster():
    """(the job record, the matrix): the distances of 8200 points on a line (broadcast from 1-D: no (n, n, k)
    intermediate) at the cutoff 1.0 -- four tight groups in shuffled order at 0, 1.5, 10 and 20, each one clique and none
    a neighbour of another, and frame PAST_THE_CAP_CENTRE = 8195 at 0.75, a neighbour of the first two groups and so
    the frame with the most neighbours: the first centre is a row that a wave of workgroup 0 meets on its second turn,
    larger than the `best` it carries from its first, and in the later rounds that row is inactive.  Three clusters:
    three rounds and one more.  540 MB of doubles: the caller builds it once, hands it on as it is and frees it."""
    from pywindow_amd import _lib

    rng = np.random.default_rng(8200)
    n = PAST_THE_CAP_FRAMES
    x = np.array([0.0, 1.5, 10.0, 20.0])[rng.integers(0, 4, n)] + rng.uniform(-0.05, 0.05, n)
    x[PAST_THE_CAP_CENTRE] = 0.75
    d = x[:, None] - x[None, :]
    np.abs(d, out=d)
    rec = np.zeros(1, dtype=_lib.CLUSTER_JOB_DTYPE)
    rec[0] = (0, n, 1.0, 0)
    return rec, d


# ---- pw_covariance and pw_project ------------------------------------------------------------------------------------------------
def cov_tiles(D):
    """pw_cov.hpp: cov_tile_of -- the tiles on or above the diagonal, row-major."""
    nt = ceil_div(D, CV.TILE)
    return [(a, b) for a in range(nt) for b in range(a, nt)]


class Covariance(TrajEntry):
    """Four jobs, each with launches of its own.  0: T = 2 CHUNK + 5, D = 2 TILE + 1 -- three chunks, the last of 5 rows
    (fewer than COV_STAGE) after full ones, and six tiles of which (0, 2) has one live column after the live (0, 1) and
    before the diagonal (1, 1): 18 items of the partial kernel.  1: moved, T = CHUNK + 1, D = 2 TILE - 1 (just under whole
    tiles).  2: the mean only, D = 2305 on two chunks: ten workgroups' worth of the mean kernel, twenty items of the
    column-sum kernel.  3: moved, T = 40, D = 3.  Runs again at a budget of two tiles of partials (the reduce kernel's
    c0 != 0 under the cap) and of one byte (every range one chunk, one tile: c0 != 0 in the mean kernel too)."""
    name = "pw_covariance"
    kernels = ("pw_cov_colsum_kernel", "pw_cov_mean_kernel", "pw_cov_partial_kernel", "pw_cov_reduce_kernel")
    cut_small = 1

    @property
    def budgets(self):
        return (None, 2 * 8 * CV.TILE * CV.TILE, 1)

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        rng = np.random.default_rng(1207)
        shapes = [(2 * CV.CHUNK + 5, 2 * CV.TILE + 1, False, True), (CV.CHUNK + 1, 2 * CV.TILE - 1, True, True),
                  (CV.CHUNK + 3, 9 * 256 + 1, False, False), (40, 3, True, True)]
        return [(np.ascontiguousarray(2.0 * rng.standard_normal((T, D)) + rng.uniform(-5, 5, D)), CV.transforms(rng, T) if mv else None, sc)
                for T, D, mv, sc in shapes]

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return CV.pack(self.jobs(), hole=1)

    def run(self, ctx, packed, budget=None):
        jobs, data, tr, mean, scatter, _ = packed
        mean, scatter = mean.copy(), scatter.copy()
        ctx.covariance(jobs, data, tr, mean=mean, scatter=scatter, workspace_bytes=budget)
        return mean, scatter

    def untouched(self, got):
        spans = self.packed()[5]
        m = ~CV.owned(len(got[0]), [s[0] for s in spans])
        s = ~CV.owned(len(got[1]), [s[1] for s in spans])
        return bool(CV.untouched(got[0][m]).all() and CV.untouched(got[1][s]).all()) and int(m.sum()) == len(spans) + 1

    def items(self, packed):
        rec = packed[0]
        lanes = S.constant("COV_LANES", "pw_cov.hip")
        chunks = [ceil_div(T, CV.CHUNK) for T in rec["T"]]
        tiles = [len(cov_tiles(D)) if s >= 0 else 0 for D, s in zip(rec["D"], rec["s_first"])]
        return {self.kernels[0]: max(c * ceil_div(D, lanes) for c, D in zip(chunks, rec["D"])),
                self.kernels[1]: max(ceil_div(D, lanes) for D in rec["D"]),
                self.kernels[2]: max(c * t for c, t in zip(chunks, tiles)),
                self.kernels[3]: max(t * CV.TILE * CV.TILE // lanes for t in tiles)}

    def properties(self, packed):
        rec = packed[0]
        stage = S.constant("COV_STAGE", "pw_cov.hip")
        T, D = int(rec["T"][0]), int(rec["D"][0])
        tiles = cov_tiles(D)
        dead = [(a + 1) * CV.TILE > D or (b + 1) * CV.TILE > D for a, b in tiles]
        budget = budget_constant("COV_WORKSPACE_BYTES", "pw_cov.hpp") // 8
        return {
            "job 0 is one launch of the partial kernel at the default budget": ceil_div(T, CV.CHUNK) * len(tiles) * CV.TILE * CV.TILE <= budget and rec["s_first"][0] >= 0,
            "D just over and just under whole tiles": any(d % CV.TILE == 1 for d in rec["D"]) and any(d % CV.TILE == CV.TILE - 1 for d in rec["D"]),
            "a tile with dead columns follows a live one": follows(dead, lambda a: not a, lambda b: b),
            "a live tile follows one with dead columns": follows(dead, lambda a: a, lambda b: not b),
            "a diagonal tile follows an off-diagonal one": follows(tiles, lambda a: a[0] != a[1], lambda b: b[0] == b[1]),
            "a last chunk shorter than COV_STAGE rows after full chunks": T > 2 * CV.CHUNK and 0 < T % CV.CHUNK < stage,
            "with and without transforms": {True, False} <= set((rec["transform_first"] >= 0).tolist()),
            "with and without the scatter matrix": {True, False} <= set((rec["s_first"] >= 0).tolist()),
        }


class Project(TrajEntry):
    """Four jobs, a launch each: k = 1, 8 and 9 (a second pass of COV_PROJ_VECTORS) and T = 41, 43, 42 and 45 rows -- no
    multiple of COV_PROJ_WAVES, eleven workgroups' worth and more -- with and without transforms, D = 3 .. 129."""
    name = "pw_project"
    kernels = ("pw_cov_project_kernel",)

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        rng = np.random.default_rng(1208)
        out = []
        for T, D, mv, k in ((41, CV.TILE + 1, False, 9), (43, 3, True, 1), (42, 2 * 63, True, 8), (45, 65, False, 9)):
            V = rng.standard_normal((k, D))
            out.append((np.ascontiguousarray(rng.standard_normal((T, D))), CV.transforms(rng, T) if mv else None, rng.standard_normal(D),
                        V / np.linalg.norm(V, axis=1, keepdims=True)))
        return out

    def packed(self):
        return tuple(self.jobs())

    def run(self, ctx, packed, budget=None):
        return (CV.project_batch(ctx, list(packed), hole=1)[1],)

    def spans(self):
        at, out = 0, []
        for X, _, _, V in self.jobs():
            out.append(slice(at + 1, at + 1 + len(X) * len(V)))
            at = out[-1].stop
        return out

    def untouched(self, got):
        mask = ~CV.owned(len(got[0]), self.spans())
        return int(mask.sum()) == len(self.jobs()) + 1 and bool(CV.untouched(got[0][mask]).all())

    def items(self, packed):
        return {self.kernels[0]: max(ceil_div(len(X), S.constant("COV_PROJ_WAVES", "pw_cov.hip")) for X, _, _, _ in packed)}

    def properties(self, packed):
        waves, vectors = S.constant("COV_PROJ_WAVES", "pw_cov.hip"), S.constant("COV_PROJ_VECTORS", "pw_cov.hip")
        ks = [len(V) for _, _, _, V in packed]
        return {
            "k of 1, COV_PROJ_VECTORS and one more": {1, vectors, vectors + 1} <= set(ks),
            "no T is a multiple of COV_PROJ_WAVES": all(len(X) % waves != 0 for X, _, _, _ in packed),
            "every launch has the items": all(ceil_div(len(X), waves) >= MIN_ITEMS for X, _, _, _ in packed),
            "with and without transforms": {True, False} <= {tr is not None for _, tr, _, _ in packed},
        }


PAST_THE_CAP_ROWS = 4 * 65536 + 5


def past_the_cap_projection():
    """pw_project past its real cap: T = 4 x 65536 + 5 rows of D = 3 on k = 2 vectors -- 65538 workgroups' worth."""
    rng = np.random.default_rng(65536)
    V = rng.standard_normal((2, 3))
    return [(np.ascontiguousarray(rng.standard_normal((PAST_THE_CAP_ROWS, 3))), None, rng.standard_normal(3), V / np.linalg.norm(V, axis=1, keepdims=True))]


# ---- pw_shape_batch (no host path: the reference is the host build of pw_shape.hpp, as in tests/test_gpu_shape.py) ----------------
class Shape:
    """Twelve of the edge units of _shape_cases in an order where a unit of one, two or three 8192-term buffers (90, 91
    and 127 .. 129 atoms: the leaf tables of ShapeScratch for a whole buffer and for the tail) is followed by a unit of
    one, two or three atoms and back: ShapeScratch is reused.  The units of 8191 atoms and more fill the same tables and
    cost the one-thread host reference seconds each: they stay with tests/test_gpu_shape.py."""
    name = "pw_shape_batch"
    caps = CAPS
    kernels = ("pw_shape_kernel",)
    ORDER = (129, 1, 129, 2, 128, 3, 127, 1, 91, 2, 90, 1)

    @functools.lru_cache(maxsize=None)
    def jobs(self):
        return [SH.sized_molecule(n) for n in self.ORDER]

    @functools.lru_cache(maxsize=None)
    def packed(self):
        return SH.pack(self.jobs())

    def items(self, packed):
        return {self.kernels[0]: len(packed[0]) - 1}

    def properties(self, packed):
        n = np.diff(packed[0]).tolist()
        return {
            "only sizes of _shape_cases.SIZES": set(n) <= set(SH.SIZES),
            "a one-atom unit follows the largest": follows(n, lambda a: a == max(n) and a * a > 2 * 8192, lambda b: b == 1),
            "a unit of three buffers follows a one-atom unit": follows(n, lambda a: a == 1, lambda b: b * b > 2 * 8192),
            "units of one, two and three buffers": {1, 2, 3} <= {-(-a * a // 8192) for a in n},
            "units of at most three atoms and of 90 and more in turn": all((a <= 3) != (b <= 3) for a, b in zip(n[:-1], n[1:])),
        }


TRAJ_ENTRIES = tuple(Trans(s) for s in TRANS_STATES) + (Superpose(), Cluster(), Covariance(), Project())
SHAPE = Shape()
