"""Edge cases of the periodic pre-processing (pywindow_amd/csrc/pw_rebuild.hpp, pw_rebuild.hip) -- TEST INFRASTRUCTURE,
numpy only and seeded, in the manner of tests/_stat_edges.py.

`cases()` is the list: synthetic systems whose bonded graph is known by construction (simple-cubic carbon blocks and
sheets, the same wrapped through the faces of a cubic and of a triclinic cell, a carbon with 15 / 16 / 17 hydrogens, a
rod through the cell), cells just above and just below the thinnest the kernel accepts, coordinates on ties of the
eighth decimal, and the two inputs the kernel used to answer wrongly without a status.

`classes(case)` restates, from a plain breadth-first walk over the bond graph, which branches of rb_wave_walk and
rebuild_frame the case takes; `all_classes()` is every class the sweep must reach.  The constants come from the
sources by regex: a changed tile or capacity moves the classes with it, and tests/test_rebuild_edges.py fails until
the list covers them again."""
import functools
import pathlib
import re
from fractions import Fraction

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "pywindow_amd" / "csrc"
TOL = 0.4
CLEAR = 1e-3            # every pair of a synthetic system stays this far from every threshold of the bond test
SMALL = 343             # cases up to this size go into the fixture made by the reference


@functools.lru_cache(maxsize=None)
def constants():
    """RB_* of pw_rebuild.hpp and the two limits on team-shared memory of pw_rebuild.hip."""
    text = (CSRC / "pw_rebuild.hpp").read_text()
    k = {name: int(value) for name, value in re.findall(r"constexpr int (RB_[A-Z_]+) = (\d+);", text)}
    for name in ("RB_NB_CAP", "RB_CHUNK", "RB_LWORK", "RB_LFINAL", "RB_SEG_CAP", "RB_NCELL", "RB_CENTRAL"):
        assert name in k, name
    hip = (CSRC / "pw_rebuild.hip").read_text()
    k["LDS_BITS"] = 1024 * int(re.search(r"fast_bytes\(n, in->rebuild, true\) <= (\d+) \* 1024", hip).group(1))
    k["LDS_SCAN"] = 1024 * int(re.search(r"with_bits != 0, true\) <= (\d+) \* 1024", hip).group(1))
    return k


def tables():
    from pywindow_amd import element_data as E

    return E


def heavy_mask(elements):
    return np.array([str(e).upper() not in tables().TERMINAL_SYMBOLS for e in elements])


def radii(elements):
    return np.array([tables().atomic_covalent_radius[str(e).upper()] for e in elements])


def max_dist(elements):
    return 2 * radii(elements).max() + TOL


def heights(lattice):
    """The three perpendicular heights V / |b x c| of a cell whose vectors are the columns of `lattice`."""
    a, b, c = (np.asarray(lattice, float)[:, k] for k in range(3))
    v = abs(np.dot(a, np.cross(b, c)))
    return np.array([v / np.linalg.norm(np.cross(b, c)), v / np.linalg.norm(np.cross(c, a)), v / np.linalg.norm(np.cross(a, b))])


def image_shifts():
    """(27, 3): the images in the order of create_supercell, a, b, c nested; 13 is the cell."""
    return np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], float)


def on_ties(xyz):
    return (np.floor(np.asarray(xyz, float) * 1e8) + 0.5) / 1e8


def make_case(name, elements, xyz, lattice=None, rebuild=False, status=0, lists=None):
    elements = np.array(elements, dtype="<U2")
    system = {"elements": elements, "atom_ids": np.array([f"{e}{k}" for k, e in enumerate(elements)]),
              "coordinates": np.ascontiguousarray(xyz, dtype=np.float64)}
    if lattice is not None:
        system["lattice"] = np.ascontiguousarray(lattice, dtype=np.float64)
    assert not rebuild or lattice is not None
    n = len(elements)
    return {"name": name, "system": system, "rebuild": bool(rebuild), "status": status, "lists": lists, "n": n,
            "fixture": n <= SMALL}


# ---- the bonded graph ------------------------------------------------------------------------------------------------
def brute_lists(case):
    """Every heavy atom's bonded partners as (image, atom) in that order, from the distances to every atom of every image
    less than max_dist + 0.5 away along x (numpy, double), how far the nearest distance of a pair with a heavy atom
    stays from a threshold of the bond test, and the largest number of pairs around one atom inside the ranges of the
    bond test widened by 5e-3 (what RB_NB_CAP counts)."""
    s = case["system"]
    x = s["coordinates"]
    n = len(x)
    el = s["elements"]
    md = max_dist(el)
    r = radii(el)
    heavy = heavy_mask(el)
    central = constants()["RB_CENTRAL"]
    shifts = image_shifts() @ s["lattice"].T if case["rebuild"] else np.zeros((1, 3))
    every = (x[None, :, :] + shifts[:, None, :]).reshape(-1, 3)            # image-major, like the supercell
    order = np.argsort(every[:, 0], kind="stable")
    xs = every[order, 0]
    reach = md + 0.5
    lists, clear, most = {}, 0.5, 0
    for p in np.nonzero(heavy)[0]:
        near = np.sort(order[np.searchsorted(xs, x[p, 0] - reach):np.searchsorted(xs, x[p, 0] + reach, side="right")])
        near = near[near != (len(shifts) // 2) * n + p]
        d = np.linalg.norm(every[near] - x[p], axis=1)
        rc = r[p] + r[near % n]
        lo, hi = np.maximum(rc - TOL, 0.1), np.minimum(rc + TOL, md)
        clear = min(clear, np.abs(d - lo).min(), np.abs(d - hi).min(), np.abs(d - md).min(), np.abs(d - 0.1).min(),
                    np.abs(d - (rc + TOL)).min())
        hit = near[(d > lo) & (d < hi)]
        lists[int(p)] = [((int(i) if case["rebuild"] else central), int(q)) for i, q in zip(hit // n, hit % n)]
        most = max(most, int(((d > lo - 5e-3) & (d < hi + 5e-3)).sum()))
    return lists, clear, most


def grid_system(name, shape, lattice=None, origin=(0.0, 0.0, 0.0), rebuild=False, centred=False, ties=False, spacing=1.5,
                split=None):
    """Carbons on a simple-cubic grid of `shape`, the first at `origin`; with a lattice, wrapped into the cell
    (fractional [0, 1), or [-0.5, 0.5) when `centred`).  The lists follow from the grid: the partners of (i, j, k) are
    its six grid neighbours, each in the image its wrap puts it in.  `split`: the planes from this one up along the
    third axis lie 3 A further: two molecules."""
    ijk = np.array([(i, j, k) for i in range(shape[0]) for j in range(shape[1]) for k in range(shape[2])])
    xyz = ijk * spacing + np.asarray(origin, float)
    if split is not None:
        xyz[ijk[:, 2] >= split, 2] += 3.0
    n = len(ijk)
    wrap = np.zeros((n, 3), int)
    if lattice is not None:
        lattice = np.asarray(lattice, float)
        frac = xyz @ np.linalg.inv(lattice).T
        wrap = np.floor(frac + (0.5 if centred else 0.0) + 1e-9).astype(int)
        xyz = xyz - wrap @ lattice.T
    if ties:
        xyz = on_ties(xyz)
    index = {tuple(v): k for k, v in enumerate(ijk.tolist())}
    central = constants()["RB_CENTRAL"]
    lists = {}
    for p, v in enumerate(ijk.tolist()):
        found = []
        for axis in range(3):
            for step in (-1, 1):
                u = list(v)
                u[axis] += step
                q = index.get(tuple(u))
                if q is None or (split is not None and (v[2] >= split) != (u[2] >= split)):
                    continue
                d = wrap[q] - wrap[p]                  # seen from x_p the partner sits at x_q + M (wrap_q - wrap_p)
                if np.abs(d).max() > 1 or (not rebuild and np.abs(d).max() > 0):
                    continue
                found.append((int((d[0] + 1) * 9 + (d[1] + 1) * 3 + d[2] + 1) if rebuild else central, q))
        lists[p] = sorted(found)
    return make_case(name, ["C"] * n, xyz, lattice, rebuild, lists=lists)


def check_graph(case):
    """The graph known by construction is the graph the distances give, CLEAR away from every threshold."""
    lists, clear, most = brute_lists(case)
    if case["lists"] is not None:
        assert clear >= CLEAR, (case["name"], clear)
        assert lists == case["lists"], case["name"]
    return lists, clear, most


def fibonacci_sphere(k, radius=1.0):
    i = np.arange(k) + 0.5
    phi = np.arccos(1 - 2 * i / k)
    theta = np.pi * (1 + 5 ** 0.5) * i
    return radius * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)


def star(k):
    """A carbon with k hydrogens 1.0 A away: k candidates around one atom."""
    xyz = np.concatenate([np.zeros((1, 3)), fibonacci_sphere(k)]) + np.array([3.0, 4.0, 5.0])
    cap = constants()["RB_NB_CAP"]
    return make_case(f"star{k}", ["C"] + ["H"] * k, xyz, status=1 if k > cap else 0,
                     lists={0: [(constants()["RB_CENTRAL"], q) for q in range(1, k + 1)]})


def triclinic(side, shear=0.18):
    return np.array([[side, -shear * side, 0.6 * shear * side], [0.0, side * 0.97, 0.8 * shear * side], [0.0, 0.0, side * 1.04]])


def random_chain(rng, n_atoms, lattice, ties=False):
    """A self-avoiding chain of C / N / O with hydrogens on some of them, 1.2 - 1.6 A steps, wrapped into the cell."""
    pts = [rng.random(3) @ lattice.T]
    el = [str(rng.choice(["C", "N", "O"]))]
    while len(pts) < n_atoms:
        base = pts[int(rng.integers(max(0, len(pts) - 3), len(pts)))]
        v = rng.normal(size=3)
        hydrogen = rng.random() < 0.3
        cand = base + v / np.linalg.norm(v) * (rng.uniform(0.9, 1.1) if hydrogen else rng.uniform(1.2, 1.6))
        if min(np.linalg.norm(cand - p) for p in pts) < 0.85:
            continue
        pts.append(cand)
        el.append("H" if hydrogen else str(rng.choice(["C", "N", "O"])))
    xyz = np.array(pts)
    frac = xyz @ np.linalg.inv(lattice).T
    xyz = (frac - np.floor(frac)) @ lattice.T
    return el, on_ties(xyz) if ties else xyz


def random_cell(rng, lo, hi):
    """A triclinic cell (columns are the cell vectors) whose three perpendicular heights lie in [lo, hi]."""
    while True:
        m = np.triu(rng.uniform(-0.5, 0.5, (3, 3)) * hi)
        m[np.diag_indices(3)] = rng.uniform(lo, 1.3 * hi, 3)
        h = heights(m)
        if h.min() >= lo and h.max() <= hi:
            return m


THIN_REPRODUCER = 11          # the trial of sheared_thin_trials() with heights 3.43 / 0.70 / 2.07 under a diagonal 8.33 / 1.95 / 2.07


def sheared_thin_trials(count=40):
    """Four carbons in sheared cells 1.8 - 3 A high (default_rng(1)): the recipe that showed the thin-cell defect."""
    rng = np.random.default_rng(1)
    out = []
    for _ in range(count):
        by, cz = rng.uniform(1.8, 3, 2)
        cy = rng.uniform(2, 8)
        ax = rng.uniform(6, 12)
        bx, cx = rng.uniform(-3, 3, 2)
        m = np.array([[ax, bx, cx], [0, by, cy], [0, 0, cz]])
        out.append((m, rng.random((4, 3)) @ m.T))
    return out


def own_copy_reproducer():
    """N O C H whose central-image copies differ from the cell atoms by value: the second walk meets N0 and C2 twice
    and its centre of mass lies inside the cell."""
    lattice = [[8.70852916557196, -1.984946622385088, -2.327352888847246], [0, 7.750207071107652, 0.8403929065596805],
               [0, 0, 6.752745821543047]]
    xyz = [[-2.141370495, 8.362198135, 6.684442925], [-0.282253935, 1.283757305, 5.142546635],
           [-3.482591455, 8.122740715, 4.617578655], [-1.130777745, 1.362030225, 5.687318645]]
    return make_case("own_copy", ["N", "O", "C", "H"], xyz, lattice, rebuild=True)


@functools.lru_cache(maxsize=None)
def cases():
    k = constants()
    out = []
    # non-periodic: the block whose layers outgrow every list in team-shared memory, and the candidate capacity
    out.append(grid_system("block25", (25, 25, 25)))
    out.append(grid_system("block3", (3, 3, 3)))
    out += [star(k["RB_NB_CAP"] - 1), star(k["RB_NB_CAP"]), star(k["RB_NB_CAP"] + 1)]
    # periodic, nothing rebuilt: a sheet walked from its corner (the pseudo origin is at fractional 0.26, 0.25, 0.25):
    # layers 1, 2, .. 65 wide, then 65 for a while
    big = np.diag([440.0, 440.0, 40.0])
    out.append(grid_system("sheet65", (65, 70, 1), big, origin=big @ np.array([0.26, 0.25, 0.25])))
    # ... and the same sheet walked from its middle: two fronts, another frame of that topology
    out.append(grid_system("sheet65_middle", (65, 70, 1), big, origin=big @ np.array([0.26, 0.25, 0.25]) - np.array([48.0, 52.5, 0.0])))
    # rebuilt: the same block through one, two and three faces of a cubic and of a triclinic cell
    for kind, lattice in (("cubic", np.eye(3) * 14.0), ("triclinic", triclinic(15.0))):
        for faces in (1, 2, 3):
            origin = lattice @ np.array([0.8 if a < faces else 0.2 for a in range(3)])
            out.append(grid_system(f"block7_{kind}_{faces}", (7, 7, 7), lattice, origin, rebuild=True))
    # the same carbons as two molecules: frames of one topology with different molecule counts
    out.append(grid_system("block7_split", (7, 7, 7), np.eye(3) * 14.0, (11.2, 2.8, 2.8), rebuild=True, split=4))
    out.append(grid_system("block5_centred", (5, 5, 5), np.eye(3) * 12.0, (2.5, -3.0, -8.5), rebuild=True, centred=True))
    out.append(grid_system("block7_ties", (7, 7, 7), triclinic(15.0), triclinic(15.0) @ np.array([0.8, 0.8, 0.2]) + 0.3, rebuild=True, ties=True))
    # a sheet on ties: sixteen atoms of a layer fill a pass, and those whose copy is an item of its own hit twice
    out.append(grid_system("sheet18_ties", (18, 18, 1), triclinic(32.0, 0.1), triclinic(32.0, 0.1) @ np.array([0.7, 0.75, 0.3]), rebuild=True, ties=True))
    # rebuilt, larger than the lists in team-shared memory
    out.append(grid_system("block12_cubic", (12, 12, 12), np.eye(3) * 22.0, (15.0, 16.0, 3.0), rebuild=True))
    out.append(grid_system("block12_cubic_3", (12, 12, 12), np.eye(3) * 22.0, (9.0, 12.5, 14.0), rebuild=True))
    # two carbons whose centre of mass lies on a cell face: no walk is predicted
    out.append(make_case("com_on_face", ["C", "C"], [[11.25, 3.0, 4.0], [0.75, 3.0, 4.0]], np.eye(3) * 12.0, rebuild=True))
    # a rod through the cell: every walk leaves the supercell
    out.append(make_case("rod", ["C"] * 4, [[0.5 + 1.5 * i, 2.0, 2.5] for i in range(4)], np.diag([6.0, 7.0, 8.0]), rebuild=True))
    # cells just above and just below the thinnest accepted, sheared and not
    for tag, dh, status in (("above", 0.01, 0), ("below", -0.01, k["RB_ST_THIN_CELL"])):
        h = max_dist(["C"]) + dh
        xyz = [[1.0, 1.0, 0.4], [2.5, 1.0, 0.4], [2.5, 2.5, 0.4]]
        out.append(make_case(f"thin_{tag}", ["C"] * 3, xyz, np.diag([9.0, 8.0, h]), rebuild=True, status=status))
        # the height of the b faces is by cz / sqrt(cy^2 + cz^2): the diagonal says 3 h
        m = np.array([[9.0, 1.0, 2.0], [0.0, 3.0 * h, 8.0 ** 0.5 * 4.0], [0.0, 0.0, 4.0]])
        assert abs(heights(m)[1] - h) < 1e-12 and m[1, 1] > 2 * max_dist(["C"])
        out.append(make_case(f"thin_sheared_{tag}", ["C"] * 3, np.array(xyz) + 0.3, m, rebuild=True, status=status))
    m, xyz = sheared_thin_trials(THIN_REPRODUCER + 1)[THIN_REPRODUCER]
    out.append(make_case("thin_reproducer", ["C"] * 4, xyz, m, rebuild=True, status=k["RB_ST_THIN_CELL"]))
    out.append(own_copy_reproducer())
    # random chains on ties of the eighth decimal
    rng = np.random.default_rng(20)
    for t in range(6):
        lattice = random_cell(rng, 5.0, 9.0)
        el, xyz = random_chain(rng, 24, lattice, ties=True)
        out.append(make_case(f"chain_ties_{t}", el, xyz, lattice, rebuild=True))
    # non-periodic and periodic without rebuild, a molecule of mixed elements
    rng = np.random.default_rng(21)
    lattice = random_cell(rng, 8.0, 12.0)
    el, xyz = random_chain(rng, 40, lattice)
    out.append(make_case("chain_cell", el, xyz, lattice))
    out.append(make_case("chain_free", el, xyz))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def topologies():
    """The cases grouped by what one launch shares: elements, periodic or not, rebuilt or not."""
    groups = {}
    for c in cases():
        key = (tuple(c["system"]["elements"]), "lattice" in c["system"], c["rebuild"])
        groups.setdefault(key, []).append(c)
    return list(groups.values())


# ---- the host build: the kernel source compiled for a one-thread team (tests/hostsim/rebuild_probe.cpp) ---------------
def topology_of(case):
    from pywindow_amd import rebuild as RB

    return RB.CellTopology(case["system"]["elements"])


def host_raw(hostsim, case, layout):
    """(status, n_mol, offsets, src_atom, src_image, xyz) of the host build; layout bit 0 = the visit bit sets, bit 1 =
    the scan coordinates in "team-shared" memory (1, 3 and 0 are the three the device uses)."""
    import ctypes

    from pywindow_amd import rebuild as RB

    lib = ctypes.CDLL(str(hostsim / "librebuildprobe.so"))
    s = case["system"]
    topo = topology_of(case)
    xyz, lat, inv = RB.pack_frames(s["coordinates"][None], s["lattice"][None] if "lattice" in s else None)
    n = topo.n
    cap = 30 * n if case["rebuild"] else n
    n_mol, status = ctypes.c_int(), ctypes.c_int()
    off, src, img, out = np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int8), np.zeros((cap, 3))
    vp = ctypes.c_void_p
    rc = lib.hs_discrete_molecules(
        ctypes.c_int(n), xyz.ctypes.data_as(vp), None if lat is None else lat.ctypes.data_as(vp),
        None if inv is None else inv.ctypes.data_as(vp), topo.cov.ctypes.data_as(vp), topo.mass.ctypes.data_as(vp),
        topo.terminal.ctypes.data_as(vp), ctypes.c_double(topo.max_dist), ctypes.c_double(topo.tol),
        ctypes.c_int(1 if case["rebuild"] else 0), ctypes.c_int(cap), ctypes.c_int(cap), ctypes.byref(n_mol),
        ctypes.byref(status), off.ctypes.data_as(vp), src.ctypes.data_as(vp), img.ctypes.data_as(vp),
        out.ctypes.data_as(vp), ctypes.c_int(layout))
    assert rc == 0
    m = n_mol.value
    a = int(off[m])
    return status.value, m, off[:m + 1].copy(), src[:a].copy(), img[:a].copy(), out[:a].copy()


def same_raw(a, b):
    """Molecule count, offsets, source atoms and images, coordinate bits."""
    return (a[0] == b[0] and a[1] == b[1] and all(np.array_equal(u, v) for u, v in zip(a[2:5], b[2:5])) and
            a[5].tobytes() == b[5].tobytes())


def oracle_flat(case):
    """The oracle's molecules as (offsets, source atoms, xyz): what the fixture holds of the reference's."""
    from oracle import pw_rebuild as R

    s = case["system"]
    mols = R.discrete_molecules(s, rebuild=R.create_supercell(s) if case["rebuild"] else None)
    return flatten(mols)


def flatten(mols):
    off = np.concatenate([[0], np.cumsum([len(m["elements"]) for m in mols])]).astype(np.int32)
    src = np.array([int(str(i).lstrip("CNOH")) for m in mols for i in m["atom_ids"]], dtype=np.int32)
    xyz = np.concatenate([np.zeros((0, 3))] + [np.asarray(m["coordinates"], float).reshape(-1, 3) for m in mols])
    return off, src, xyz


# ---- which branches a case takes -------------------------------------------------------------------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def mat3(m, v):
    """rb_mat3: y_i = fma(m_i2, v2, fma(m_i0, v0, m_i1 * v1))."""
    return [fma(m[i][2], v[2], fma(m[i][0], v[0], m[i][1] * v[1])) for i in range(3)]


def own_copies(case):
    """Atoms whose copy in the central image, round(M (M^-1 x), 8), differs by value from round(x, 8)."""
    if not case["rebuild"]:
        return np.zeros(case["n"], bool)
    s = case["system"]
    m = s["lattice"].tolist()
    inv = np.linalg.inv(s["lattice"][None])[0].tolist()
    out = []
    for x in s["coordinates"].tolist():
        c = mat3(m, [f + 0.0 for f in mat3(inv, x)])
        out.append(any(round(a, 8) != round(b, 8) for a, b in zip(c, x)))
    return np.array(out)


def shared_bytes():
    """sizeof(RebuildShared), from the host build (tests/hostsim/rebuild_probe.cpp; the `hostsim` fixture builds it)."""
    import ctypes

    lib = ctypes.CDLL(str(ROOT / "tests" / "hostsim" / "librebuildprobe.so"))
    lib.hs_rebuild_shared_bytes.restype = ctypes.c_long
    return int(lib.hs_rebuild_shared_bytes())


def scan_bytes(n):
    return n * 16 + ((n * 4 + 15) & ~15) + (constants()["RB_NCELL"] + 4) * 4


def fast_bytes(n, rebuild, with_bits, with_scan):
    k = constants()
    words = ((28 * n if rebuild else n) + 63) // 64
    pad = (n + 15) & ~15
    return (k["RB_CHUNK"] * k["RB_SEG_CAP"] * 8 + k["RB_CHUNK"] * 4 + (2 * words * 8 if with_bits else 0) +
            ((shared_bytes() + 15) & ~15) + (2 * pad if with_bits else 0) + (scan_bytes(n) if with_scan else 0))


def device_layout(n, rebuild, allowed=3):
    """(bit sets, scan coordinates) in team-shared memory, as pw_rebuild.hip chooses; `allowed` as its test hook."""
    k = constants()
    bits = bool(allowed & 1) and fast_bytes(n, rebuild, True, False) <= k["LDS_BITS"]
    scan = bool(allowed & 2) and fast_bytes(n, rebuild, bits, True) <= k["LDS_SCAN"]
    return bits, scan


def width_class(nw):
    k = constants()
    c = k["RB_CHUNK"]
    if nw < c:
        return f"1..{c - 1}"
    if nw in (c, c + 1):
        return str(nw)
    if nw <= 2 * c:
        return f"{c + 2}..{2 * c}"
    return f">={2 * c + 1}"


def classes(case):
    """The branches of rebuild_frame and rb_wave_walk this case takes, from a breadth-first walk over its lists."""
    k = constants()
    s = case["system"]
    n, rebuild = case["n"], case["rebuild"]
    el, x = s["elements"], s["coordinates"]
    periodic = "lattice" in s
    got = {("mode", "rebuilt" if rebuild else "periodic" if periodic else "free")}
    got.add(("status", case["status"]))
    lists = case["lists"] if case["lists"] is not None else brute_lists(case)[0]
    heavy = heavy_mask(el)
    if case["status"] & k["RB_ST_THIN_CELL"]:
        return got | {("cell", "thin", "sheared" if abs(s["lattice"][0, 1]) > 0 else "straight")}
    if rebuild and heights(s["lattice"]).min() < max_dist(el) + 0.02:
        got.add(("cell", "just high enough", "sheared" if abs(s["lattice"][0, 1]) > 0 else "straight"))
    # the candidate grid and where the lists live
    md = max_dist(el)
    ext = np.abs(x).max() + (np.abs(s["lattice"]).sum() if rebuild else 0.0) + 1.0
    slack = 2e-3 + 1e-6 * ext
    gh = md + 2 * slack
    span = x.max(axis=0) - x.min(axis=0)
    got.add(("grid", "cells grown" if np.prod(np.floor(span / gh) + 1) > k["RB_NCELL"] else "first cell size"))
    total = sum(len(v) for v in lists.values())
    most = max([len(v) for v in lists.values()] + [0])
    if most >= k["RB_NB_CAP"]:
        got.add(("candidates", min(most, k["RB_NB_CAP"] + 1)))
    if case["status"] & k["RB_ST_NB_OVERFLOW"]:
        return got
    scan_fast = device_layout(n, rebuild)[1]
    got.add(("lists", "team-shared memory" if scan_fast and 3 * n + 1 + total <= scan_bytes(n) // 4 else "slab",
             "rebuilt" if rebuild else "as it is"))
    # start atoms: nearest to the pseudo origin
    mass = tables().MASS[tables().element_ids(el)]
    com = (x * mass[:, None]).sum(axis=0) / mass.sum()
    if periodic:
        origin = s["lattice"] @ np.array([0.26, 0.25, 0.25])
        bound = (-0.5, 0.5) if np.allclose(com, [0.01, 0, 0], atol=1.0) else (0.0, 1.0)
        got.add(("bounds", bound))
        inv = np.linalg.inv(s["lattice"])
    else:
        origin = com + np.array([0.01, 0.0, 0.0])
    dorig = np.where(heavy, np.linalg.norm(x - origin, axis=1), np.inf)
    own = own_copies(case)
    shifts = image_shifts()
    central = k["RB_CENTRAL"]
    remaining = np.ones(n, bool)
    cage_of = np.zeros(n, int)
    cage_img = np.zeros(n, int)
    cage = {}
    serial = 0
    while True:
        left = np.nonzero(remaining & heavy)[0]
        if len(left) == 0:
            break
        start = int(left[np.argmin(dorig[left])])
        if rebuild and cage_of[start]:
            c = cage[cage_of[start]]
            if not c["clean"]:
                got.add(("walk", "made: the first walk was not clean"))
            else:
                o = shifts[cage_img[start]]
                f = c["f"] - o
                in_range = all(c["lo"][a] - o[a] >= -1 and c["hi"][a] - o[a] <= 1 for a in range(3))
                sure = not any(abs(f[a] - b) < 1e-6 for a in range(3) for b in bound)
                inside = all(bound[0] <= f[a] < bound[1] for a in range(3))
                if in_range and sure and not inside:
                    got.add(("walk", "predicted and skipped"))
                    remaining[(cage_of == cage_of[start]) & (cage_img == cage_img[start])] = False
                    continue
                got.add(("walk", "made: centre of mass within 1e-6 of the bound" if not sure else
                         "made: predicted to be kept" if in_range else "made: prediction leaves the supercell"))
        elif rebuild:
            got.add(("walk", "first"))
        serial += 1
        first_walk = rebuild and cage_of[start] == 0
        layer = [start]
        final = []
        in_final = set()
        truncated = False
        while layer:
            nw, nf = len(layer), len(final)
            got.add(("layer width", width_class(nw)))
            if nw > k["RB_LWORK"]:
                got.add(("layer", "tail in the global lists"))
            if nf < k["RB_LFINAL"] < nf + nw:
                got.add(("layer", "straddles the end of the molecule in team-shared memory"))
            final += layer
            in_final.update(layer)
            nxt, seen = [], set()
            a0 = 0
            while a0 < nw:
                atoms = layer[a0:a0 + 64]
                counts = [len(lists.get(i if i < n else (i - n) % n, ())) for i in atoms]
                incl = np.cumsum(counts)
                na = int((incl <= 64).sum())
                if incl[na - 1] == 64:
                    got.add(("pass", "ends at exactly 64 entries"))
                if na < len(atoms):
                    got.add(("pass", "cut: the next atom's list would pass 64"))
                hits = []
                for i in atoms[:na]:
                    q0, a = (i, shifts[central]) if i < n else ((i - n) % n, shifts[(i - n) // n])
                    cell, image = [], []
                    for dimg, q in lists.get(q0, ()):
                        b = a + shifts[dimg]
                        is_central = not b.any()
                        outside = np.abs(b).max() > 1
                        truncated = truncated or (rebuild and outside)
                        same_item = is_central and not own[q]
                        do0 = is_central and remaining[q]
                        do1 = rebuild and not outside and not (same_item and remaining[q])
                        if do0:
                            cell.append(q)
                        if do1:
                            image.append(q if same_item else n + int((b[0] + 1) * 9 + (b[1] + 1) * 3 + b[2] + 1) * n + q)
                        if do0 and do1:
                            got.add(("entry", "hit as cell atom and as image atom"))
                    hits += cell + image
                if hits:
                    use_temp = not (a0 == 0 and na >= nw and len(hits) <= 64)
                    got.add(("merge", "across rounds, with the bits of the layer" if use_temp else "one round, lane to lane"))
                    if len(hits) > 64:
                        got.add(("merge", "more than 64 hits in a pass"))
                    for h0 in range(0, len(hits), 64):
                        rnd = hits[h0:h0 + 64]
                        for t, i in enumerate(rnd):
                            if i in rnd[:t]:
                                got.add(("duplicate", "inside a round"))
                                continue
                            if i in seen:
                                got.add(("duplicate", "across rounds"))
                                continue
                            seen.add(i)
                            if i not in in_final:
                                nxt.append(i)
                a0 += na
            for i in layer:
                if i < n:
                    remaining[i] = False
            layer = nxt
        if len(final) > k["RB_LFINAL"]:
            got.add(("molecule", "longer than team-shared memory holds"))
        if first_walk:
            qs = np.array([i if i < n else (i - n) % n for i in final])
            imgs = np.array([central if i < n else (i - n) // n for i in final])
            xyz = x[qs] + shifts[imgs] @ s["lattice"].T
            f = inv @ ((xyz * mass[qs][:, None]).sum(axis=0) / mass[qs].sum())
            repeat = len(set(qs.tolist())) < len(qs) or cage_of[qs].any()
            cage_of[qs], cage_img[qs] = serial, imgs
            cage[serial] = {"clean": not (truncated or repeat or own[qs].any()), "f": f,
                            "lo": shifts[imgs].min(axis=0), "hi": shifts[imgs].max(axis=0)}
            if truncated:
                got.add(("first walk", "leaves the supercell"))
            if own[qs].any():
                got.add(("first walk", "through an atom whose copy is an item of its own"))
    return got


def all_classes():
    k = constants()
    c = k["RB_CHUNK"]
    return ({("mode", m) for m in ("free", "periodic", "rebuilt")} |
            {("status", 0), ("status", k["RB_ST_NB_OVERFLOW"]), ("status", k["RB_ST_THIN_CELL"])} |
            {("cell", h, t) for h in ("thin", "just high enough") for t in ("sheared", "straight")} |
            {("grid", "cells grown"), ("grid", "first cell size")} |
            {("candidates", k["RB_NB_CAP"]), ("candidates", k["RB_NB_CAP"] + 1)} |
            {("lists", where, mode) for where in ("team-shared memory", "slab") for mode in ("rebuilt", "as it is")} |
            {("bounds", (-0.5, 0.5)), ("bounds", (0.0, 1.0))} |
            {("walk", w) for w in ("first", "predicted and skipped", "made: the first walk was not clean",
                                   "made: centre of mass within 1e-6 of the bound")} |
            {("layer width", w) for w in (f"1..{c - 1}", str(c), str(c + 1), f"{c + 2}..{2 * c}", f">={2 * c + 1}")} |
            {("layer", "tail in the global lists"), ("layer", "straddles the end of the molecule in team-shared memory")} |
            {("pass", "ends at exactly 64 entries"), ("pass", "cut: the next atom's list would pass 64")} |
            {("entry", "hit as cell atom and as image atom")} |
            {("merge", "across rounds, with the bits of the layer"), ("merge", "one round, lane to lane"),
             ("merge", "more than 64 hits in a pass")} |
            {("duplicate", "inside a round"), ("duplicate", "across rounds")} |
            {("molecule", "longer than team-shared memory holds")} |
            {("first walk", "leaves the supercell"), ("first walk", "through an atom whose copy is an item of its own")})


OPTIONAL = {("walk", "made: predicted to be kept"), ("walk", "made: prediction leaves the supercell")}
