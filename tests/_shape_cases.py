"""Inputs shared by tests/test_shape.py (host build of pw_shape.hpp against the oracle and a 50-digit
eigensolver) and tests/test_gpu_shape.py (device against host build, bit for bit).  numpy only.

Every generator is seeded: the same cases on every machine."""
import ctypes

import numpy as np

#: shifts of the hard molecules from the origin, in Angstrom
SHIFTS = (0.0, 1.0, 10.0, 1000.0)
#: rotations of every hard molecule at every shift
ROTATIONS = 40
#: unit sizes around numpy's summation blocks: N^2 crosses 8192 between 90 and 91, 128 is one pairwise leaf,
#: 8192 is one buffer of the mass sum and the row sums, and 16411 puts N^2 = 2.7e8 terms into 32877 buffers
SIZES = (1, 2, 3, 90, 91, 127, 128, 129, 8191, 8192, 8193, 16411)
#: the largest N whose N x N inertia terms the oracle may build as written (0.5 GiB per array)
ORACLE_MAX_N = 8193
#: units of the large batch: above the 4096 workgroups of pw_shape_batch's grid
LARGE_BATCH_UNITS = 5003
#: circumcircle triples sent in one call (100003 = 1562 * 64 + 35: the last block is partial)
N_TRIPLES = 100_003
#: elements that the mixed-mass variants draw from: H with heavy atoms
HEAVY = ("C", "N", "O", "S", "CL", "BR", "I")


def _masses(symbols):
    from pywindow_amd import element_data as E

    return E.MASS[E.element_ids(symbols)]


def _mixed_masses(rng, n):
    sym = np.where(rng.random(n) < 0.5, "H", rng.choice(HEAVY, n))
    return _masses(sym)


def rotation(rng):
    """A random proper rotation (QR of a Gaussian matrix, signs fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _icosahedron():
    phi = (1.0 + 5.0 ** 0.5) / 2.0
    v = []
    for a in (-1.0, 1.0):
        for b in (-phi, phi):
            v += [(0.0, a, b), (a, b, 0.0), (b, 0.0, a)]
    return np.array(v)


#: the hard shapes at the origin: two or three equal eigenvalues, planar, linear, one and two atoms
SHAPES = {
    "tetrahedron": np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], float) * 0.89,
    "octahedron": np.vstack([np.eye(3), -np.eye(3)]) * 1.54,
    "icosahedron": _icosahedron() * 0.93,
    "hexagon": np.array([(1.39 * np.cos(k * np.pi / 3), 1.39 * np.sin(k * np.pi / 3), 0.0) for k in range(6)]),
    "chain": np.array([(1.2 * (k - 2), 0.0, 0.0) for k in range(5)]),
    "one_atom": np.zeros((1, 3)),
    "two_atoms": np.array([(-0.55, 0.0, 0.0), (0.55, 0.0, 0.0)]),
}
#: nearly degenerate spectra: the spherical tops with every atom moved by about 1e-3 and 1e-6 A, so that two or three
#: eigenvalues lie that close (relative) and an early stop of the Jacobi shows in the eigenvalues (an off-diagonal
#: entry o left behind moves them by about o^2 / gap, not below an ulp when the gap is small)
NEAR = (1e-3, 1e-6)
_near_rng = np.random.default_rng(5)
for _name in ("tetrahedron", "octahedron", "icosahedron"):
    for _d in NEAR:
        SHAPES[f"{_name}~{_d:g}"] = SHAPES[_name] + _d * _near_rng.normal(size=SHAPES[_name].shape)
MASS_VARIANTS = ("carbon", "mixed")


def shape_masses(name, variant):
    """One mass table per (shape, variant): the template of that group."""
    n = len(SHAPES[name])
    if variant == "carbon":
        return _masses(["C"] * n)
    return _mixed_masses(np.random.default_rng(sorted(SHAPES).index(name) + 100), n)


def hard_molecules():
    """[(tag, xyz, mass)]: every shape x every shift x ROTATIONS rotations; the mass variant alternates with
    the rotation, so that every (shape, shift) has both.  The shift goes along a random direction.

    The reference's eigensolver (np.linalg.eigvals, LAPACK dgeev) does not know the tensors are symmetric: for
    some spherical tops at the origin it returns a complex pair whose imaginary parts are at rounding level,
    and which ones depends on the BLAS kernels the host runs.  tests/test_shape.py scores what the reference
    returns, the real parts, for every case."""
    rng = np.random.default_rng(1)
    out = []
    for name, base in SHAPES.items():
        for shift in SHIFTS:
            for k in range(ROTATIONS):
                variant = MASS_VARIANTS[k % 2]
                d = rng.normal(size=3)
                xyz = base @ rotation(rng).T + shift * d / np.linalg.norm(d)
                out.append((f"{name}/{variant}/shift{shift:g}/rot{k}", np.ascontiguousarray(xyz),
                            shape_masses(name, variant)))
    return out


def template_groups(mols=None):
    """The hard molecules grouped by (shape, mass variant): [(tag, coords (U, N, 3), mass (N,), indices)]."""
    mols = hard_molecules() if mols is None else mols
    groups = {}
    for i, (tag, xyz, _) in enumerate(mols):
        name, variant = tag.split("/")[:2]
        groups.setdefault((name, variant), []).append(i)
    return [(f"{name}/{variant}", np.stack([mols[i][1] for i in idx]), shape_masses(name, variant), idx)
            for (name, variant), idx in groups.items()]


def sized_molecule(n):
    """A random molecule of n atoms, about 1 atom per 10 A^3, H mixed with heavy atoms, off the origin."""
    rng = np.random.default_rng(1000 + n)
    side = (10.0 * n) ** (1.0 / 3.0)
    xyz = rng.uniform(-side / 2, side / 2, (n, 3)) + rng.normal(0.0, 5.0, 3)
    return (f"N{n}", xyz, _mixed_masses(rng, n))


def sized_molecules(max_n=None):
    return [sized_molecule(n) for n in SIZES if max_n is None or n <= max_n]


def large_batch():
    """LARGE_BATCH_UNITS random units of 1 to 48 atoms: (atom_offset, xyz, mass)."""
    rng = np.random.default_rng(7)
    sizes = rng.integers(1, 49, LARGE_BATCH_UNITS)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xyz = rng.normal(0.0, 4.0, (int(off[-1]), 3)) + np.repeat(rng.uniform(-50, 50, (len(sizes), 3)), sizes, axis=0)
    return off, xyz, _mixed_masses(rng, int(off[-1]))


def pack(mols):
    """(atom_offset, xyz, mass) of a ragged batch."""
    off = np.concatenate([[0], np.cumsum([len(x) for _, x, _ in mols])]).astype(np.int64)
    xyz = np.ascontiguousarray(np.concatenate([x for _, x, _ in mols]))
    mass = np.ascontiguousarray(np.concatenate([m for _, _, m in mols]))
    return off, xyz, mass


def unpack(off, xyz, mass):
    return [(f"u{u}", xyz[off[u]:off[u + 1]], mass[off[u]:off[u + 1]]) for u in range(len(off) - 1)]


def _triangle(rng, rots, a, b, c):
    """Three points with side lengths |BC| = a, |CA| = b, |AB| = c, randomly placed and rotated."""
    cx = (b * b + c * c - a * a) / (2.0 * c)
    cy = np.sqrt(max(b * b - cx * cx, 0.0))
    p = np.array([(0.0, 0.0, 0.0), (c, 0.0, 0.0), (cx, cy, 0.0)])
    return p @ rots[rng.integers(len(rots))].T + rng.uniform(-30.0, 30.0, 3)


def circumcircle_triples():
    """(xyz (A, 3), sets (N_TRIPLES, 3) int32): sides from 0.1 to 1000 A; acute, right and obtuse triangles;
    nearly collinear triples bent by 1e-1 ... 1e-9 rad; exactly collinear triples, repeated indices and
    coincident atoms.  Every kind is spread over the whole call."""
    rng = np.random.default_rng(11)
    rots = [rotation(rng) for _ in range(1024)]
    pts, sets, count = [], [], [0]

    def add(p):
        i = count[0]
        pts.append(np.asarray(p, float))
        count[0] += len(p)
        return i

    kinds = ("acute", "right", "obtuse", "bent", "collinear", "repeated", "coincident")
    for k in range(N_TRIPLES):
        kind = kinds[k % len(kinds)]
        s = 10.0 ** rng.uniform(-1.0, 3.0)                   # a side length, 0.1 ... 1000 A
        if kind in ("acute", "right", "obtuse"):
            # the angle at C: below, at or above 90 degrees
            gamma = {"acute": rng.uniform(0.2, 1.5), "right": np.pi / 2, "obtuse": rng.uniform(1.65, 3.0)}[kind]
            a, b = s, 10.0 ** rng.uniform(-1.0, 3.0)
            c = np.sqrt(a * a + b * b - 2.0 * a * b * np.cos(gamma))
            i = add(_triangle(rng, rots, a, b, c))
            sets.append((i, i + 1, i + 2)[:: 1 if k % 2 else -1])
        elif kind == "bent":
            eps = 10.0 ** -(1 + (k // len(kinds)) % 9)     # 1e-1 ... 1e-9 rad off a straight line
            u = rng.uniform(0.05, 0.95)
            # A and B at the ends of a segment of length s, C near it, the angle at A is eps
            p = np.array([(0.0, 0.0, 0.0), (s, 0.0, 0.0), (u * s * np.cos(eps), u * s * np.sin(eps), 0.0)])
            i = add(p @ rots[rng.integers(len(rots))].T + rng.uniform(-30.0, 30.0, 3))
            sets.append((i, i + 1, i + 2))
        elif kind == "collinear":
            # on a line through a point, with a direction of small integers: every coordinate exact
            o = np.round(rng.uniform(-50.0, 50.0, 3) * 8.0) / 8.0
            d = rng.integers(-3, 4, 3).astype(float)
            d[rng.integers(0, 3)] = rng.choice((-1.0, 1.0)) * rng.integers(1, 4)
            t = rng.choice(np.arange(-8, 9), 3, replace=False) * (2.0 ** rng.integers(-3, 4))
            i = add(o + t[:, None] * d)
            sets.append((i, i + 1, i + 2))
        elif kind == "repeated":
            i = add(_triangle(rng, rots, s, s * 0.8, s * 0.6))
            sets.append(((i, i, i + 1), (i + 1, i, i), (i, i + 2, i), (i + 2, i + 2, i + 2))[(k // len(kinds)) % 4])
        else:
            p = _triangle(rng, rots, s, s * 0.7, s * 0.9)
            p[1] = p[0] if k % 2 else p[1]
            p[2] = p[0] if not k % 2 else p[2]
            p[2] = p[1] if (k // len(kinds)) % 3 == 0 else p[2]      # some with all three atoms coincident
            i = add(p)
            sets.append((i, i + 1, i + 2))
    return np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.array(sets, dtype=np.int32))


def block_inertia(xyz, mass, block=8192):
    """The oracle's inertia tensor (oracle/pw_shape.py: inertia_tensor) without its N x N arrays: numpy
    sums the N^2 terms of every entry in consecutive buffers of 8192 (pairwise inside a buffer), the
    buffer sums added in order.  The terms are the oracle's, operation for operation, made a band of
    rows at a time."""
    xyz = np.asarray(xyz, float)
    m = np.asarray(mass, float).reshape(-1, 1)
    n = len(xyz)
    p2 = xyz ** 2
    terms = (
        lambda r: m[r] * (p2[:, 1] + p2[:, 2]),
        lambda r: m[r] * (p2[:, 0] + p2[:, 2]),
        lambda r: m[r] * (p2[:, 0] + p2[:, 1]),
        lambda r: -m[r] * xyz[:, 0] * xyz[:, 1],
        lambda r: -m[r] * xyz[:, 0] * xyz[:, 2],
        lambda r: -m[r] * xyz[:, 1] * xyz[:, 2],
    )
    rows = max(1, (1 << 22) // n)
    sums = []
    for f in terms:
        acc, rest = None, np.zeros(0)
        for i0 in range(0, n, rows):
            t = np.concatenate([rest, f(slice(i0, min(i0 + rows, n))).reshape(-1)])
            full = len(t) // block * block
            for p in t[:full].reshape(-1, block).sum(axis=1):
                acc = p if acc is None else acc + p
            rest = t[full:]
        if len(rest):
            p = rest.sum()
            acc = p if acc is None else acc + p
        sums.append(acc)
    d1, d2, d3, mxy, mxz, myz = (np.float64(s) for s in sums)
    return np.array([[d1, mxy, mxz], [mxy, d2, myz], [mxz, myz, d3]]) / n


def host_shape(lib, off, xyz, mass):
    """hs_shape_batch of tests/hostsim/shape_probe.cpp: the host build of pw_shape.hpp, one-thread team."""
    from pywindow_amd import _lib

    off, xyz, mass = (np.ascontiguousarray(a) for a in (off, xyz, mass))
    out = np.zeros(len(off) - 1, dtype=_lib.SHAPE_OUT_DTYPE)
    vp = ctypes.c_void_p
    assert lib.hs_shape_batch(ctypes.c_long(len(out)), off.ctypes.data_as(vp), xyz.ctypes.data_as(vp),
                              mass.ctypes.data_as(vp), out.ctypes.data_as(vp)) == 0
    return out


def host_circumcircle(lib, xyz, sets):
    xyz, sets = np.ascontiguousarray(xyz, dtype=np.float64), np.ascontiguousarray(sets, dtype=np.int32)
    d, c = np.zeros(len(sets)), np.zeros((len(sets), 3))
    vp = ctypes.c_void_p
    lib.hs_circumcircle(xyz.ctypes.data_as(vp), sets.ctypes.data_as(vp), ctypes.c_long(len(sets)),
                        d.ctypes.data_as(vp), c.ctypes.data_as(vp))
    return d, c
