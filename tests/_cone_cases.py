"""Molecules for the ray tests' cone lattice (tests/test_cone_lattice.py, tests/test_gpu_cone_lattice.py): atoms on the
+-z axis through the centre (their cone holds a pole), at azimuth +-pi (their window of azimuths wraps), and one atom
whose sphere nearly contains the centre (the widest cones, or none)."""
import numpy as np

VDW_C = 1.70


def special_molecules(n_mol, seed):
    """Point-symmetric carbon shells (centroid and centre of mass at the origin to rounding) with the special atoms
    among them.  Returns [(elements, coordinates)]."""
    rng = np.random.default_rng(seed)
    out = []
    for m in range(n_mol):
        half = int(rng.integers(2, 90))
        p = rng.normal(size=(half, 3))
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(4.0, 11.0) + rng.normal(scale=0.3, size=(half, 3))
        d = float(rng.uniform(3.0, 9.0))
        tiny = float(rng.choice([0.0, 1e-300, 1e-16, 1e-12, 1e-9, 1e-6, 1e-3]))
        kind = m % 4
        extra = []
        if kind in (0, 3):                  # on the z axis, and beside it by a hair
            extra += [(0.0, 0.0, d), (tiny, -tiny, 0.8 * d)]
        if kind in (1, 3):                  # at azimuth +pi and -pi (y = +0, -0, +-tiny) and at 0
            extra += [(-d, 0.0, 0.3), (-d, -0.0, -0.5), (-0.9 * d, tiny, 1.0), (-1.1 * d, -tiny, -1.0), (d, tiny, 2.0)]
        if kind in (2, 3):                  # a sphere that nearly contains the centre, from either side of containing it
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            f = float(rng.choice([1.0 - 1e-6, 1.0 - 1e-10, 1.0, 1.0 + 1e-10, 1.0 + 1e-6, 1.0 + 1e-3, 1.05]))
            extra += [tuple(u * VDW_C * f)]
        if extra:
            p = np.concatenate([p, np.array(extra, dtype=np.float64)])
        p = np.concatenate([p, -p])         # (-p: the same atoms at azimuth + pi, the other pole)
        if m % 8 >= 6:                      # ... and some about an offset centre: two-sided bands
            p = p + rng.normal(scale=5.0, size=3)
        out.append((np.array(["C"] * len(p)), np.ascontiguousarray(p)))
    return out
