"""Molecules for tests/test_gpu_path_brackets.py: small random shells by seed, and the seeds whose ray tests leave a
given number of sampling vectors for the path scans (found with a host probe that reports the count)."""
import numpy as np

POOL = np.array(["C", "H", "N", "O", "S", "F", "Cl", "Br", "P", "I", "Si", "Se", "He"])


def shell(seed, n=None, n_elements=3):
    """A shell of n atoms (4 .. 63 by the seed where not given) of the first n_elements of POOL, cycled so that each occurs."""
    rng = np.random.default_rng(seed)
    if n is None:
        n = 4 + seed % 60
    p = rng.normal(size=(n, 3))
    p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(3.0, 9.0) + rng.normal(scale=0.3, size=(n, 3))
    el = POOL[(np.arange(n) + rng.integers(0, n_elements)) % n_elements] if n_elements > 3 else POOL[rng.integers(0, n_elements, size=n)]
    return el, np.ascontiguousarray(p - p.mean(axis=0))


# seed -> (the sampling vectors its ray tests leave for the path scans, those that pass: the record's n_survivors).  The
# first number is not in the record: it comes from a host probe made to report it.  A team has 256 threads: 255 is one
# partial round, 256 one whole round, 257 and 271 a whole round and 1 / 15 left-over paths (a wave each), 272 two rounds
# (sixteen left over fill a round of their own: the quarter-team rule's lower edge), 512 and 513 the same after two rounds.
SURVIVORS = {984: (255, 234), 590: (256, 184), 565: (257, 223), 307: (271, 217), 1055: (272, 207), 287: (512, 495), 375: (513, 471)}
