"""Inputs shared by tests/test_kde.py (host path, against SciPy and a long-double sum) and
tests/test_gpu_kde.py (device against host path, bit for bit)."""
import re

import numpy as np

from _util import GOLDEN, ROOT

BW_METHODS = ("scott", "silverman", 0.37)


def source_constant(name: str) -> int:
    text = (ROOT / "pywindow_amd" / "csrc" / "pw_kde.hpp").read_text()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def golden_cc3():
    """Window / optimised pore / maximum diameters of the 20 golden CC3 frames (what examples/example_7.py
    collects from a trajectory)."""
    g = np.load(GOLDEN / "md20.npz")
    windows = np.concatenate([g["win_d"][u][: int(g["n_windows"][u])] for u in range(len(g["n_windows"]))])
    return {"windows": windows, "pore_diameter_opt": np.array(g["pore_opt_d"]), "maximum_diameter": np.array(g["maxd"])}


def synthetic(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n + (0 if kind == "normal" else 1))
    if kind == "normal":
        return rng.normal(7.2, 0.6, n)
    return np.where(rng.random(n) < 0.35, rng.normal(3.6, 0.25, n), rng.normal(5.1, 0.4, n))


def example_grid(x: np.ndarray, m: int) -> np.ndarray:
    return np.linspace(x.min() - 1.0, x.max() + 1.0, m)


def scipy_cases():
    """(name, samples, points): the grid is the examples' 1000 points, 64 where the long-double reference sum of
    400 000 samples would take minutes."""
    out = [(f"cc3-{k}", v, example_grid(v, 1000)) for k, v in golden_cc3().items()]
    for kind in ("normal", "bimodal"):
        for n in (10, 4000, 400000):
            x = synthetic(kind, n)
            out.append((f"{kind}-{n}", x, example_grid(x, 1000 if n <= 4000 else 64)))
    x = synthetic("normal", 4000)
    far = 60.0 * x.std(ddof=1)          # (every bandwidth factor used here is below 1)
    out.append(("far-tails", x, np.linspace(x.min() - far, x.max() + far, 1000)))
    return out


def exp_arguments() -> np.ndarray:
    """>= 1e6 arguments of pw_exp: a dense sweep of [-745, 0], both neighbours of every reduction boundary
    (i + 1/2) ln2/128 down to -745 and the boundary's own rounding, and every -0.5 z^2 of a real job."""
    sweep = np.linspace(-745.0, 0.0, 1_500_001)
    i = np.arange(-137600, 1)
    b = (i + 0.5) * (np.log(2.0) / 128.0)
    edges = np.concatenate([np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)])
    edges = edges[edges <= 0.0]
    x = golden_cc3()["windows"]
    g = example_grid(x, 1000)
    r = 1.0 / (x.std(ddof=1) * len(x) ** -0.2)
    z = (g[:, None] - x[None, :]) * r
    job = (-0.5 * (z * z)).reshape(-1)
    x2 = synthetic("bimodal", 4000)
    z2 = (example_grid(x2, 200)[:, None] - x2[None, :]) * (1.0 / (x2.std(ddof=1) * 4000 ** -0.2))
    special = np.array([0.0, -0.0, -1e-300, -2.0 ** -54, -2.0 ** -30, -708.3964185322641, -708.3964185322642, -708.39,
                        -709.0, -745.0, -1e4, -np.inf])
    return np.concatenate([sweep, edges, job, (-0.5 * (z2 * z2)).reshape(-1), special])


def mixed_batch():
    """64 small jobs of different sizes around the chunk length and the tile width, n = 0 / 1 and m = 1 included:
    (jobs as (samples, points, inv_bandwidth))."""
    chunk, tile = source_constant("KDE_CHUNK"), source_constant("KDE_WAVE") * source_constant("KDE_LANE_POINTS")
    rng = np.random.default_rng(64)
    ns = [0, 1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3, 17]
    ms = [1, 2, tile - 1, tile, tile + 1, 63, 64, 65, 2 * tile + 1, 5]
    jobs = []
    for k in range(64):
        n, m = ns[k % len(ns)], ms[(k // 3 + k) % len(ms)]
        x = rng.normal(5.0 + 0.1 * k, 0.5 + 0.01 * k, n)
        jobs.append((x, np.linspace(2.0, 9.0 + 0.1 * k, m), 1.0 / (0.05 + 0.01 * k)))
    return jobs


def pack(jobs):
    """(KDE_JOB_DTYPE array, samples, points) of a list of (samples, points, inv_bandwidth)."""
    from pywindow_amd import _lib

    rec = np.zeros(len(jobs), dtype=_lib.KDE_JOB_DTYPE)
    rec["n_samples"] = [len(j[0]) for j in jobs]
    rec["n_points"] = [len(j[1]) for j in jobs]
    rec["sample_first"] = np.cumsum(rec["n_samples"]) - rec["n_samples"]
    rec["point_first"] = np.cumsum(rec["n_points"]) - rec["n_points"]
    rec["inv_bandwidth"] = [j[2] for j in jobs]
    cat = lambda parts: np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]) if parts else np.zeros(0)
    return rec, cat([j[0] for j in jobs]), cat([j[1] for j in jobs])


def internal_exp(ctx, x: np.ndarray) -> np.ndarray:
    """pw_exp element by element through the library's test entry, on the context's device or host path."""
    import ctypes

    from pywindow_amd import _lib

    L = _lib.load()
    L.pw_internal_exp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    rc = L.pw_internal_exp(ctx._h, x.ctypes.data, len(x), y.ctypes.data)
    assert rc == 0, L.pw_last_error()
    return y
