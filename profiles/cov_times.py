"""Times of pw_covariance for DESIGN.md ("Essential dynamics"): writes profiles/cov_times.json.

    python profiles/cov_times.py [--out profiles/cov_times.json]    # needs a gfx950 device
    python profiles/cov_times.py --case frames-10000 --once         # one call of a case (for a kernel trace)

168 atoms (CC3, D = 504) at 1 000, 10 000 and 100 000 frames, every frame the base with noise of 0.1, rotated and moved at
random.  Every case runs in a process of its own under a time limit.  One warm-up call, median of 5 (3 for the host
path and numpy).  kernel ms: HIP events around all kernels of a pw_covariance call -- the mean's two, the partial and
the reduce kernels (the library's measurement hook); call ms: perf_counter around pw_superpose onto frame 0 and
pw_covariance with those rows, from and into pageable host arrays, the finiteness scan of the matrix on the host
included; covariance call ms: pw_covariance alone; host path: the same two calls on a device = -1 context with 16
threads; numpy: the same pipeline -- every frame aligned onto frame 0 by a batched SVD, then np.cov -- with the BLAS
threads the environment gives (16 on the machine the figures in DESIGN.md were taken on), in the same run.
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ATOMS = 168
#: name -> (frames, time limit of the case in seconds)
CASES = {f"frames-{n}": (n, limit) for n, limit in ((1000, 120), (10_000, 180), (100_000, 420))}


def trajectory(frames):
    from pywindow_amd import synth

    rng = np.random.default_rng(500 + frames)
    base = synth.load_cc3_base()[1]
    assert base.shape == (ATOMS, 3)
    q = rng.standard_normal((frames, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b, c, d = q.T
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]]).transpose(2, 0, 1)
    x = base[None] + 0.1 * rng.standard_normal((frames, ATOMS, 3))
    return np.ascontiguousarray(np.einsum("fij,fnj->fni", R, x) + rng.uniform(-5, 5, (frames, 1, 3)))


def numpy_pipeline(coords):
    """Align every frame onto frame 0 (Kabsch, batched SVD), then np.cov of the aligned coordinates."""
    F = len(coords)
    cx = coords.mean(axis=1, keepdims=True)
    d = coords - cx
    ref = d[0]
    u, _, vt = np.linalg.svd(np.einsum("fni,nj->fij", d, ref))
    sign = np.sign(np.linalg.det(u @ vt))
    u[:, :, 2] *= sign[:, None]
    R = np.transpose(u @ vt, (0, 2, 1))
    aligned = np.einsum("fij,fnj->fni", R, d) + cx[0]
    return np.cov(aligned.reshape(F, -1).T)


def median_of(f, repeats, warm=1):
    for _ in range(warm):
        f()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def run_case(name, once):
    from pywindow_amd import _lib
    from pywindow_amd import superposition as SP

    frames, _ = CASES[name]
    coords = trajectory(frames)
    X = coords.reshape(frames, -1)
    D = X.shape[1]
    jobs = np.zeros(1, dtype=_lib.COV_JOB_DTYPE)
    jobs["T"], jobs["D"] = frames, D
    from pywindow_amd import engine

    dev = engine.context(0)                                    # (the context superpose_onto uses: one per device)
    mean, scatter = np.zeros(D), np.zeros(D * D)

    def both(ctx, device):
        rows = SP.superpose_onto(coords, 0, None, device)
        return ctx.covariance(jobs, X, rows, mean=mean, scatter=scatter)

    if once:
        both(dev, 0)
        print("one call:", float(scatter[0]), float(mean[0]))
        return
    host = engine.context(-1)
    _lib.load().pw_context_host_threads(host._h, 16)
    rows = SP.superpose_onto(coords, 0, None, 0)
    kernel = []
    for k in range(6):
        dev.covariance(jobs, X, rows, mean=mean, scatter=scatter, kernel_ms=kernel)
    kernel = kernel[1:]
    got = (mean.copy(), scatter.copy())
    cov_call = median_of(lambda: dev.covariance(jobs, X, rows, mean=mean, scatter=scatter), 5)
    call = median_of(lambda: both(dev, 0), 5)
    host_ms = median_of(lambda: both(host, -1), 3, warm=0 if frames >= 100_000 else 1)
    same = got[0].tobytes() == mean.tobytes() and got[1].tobytes() == scatter.tobytes()
    numpy_ms = median_of(lambda: numpy_pipeline(coords), 3, warm=0 if frames >= 100_000 else 1)
    rel = float(np.abs(scatter.reshape(D, D) / (frames - 1) - numpy_pipeline(coords)).max() / np.abs(scatter).max() * (frames - 1))
    tiles = (D + 127) // 128
    computed = tiles * (tiles + 1) // 2 * 128 * 128 * frames
    k_ms = float(np.median(kernel))
    result = {
        "case": name, "frames": frames, "atoms": ATOMS, "D": D, "matrix_bytes": int(X.nbytes), "scatter_bytes": int(scatter.nbytes),
        "fma_of_the_definition": int(frames * D * D), "fma_computed_in_upper_tiles": int(computed),
        "kernel_ms_median": k_ms, "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
        "kernel_fp64_tflops_of_computed_fma": 2.0 * computed / (k_ms * 1e-3) / 1e12,
        "covariance_call_ms_median": cov_call[0], "covariance_call_ms_min": cov_call[1], "covariance_call_ms_max": cov_call[2],
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 5,
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "host_repeats": 3, "device_equals_host": bool(same),
        "numpy_pipeline_ms_median": numpy_ms[0], "numpy_pipeline_ms_min": numpy_ms[1], "numpy_pipeline_ms_max": numpy_ms[2],
        "numpy_threads": os.environ.get("OMP_NUM_THREADS"), "largest_difference_from_numpy_relative": rel,
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cov_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.once)
        return
    results = []
    for name, spec in CASES.items():
        try:
            done = subprocess.run([sys.executable, __file__, "--case", name], capture_output=True, text=True, timeout=spec[1])
        except subprocess.TimeoutExpired:
            results.append({"case": name, "error": f"no result within {spec[1]} s"})
            break                                                  # (nothing more is started after a case that hung)
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not line:
            results.append({"case": name, "error": f"exit status {done.returncode}", "stderr": done.stderr[-2000:]})
            break                                                  # (nor after one that failed)
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/cov_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 1 warm-up call, median of 5"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
