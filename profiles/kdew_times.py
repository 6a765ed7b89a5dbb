"""Times of pw_kde_wsums for DESIGN.md ("Weights and bootstrap bands"): writes profiles/kdew_times.json.

    python profiles/kdew_times.py [--out profiles/kdew_times.json]     # needs a gfx950 device

Two warm-up calls, median of 7.  kernel ms: HIP events around the kernels of a call (the library's measurement hook);
call ms: perf_counter around the C call from pageable host arrays; host path: the same call on a device = -1 context
with 16 threads; "as R jobs": the same samples and points as one pw_kde_sums job per replica (what a band would cost
without the shared exponentials), kernel ms through that entry's hook; SciPy: gaussian_kde(weights=) on one core of
the same machine for a few replicas, scaled to all.
"""
import argparse
import ctypes
import json
import os
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import _kde_cases as K  # noqa: E402
import _kdew_cases as W  # noqa: E402
from pywindow_amd import _lib, distributions  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12


def job(n, m, replicas, seed):
    x = K.synthetic("bimodal", n) + 0.01 * seed
    frames = max(2, n // 4)                                     # four windows a frame
    w = distributions.block_bootstrap_counts(frames, 30, replicas, seed=seed)[:, np.arange(n) * frames // n]
    return x, K.example_grid(x, m), w.astype(np.float64), 1.0 / distributions.bandwidth(x)[0]


def cases():
    return [
        ("4000 x 1000 x 200 (the band of the example trajectory's window diameters)", [job(4000, 1000, 200, 1)], 3),
        ("400 000 x 1000 x 64", [job(400_000, 1000, 64, 2)], 1),
        ("64 jobs of 4000 x 1000 x 200", [job(4000, 1000, 200, 10 + k) for k in range(64)], 3),
    ]


def median_of(f, repeats=7, warm=2):
    for _ in range(warm):
        f()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def plain_kernel_ms(ctx, jobs):
    """Kernel ms of the same work as one pw_kde_sums job per replica, all in one call."""
    L = _lib.load()
    vp = ctypes.c_void_p
    L.pw_internal_kde_sums_timed.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.POINTER(ctypes.c_float)]
    rec = np.zeros(sum(len(w) for _, _, w, _ in jobs), dtype=_lib.KDE_JOB_DTYPE)
    at = s0 = p0 = 0
    for x, g, w, r in jobs:
        for _ in range(len(w)):
            rec[at] = (s0, len(x), p0, len(g), r)
            at, p0 = at + 1, p0 + len(g)
        s0 += len(x)
    xs = np.concatenate([j[0] for j in jobs])
    gs = np.concatenate([np.tile(j[1], len(j[2])) for j in jobs])
    sums = np.zeros(len(gs))
    ms = ctypes.c_float(0.0)
    out = []
    for k in range(5):
        rc = L.pw_internal_kde_sums_timed(ctx._h, rec.ctypes.data, len(rec), xs.ctypes.data, gs.ctypes.data, sums.ctypes.data,
                                          ctypes.byref(ms))
        assert rc == 0, L.pw_last_error()
        if k >= 2:
            out.append(float(ms.value))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kdew_times.json"))
    args = ap.parse_args()
    dev, host = _lib.Context(0), _lib.Context(-1, host_threads=16)
    from scipy import stats

    os.environ["OMP_NUM_THREADS"] = "1"
    results = []
    for name, jobs, scipy_replicas in cases():
        packed = W.pack(jobs)
        weighted = float(sum(len(x) * len(g) * len(w) for x, g, w, _ in jobs))
        exps = float(sum(len(x) * len(g) for x, g, _, _ in jobs))
        kernel = []
        for k in range(9):
            got, ms = W.internal_wsums(dev, *packed, timed=True)
            if k >= 2:
                kernel.append(ms)
        call = median_of(lambda: dev.kde_wsums(*packed))
        t0 = time.perf_counter()
        want = host.kde_wsums(*packed)
        host_ms = (time.perf_counter() - t0) * 1e3
        plain_ms = plain_kernel_ms(dev, jobs)
        x, g, w, r = jobs[0]
        t0 = time.perf_counter()
        for b in range(scipy_replicas):
            stats.gaussian_kde(x, bw_method="scott", weights=w[b])(g)
        per_replica = (time.perf_counter() - t0) * 1e3 / scipy_replicas
        k_med = float(np.median(kernel))
        results.append({
            "case": name, "jobs": len(jobs), "weighted_terms": weighted, "exponentials": exps,
            "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
            "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 7,
            "host_path_16_threads_ms": host_ms, "device_equals_host_bits": bool(got.tobytes() == want.tobytes()),
            "as_one_pw_kde_sums_job_per_replica_kernel_ms": plain_ms, "kernel_ms_over_per_replica_jobs": k_med / plain_ms,
            "weighted_terms_per_s_kernel": weighted / (k_med * 1e-3),
            "scipy_one_core_ms": per_replica * sum(len(j[2]) for j in jobs),
            "scipy_note": f"{scipy_replicas} replica(s) of the first job timed, times the number of replicas of the call",
        })
        print(json.dumps(results[-1]), flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/kdew_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
