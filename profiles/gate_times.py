"""Times of pw_gate_counts for DESIGN.md ("Gating statistics"): writes profiles/gate_times.json.

    python profiles/gate_times.py [--out profiles/gate_times.json]     # needs a gfx950 device
    python profiles/gate_times.py --once                               # one call of the workload (for a kernel trace)

The workload: 80 series of 10 000 frames x 1000 thresholds each, n_bins = 64 (8e8 steps; 80 000 rows of counts, 82 MB of
histograms).  Two warm-up calls, median of 7.  kernel ms: HIP events around the zeroing of the result and the kernels of
a call (the library's measurement hook); call ms: perf_counter around the C call from and into pageable host arrays,
copies included; host path: the same call on a device = -1 context with 16 threads; the Python definition
(tests/_gate_cases.py: reference) on ONE series x 20 of its thresholds on one core, SCALED to the workload.
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
sys.path.insert(0, str(ROOT / "tests"))

import _gate_cases as C  # noqa: E402
from pywindow_amd import _lib  # noqa: E402

FRAMES, THRESHOLDS, SERIES, BINS = 10_000, 1000, 80, 64


def workload():
    """Slow breathing plus noise, 1 % gaps; the thresholds sweep each series from its minimum to its maximum."""
    jobs = []
    for k in range(SERIES):
        rng = np.random.default_rng(500 + k)
        t = np.arange(FRAMES)
        x = 3.5 + 0.25 * np.sin(t * (0.01 + 0.0005 * k)) + 0.1 * np.convolve(rng.standard_normal(FRAMES + 15), np.ones(16) / 4.0, "valid")
        x[rng.random(FRAMES) < 0.01] = np.nan
        jobs.append((x, np.linspace(np.nanmin(x), np.nanmax(x), THRESHOLDS)))
    return jobs


def median_of(f, repeats=7, warm=2):
    for _ in range(warm):
        f()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gate_times.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    jobs = workload()
    rec, series, thr = C.pack(jobs)
    dev = _lib.Context(0)
    if args.once:
        counts, hist = dev.gate_counts(rec, series, thr, BINS)
        print("one call:", counts[:2].tolist(), int(hist.sum()))
        return
    host = _lib.Context(-1, host_threads=16)
    steps = float(FRAMES) * THRESHOLDS * SERIES
    rows = THRESHOLDS * SERIES
    counts = np.zeros((rows, C.FIELDS), dtype=np.int64)
    hist = np.zeros((rows, 2, BINS), dtype=np.int64)
    kernel = []
    for k in range(9):
        rc, _, _, ms = C.raw_counts(dev, rec, series, thr, BINS, counts, hist, workspace_bytes=0, timed=True)
        assert rc == 0
        if k >= 2:
            kernel.append(ms)
    call = median_of(lambda: C.raw_counts(dev, rec, series, thr, BINS, counts, hist))
    got = (counts.copy(), hist.copy())
    host_ms = median_of(lambda: C.raw_counts(host, rec, series, thr, BINS, counts, hist), 3, 1)
    same = bool(np.array_equal(got[0], counts) and np.array_equal(got[1], hist))
    a, d = jobs[0]
    t0 = time.perf_counter()
    for q in range(0, THRESHOLDS, THRESHOLDS // 20):
        with np.errstate(invalid="ignore"):
            C.reference(a, d[q], BINS)
    sample_ms = (time.perf_counter() - t0) * 1e3
    k_med = float(np.median(kernel))
    result = {
        "case": f"{SERIES} series of {FRAMES} frames x {THRESHOLDS} thresholds, n_bins = {BINS}", "steps": steps, "rows": rows,
        "result_bytes": int(counts.nbytes + hist.nbytes), "complete_runs": int(got[1].sum()),
        "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 7,
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "host_repeats": 3, "device_equals_host": same,
        "steps_per_s_kernel": steps / (k_med * 1e-3), "steps_per_s_call": steps / (call[0] * 1e-3),
        "python_reference_one_core_ms_scaled": sample_ms * (THRESHOLDS / 20) * SERIES,
        "python_reference_note": "one series x 20 of its 1000 thresholds timed on one core, scaled by 50 x 80",
    }
    print(json.dumps(result), flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/gate_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": [result]}, indent=1) + "\n")


if __name__ == "__main__":
    main()
