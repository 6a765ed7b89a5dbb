"""Times of pw_trans_counts for DESIGN.md ("Trajectory kinetics"): writes profiles/trans_times.json.

    python profiles/trans_times.py [--out profiles/trans_times.json]    # needs a gfx950 device
    python profiles/trans_times.py --case long --once                   # one call of a case (for a kernel trace)

Every case runs in a process of its own under a time limit.  Two warm-up calls, median of 7 (3 for the host path).  kernel
ms: HIP events around the zeroing of the result and the kernels of a call (the library's measurement hook); call ms:
perf_counter around the C call from and into pageable host arrays, copies included; host path: the same call on a device
= -1 context with 16 threads; the numpy definition (tests/_trans_cases.py: reference) on ONE series x 10 of its lags on
one core, SCALED to the case.
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

#: name -> (series, frames, lags, states, time limit of the case in seconds)
CASES = {
    "cages-2": (80, 10_000, 1000, 2, 240),
    "cages-5": (80, 10_000, 1000, 5, 240),
    "long": (1, 1_000_000, 32_768, 2, 420),
    "many": (512, 10_000, 5000, 2, 420),
    "one-trajectory": (1, 1000, 500, 2, 120),
}


def workload(series, frames, lags, states):
    """Slow breathing plus noise, 1 % gaps; the edges at the quantiles of each series."""
    jobs = []
    for k in range(series):
        rng = np.random.default_rng(700 + k)
        t = np.arange(frames)
        x = 3.5 + 0.25 * np.sin(t * (0.01 + 0.0005 * (k % 80))) + 0.1 * np.convolve(rng.standard_normal(frames + 15), np.ones(16) / 4.0, "valid")
        x[rng.random(frames) < 0.01] = np.nan
        jobs.append((x, np.nanquantile(x, np.arange(1, states) / states), (0, 1, lags)))
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


def run_case(name, once):
    import _trans_cases as C
    from pywindow_amd import _lib

    series, frames, lags, states, _ = CASES[name]
    jobs = workload(series, frames, lags, states)
    rec, x, e = C.pack(jobs)
    dev = _lib.Context(0)
    if once:
        counts = dev.trans_counts(rec, x, e, states)
        print("one call:", counts[1].tolist(), int(counts.sum()))
        return
    host = _lib.Context(-1, host_threads=16)
    steps = float(sum(max(frames - k, 0) for k in range(lags))) * series
    counts = np.zeros((series * lags, states, states), dtype=np.int64)
    kernel = []
    for k in range(9):
        rc, _, ms = C.raw_counts(dev, rec, x, e, states, counts, workspace_bytes=0, timed=True)
        assert rc == 0
        if k >= 2:
            kernel.append(ms)
    call = median_of(lambda: C.raw_counts(dev, rec, x, e, states, counts))
    got = counts.copy()
    host_ms = median_of(lambda: C.raw_counts(host, rec, x, e, states, counts), 3, 1)
    same = bool(np.array_equal(got, counts))
    sample = np.arange(0, lags, max(lags // 10, 1))[:10]
    t0 = time.perf_counter()
    ref = C.reference(jobs[0][0], jobs[0][1], sample, states)
    sample_ms = (time.perf_counter() - t0) * 1e3
    k_med = float(np.median(kernel))
    result = {
        "case": name, "shape": f"{series} series of {frames} frames x {lags} lags, {states} states", "pair_steps": steps,
        "result_bytes": int(counts.nbytes), "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)),
        "kernel_ms_max": float(max(kernel)), "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "repeats": 7, "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "host_repeats": 3, "device_equals_host": same,
        "device_equals_reference_on_the_sample": bool(np.array_equal(got[sample], ref)),
        "pair_steps_per_s_kernel": steps / (k_med * 1e-3), "pair_steps_per_s_call": steps / (call[0] * 1e-3),
        "pair_steps_per_s_host": steps / (host_ms[0] * 1e-3),
        "numpy_reference_one_core_ms_scaled": sample_ms * (lags / len(sample)) * series,
        "numpy_reference_note": f"one series x {len(sample)} of its {lags} lags timed on one core, scaled",
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trans_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.once)
        return
    results = []
    for name, spec in CASES.items():
        try:
            done = subprocess.run([sys.executable, __file__, "--case", name], capture_output=True, text=True, timeout=spec[4])
        except subprocess.TimeoutExpired:
            results.append({"case": name, "error": f"no result within {spec[4]} s"})
            break                                                  # (nothing more is started after a case that hung)
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not line:
            results.append({"case": name, "error": f"exit status {done.returncode}", "stderr": done.stderr[-2000:]})
            break                                                  # (nor after one that failed)
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/trans_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
