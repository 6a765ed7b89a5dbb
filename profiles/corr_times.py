"""Times of pw_corr_sums for DESIGN.md ("Trajectory dynamics"): writes profiles/corr_times.json.

    python profiles/corr_times.py [--out profiles/corr_times.json]     # needs a gfx950 device
    python profiles/corr_times.py --long-once                         # one call of the long job (for a kernel trace)

Two warm-up calls, median of 7.  kernel ms: HIP events around the kernels of a call (the library's measurement hook);
call ms: perf_counter around the C call from pageable host arrays; host path: the same call on a device = -1 context
with 16 threads; np.correlate and scipy.signal.correlate(method="fft") on one core of the same machine.
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

import _corr_cases as C  # noqa: E402
from pywindow_amd import _lib  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12


def series(n, seed):
    return C.centred(C.ar1(n, 0.99, seed))


def cases():
    return [
        ("1000 x 500 (one cage, one trajectory of the headline workload)", [(series(1000, 1), None, 500)]),
        ("8 x 4 series of 10 000 x 5000 (the periodic example, every cage, four quantities)",
         [(series(10_000, k), None, 5000) for k in range(32)]),
        ("1 000 000 x 32 768", [(series(1_000_000, 2), None, 32_768)]),
        ("512 jobs of 10 000 x 5000", [(series(10_000, 100 + k), None, 5000) for k in range(512)]),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "corr_times.json"))
    ap.add_argument("--long-once", action="store_true")
    args = ap.parse_args()
    dev, host = _lib.Context(0), _lib.Context(-1, host_threads=16)
    if args.long_once:
        got = dev.corr_sums(*C.pack(cases()[2][1]))
        print("long job:", got[:2])
        return
    from scipy import signal

    os.environ["OMP_NUM_THREADS"] = "1"
    results = []
    for name, jobs in cases():
        packed = C.pack(jobs)
        terms = float(sum(lags * len(a) - lags * (lags - 1) // 2 for a, _, lags in jobs))
        kernel = []
        for k in range(9):
            got, ms = C.internal_sums(dev, *packed, timed=True)
            if k >= 2:
                kernel.append(ms)
        call = median_of(lambda: dev.corr_sums(*packed))
        t0 = time.perf_counter()
        want = host.corr_sums(*packed)
        host_ms = (time.perf_counter() - t0) * 1e3
        a, _, lags = jobs[0]
        fft = median_of(lambda: signal.correlate(a, a, mode="full", method="fft"), 3, 1)[0] * len(jobs)
        direct = median_of(lambda: np.correlate(a, a, "full"), 3, 1)[0] * len(jobs) if len(a) <= 10_000 else None
        k_med = float(np.median(kernel))
        results.append({
            "case": name, "jobs": len(jobs), "terms": terms,
            "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
            "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 7,
            "host_path_16_threads_ms": host_ms, "device_equals_host_bits": bool(got.tobytes() == want.tobytes()),
            "fma_per_s_kernel": terms / (k_med * 1e-3), "flop_per_term": 2,
            "fraction_of_78.6_TFs_fp64_vector_peak": 2.0 * terms / (k_med * 1e-3) / PEAK_FP64_VECTOR,
            "numpy_correlate_one_core_ms": direct, "scipy_fft_one_core_ms": fft,
            "one_core_note": "one series timed, times the number of jobs",
        })
        print(json.dumps(results[-1]), flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/corr_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
