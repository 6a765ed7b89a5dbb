"""Times of pw_dft_sums for DESIGN.md ("Trajectory spectra"): writes profiles/dft_times.json.

    python profiles/dft_times.py [--out profiles/dft_times.json]      # needs a gfx950 device
    python profiles/dft_times.py --long-once                          # one call of the long job (for a kernel trace)

Every case runs in a process of its own under `timeout`, and the first one that fails ends the run.  Two warm-up
calls, median of 7.  kernel ms: HIP events around the kernels of a call (the library's measurement hook); call ms:
perf_counter around the C call from pageable host arrays; host path: the same call on a device = -1 context with 16
threads; scipy.signal.lombscargle(normalize=True, floating_mean=True) on one core of the same machine, timed on a
subset of the frequencies of one series and scaled to the case (said so in the record).
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

import _dft_cases as C  # noqa: E402
from pywindow_amd import _lib  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12
CASE_SECONDS = 420


def series(n, seed):
    return C.centred(C.ar1(n, 0.99, seed))


def cases():
    """(name, jobs as _dft_cases.pack takes them)"""
    return [
        ("1000 x 2000 (one cage, one trajectory of the headline workload, oversample 4)", [(series(1000, 1), 4000, 1, 1, 1999)]),
        ("8 series of 10 000 x 20 000 (the periodic example, every cage)",
         [(series(10_000, k), 40_000, 1, 1, 19_999) for k in range(8)]),
        ("1 000 000 x 16 384", [(series(1_000_000, 2), 4_000_000, 1, 1, 16_384)]),
        ("512 jobs of 10 000 x 5000", [(series(10_000, 100 + k), 40_000, 1, 1, 5000) for k in range(512)]),
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


def one_case(index: int) -> dict:
    from scipy import signal

    name, jobs = cases()[index]
    dev, host = _lib.Context(0), _lib.Context(-1, host_threads=16)
    packed = C.pack(jobs)
    terms = float(sum(len(a) * nf for a, _, _, _, nf in jobs))
    kernel = []
    for k in range(9):
        got, ms = C.internal_sums(dev, *packed, timed=True)
        if k >= 2:
            kernel.append(ms)
    call = median_of(lambda: dev.dft_sums(*packed))
    t0 = time.perf_counter()
    want = host.dft_sums(*packed)
    host_ms = (time.perf_counter() - t0) * 1e3
    a, period, first, step, nf = jobs[0]
    sub = min(nf, max(1, int(2e7 // len(a))))                    # frequencies SciPy is timed on: about 2e7 terms
    t = np.arange(len(a), dtype=np.float64)
    w = 2.0 * np.pi * (first + step * np.arange(sub)) / period
    t0 = time.perf_counter()
    signal.lombscargle(t, a, w, normalize=True, floating_mean=True)
    scipy_ms = (time.perf_counter() - t0) * 1e3 * (terms / (len(a) * sub))
    k_med = float(np.median(kernel))
    return {
        "case": name, "jobs": len(jobs), "terms": terms,
        "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 7,
        "host_path_16_threads_ms": host_ms, "device_equals_host_bits": bool(got.tobytes() == want.tobytes()),
        "fma_per_s_kernel": 2.0 * terms / (k_med * 1e-3), "flop_per_term": 4,
        "fraction_of_78.6_TFs_fp64_vector_peak": 4.0 * terms / (k_med * 1e-3) / PEAK_FP64_VECTOR,
        "scipy_lombscargle_one_core_ms": scipy_ms,
        "one_core_note": f"extrapolated: {sub} of the {nf} frequencies of one series timed, scaled by the number of terms",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dft_times.json"))
    ap.add_argument("--long-once", action="store_true")
    ap.add_argument("--case", type=int, default=None, help="run one case in this process and print its record")
    args = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = "1"
    if args.long_once:
        got = _lib.Context(0).dft_sums(*C.pack(cases()[2][1]))
        print("long job:", got[:2])
        return
    if args.case is not None:
        print("RESULT " + json.dumps(one_case(args.case)), flush=True)
        return
    results = []
    for index in range(len(cases())):
        run = subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, __file__, "--case", str(index)],
                             cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not lines:
            print(f"case {index} ended with status {run.returncode}; nothing further is started\n{run.stderr[-2000:]}", flush=True)
            sys.exit(run.returncode or 1)
        results.append(json.loads(lines[-1][len("RESULT "):]))
        print(json.dumps(results[-1]), flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/dft_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
