"""Times of pw_superpose for DESIGN.md ("Window identity"): writes profiles/superpose_times.json.

    python profiles/superpose_times.py [--out profiles/superpose_times.json]    # needs a gfx950 device
    python profiles/superpose_times.py --case onto-1000 --once                  # one call of a case (for a kernel trace)

Every case runs in a process of its own under a time limit.  Two warm-up calls, median of 7 (3 for the host path).  kernel
ms: HIP events around the kernels of the calls of a case (the library's measurement hook), summed over its slabs; call
ms: perf_counter around the C calls from and into pageable host arrays, copies included; host path: the same calls on a
device = -1 context with 16 threads; the numpy SVD-Kabsch loop (tests/_superpose_cases.py: kabsch) on a SAMPLE of the
jobs on one core, SCALED to the case.
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

ATOMS = 168
#: name -> (frames, all pairs?, time limit of the case in seconds)
CASES = {
    "onto-1000": (1000, False, 180),
    "pairs-1000": (1000, True, 300),
    "pairs-4000": (4000, True, 900),
}


def workload(frames):
    """A cage of 168 atoms that tumbles and breathes: a random rotation, a shift and thermal noise a frame."""
    import _superpose_cases as C

    rng = np.random.default_rng(168)
    base = 5.0 * rng.standard_normal((ATOMS, 3))
    return np.array([C.moved(base, C.random_rotation(rng), rng.uniform(-2, 2, 3), 0.1, rng) for _ in range(frames)])


def slabs(frames, pairs):
    """The job arrays of the case, as pywindow_amd.superposition cuts them."""
    from pywindow_amd import _lib, superposition as SP

    if pairs:
        i, j = np.triu_indices(frames, 1)
    else:
        i, j = np.arange(frames), np.zeros(frames, dtype=np.int64)
    out = []
    for lo in range(0, len(i), SP.MATRIX_SLAB):
        a, b = i[lo:lo + SP.MATRIX_SLAB], j[lo:lo + SP.MATRIX_SLAB]
        jobs = np.zeros(len(a), dtype=_lib.SUPERPOSE_JOB_DTYPE)
        jobs["mobile_first"], jobs["target_first"], jobs["weight_first"] = a * ATOMS, b * ATOMS, -1
        jobs["n"], jobs["out"] = ATOMS, np.arange(len(a))
        out.append(jobs)
    return out


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
    import _superpose_cases as C
    from pywindow_amd import _lib

    frames, pairs, _ = CASES[name]
    coords = workload(frames)
    xyz = coords.reshape(-1, 3)
    work = slabs(frames, pairs)
    rows = [np.zeros(len(j), dtype=_lib.SUPERPOSE_OUT_DTYPE) for j in work]
    n_jobs = sum(len(j) for j in work)
    dev = _lib.Context(0)
    if once:
        C.raw(dev, work[0], xyz, None, rows[0])
        print("one call:", rows[0]["rmsd"][:3].tolist())
        return
    host = _lib.Context(-1, host_threads=16)

    def calls(ctx, timed=False):
        total = 0.0
        for j, r in zip(work, rows):
            got = C.raw(ctx, j, xyz, None, r, workspace_bytes=0 if timed else None, timed=timed)
            assert got[0] == 0
            total += got[2] if timed else 0.0
        return total

    kernel = [calls(dev, True) for _ in range(9)][2:]
    call = median_of(lambda: calls(dev))
    got = [r.copy() for r in rows]
    host_ms = median_of(lambda: calls(host), 3, 1)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(got, rows))
    sample = np.arange(0, len(work[0]), max(len(work[0]) // 200, 1))[:200]
    t0 = time.perf_counter()
    ref = [C.kabsch(xyz[m:m + ATOMS], xyz[t:t + ATOMS])[1] for m, t in zip(work[0]["mobile_first"][sample], work[0]["target_first"][sample])]
    sample_ms = (time.perf_counter() - t0) * 1e3
    k_med = float(np.median(kernel))
    result = {
        "case": name, "shape": f"{n_jobs} jobs of {ATOMS} atoms over {frames} frames, {len(work)} call(s)", "jobs": n_jobs,
        "result_bytes": int(sum(r.nbytes for r in rows)), "kernel_ms_median": k_med, "kernel_ms_min": float(min(kernel)),
        "kernel_ms_max": float(max(kernel)), "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "repeats": 7, "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "host_repeats": 3, "device_equals_host": bool(same),
        "largest_rmsd_difference_to_numpy_kabsch_on_the_sample": float(np.abs(got[0]["rmsd"][sample] - np.array(ref)).max()),
        "jobs_per_s_kernel": n_jobs / (k_med * 1e-3), "jobs_per_s_call": n_jobs / (call[0] * 1e-3),
        "jobs_per_s_host": n_jobs / (host_ms[0] * 1e-3),
        "numpy_kabsch_one_core_ms_scaled": sample_ms * (n_jobs / len(sample)),
        "numpy_kabsch_note": f"{len(sample)} of the {n_jobs} jobs timed on one core, scaled",
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "superpose_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.once)
        return
    results = []
    for name, spec in CASES.items():
        try:
            done = subprocess.run([sys.executable, __file__, "--case", name], capture_output=True, text=True, timeout=spec[2])
        except subprocess.TimeoutExpired:
            results.append({"case": name, "error": f"no result within {spec[2]} s"})
            break                                                  # (nothing more is started after a case that hung)
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not line:
            results.append({"case": name, "error": f"exit status {done.returncode}", "stderr": done.stderr[-2000:]})
            break                                                  # (nor after one that failed)
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/superpose_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
