"""Times of pw_cluster_gromos for DESIGN.md ("Conformational clustering"): writes profiles/cluster_times.json.

    python profiles/cluster_times.py [--out profiles/cluster_times.json]    # needs a gfx950 device
    python profiles/cluster_times.py --case few-4000 --once                 # one call of a case (for a kernel trace)

Every case runs in a process of its own under a time limit.  One warm-up call, median of 5 (3 for the host path).  device
ms: HIP events from the first kernel of a call to its last, the uploads of the slabs of the matrix and the copies of the
done flags included (the library's measurement hook); call ms: perf_counter around the C call from and into pageable host
arrays, the NaN scan of the matrix on the host included; host path: the same call on a device = -1 context with 16
threads; numpy: the definition (tests/_cluster_cases.py: reference) on one core, its first rounds timed and SCALED to the
number of clusters when there are more than 25 (every round of it is one n x n product, whatever is still active).

"few": frames around 6 centres at the 15 % quantile of the distances as the cutoff, some tens of clusters.  "singletons": the same matrix at a cutoff
below every distance -- n clusters, n + 1 rounds of two launches each: what a cutoff chosen far too small costs.
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

#: name -> (frames, kind, time limit of the case in seconds)
CASES = {f"{kind}-{n}": (n, kind, limit) for n, limit in ((1000, 120), (4000, 180), (10_000, 420)) for kind in ("few", "singletons")}


def matrix(n):
    rng = np.random.default_rng(900 + n)
    centres = rng.uniform(-4.0, 4.0, (6, 3))
    p = centres[rng.integers(0, 6, n)] + rng.normal(0.0, 0.7, (n, 3))
    sq = (p * p).sum(axis=1)
    d = sq[:, None] + sq[None, :] - 2.0 * (p @ p.T)
    np.maximum(d, 0.0, out=d)
    np.sqrt(d, out=d)
    np.fill_diagonal(d, 0.0)
    return d


def numpy_rounds(d, cutoff, most):
    """The loop of tests/_cluster_cases.py: reference, stopped after `most` rounds: (rounds run, frames left, seconds)."""
    n = len(d)
    t0 = time.perf_counter()
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    nb = np.zeros((n, n), dtype=bool)
    nb[upper] = d[upper] <= cutoff
    nb |= nb.T
    np.fill_diagonal(nb, True)
    nbf = nb.astype(np.float64)
    setup = time.perf_counter() - t0
    active = np.ones(n, dtype=bool)
    rounds = 0
    t0 = time.perf_counter()
    while active.any() and rounds < most:
        counts = np.where(active, nbf @ active.astype(np.float64), 0.0)
        active &= ~(nb[int(np.argmax(counts))] & active)
        rounds += 1
    return rounds, int(active.sum()), setup, time.perf_counter() - t0


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
    import _cluster_cases as C
    from pywindow_amd import _lib

    n, kind, _ = CASES[name]
    d = matrix(n)
    sample = d[np.triu_indices(min(n, 2000), 1)]
    cutoff = float(np.quantile(sample, 0.15)) if kind == "few" else 0.5 * float(d[np.triu_indices(n, 1)].min())
    rec, dist = C.pack([(d, cutoff)])
    dev = _lib.Context(0)
    if once:
        rc, out = C.raw(dev, rec, dist)
        print("one call:", rc, int(out[3][0]), out[2][:5].tolist())
        return
    host = _lib.Context(-1, host_threads=16)
    device = []
    for k in range(6):
        rc, got, ms = C.raw(dev, rec, dist, workspace_bytes=0, timed=True)
        assert rc == 0
        if k >= 1:
            device.append(ms)
    call = median_of(lambda: C.raw(dev, rec, dist), 5)
    host_ms = median_of(lambda: C.raw(host, rec, dist), 3)
    same = C.same(got, C.raw(host, rec, dist)[1])
    clusters = int(got[3][0])
    rounds, left, setup_s, loop_s = numpy_rounds(d, cutoff, 25)
    numpy_ms = (setup_s + loop_s * (clusters / rounds if left else 1.0)) * 1e3
    result = {
        "case": name, "frames": n, "cutoff": cutoff, "clusters": clusters, "largest_cluster": int(got[2][0]),
        "rounds_of_two_launches": clusters + 1, "matrix_bytes": int(d.nbytes), "bit_matrix_bytes": int(n * ((((n + 63) // 64) + 1) // 2 * 2) * 8),
        "device_ms_median": float(np.median(device)), "device_ms_min": float(min(device)), "device_ms_max": float(max(device)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2], "repeats": 5,
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "host_repeats": 3, "device_equals_host": bool(same),
        "numpy_one_core_ms": numpy_ms, "numpy_note": "complete" if not left else f"{rounds} of {clusters} rounds timed, scaled",
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cluster_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/cluster_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 1 warm-up call, median of 5"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
