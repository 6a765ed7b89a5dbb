"""Times of pw_charges for DESIGN.md ("Framework charges"): writes profiles/charges_times.json.

    python profiles/charges_times.py [--out profiles/charges_times.json]    # needs a gfx950 device
    python profiles/charges_times.py --case cc3-1000 --quick                # device times only, 3 repeats

The case runs in a process of its own under a time limit.  The workload is that of profiles/rigid_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), all in ONE pw_charges call
(total charge 0, tol 1e-10, max_iter 1000).  Two warm-up calls, median of 7.  device ms: HIP events around the kernels
of a call (the library's measurement hook); public ms: perf_counter around pywindow_amd.equilibrate_charges_batch; host
path: the public call on a device = -1 context with 16 threads, once, and its bytes against the device's.  pair
evaluations: n^2 a step of a frame, one evaluation serving both systems, so n^2 max(iterations) a frame.  Then the same
frames as a trajectory: DLPOLY.rigid_affinity("CO2", charges="qeq") against the uncharged call, and the CO2 / N2
selectivity at 298 K with and without charges.
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

#: name -> (frames, time limit of the case in seconds)
CASES = {"cc3-1000": (1000, 560)}


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def run_case(name, quick):
    import pywindow_amd as pw
    from pywindow_amd import engine, synth

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    n = len(elements)
    repeats, warm = (3, 1) if quick else (7, 2)
    ms = []
    got = None
    for _ in range(warm + repeats):
        got = pw.equilibrate_charges_batch(frames, elements, device=0, kernel_ms=ms)
    device = spread(ms[warm:])
    its = np.asarray(got.iterations)
    evaluations = float(n) * n * float(its.max(axis=1).sum())
    result = {"case": name, "frames": n_frames, "atoms": n, "tol": 1e-10, "max_iter": 1000, "repeats": repeats, "warm_ups": warm,
              "device_ms": device, "converged_frames": int(np.asarray(got.converged).sum()),
              "iterations_system_s": {"min": int(its[:, 0].min()), "median": float(np.median(its[:, 0])), "max": int(its[:, 0].max())},
              "iterations_system_t": {"min": int(its[:, 1].min()), "median": float(np.median(its[:, 1])), "max": int(its[:, 1].max())},
              "pair_evaluations": evaluations, "pair_evaluations_per_s": evaluations / (device["median"] * 1e-3),
              "charge_n_median": float(np.median(got.charges[:, np.asarray(elements) == "N"])),
              "charge_h_median": float(np.median(got.charges[:, np.asarray(elements) == "H"])),
              "dipole_norm_median": float(np.median(got.dipole_norm))}
    if not quick:
        times = []
        for _ in range(2 + 7):
            t0 = time.perf_counter()
            pw.equilibrate_charges_batch(frames, elements, device=0)
            times.append((time.perf_counter() - t0) * 1e3)
        result["public_ms"] = spread(times[2:])
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
        t0 = time.perf_counter()
        ref = pw.equilibrate_charges_batch(frames, elements, device=-1)
        result["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        result["device_equals_host"] = bool(got.charges.tobytes() == ref.charges.tobytes() and got.raw.tobytes() == ref.raw.tobytes())
        # the same frames as a trajectory: CO2 and N2, with the library's charges and without
        with tempfile.TemporaryDirectory() as tmp:
            traj = pw.DLPOLY(synth.write_history(pathlib.Path(tmp) / "HISTORY", elements, list(frames)))
            traj.analysis()
            calls = {}
            for guest in ("CO2", "N2"):
                for kind, charges in (("uncharged", None), ("qeq", "qeq")):
                    wall = []
                    for _ in range(1 + 3):
                        t0 = time.perf_counter()
                        af = traj.rigid_affinity(guest, 298.0, charges=charges, device=0)
                        wall.append((time.perf_counter() - t0) * 1e3)
                    calls[(guest, kind)] = af
                    result[f"rigid_affinity_{guest}_{kind}_public_ms"] = spread(wall[1:])
            for kind in ("uncharged", "qeq"):
                sel = calls[("CO2", kind)].selectivity(calls[("N2", kind)])[:, 0]
                ok = calls[("CO2", kind)].series("henry")[1] & calls[("N2", kind)].series("henry")[1]
                result[f"selectivity_co2_n2_{kind}"] = {"median": float(np.median(sel[ok])), "min": float(sel[ok].min()),
                                                        "max": float(sel[ok].max()), "frames": int(ok.sum())}
                result[f"heat_co2_{kind}_median"] = float(np.median(calls[("CO2", kind)].heat[ok, 0]))
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "charges_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.quick)
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
    meta = {"commit_parent": head or None, "command": "python profiles/charges_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
