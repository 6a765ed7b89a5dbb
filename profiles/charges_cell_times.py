"""Times of pw_charges_cell for DESIGN.md ("Periodic charge equilibration"): writes profiles/charges_cell_times.json.

    python profiles/charges_cell_times.py [--out profiles/charges_cell_times.json]      # needs a gfx950 device
    python profiles/charges_cell_times.py --case cc3-cell-1000 --frames 16 --quick      # fewer frames, 3 repeats

The case runs in a process of its own under a time limit.  The workload is profiles/ewald_times.py's cell: the 1344-atom
CC3 cell of tests/golden/rebuild.npz with Gaussian noise of 0.02 A an atom (frame k from default_rng(4 + k)), 1000 frames in
ONE call at the defaults (cutoff 12, Ewald tolerance 1e-6, shield (4, 6), tol 1e-10).  One warm-up call, median of 3 with
min and max (a call is seconds long).  device ms: HIP events around the count kernel, the rows kernels (phase one: every row
of R and the phase tables) and the solver kernels, through the library's measurement hook; the public call: wall time of
pw.equilibrate_cell_charges_batch; host path: the same jobs on a device = -1 context with 16 threads, on --host-frames
frames, once, and its bytes against the device's; the diffusion coefficients of CO2 and N2 at 250 K and 350 K over 8 frames
with charges="qeq-cell", and their ratio beside the molecule-by-molecule figure of profiles/ewald_times.json."""
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

#: name -> (frames, time limit of the case in seconds)
CASES = {"cc3-cell-1000": (1000, 1100)}
TEMPERATURES = [250.0, 350.0]


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def run_case(name, quick, n_frames, host_frames, diffusion_frames):
    import pywindow_amd as pw
    from pywindow_amd import charges_cell as CC
    from pywindow_amd import engine

    n_frames = n_frames or CASES[name][0]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    elements = [str(e) for e in elements]
    noisy = lambda k: base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape)
    frames = np.stack([noisy(k) for k in range(n_frames)])
    repeats, warm = (3, 1)
    ctx = engine.context(0)
    jobs, atoms, params, kvecs = CC.plan_cell_charges(frames, elements, lattice)
    times, wall = [], []
    for _ in range(warm + repeats):
        q, out = ctx.charges_cell(jobs, atoms, params, kvecs, kernel_ms=times)
        t0 = time.perf_counter()
        made = pw.equilibrate_cell_charges_batch(frames, elements, lattice, device=0)
        wall.append((time.perf_counter() - t0) * 1e3)
    times = np.array(times[warm:])
    result = {"case": name, "frames": n_frames, "atoms": len(elements), "cutoff": 12.0, "ewald_tolerance": 1e-6, "shield": [4.0, 6.0],
              "tol": 1e-10, "alpha": float(jobs["alpha"][0]), "reciprocal_rows": int(jobs["n_k"][0]), "repeats": repeats,
              "warm_ups": warm, "device_ms_count": spread(times[:, 0]), "device_ms_rows": spread(times[:, 1]),
              "device_ms_solver": spread(times[:, 2]), "device_ms_all": spread(times.sum(axis=1)),
              "public_call_ms": spread(wall[warm:]), "iterations": spread(out["iterations"]),
              "frames_converged": int((out["flags"] == 0).sum()), "charge_min_max": [float(q.min()), float(q.max())],
              "public_call_equals_raw_call": bool(made.charges.tobytes() == q.tobytes())}
    result["device_ms_per_frame"] = result["device_ms_all"]["median"] / n_frames
    host = engine.context(-1)
    result["host_threads"] = int(pw._lib.load().pw_context_host_threads(host._h, 16))   # (sets, then reports)
    m = min(host_frames, n_frames)
    t0 = time.perf_counter()
    ref_q, ref_out = host.charges_cell(jobs[:m], atoms, params, kvecs)
    result["host_path_frames"] = m
    result["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
    result["host_path_16_threads_ms_per_frame"] = result["host_path_16_threads_ms"] / m
    result["device_equals_host"] = bool(ref_q.tobytes() == q[:len(ref_q)].tobytes() and ref_out.tobytes() == out[:m].tobytes())
    if not quick:
        few = frames[:diffusion_frames]
        coefficients = {}
        for guest in ("CO2", "N2"):
            d = pw.rigid_guest_diffusion_batch(few, elements, lattice, guest, TEMPERATURES, spacing=0.5, cutoff=12.0, device=0,
                                               charges="qeq-cell")
            coefficients[f"{guest}_qeq_cell"] = {"coefficient_A2_per_s": [spread(d.coefficient[:, l]) for l in range(len(TEMPERATURES))],
                                                 "frames_valid": int(d.valid.sum()), "charges_converged": int(d.charges_converged.sum())}
        result["diffusion_frames"] = len(few)
        result["temperatures"] = TEMPERATURES
        result["diffusion"] = coefficients
        result["CO2_over_N2_median_coefficient_qeq_cell"] = [
            coefficients["CO2_qeq_cell"]["coefficient_A2_per_s"][l]["median"] /
            max(coefficients["N2_qeq_cell"]["coefficient_A2_per_s"][l]["median"], 1e-300) for l in range(len(TEMPERATURES))]
        other = ROOT / "profiles" / "ewald_times.json"
        if other.exists():
            result["CO2_over_N2_median_coefficient_molecule_by_molecule"] = \
                json.loads(other.read_text())["results"][0].get("CO2_over_N2_median_coefficient_charged")
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "charges_cell_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--diffusion-frames", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.quick, args.frames, args.host_frames, args.diffusion_frames)
        return
    results = []
    for name, spec in CASES.items():
        command = [sys.executable, __file__, "--case", name, "--host-frames", str(args.host_frames), "--diffusion-frames",
                   str(args.diffusion_frames)] + (["--frames", str(args.frames)] if args.frames else []) + \
                  (["--quick"] if args.quick else [])
        try:
            done = subprocess.run(command, capture_output=True, text=True, timeout=spec[1])
        except subprocess.TimeoutExpired:
            results.append({"case": name, "error": f"no result within {spec[1]} s"})
            break                                                  # (nothing more is started after a case that hung)
        line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not line:
            results.append({"case": name, "error": f"exit status {done.returncode}", "stderr": done.stderr[-2000:]})
            break                                                  # (nor after one that failed)
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/charges_cell_times.py" +
            (f" --frames {args.frames}" if args.frames else "") + (" --quick" if args.quick else ""), "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 1 warm-up call, median of 3"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
