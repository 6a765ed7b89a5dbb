"""Times of pw_basins for DESIGN.md ("Crystal diffusion"): writes profiles/basins_times.json.

    python profiles/basins_times.py [--out profiles/basins_times.json]              # needs a gfx950 device
    python profiles/basins_times.py --case cc3-cell-100 --frames 20 --quick         # fewer frames, 3 repeats, no host path

The case runs in a process of its own under a time limit.  The workload is the periodic trajectory that
profiles/percolation_times.py times, cut to 100 frames: the 1344-atom CC3 cell of tests/golden/rebuild.npz with Gaussian
noise of 0.02 A an atom (frame k from default_rng(4 + k)), Xe at spacing 0.5 and cutoff 12, two temperatures, all in ONE
pw_basins call.  Two warm-up calls, median of 7 with min and max.  device ms: HIP events around the launches of a call (the
library's measurement hook); basins ms: the same call with the maps of the first call as the caller's fields (their
upload included), so field = device - basins; public ms: perf_counter around pywindow_amd.guest_diffusion_batch, the
images, the plan and the numpy layer included; host path: the public call on a device = -1 context with 16 threads,
once, and its bytes against the device's; pw_percolation on the same frames in the same run, for scale.  Also the
coefficient of the undisturbed cell at merge = 0, 0.5, 1 and 2 RT (limit (2))."""
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
CASES = {"cc3-cell-100": (100, 900)}
TEMPERATURES = [250.0, 350.0]


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def run_case(name, quick, n_frames):
    import pywindow_amd as pw
    from pywindow_amd import diffusion as DF
    from pywindow_amd import engine
    from pywindow_amd import percolation as PC
    from pywindow_amd.affinity import R

    n_frames = n_frames or CASES[name][0]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    frames = np.stack([base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape) for k in range(n_frames)])
    kw = dict(guest="Xe", spacing=0.5, cutoff=12.0)
    repeats, warm = (3, 1) if quick else (7, 2)
    ctx = engine.context(0)
    perc_jobs, atoms, coef, *_ = PC.plan_jobs(frames, elements, lattice, maps=False, **kw)
    jobs = DF._basins_jobs(perc_jobs, np.array(TEMPERATURES), 100.0, True, False)
    ms, diagnostics = [], []
    for _ in range(warm + repeats):
        out, basins, edges, maps, _ = ctx.basins(jobs, atoms, coef, kernel_ms=ms, diagnostics=diagnostics)
    device = spread(ms[warm:])
    n_rounds, n_faces = diagnostics[-1]
    given = jobs.copy()
    given["field_first"], given["map_first"] = jobs["map_first"], -1
    alone = []
    for _ in range(warm + repeats):
        again = ctx.basins(given, field=maps, kernel_ms=alone)
    alone = spread(alone[warm:])
    perc = []
    for _ in range(warm + repeats):
        ctx.percolation(perc_jobs, atoms, coef, kernel_ms=perc)
    got = pw.guest_diffusion_batch(frames, elements, lattice, temperatures=TEMPERATURES, device=0, **kw)
    result = {"case": name, "frames": n_frames, "atoms": int(len(elements)), "grid": [int(v) for v in got.shape[0]], "guest": "Xe",
              "spacing": 0.5, "cutoff": 12.0, "temperatures": TEMPERATURES, "repeats": repeats, "warm_ups": warm, "device_ms": device,
              "basins_alone_ms": alone, "field_ms_by_difference": device["median"] - alone["median"],
              "basins_alone_equal_the_call": bool(all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (out, basins, edges)))),
              "pw_percolation_device_ms_same_frames": spread(perc[warm:]),
              "n_basins_per_job": spread(out["n_basins"]), "n_edges_per_job": spread(out["n_edges"]),
              "n_rounds_per_job": spread(n_rounds), "n_boundary_faces_per_job": spread(n_faces),
              "jobs_overflowed_first_capacities": int(((out["flags"] & 1) != 0).sum()), "n_sites_per_frame": spread(got.n_sites),
              "frames_valid": int(got.valid.sum()), "frames_barrierless": int(got.barrierless.sum()),
              "coefficient_A2_per_s": [spread(got.coefficient[:, l]) for l in range(len(TEMPERATURES))],
              "trapped_fraction": [spread(got.trapped_fraction[:, l]) for l in range(len(TEMPERATURES))]}
    table = {}
    for factor in (0.0, 0.5, 1.0, 2.0):
        one = pw.guest_diffusion(base, elements, lattice, temperatures=TEMPERATURES, merge=factor * R * min(TEMPERATURES), device=0, **kw)
        table[str(factor)] = {"n_sites": int(one.n_sites), "barrierless": bool(one.barrierless), "coefficient_A2_per_s": one.coefficient.tolist(),
                              "activation_energy_kJ_per_mol": float(one.activation_energy())}
    result["merge_in_RT_of_the_lowest_temperature"] = table
    if not quick:
        times = []
        for _ in range(2 + 7):
            t0 = time.perf_counter()
            pw.guest_diffusion_batch(frames, elements, lattice, temperatures=TEMPERATURES, device=0, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
        result["public_ms"] = spread(times[2:])
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
        t0 = time.perf_counter()
        ref = pw.guest_diffusion_batch(frames, elements, lattice, temperatures=TEMPERATURES, device=-1, **kw)
        result["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        result["device_equals_host"] = bool(got.tensor.tobytes() == ref.tensor.tobytes() and got.raw.tobytes() == ref.raw.tobytes())
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "basins_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.quick, args.frames)
        return
    results = []
    for name, spec in CASES.items():
        command = [sys.executable, __file__, "--case", name] + (["--frames", str(args.frames)] if args.frames else []) + \
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
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    meta = {"commit_parent": head or None, "command": "python profiles/basins_times.py" + (f" --frames {args.frames}" if args.frames else "") +
            (" --quick" if args.quick else ""), "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
