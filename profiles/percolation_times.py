"""Times of pw_percolation for DESIGN.md ("Guest percolation"): writes profiles/percolation_times.json.

    python profiles/percolation_times.py [--out profiles/percolation_times.json]    # needs a gfx950 device
    python profiles/percolation_times.py --case cc3-cell-1000 --frames 100 --quick  # fewer frames, 3 repeats, no host path

The case runs in a process of its own under a time limit.  The workload is the periodic trajectory that
profiles/channels_times.py times: 1000 frames of the 1344-atom CC3 cell of tests/golden/rebuild.npz with Gaussian noise
of 0.02 A an atom (frame k from default_rng(4 + k)), Xe at spacing 0.5 and cutoff 12, all in ONE pw_percolation call.  Two
warm-up calls, median of 7.  device ms: HIP events around the launches of a call (the library's measurement hook);
levels ms: the same call with the maps of the first call as the caller's fields (their upload included), so field =
device - levels; public ms: perf_counter around pywindow_amd.guest_percolation_batch, the images and the plan included;
host path: the public call on a device = -1 context with 16 threads, once, and its bytes against the device's;
pw_channels (probe 1.2) on the same frames in the same run, for scale."""
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


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def run_case(name, quick, n_frames):
    import pywindow_amd as pw
    from pywindow_amd import engine
    from pywindow_amd import percolation as PC

    n_frames = n_frames or CASES[name][0]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    frames = np.stack([base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape) for k in range(n_frames)])
    kw = dict(guest="Xe", spacing=0.5, cutoff=12.0)
    repeats, warm = (3, 1) if quick else (7, 2)
    ctx = engine.context(0)
    jobs, atoms, coef, *_ = PC.plan_jobs(frames, elements, lattice, maps=True, **kw)
    ms, diagnostics = [], []
    for _ in range(warm + repeats):
        levels, out, maps = ctx.percolation(jobs, atoms, coef, kernel_ms=ms, diagnostics=diagnostics)
    device = spread(ms[warm:])
    n_eval, n_fill = diagnostics[-1]
    # the levels alone: the same jobs with the maps of the first call as the caller's fields
    given = jobs.copy()
    given["field_first"], given["map_first"] = jobs["map_first"], -1
    alone = []
    for _ in range(warm + repeats):
        again = ctx.percolation(given, field=maps, kernel_ms=alone)
    alone = spread(alone[warm:])
    got = pw.guest_percolation_batch(frames, elements, lattice, device=0, **kw)
    act = np.asarray(got.activation)
    ok = np.isfinite(act[:, 2])
    voxels = int(np.prod(got.shape[0]))
    result = {"case": name, "frames": n_frames, "atoms": int(len(elements)), "atoms_with_images_per_frame": int(len(atoms) // n_frames),
              "grid": [int(v) for v in got.shape[0]], "guest": "Xe", "spacing": 0.5, "cutoff": 12.0, "repeats": repeats,
              "warm_ups": warm, "device_ms": device, "levels_alone_ms": alone,
              "field_ms_by_difference": device["median"] - alone["median"],
              "levels_alone_equal_the_call": bool(again[0].tobytes() == levels.tobytes() and again[1].tobytes() == out.tobytes()),
              "pair_terms_per_s": n_frames * voxels * (len(atoms) / n_frames) / max((device["median"] - alone["median"]) * 1e-3, 1e-9),
              "n_evaluations_per_job": spread(n_eval), "n_fills_per_job": spread(n_fill),
              "frames_connected_in_3d": int(ok.sum()),
              "barrier_3d_kJ_per_mol": spread(np.asarray(got.barrier)[ok, 2]) if ok.any() else None,
              "activation_3d_kJ_per_mol": dict(spread(act[ok, 2]), mean=float(act[ok, 2].mean()), std=float(act[ok, 2].std()),
                                               quartiles=[float(q) for q in np.percentile(act[ok, 2], (25, 75))]) if ok.any() else None}
    chan = []
    for _ in range(warm + repeats):
        pw.channel_network_batch(frames, elements, lattice, probe=1.2, spacing=0.5, device=0, kernel_ms=chan)
    result["pw_channels_device_ms_same_frames"] = spread(chan[warm:])
    if not quick:
        times = []
        for _ in range(2 + 7):
            t0 = time.perf_counter()
            pw.guest_percolation_batch(frames, elements, lattice, device=0, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
        result["public_ms"] = spread(times[2:])
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
        t0 = time.perf_counter()
        ref = pw.guest_percolation_batch(frames, elements, lattice, device=-1, **kw)
        result["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        result["device_equals_host"] = bool(got.levels.tobytes() == ref.levels.tobytes() and got.raw.tobytes() == ref.raw.tobytes())
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "percolation_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/percolation_times.py" + (f" --frames {args.frames}" if args.frames else "") +
            (" --quick" if args.quick else ""), "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
