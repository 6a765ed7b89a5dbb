"""Times of pw_channels for DESIGN.md ("Crystal pore networks"): writes profiles/channels_times.json.

    python profiles/channels_times.py [--out profiles/channels_times.json]    # needs a gfx950 device
    python profiles/channels_times.py --case cc3-cell-1000 --quick            # device times only, 3 repeats

The case runs in a process of its own under a time limit.  The workload is the periodic trajectory the README times:
1000 frames of the 1344-atom CC3 cell of tests/golden/rebuild.npz with Gaussian noise of 0.02 A an atom (frame k from
default_rng(4 + k), as tests/test_gpu_scale.py), at spacing 0.5 and probe 1.2, all in ONE pw_channels call.  Two warm-up
calls, median of 7.  device ms: HIP events around the launches of a call (the library's measurement hook); fills ms: the
same call with ready-made open words (those of the first call, from its labels), so classification = device - fills;
public ms: perf_counter around pywindow_amd.channel_network_batch, the images and the plan included; host path: the
public call on a device = -1 context with 16 threads, once, and its bytes against the device's.  For context the same
frames as a HISTORY file through DLPOLY.analysis(modular=True, rebuild=True), once after one warm-up."""
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
CASES = {"cc3-cell-1000": (1000, 560)}


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def run_case(name, quick):
    import pywindow_amd as pw
    from pywindow_amd import channels as CN
    from pywindow_amd import engine, synth

    n_frames, _ = CASES[name]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    frames = np.stack([base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape) for k in range(n_frames)])
    kw = dict(probe=1.2, spacing=0.5, c_max=64)
    repeats, warm = (3, 1) if quick else (7, 2)
    ms = []
    got = None
    for _ in range(warm + repeats):
        got = pw.channel_network_batch(frames, elements, lattice, device=0, kernel_ms=ms, **kw)
    device = spread(ms[warm:])
    # the fills alone: the same jobs with the open words the first call found
    jobs, atoms, reach, *_ = CN.plan_jobs(frames, elements, lattice, labels=True, **kw)
    ctx = engine.context(0)
    labels = ctx.channels(jobs, atoms, reach)[3].reshape(n_frames, 50, 50, 50)
    words = ((labels != 255).astype(np.uint64) << np.arange(50, dtype=np.uint64)).sum(axis=3, dtype=np.uint64).reshape(-1)
    jobs["label_first"] = -1
    first = np.arange(n_frames, dtype=np.int64) * 2500
    fills, given = [], None
    for _ in range(warm + repeats):
        given = ctx.channels(jobs, atoms, reach, open_words=words, open_first=first, kernel_ms=fills)
    fills = spread(fills[warm:])
    raw = got.raw[:, 0]
    result = {"case": name, "frames": n_frames, "atoms": int(len(elements)), "atoms_with_images_per_frame": int(len(reach) // n_frames),
              "grid": [50, 50, 50], "probe": 1.2, "spacing": 0.5, "repeats": repeats, "warm_ups": warm, "device_ms": device,
              "fills_alone_ms": fills, "classification_ms_by_difference": device["median"] - fills["median"],
              "fills_alone_equal_the_call": bool(given[0].tobytes() == got.raw.tobytes()),
              "components_per_frame": {"min": int(raw["n_components"].min()), "median": float(np.median(raw["n_components"])),
                                       "max": int(raw["n_components"].max())},
              "frames_with_a_3d_network": int((np.asarray(got.dimensionality)[:, 0] == 3).sum()),
              "accessible_volume_A3": spread(np.asarray(got.accessible_volume)[:, 0]),
              "voxels_per_s": n_frames * 125000 / (device["median"] * 1e-3)}
    if not quick:
        times = []
        for _ in range(2 + 7):
            t0 = time.perf_counter()
            pw.channel_network_batch(frames, elements, lattice, device=0, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
        result["public_ms"] = spread(times[2:])
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
        t0 = time.perf_counter()
        ref = pw.channel_network_batch(frames, elements, lattice, device=-1, **kw)
        result["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        result["device_equals_host"] = bool(got.raw.tobytes() == ref.raw.tobytes() and got.components.tobytes() == ref.components.tobytes())
        with tempfile.TemporaryDirectory() as tmp:
            path = synth.write_history(pathlib.Path(tmp) / "HISTORY", elements, list(frames), cell=np.asarray(lattice, float).T)
            wall = []
            for _ in range(2):
                traj = pw.DLPOLY(path)
                t0 = time.perf_counter()
                traj.analysis(modular=True, rebuild=True)
                wall.append((time.perf_counter() - t0) * 1e3)
            result["analysis_modular_rebuild_ms"] = wall[1]
            t0 = time.perf_counter()
            through = pw.DLPOLY(path).channels(probe=1.2, device=0)
            result["dlpoly_channels_ms_reading_included"] = (time.perf_counter() - t0) * 1e3
            result["dlpoly_frames_with_a_3d_network"] = int((np.asarray(through.dimensionality)[:, 0] == 3).sum())
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "channels_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/channels_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
