"""Times of pw_cavity for DESIGN.md ("Cavity volume and shape"): writes profiles/cavity_times.json.

    python profiles/cavity_times.py [--out profiles/cavity_times.json]    # needs a gfx950 device
    python profiles/cavity_times.py --case cc3-1000 --once                # one call (for a kernel trace)

The case runs in a process of its own under a time limit.  1000 synthetic CC3 frames (pywindow_amd.synth: the cage with
Gaussian noise of 0.05 A an atom), each seeded at its optimised pore centre in a box of half its maximum diameter at
spacing 0.5 A (a 46^3 grid) and closed at planes through its own four windows, all frames in ONE pw_cavity call, without
masks and with them.  Two warm-up calls, median of 7 (3 for the host path).  device ms: HIP events from the first
launch of a call to its last (the library's measurement hook); call ms: perf_counter around the C call from and into
pageable host arrays, the finiteness scan on the host and the copies included; host path: the same call on a
device = -1 context with 16 threads; analysis ms: the full analysis of the same 1000 frames on the device (Context.analyse
after a warm-up), which is where the centres, windows and diameters the cavity needs come from.
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

#: name -> (frames, time limit of the case in seconds)
CASES = {"cc3-1000": (1000, 420)}


def median_of(f, repeats, warm=2):
    for _ in range(warm):
        f()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def run_case(name, once):
    import _cavity_cases as C
    from pywindow_amd import _lib, engine, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)]
    units = [(elements, f) for f in frames]
    dev = engine.context(0)
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    engine.analyse(units, device=0)
    analysis = median_of(lambda: engine.analyse(units, device=0), 3, warm=0)
    recs = engine.analyse(units, device=0)
    radii = VDW[element_ids(elements)]
    jobs = []
    for f, r in zip(frames, recs):
        win = engine.windows_of(r)
        g = 2 * int(np.ceil(float(r["maxd"]) / 2.0 / 0.5))
        jobs.append(C.Case("frame", (g, g, g), (g // 2 - 1,) * 3, f, radii, 0.0, r["pore_opt_c"] - 0.5 * (g // 2 - 0.5), 0.5,
                           None if win is None else window_planes(r["pore_opt_c"], win[1])))
    grids = sorted({c.dims[0] for c in jobs})
    result = {"case": name, "frames": n_frames, "atoms": len(elements), "grids": grids, "spacing": 0.5, "probe": 0.0,
              "analysis_ms_median": analysis[0], "analysis_ms_min": analysis[1], "analysis_ms_max": analysis[2],
              "analysis_repeats": 3, "repeats": 7, "host_repeats": 3}
    host = _lib.Context(-1, host_threads=16)
    for mask in (False, True):
        packed = C.pack(jobs, mask=mask)
        if once:
            rc, out = C.raw(dev, packed)
            print("one call:", rc, out[0]["n_voxels"][:5].tolist())
            return
        device = []
        for k in range(9):
            rc, got, ms = C.raw(dev, packed, workspace_bytes=0, timed=True)
            assert rc == 0
            if k >= 2:
                device.append(ms)
        call = median_of(lambda: C.raw(dev, packed), 7)
        host_ms = median_of(lambda: C.raw(host, packed), 3, warm=1)
        same = C.same(got, C.raw(host, packed)[1])
        key = "with_masks" if mask else "without_masks"
        result[key] = {
            "device_ms_median": float(np.median(device)), "device_ms_min": float(min(device)), "device_ms_max": float(max(device)),
            "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
            "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
            "host_path_16_threads_ms_max": host_ms[2], "device_equals_host": bool(same),
            "host_over_call": host_ms[0] / call[0], "analysis_over_call": analysis[0] / call[0],
        }
        result["closed_frames"] = int((got[0]["n_face"] == 0).sum())
        result["voxels_median"] = float(np.median(got[0]["n_voxels"]))
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cavity_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.once)
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
    meta = {"commit_parent": head or None, "command": "python profiles/cavity_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
