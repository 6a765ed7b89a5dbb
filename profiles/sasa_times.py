"""Times of pw_sasa for DESIGN.md ("Accessible surface"): writes profiles/sasa_times.json.

    python profiles/sasa_times.py [--out profiles/sasa_times.json]    # needs a gfx950 device
    python profiles/sasa_times.py --case cc3-1000 --once              # one call (for a kernel trace)

The case runs in a process of its own under a time limit.  1000 synthetic CC3 frames (pywindow_amd.synth: the cage with
Gaussian noise of 0.05 A an atom) with their cavities (pw.cavity_grid_batch with masks: seeded at the optimised pore
centre, closed at planes through the four windows, 46^3 .. 48^3 voxels), all frames in ONE pw.surface_area_batch call at
points = 960 and probe 0.  Two warm-up calls, median of 7 (3 for the host path) with the smallest and the largest.
kernel ms: HIP events around the kernel (the library's measurement hook); call ms: perf_counter around
pw.surface_area_batch on device 0 from and into pageable host arrays -- the directions, the job records, the finiteness
scan on the host and the copies included; host path: the same call on the device = -1 context with 16 threads; cavity
kernel ms: pw_cavity's device time on the same frames with masks, for comparison.
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

#: name -> (frames, time limit of the case in seconds)
CASES = {"cc3-1000": (1000, 420)}
POINTS = 960


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
    import pywindow_amd as pw
    from pywindow_amd import _lib, engine, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    recs = engine.analyse([(elements, f) for f in frames], device=0)
    radii = VDW[element_ids(elements)]
    planes = [None if engine.windows_of(r) is None else window_planes(r["pore_opt_c"], engine.windows_of(r)[1]) for r in recs]
    cavity_ms = []
    kw = dict(probe=0.0, spacing=0.5, half_widths=recs["maxd"] / 2.0, planes=planes, mask=True)
    cav = pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], device=0, **kw)
    if once:
        s = pw.surface_area_batch(frames, radii, points=POINTS, cavity=cav, device=0)
        print("one call:", s.raw["exposed"][:5].tolist(), s.raw["inside"][:5].tolist())
        return
    kernel = []
    for k in range(9):
        ms = []
        got = pw.surface_area_batch(frames, radii, points=POINTS, cavity=cav, device=0, kernel_ms=ms)
        if k >= 2:
            kernel.append(ms[0])
    call = median_of(lambda: pw.surface_area_batch(frames, radii, points=POINTS, cavity=cav, device=0), 7)
    _lib.load().pw_context_host_threads(engine.context(-1)._h, 16)
    host = median_of(lambda: pw.surface_area_batch(frames, radii, points=POINTS, cavity=cav, device=-1), 3, warm=1)
    ref = pw.surface_area_batch(frames, radii, points=POINTS, cavity=cav, device=-1)
    same = got.raw.tobytes() == ref.raw.tobytes() and got.exposed.tobytes() == ref.exposed.tobytes() and \
        got.inside.tobytes() == ref.inside.tobytes()
    # pw_cavity's device time on the same frames, through its own measurement hook
    import _cavity_cases as C
    jobs = []
    for f, r, p in zip(frames, recs, planes):
        g = 2 * int(np.ceil(float(r["maxd"]) / 2.0 / 0.5))
        jobs.append(C.Case("frame", (g, g, g), (g // 2 - 1,) * 3, f, radii, 0.0, r["pore_opt_c"] - 0.5 * (g // 2 - 0.5), 0.5, p))
    packed = C.pack(jobs, mask=True)
    for k in range(9):
        rc, _, ms = C.raw(engine.context(0), packed, workspace_bytes=0, timed=True)
        assert rc == 0
        if k >= 2:
            cavity_ms.append(ms)
    tests = n_frames * len(elements) * POINTS
    result = {
        "case": name, "frames": n_frames, "atoms": len(elements), "points": POINTS, "probe": 0.0,
        "grids": sorted({int(s[0]) for s in cav.shape}), "repeats": 7, "host_repeats": 3,
        "kernel_ms_median": float(np.median(kernel)), "kernel_ms_min": float(min(kernel)), "kernel_ms_max": float(max(kernel)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "host_path_16_threads_ms_median": host[0], "host_path_16_threads_ms_min": host[1], "host_path_16_threads_ms_max": host[2],
        "host_over_call": host[0] / call[0], "device_equals_host": bool(same),
        "cavity_kernel_ms_median": float(np.median(cavity_ms)), "cavity_kernel_ms_min": float(min(cavity_ms)),
        "cavity_kernel_ms_max": float(max(cavity_ms)),
        "test_points": tests, "test_points_per_second_kernel": tests / (float(np.median(kernel)) * 1e-3),
        "exposed_median": float(np.median(got.raw["exposed"])), "inside_median": float(np.median(got.raw["inside"])),
        "area_median": float(np.median(got.area)), "internal_area_median": float(np.median(got.internal_area)),
        "closed_frames": int(np.count_nonzero(got.closed)),
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sasa_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.case:
        sys.path.insert(0, str(ROOT / "tests"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/sasa_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
