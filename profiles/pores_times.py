"""Times of pw_pore_sizes for DESIGN.md ("Pore sizes"): writes profiles/pores_times.json.

    python profiles/pores_times.py [--out profiles/pores_times.json]    # needs a gfx950 device
    python profiles/pores_times.py --case cc3-1000 --once               # one call (for a kernel trace)

The case runs in a process of its own under a time limit.  The workload is that of profiles/cavity_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each seeded at its optimised
pore centre in a box of half its maximum diameter at spacing 0.5 A (a 46^3 grid) and closed at planes through its own
four windows -- here with a ladder of 12 probes, 0 .. 2.75 A in steps of 0.25, all frames in ONE pw_pore_sizes call
without masks.  Two warm-up calls, median of 7 (3 for the host path).  device ms: HIP events from the first launch of
a call to its last (the library's measurement hook); public ms: perf_counter around
pywindow_amd.pore_size_distribution_batch from and into host arrays; host path: the C call on a device = -1 context
with 16 threads; cavity floor: in the same run, the sum of the device ms of 12 pw_cavity calls without masks on the
same frames, one a probe of the ladder -- what the levels' classification and fill cost without any sweep.
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
PROBES = 0.25 * np.arange(12)


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
    import _pores_cases as P
    import pywindow_amd as pw
    from pywindow_amd import _lib, engine, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = [synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)]
    units = [(elements, f) for f in frames]
    dev = engine.context(0)
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    recs = engine.analyse(units, device=0)
    radii = VDW[element_ids(elements)]
    jobs, planes = [], []
    for f, r in zip(frames, recs):
        win = engine.windows_of(r)
        g = 2 * int(np.ceil(float(r["maxd"]) / 2.0 / 0.5))
        planes.append(None if win is None else window_planes(r["pore_opt_c"], win[1]))
        jobs.append(P.Case("frame", (g, g, g), (g // 2 - 1,) * 3, PROBES, 0.5, r["pore_opt_c"] - 0.5 * (g // 2 - 0.5), f, radii, planes[-1]))
    packed = P.Packed(jobs, masks=False)
    if once:
        rc, got = P.raw(dev, packed)
        print("one call:", rc, got[0]["n_swept"][:12].tolist())
        return
    host = _lib.Context(-1, host_threads=16)
    device = []
    for k in range(9):
        rc, got, ms = P.raw(dev, packed, workspace_bytes=0, timed=True)
        assert rc == 0
        if k >= 2:
            device.append(ms)
    call = median_of(lambda: P.raw(dev, packed), 7)
    stacked = np.stack(frames)
    kw = dict(probes=PROBES, spacing=0.5, half_widths=recs["maxd"] / 2.0, planes=planes)
    public = median_of(lambda: pw.pore_size_distribution_batch(stacked, radii, recs["pore_opt_c"], device=0, **kw), 7)
    host_ms = median_of(lambda: P.raw(host, packed), 3, warm=1)
    same = P.same(got, P.raw(host, packed)[1])
    # the floor: 12 pw_cavity calls without masks on the same frames, one a level
    floor = []
    for k in range(9):
        total = 0.0
        for q in range(len(PROBES)):
            rc, _, ms = C.raw(dev, C.pack([c.level(q) for c in jobs], mask=False), workspace_bytes=0, timed=True)
            assert rc == 0
            total += ms
        if k >= 2:
            floor.append(total)
    levels = got[0].reshape(n_frames, len(PROBES))
    result = {
        "case": name, "frames": n_frames, "atoms": len(elements), "grids": sorted({c.dims[0] for c in jobs}), "spacing": 0.5,
        "probes": PROBES.tolist(), "k2": levels["k2"][0].tolist(), "repeats": 7, "host_repeats": 3,
        "device_ms_median": float(np.median(device)), "device_ms_min": float(min(device)), "device_ms_max": float(max(device)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "public_ms_median": public[0], "public_ms_min": public[1], "public_ms_max": public[2],
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "device_equals_host": bool(same),
        "cavity_12_calls_device_ms_median": float(np.median(floor)), "cavity_12_calls_device_ms_min": float(min(floor)),
        "cavity_12_calls_device_ms_max": float(max(floor)),
        "device_over_cavity_floor": float(np.median(device) / np.median(floor)), "host_over_call": host_ms[0] / call[0],
        "closed_frames": int(((levels["n_face"][:, 0] == 0) & (levels["flags"][:, 0] == 0)).sum()),
        "levels_with_a_reach_median": float(np.median((levels["n_reach"] > 0).sum(axis=1))),
        "swept_voxels_median": np.median(levels["n_swept"], axis=0).tolist(),
        "largest_voxels_median": np.median(levels["n_largest"], axis=0).tolist(),
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pores_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/pores_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
