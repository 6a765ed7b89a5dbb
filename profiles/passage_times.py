"""Times of pw_passage for DESIGN.md ("Guest passage"): writes profiles/passage_times.json.

    python profiles/passage_times.py [--out profiles/passage_times.json]    # needs a gfx950 device
    python profiles/passage_times.py --case cc3-1000 --once                 # one call (for a kernel trace)

The case runs in a process of its own under a time limit.  The workload is that of profiles/cavity_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each seeded at its optimised
pore centre in a box of half its maximum diameter at spacing 0.5 A (a 46^3 grid) with planes through its own four
windows.  Xe over the full boxes of all frames in ONE pw_passage call (core2 = 0.25, no cutoff): four rows a frame.
Two warm-up calls, median of 7 (1 and 3 for the host path).  device ms: HIP events from the first launch of a call to
its last (the library's measurement hook); call ms: perf_counter around Context.passage (ctypes, from and into host
arrays, job records ready); public ms: around pywindow_amd.guest_passage_batch; host path: the public call on a
device = -1 context with 16 threads; field: in the same run, pw_affinity over the full boxes of the same frames
(word_first = -1, no energy map) -- the same pair terms as the field kernel, its share of the device time; fills: the
flood fills a row took (the measurement hook's count); three / four grids: the device time of the same call with the
passage kernel that has no fourth bit grid and with the one that has, alternated in this process, 2 warm-up rounds and 7.
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


def median_of(f, repeats, warm=2):
    for _ in range(warm):
        f()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


def device_ms_of(f, repeats=7, warm=2):
    """f(list) appends the device time of one call to the list."""
    ms = []
    for _ in range(warm + repeats):
        f(ms)
    ms = ms[warm:]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def run_case(name, once):
    import pywindow_amd as pw
    from pywindow_amd import affinity, engine, synth
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    units = [(elements, f) for f in frames]
    dev = engine.context(0)
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    recs = engine.analyse(units, device=0)
    planes = []
    for r in recs:
        win = engine.windows_of(r)
        planes.append(None if win is None else window_planes(r["pore_opt_c"], win[1]))
    coef = affinity.lj_coefficients(elements, "Xe")
    kw = dict(planes=planes, spacing=0.5, half_widths=recs["maxd"] / 2.0)
    public_call = lambda device, ms=None, fills=None: pw.guest_passage_batch(frames, coef, "Xe", recs["pore_opt_c"], device=device,
                                                                              kernel_ms=ms, fills=fills, **kw)
    if once:
        print("one call:", public_call(0).barrier[:2].tolist())
        return
    fills, host_fills = [], []
    got = public_call(0, fills=fills)
    host_ctx_threads = pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16)   # (sets, then reports)
    same = got.raw.tobytes() == public_call(-1, fills=host_fills).raw.tobytes()
    # the same call on the context, from ready job records
    jobs = np.zeros(n_frames, dtype=pw._lib.PASSAGE_JOB_DTYPE)
    cuts, at, rows = [], 0, 0
    for t in range(n_frames):
        g = int(got.shape[t][0])
        p = np.zeros((0, 4)) if planes[t] is None else planes[t]
        jobs[t] = (t * len(elements), len(elements), 0, at, len(p), -1, rows, got.origin[t], 0.5, 0.25, 0.0, g, g, g, (g // 2 - 1,) * 3)
        cuts.append(p)
        at += len(p)
        rows += max(len(p), 1)
    cuts = np.concatenate(cuts)
    raw_call = lambda ms=None, grids=None: dev.passage(jobs, frames.reshape(-1, 3), coef, cuts, kernel_ms=ms, grids=grids)
    first = raw_call()
    assert all(first[int(j["out_first"]):int(j["out_first"]) + max(int(j["m"]), 1)].tobytes() == got.raw[t, :max(int(j["m"]), 1)].tobytes()
               for t, j in enumerate(jobs))
    device = device_ms_of(lambda ms: raw_call(ms))
    # what the fourth bit grid buys: the kernel without it and with it, turn and turn about in this process
    assert raw_call(grids=3).tobytes() == first.tobytes()
    three, four = [], []
    for _ in range(2 + 7):
        raw_call(three, 3)
        raw_call(four, 4)
    three, four = three[2:], four[2:]
    call = median_of(raw_call, 7)
    public = median_of(lambda: public_call(0), 7)
    host_ms = median_of(lambda: public_call(-1), 3, warm=1)
    # the field kernel's share: pw_affinity over the full boxes of the same frames
    shape = got.shape[0]
    same_grid = (got.shape == shape).all(axis=1)
    full = lambda ms=None: pw.guest_affinity_batch(frames[same_grid], coef, "Xe", [298.0], grid=(got.origin[same_grid], 0.5, shape),
                                                   device=0, kernel_ms=ms)
    field_device = device_ms_of(lambda ms: full(ms), repeats=5, warm=1)
    valid = (got.raw["flags"] == 0) & ~got.padding
    act = got.activation[valid]
    result = {
        "case": name, "frames": n_frames, "atoms": len(elements), "grids": sorted({int(s[0]) for s in got.shape}), "spacing": 0.5,
        "guest": "Xe", "rows": int(rows), "repeats": 7, "host_repeats": 3, "host_threads": int(host_ctx_threads),
        "device_ms_median": device[0], "device_ms_min": device[1], "device_ms_max": device[2],
        "three_grids_device_ms_median": float(np.median(three)), "three_grids_device_ms_min": float(min(three)),
        "three_grids_device_ms_max": float(max(three)), "four_grids_device_ms_median": float(np.median(four)),
        "four_grids_device_ms_min": float(min(four)), "four_grids_device_ms_max": float(max(four)),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "public_ms_median": public[0], "public_ms_min": public[1], "public_ms_max": public[2],
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "device_equals_host": bool(same), "host_over_public": host_ms[0] / public[0],
        "field_frames": int(same_grid.sum()),
        "field_device_ms_median": field_device[0], "field_device_ms_min": field_device[1], "field_device_ms_max": field_device[2],
        "field_share_of_device": field_device[0] * (n_frames / float(same_grid.sum())) / device[0],
        "fills_per_row_median": float(np.median(fills[0])), "fills_per_row_min": int(fills[0].min()),
        "fills_per_row_max": int(fills[0].max()), "fills_total": int(fills[0].sum()),
        "host_fills_equal_device_fills": bool(np.array_equal(fills[0], host_fills[0])),
        "rows_valid": int(valid.sum()), "rows_free_exit": int((got.free_exit & valid).sum()),
        "rows_no_exit": int(got.no_exit.sum()), "rows_seed_closed": int(got.seed_closed.sum()),
        "barrier_median": float(np.median(got.barrier[valid])), "well_median": float(np.median(got.well[valid])),
        "activation_median": float(np.median(act)), "activation_min": float(act.min()), "activation_max": float(act.max()),
        "activation_of_the_easiest_window_median": float(np.median(got.series("activation")[0])),
        "n_basin_median": float(np.median(got.n_basin[valid])),
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "passage_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/passage_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
