"""Times of pw_affinity for DESIGN.md ("Guest affinity"): writes profiles/affinity_times.json.

    python profiles/affinity_times.py [--out profiles/affinity_times.json]    # needs a gfx950 device
    python profiles/affinity_times.py --case cc3-1000 --once                  # one call (for a kernel trace)

The case runs in a process of its own under a time limit.  The workload is that of profiles/cavity_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each seeded at its optimised
pore centre in a box of half its maximum diameter at spacing 0.5 A (a 46^3 grid) and closed at planes through its own
four windows.  Xe at 298 K over the probe-0 cavities of all frames in ONE pw_affinity call (core2 = 0.25, no cutoff, no
histogram, no energy map).  Two warm-up calls, median of 7 (3 for the host path).  device ms: HIP events from the first
launch of a call to its last (the library's measurement hook); call ms: perf_counter around Context.affinity (ctypes,
from and into host arrays, job records ready); public ms: around pywindow_amd.guest_affinity_batch; host path: the
public call on a device = -1 context with 16 threads; cavity: in the same run, the pw_cavity call with masks that makes
the regions -- device ms, call ms and public ms (pywindow_amd.cavity_grid_batch) in the same senses; full
box: the same frames over every voxel of their boxes (word_first = -1), where the kernel is compute-bound -- pairs
(voxel, atom) a second, and the share of the 78.6 TF/s FP64 vector peak at FLOPS_PER_PAIR operations a pair (the
division counted as one, as an algorithm's operations are; the hardware expands it to about a dozen).
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
#: 3 differences, r2 (3 products, 2 sums), 1 division, s (2 products), u (2 products, 1 difference), 1 sum
FLOPS_PER_PAIR = 15
FP64_PEAK = 78.6e12


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
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    units = [(elements, f) for f in frames]
    dev = engine.context(0)
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    recs = engine.analyse(units, device=0)
    radii = VDW[element_ids(elements)]
    planes = []
    for r in recs:
        win = engine.windows_of(r)
        planes.append(None if win is None else window_planes(r["pore_opt_c"], win[1]))
    kw = dict(probe=0.0, spacing=0.5, half_widths=recs["maxd"] / 2.0, planes=planes, mask=True)
    cav = pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], device=0, **kw)
    coef = affinity.lj_coefficients(elements, "Xe")
    masked = lambda device, ms=None: pw.guest_affinity_batch(frames, coef, "Xe", [298.0], cavity=cav, device=device, kernel_ms=ms)
    if once:
        af = masked(0)
        print("one call:", af.boltzmann_volume[:4, 0].tolist())
        return
    got = masked(0)
    same = got.raw.tobytes() == masked(-1).raw.tobytes() and got.levels.tobytes() == masked(-1).levels.tobytes()
    # the same call on the context, from ready job records
    aj = np.zeros(n_frames, dtype=pw._lib.AFFINITY_JOB_DTYPE)
    rows = (cav.shape[:, 1] * cav.shape[:, 2]).astype(np.int64)
    aj["atom_first"], aj["n"], aj["n_betas"] = np.arange(n_frames) * len(elements), len(elements), 1
    aj["word_first"] = np.concatenate([[0], np.cumsum(rows)[:-1]])
    aj["beta_first"], aj["level_first"], aj["out"], aj["energy_first"] = 0, np.arange(n_frames), np.arange(n_frames), -1
    aj["origin"], aj["spacing"], aj["core2"] = cav.origin, 0.5, 0.25
    aj["nx"], aj["ny"], aj["nz"] = cav.shape[:, 0], cav.shape[:, 1], cav.shape[:, 2]
    region = np.concatenate(cav.words)
    raw_call = lambda ms=None: dev.affinity(aj, frames.reshape(-1, 3), coef, [1.0 / (affinity.R * 298.0)], region, kernel_ms=ms)
    assert raw_call()[0].tobytes() == got.raw.tobytes() and raw_call()[1].tobytes() == got.levels.tobytes()
    device = device_ms_of(lambda ms: raw_call(ms))
    call = median_of(raw_call, 7)
    public = median_of(lambda: masked(0), 7)
    host_ctx_threads = pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16)   # (sets, then reports)
    host_ms = median_of(lambda: masked(-1), 3, warm=1)
    # the pw_cavity call that makes the regions, in the same run
    jobs = np.zeros(n_frames, dtype=pw._lib.CAVITY_JOB_DTYPE)
    cuts, at, words = [], 0, 0
    for t in range(n_frames):
        g = int(cav.shape[t][0])
        p = np.zeros((0, 4)) if planes[t] is None else planes[t]
        jobs[t] = (t * len(elements), len(elements), 0, at, len(p), words, t, cav.origin[t], 0.5, 0.0, g, g, g, (g // 2 - 1,) * 3)
        cuts.append(p)
        at += len(p)
        words += g * g
    cuts = np.concatenate(cuts)
    cavity_call = lambda ms=None: dev.cavity(jobs, frames.reshape(-1, 3), radii, cuts, kernel_ms=ms)
    assert cavity_call()[0].tobytes() == cav.raw.tobytes()
    cavity_device = device_ms_of(lambda ms: cavity_call(ms))
    cavity_ms = median_of(cavity_call, 7)
    cavity_public = median_of(lambda: pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], device=0, **kw), 7)
    # the full boxes: compute-bound
    shape = cav.shape[0]
    same_grid = (cav.shape == shape).all(axis=1)
    full = lambda ms=None: pw.guest_affinity_batch(frames[same_grid], coef, "Xe", [298.0], grid=(cav.origin[same_grid], 0.5, shape),
                                                   device=0, kernel_ms=ms)
    full_device = device_ms_of(lambda ms: full(ms), repeats=5, warm=1)
    pairs = float(same_grid.sum()) * float(np.prod(shape)) * len(elements)
    masked_pairs = float(cav.n_voxels.sum()) * len(elements)
    result = {
        "case": name, "frames": n_frames, "atoms": len(elements), "grids": sorted({int(s[0]) for s in cav.shape}), "spacing": 0.5,
        "guest": "Xe", "temperature": 298.0, "repeats": 7, "host_repeats": 3, "host_threads": int(host_ctx_threads),
        "voxels_median": float(np.median(cav.n_voxels)), "chunks_total": int(((cav.n_voxels + 63) // 64).sum()),
        "device_ms_median": device[0], "device_ms_min": device[1], "device_ms_max": device[2],
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "public_ms_median": public[0], "public_ms_min": public[1], "public_ms_max": public[2],
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "device_equals_host": bool(same), "host_over_public": host_ms[0] / public[0],
        "cavity_device_ms_median": cavity_device[0], "cavity_device_ms_min": cavity_device[1], "cavity_device_ms_max": cavity_device[2],
        "cavity_call_ms_median": cavity_ms[0], "cavity_call_ms_min": cavity_ms[1], "cavity_call_ms_max": cavity_ms[2],
        "cavity_public_ms_median": cavity_public[0], "cavity_public_ms_min": cavity_public[1], "cavity_public_ms_max": cavity_public[2],
        "public_over_cavity_public": public[0] / cavity_public[0],
        "device_over_cavity_device": device[0] / cavity_device[0], "call_over_cavity_call": call[0] / cavity_ms[0],
        "masked_pairs": masked_pairs, "masked_pairs_per_s": masked_pairs / (device[0] * 1e-3),
        "full_box_frames": int(same_grid.sum()), "full_box_pairs": pairs,
        "full_box_device_ms_median": full_device[0], "full_box_device_ms_min": full_device[1], "full_box_device_ms_max": full_device[2],
        "full_box_pairs_per_s": pairs / (full_device[0] * 1e-3), "flops_per_pair": FLOPS_PER_PAIR,
        "full_box_share_of_fp64_vector_peak": pairs * FLOPS_PER_PAIR / (full_device[0] * 1e-3) / FP64_PEAK,
        "closed_frames": int(np.asarray(got.closed).sum()), "clamped_frames": int(np.asarray(got.clamped).sum()),
        "boltzmann_volume_median": float(np.median(got.boltzmann_volume[:, 0])), "heat_median": float(np.median(got.heat[:, 0])),
        "min_energy_median": float(np.median(got.min_energy)),
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "affinity_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/affinity_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
