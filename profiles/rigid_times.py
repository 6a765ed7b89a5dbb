"""Times of pw_rigid_affinity for DESIGN.md ("Rigid linear guests"): writes profiles/rigid_times.json.

    python profiles/rigid_times.py [--out profiles/rigid_times.json]    # needs a gfx950 device
    python profiles/rigid_times.py --case cc3-1000 --quick              # device times only, 3 repeats (for comparing builds)

The case runs in a process of its own under a time limit.  The workload is that of profiles/affinity_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each seeded at its optimised
pore centre in a box of half its maximum diameter at spacing 0.5 A (a 46^3 grid) and closed at planes through its own
four windows.  CO2 (three sites) at 298 K in M_DEFAULT orientations over the probe-0 cavities of all frames in ONE
pw_rigid_affinity call (core2 = 0.25, no cutoff, no maps), uncharged and charged -- the charged job with synthetic
framework charges that sum to zero --, and the same over every voxel of the boxes (word_first = -1), where the kernel is
compute-bound.  Two warm-up calls, median of 7.  device ms: HIP events from the first launch of a call to its last (the
library's measurement hook); public ms: perf_counter around pywindow_amd.rigid_guest_affinity_batch; host path: the
public call on a device = -1 context with 16 threads, once, and its bytes against the device's.  pair terms: (voxel,
orientation, site, atom) evaluations; beside them pw_affinity's full-box rate (Xe, one site, pairs (voxel, atom))
measured in the same run.
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
CASES = {"cc3-1000": (1000, 560)}


def device_ms_of(f, repeats=7, warm=2):
    """f(list) appends the device time of one call to the list."""
    ms = []
    for _ in range(warm + repeats):
        f(ms)
    ms = ms[warm:]
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def run_case(name, quick):
    import pywindow_amd as pw
    from pywindow_amd import affinity, engine, rigid, synth
    from pywindow_amd.element_data import VDW, element_ids
    from pywindow_amd.utilities import window_planes

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    units = [(elements, f) for f in frames]
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    recs = engine.analyse(units, device=0)
    radii = VDW[element_ids(elements)]
    planes = []
    for r in recs:
        win = engine.windows_of(r)
        planes.append(None if win is None else window_planes(r["pore_opt_c"], win[1]))
    cav = pw.cavity_grid_batch(frames, radii, recs["pore_opt_c"], probe=0.0, spacing=0.5, half_widths=recs["maxd"] / 2.0,
                               planes=planes, mask=True, device=0)
    guest = rigid.RIGID_GUESTS["CO2"]
    S, M, n = len(guest.offsets), rigid.M_DEFAULT, len(elements)
    dirs = pw.sphere_directions(M)
    q = np.random.default_rng(11).uniform(-0.5, 0.5, n)
    q -= q.mean()                                                    # synthetic framework charges, net zero
    coefs = {"uncharged": rigid.rigid_coefficients(elements, guest), "charged": rigid.rigid_coefficients(elements, guest, q)}
    shape = cav.shape[0]
    same_grid = (cav.shape == shape).all(axis=1)
    box = (cav.origin[same_grid], 0.5, shape)
    repeats, warm = (3, 1) if quick else (7, 2)
    result = {"case": name, "frames": n_frames, "atoms": n, "sites": S, "orientations": M, "guest": "CO2", "temperature": 298.0,
              "spacing": 0.5, "grids": sorted({int(s[0]) for s in cav.shape}), "repeats": repeats, "warm_ups": warm,
              "voxels_median": float(np.median(cav.n_voxels)), "chunks_total": int(((cav.n_voxels + 63) // 64).sum()),
              "full_box_frames": int(same_grid.sum())}
    terms = float(cav.n_voxels.sum()) * M * S * n
    box_terms = float(same_grid.sum()) * float(np.prod(shape)) * M * S * n
    for kind, coef in coefs.items():
        masked = lambda device, ms=None: pw.rigid_guest_affinity_batch(frames, coef, guest, [298.0], cavity=cav, directions=dirs,
                                                                       device=device, kernel_ms=ms)
        full = lambda ms=None: pw.rigid_guest_affinity_batch(frames[same_grid], coef, guest, [298.0], grid=box, directions=dirs,
                                                             device=0, kernel_ms=ms)
        got = masked(0)
        assert got.charged == (kind == "charged")
        device = device_ms_of(lambda ms: masked(0, ms), repeats, warm)
        full_device = device_ms_of(full, repeats, warm)
        r = {"pair_terms": terms, "device_ms": device, "pair_terms_per_s": terms / (device["median"] * 1e-3),
             "full_box_pair_terms": box_terms, "full_box_device_ms": full_device,
             "full_box_pair_terms_per_s": box_terms / (full_device["median"] * 1e-3),
             "clamped_frames": int(np.asarray(got.clamped).sum()), "henry_median": float(np.median(got.henry[:, 0])),
             "heat_median": float(np.median(got.heat[:, 0])), "min_energy_median": float(np.median(got.min_energy))}
        if not quick:
            times = []
            for _ in range(2 + 7):
                t0 = time.perf_counter()
                masked(0)
                times.append((time.perf_counter() - t0) * 1e3)
            r["public_ms"] = {"median": float(np.median(times[2:])), "min": float(min(times[2:])), "max": float(max(times[2:]))}
            r["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
            t0 = time.perf_counter()
            ref = masked(-1)
            r["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
            r["device_equals_host"] = bool(got.raw.tobytes() == ref.raw.tobytes() and got.levels.tobytes() == ref.levels.tobytes())
        result[kind] = r
    # pw_affinity over the same full boxes in the same run: Xe, one site, pairs (voxel, atom)
    xe = affinity.lj_coefficients(elements, "Xe")
    one = device_ms_of(lambda ms: pw.guest_affinity_batch(frames[same_grid], xe, "Xe", [298.0], grid=box, device=0, kernel_ms=ms), 5, 1)
    pairs = float(same_grid.sum()) * float(np.prod(shape)) * n
    result["pw_affinity_full_box"] = {"pairs": pairs, "device_ms": one, "pairs_per_s": pairs / (one["median"] * 1e-3),
                                     "pairs_per_s_slowest": pairs / (one["max"] * 1e-3), "pairs_per_s_fastest": pairs / (one["min"] * 1e-3)}
    result["uncharged_full_box_rate_over_pw_affinity"] = result["uncharged"]["full_box_pair_terms_per_s"] / result["pw_affinity_full_box"]["pairs_per_s"]
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rigid_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/rigid_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
