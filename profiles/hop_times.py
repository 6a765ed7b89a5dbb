"""Times of pw_hop for DESIGN.md ("Guest hopping"): writes profiles/hop_times.json.

    python profiles/hop_times.py [--out profiles/hop_times.json]    # needs a gfx950 device

The case runs in a process of its own under a time limit.  The workload is that of profiles/cavity_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each with its optimised pore
centre and its own four windows.  Xe at 298 K, every (frame, window) a job of ONE pw_hop call (spacing 0.25 A, a 47 x 47
lattice across, slabs from 4 A behind the pore centre to 4 A beyond the window, cap 100 kJ/mol, core2 = 0.25, no
cutoff).  Two warm-up calls, median of 7 (1 and 3 for the host path).  device ms: HIP events from the first launch of a
call to its last, and the field kernels' and the slab kernels' share of it (the library's measurement hook); call ms:
perf_counter around Context.hop (ctypes, from and into host arrays, job records ready); public ms: around
pywindow_amd.guest_hopping_batch; host path: the public call on a device = -1 context with 16 threads; affinity: in the
same run, pw_affinity over the same boxes (the same atoms, origins and dimensions, word_first = -1, no energy map) --
the same pair terms as the field kernel, against which its pairs per second are judged.
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


def run_case(name):
    import pywindow_amd as pw
    from pywindow_amd import affinity, engine, hopping, synth

    n_frames, _ = CASES[name]
    elements, base = synth.load_cc3_base()
    frames = np.stack([synth.noisy_frame(base, 7000 + t, sigma=0.05) for t in range(n_frames)])
    units = [(elements, f) for f in frames]
    dev = engine.context(0)
    engine.analyse(units[:64], device=0)                             # (warm-up: code objects, workspaces)
    recs = engine.analyse(units, device=0)
    wins = []
    for r in recs:
        win = engine.windows_of(r)
        wins.append(None if win is None else np.asarray(win[1], dtype=np.float64).reshape(-1, 3))
    coef = affinity.lj_coefficients(elements, "Xe")
    centres = np.asarray(recs["pore_opt_c"], dtype=np.float64)
    public_call = lambda device, ms=None: pw.guest_hopping_batch(frames, coef, "Xe", centres, wins, [298.0], device=device,
                                                                 kernel_ms=ms)
    got = public_call(0)
    host_ctx_threads = pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16)   # (sets, then reports)
    ref = public_call(-1)
    same = got.slabs.tobytes() == ref.slabs.tobytes() and got.Z.tobytes() == ref.Z.tobytes() and got.E.tobytes() == ref.E.tobytes()
    # the same call on the context, from ready job records
    clean = [np.zeros((0, 3)) if w is None else w for w in wins]
    jobs, atoms, cuts, distance, n_slabs, where = hopping.hop_jobs(frames, centres, clean, 47, 0.25, 4.0, 4.0, 1, 100.0, 0.25, 0.0)
    cuts = np.concatenate(cuts)
    betas = 1.0 / (affinity.R * np.array([298.0]))
    raw_call = lambda ms=None: dev.hop(jobs, betas, atoms.reshape(-1, 3), coef, cuts, kernel_ms=ms)
    first = raw_call()
    assert int(first[2]["n"].sum()) == int(got.slabs["n"][got.slabs["n"] >= 0].sum())
    ms = []
    for _ in range(2 + 7):
        raw_call(ms)
    ms = np.array(ms[2:])
    call = median_of(raw_call, 7)
    public = median_of(lambda: public_call(0), 7)
    host_ms = median_of(lambda: public_call(-1), 3, warm=1)
    # pw_affinity over the same boxes: the same pair terms as the field kernel
    aj = np.zeros(len(jobs), dtype=pw._lib.AFFINITY_JOB_DTYPE)
    for k, j in enumerate(jobs):
        aj[k] = (j["atom_first"], j["n"], 0, -1, 0, 1, 0, 0, k, 0, -1, k, j["origin"], j["spacing"], j["core2"], j["cutoff2"],
                 j["nx"], j["ny"], j["nz"], 0)
    aff_ms = []
    for _ in range(1 + 5):
        dev.affinity(aj, atoms.reshape(-1, 3), coef, betas, kernel_ms=aff_ms)
    aff_ms = np.array(aff_ms[1:])
    voxels = int((jobs["nx"].astype(np.int64) * jobs["ny"] * jobs["nz"]).sum())
    pairs = voxels * len(elements)
    slabs = int(jobs["nz"].sum())
    valid = got.valid[:, :, 0]
    rate = got.rate[:, :, 0][valid]
    result = {
        "case": name, "frames": n_frames, "atoms": len(elements), "jobs": int(len(jobs)), "lattice": 47, "spacing": 0.25,
        "slabs": slabs, "slabs_per_job_median": float(np.median(jobs["nz"])), "voxels": voxels, "pairs": pairs, "guest": "Xe",
        "temperature": 298.0, "cap": 100.0, "repeats": 7, "host_repeats": 3, "host_threads": int(host_ctx_threads),
        "device_ms_median": float(np.median(ms[:, 0])), "device_ms_min": float(ms[:, 0].min()), "device_ms_max": float(ms[:, 0].max()),
        "field_kernel_ms_median": float(np.median(ms[:, 1])), "field_kernel_ms_min": float(ms[:, 1].min()),
        "field_kernel_ms_max": float(ms[:, 1].max()),
        "slab_kernel_ms_median": float(np.median(ms[:, 2])), "slab_kernel_ms_min": float(ms[:, 2].min()),
        "slab_kernel_ms_max": float(ms[:, 2].max()),
        "slab_kernel_us_per_slab": float(np.median(ms[:, 2])) * 1e3 / slabs,
        "field_pairs_per_second": pairs / (float(np.median(ms[:, 1])) * 1e-3),
        "call_ms_median": call[0], "call_ms_min": call[1], "call_ms_max": call[2],
        "public_ms_median": public[0], "public_ms_min": public[1], "public_ms_max": public[2],
        "host_path_16_threads_ms_median": host_ms[0], "host_path_16_threads_ms_min": host_ms[1],
        "host_path_16_threads_ms_max": host_ms[2], "device_equals_host": bool(same), "host_over_public": host_ms[0] / public[0],
        "affinity_same_boxes_device_ms_median": float(np.median(aff_ms)), "affinity_same_boxes_device_ms_min": float(aff_ms.min()),
        "affinity_same_boxes_device_ms_max": float(aff_ms.max()),
        "affinity_pairs_per_second": pairs / (float(np.median(aff_ms)) * 1e-3),
        "voxels_filled": int(first[2]["n"].sum()), "windows_valid": int(valid.sum()), "windows_free_exit": int(got.free_exit[:, :, 0].sum()),
        "windows_seed_closed": int((got.seed_closed[:, :, 0] & ~got.padding).sum()),
        "rate_median": float(np.median(rate)), "rate_min": float(rate.min()), "rate_max": float(rate.max()),
        "mean_rate_per_window": [float(v) for v in got.mean_rate()[:, 0]],
        "free_barrier_median": float(np.median(got.free_barrier[:, :, 0][valid])),
    }
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hop_times.json"))
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
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
    meta = {"commit_parent": head or None, "command": "python profiles/hop_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
