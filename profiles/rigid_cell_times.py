"""Times of pw_rigid_cell for DESIGN.md ("Rigid guests in the crystal"): writes profiles/rigid_cell_times.json.

    python profiles/rigid_cell_times.py [--out profiles/rigid_cell_times.json]       # needs a gfx950 device
    python profiles/rigid_cell_times.py --case cc3-cell-8 --frames 2 --quick         # fewer frames, 3 repeats, no host path

The case runs in a process of its own under a time limit.  The workload is the periodic trajectory that
profiles/percolation_times.py and profiles/basins_times.py time, cut to a few frames: the 1344-atom CC3 cell of
tests/golden/rebuild.npz with Gaussian noise of 0.02 A an atom (frame k from default_rng(4 + k)), CO2 with 64 orientations
at spacing 0.5 and cutoff 12, two temperatures, all frames in ONE pw_rigid_cell call.  Two warm-up calls, median of 7 with
min and max.  device ms: HIP events around the launches of a call (the library's measurement hook), with the skip and --
alternated in the same process -- with the reach handed to the kernel as +inf, so that no atom is left out; n_pairs against
V M S n; pw_percolation's field-and-levels call on the same frames in the same run and, by the difference to the same
call on its own maps, its field kernel, for the rate per pair term; public ms: perf_counter around
pywindow_amd.rigid_guest_diffusion_batch, the images, the plan, the three entries and the numpy layer included; host
path: Context.rigid_cell on a device = -1 context with 16 threads, once, on one frame, and its bytes against the
device's; the coefficients of CO2 and N2 and their ratio at the two temperatures."""
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
CASES = {"cc3-cell-8": (8, 900)}
TEMPERATURES = [250.0, 350.0]


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def run_case(name, quick, n_frames):
    import pywindow_amd as pw
    from pywindow_amd import engine
    from pywindow_amd import percolation as PC
    from pywindow_amd import rigid_cell as RC

    n_frames = n_frames or CASES[name][0]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    frames = np.stack([base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape) for k in range(n_frames)])
    kw = dict(spacing=0.5, cutoff=12.0)
    repeats, warm = (3, 1) if quick else (7, 2)
    ctx = engine.context(0)
    planned = RC.plan_field(frames, elements, lattice, "CO2", TEMPERATURES, **kw)
    jobs, atoms, coef, offsets, dirs, betas = planned[:6]
    on, off, diag_on, diag_off = [], [], [], []
    for _ in range(warm + repeats):                                  # (alternated: the two see the same machine)
        got = ctx.rigid_cell(jobs, atoms, coef, offsets, dirs, betas, kernel_ms=on, diagnostics=diag_on)
        all_atoms = ctx.rigid_cell(jobs, atoms, coef, offsets, dirs, betas, kernel_ms=off, diagnostics=diag_off, skip=False)
    device, no_skip = spread(on[warm:]), spread(off[warm:])
    voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
    every = int((voxels * jobs["n_dirs"] * jobs["n_sites"] * jobs["n"]).sum())
    pairs = int(diag_on[-1][0].sum())
    perc_jobs, p_atoms, p_coef, *_ = PC.plan_jobs(frames, elements, lattice, "Xe", maps=True, **kw)
    perc, perc_alone = [], []
    for _ in range(warm + repeats):
        _, _, maps = ctx.percolation(perc_jobs, p_atoms, p_coef, kernel_ms=perc)
    given = perc_jobs.copy()
    given["field_first"], given["map_first"] = perc_jobs["map_first"], -1
    for _ in range(warm + repeats):
        ctx.percolation(given, field=maps, kernel_ms=perc_alone)
    perc, perc_alone = spread(perc[warm:]), spread(perc_alone[warm:])
    perc_field_ms = perc["median"] - perc_alone["median"]
    perc_pairs = int((voxels * perc_jobs["n"]).sum())
    result = {"case": name, "frames": n_frames, "atoms": int(len(elements)), "listed_atoms_per_frame": spread(jobs["n"]),
              "grid": [int(jobs[0]["nx"]), int(jobs[0]["ny"]), int(jobs[0]["nz"])], "guest": "CO2", "orientations": int(jobs[0]["n_dirs"]),
              "sites": int(jobs[0]["n_sites"]), "spacing": 0.5, "cutoff": 12.0, "temperatures": TEMPERATURES, "repeats": repeats,
              "warm_ups": warm, "device_ms": device, "device_ms_without_the_skip": no_skip,
              "factor_the_list_buys": no_skip["median"] / device["median"],
              "bytes_equal_with_and_without_the_skip": bool(all(a.tobytes() == b.tobytes() for a, b in zip(got, all_atoms))),
              "pair_terms_V_M_S_n": every, "pair_terms_evaluated": pairs, "share_the_skip_leaves": pairs / every,
              "pair_terms_evaluated_without_the_skip": int(diag_off[-1][0].sum()),
              "pair_terms_per_second": pairs / (device["median"] * 1e-3),
              "pair_terms_per_second_without_the_skip": every / (no_skip["median"] * 1e-3),
              "instances_launched_bits": int(diag_on[-1][1]),
              "pw_percolation_device_ms_same_frames": perc, "pw_percolation_on_its_own_maps_ms": perc_alone,
              "pw_percolation_field_ms_by_difference": perc_field_ms, "pw_percolation_field_pair_terms": perc_pairs,
              "pw_percolation_field_pair_terms_per_second": perc_pairs / (perc_field_ms * 1e-3) if perc_field_ms > 0.0 else None}
    coefficients = {}
    for guest in ("CO2", "N2"):
        d = pw.rigid_guest_diffusion_batch(frames, elements, lattice, guest, TEMPERATURES, device=0, **kw)
        coefficients[guest] = {"coefficient_A2_per_s": [spread(d.coefficient[:, l]) for l in range(len(TEMPERATURES))],
                               "frames_valid": int(d.valid.sum()), "frames_barrierless": int(d.barrierless.any(axis=1).sum()),
                               "n_sites_per_job": spread(d.n_sites)}
    result["diffusion"] = coefficients
    result["CO2_over_N2_median_coefficient"] = [coefficients["CO2"]["coefficient_A2_per_s"][l]["median"] /
                                                max(coefficients["N2"]["coefficient_A2_per_s"][l]["median"], 1e-300)
                                                for l in range(len(TEMPERATURES))]
    if not quick:
        times = []
        for _ in range(1 + 3):
            t0 = time.perf_counter()
            pw.rigid_guest_diffusion_batch(frames, elements, lattice, "CO2", TEMPERATURES, device=0, **kw)
            times.append((time.perf_counter() - t0) * 1e3)
        result["public_diffusion_ms_1_warm_up_3_repeats"] = spread(times[1:])
        host = engine.context(-1)
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(host._h, 16))   # (sets, then reports)
        one = RC.plan_field(frames[:1], elements, lattice, "CO2", TEMPERATURES, **kw)[:6]
        t0 = time.perf_counter()
        ref = host.rigid_cell(*one)
        result["host_path_16_threads_ms_one_frame"] = (time.perf_counter() - t0) * 1e3
        dev = ctx.rigid_cell(*one)
        result["device_equals_host_one_frame"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(dev, ref)))
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rigid_cell_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/rigid_cell_times.py" + (f" --frames {args.frames}" if args.frames else "") +
            (" --quick" if args.quick else ""), "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
