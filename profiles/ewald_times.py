"""Times of pw_rigid_cell_ewald for DESIGN.md ("Charged rigid guests in the crystal"): writes profiles/ewald_times.json.

    python profiles/ewald_times.py [--out profiles/ewald_times.json]       # needs a gfx950 device
    python profiles/ewald_times.py --case cc3-cell-8 --frames 2 --quick    # fewer frames, 3 repeats, no host path

The case runs in a process of its own under a time limit.  The workload is profiles/rigid_cell_times.py's: the 1344-atom CC3
cell of tests/golden/rebuild.npz with Gaussian noise of 0.02 A an atom (frame k from default_rng(4 + k)), CO2 with 64
orientations at spacing 0.5 and cutoff 12, two temperatures, all frames in ONE call.  The framework's charges are the
library's own for an isolated molecule, molecule by molecule: the cell's atoms are joined into molecules over the periodic
boundary (a bond is a minimum-image distance below 1.25 A with a hydrogen, 1.85 A without), each molecule is made whole
and equilibrated on its own (pywindow_amd.equilibrate_charges, total charge 0) -- the charges of the noise-free cell, used
for every frame; periodic charge equilibration is not built.  Two warm-up calls, median of 7 with min and max.
device ms: HIP events around the launches of a call (the library's measurement hook) -- the charged call
(pw_rigid_cell_ewald, Ewald tolerance 1e-6) and the uncharged one (pw_rigid_cell) alternated in the same process; the
reciprocal part alone: the charged jobs with their listed atoms taken away, so that the tables, Urec and a field kernel
without pair terms remain; host path: the charged call on a device = -1 context with 16 threads, once, on one frame, and
its bytes against the device's; the diffusion coefficients of CO2 and N2 with and without charges and their ratios."""
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


def molecule_charges(elements, xyz, lattice, device):
    """QEq charges of the cell's atoms, molecule by molecule: (charges (n,), the sizes of the molecules)."""
    import pywindow_amd as pw

    n = len(xyz)
    inv = np.linalg.inv(lattice)
    frac = xyz @ inv.T                                               # (columns as vectors: x = lattice @ f)
    d = frac[:, None, :] - frac[None, :, :]
    d -= np.round(d)
    dist = np.linalg.norm(d @ lattice.T, axis=2)
    hydrogen = np.array([str(e).upper() == "H" for e in elements])
    limit = np.where(hydrogen[:, None] | hydrogen[None, :], 1.25, 1.85)
    bonded = (dist < limit) & ~np.eye(n, dtype=bool)
    label = -np.ones(n, dtype=np.int64)
    whole = frac.copy()
    sizes = []
    for seed in range(n):
        if label[seed] >= 0:
            continue
        label[seed] = len(sizes)
        stack, members = [seed], [seed]
        while stack:                                                 # (every atom is made whole against the one that found it)
            a = stack.pop()
            for b in np.nonzero(bonded[a] & (label < 0))[0]:
                label[b] = label[seed]
                whole[b] = whole[a] + (frac[b] - frac[a] - np.round(frac[b] - frac[a]))
                stack.append(b)
                members.append(b)
        sizes.append(len(members))
    q = np.zeros(n)
    for m in range(len(sizes)):
        idx = np.nonzero(label == m)[0]
        got = pw.equilibrate_charges(whole[idx] @ lattice.T, [elements[i] for i in idx], 0.0, device=device).charges
        q[idx] = got - got.mean()
    return q, sizes


def run_case(name, quick, n_frames):
    import pywindow_amd as pw
    from pywindow_amd import engine
    from pywindow_amd import rigid_cell as RC

    n_frames = n_frames or CASES[name][0]
    with np.load(ROOT / "tests" / "golden" / "rebuild.npz", allow_pickle=True) as g:
        elements, base, lattice = g["cc3_cell__in_elements"], g["cc3_cell__in_coordinates"], g["cc3_cell__in_lattice"]
    elements = [str(e) for e in elements]
    frames = np.stack([base + np.random.default_rng(4 + k).normal(0.0, 0.02, size=base.shape) for k in range(n_frames)])
    kw = dict(spacing=0.5, cutoff=12.0)
    repeats, warm = (3, 1) if quick else (7, 2)
    ctx = engine.context(0)
    q, sizes = molecule_charges(elements, np.asarray(base, dtype=np.float64), np.asarray(lattice, dtype=np.float64), 0)
    planned, ew = RC.plan_charged_field(frames, elements, lattice, "CO2", TEMPERATURES, charges=q, **kw)
    jobs, atoms, coef, offsets, dirs, betas = planned[:6]
    args = (ew["jobs"], atoms, ew["coef"], offsets, dirs, betas, ew["site_q"], ew["cell"], ew["kvecs"])
    bare = ew["jobs"].copy()
    bare["cell"]["n"] = 0                                            # (no listed atoms: the reciprocal part and an empty pair loop)
    charged, plain, recip, diag = [], [], [], []
    for _ in range(warm + repeats):                                  # (alternated: the three see the same machine)
        got = ctx.rigid_cell_ewald(*args, kernel_ms=charged, diagnostics=diag)
        ctx.rigid_cell(jobs, atoms, coef, offsets, dirs, betas, kernel_ms=plain)
        ctx.rigid_cell_ewald(bare, *args[1:], kernel_ms=recip)
    charged, plain, recip = spread(charged[warm:]), spread(plain[warm:]), spread(recip[warm:])
    voxels = np.int64(1) * jobs["nx"] * jobs["ny"] * jobs["nz"]
    K = ew["jobs"]["n_k"]
    result = {"case": name, "frames": n_frames, "atoms": len(elements), "molecules": sizes, "charge_min_max": [float(q.min()), float(q.max())],
              "sum_abs_charge": float(np.abs(q).sum()), "listed_atoms_per_frame": spread(jobs["n"]),
              "grid": [int(jobs[0]["nx"]), int(jobs[0]["ny"]), int(jobs[0]["nz"])], "guest": "CO2", "orientations": int(jobs[0]["n_dirs"]),
              "sites": int(jobs[0]["n_sites"]), "spacing": 0.5, "cutoff": 12.0, "ewald_tolerance": 1e-6,
              "alpha": float(ew["jobs"]["alpha"][0]), "reciprocal_rows_per_frame": spread(K), "temperatures": TEMPERATURES,
              "repeats": repeats, "warm_ups": warm, "device_ms_charged": charged, "device_ms_uncharged": plain,
              "charged_over_uncharged": charged["median"] / plain["median"], "device_ms_reciprocal_part_alone": recip,
              "reciprocal_share_of_charged": recip["median"] / charged["median"],
              "reciprocal_multiply_adds": int((2 * voxels * jobs["n_dirs"] * K).sum()),
              "reciprocal_multiply_adds_per_second": float((2 * voxels * jobs["n_dirs"] * K).sum() / (recip["median"] * 1e-3)),
              "pair_terms_evaluated": int(diag[-1][0].sum()),
              "pair_terms_per_second_charged": float(diag[-1][0].sum() / (charged["median"] * 1e-3)),
              "pair_terms_per_second_uncharged": float(diag[-1][0].sum() / (plain["median"] * 1e-3))}
    coefficients = {}
    for guest in ("CO2", "N2"):
        for label, ch in (("uncharged", None), ("charged", q)):
            d = pw.rigid_guest_diffusion_batch(frames, elements, lattice, guest, TEMPERATURES, device=0, charges=ch, **kw)
            coefficients[f"{guest}_{label}"] = {"coefficient_A2_per_s": [spread(d.coefficient[:, l]) for l in range(len(TEMPERATURES))],
                                                "frames_valid": int(d.valid.sum()), "n_sites_per_job": spread(d.n_sites)}
    result["diffusion"] = coefficients
    for label in ("uncharged", "charged"):
        result[f"CO2_over_N2_median_coefficient_{label}"] = [
            coefficients[f"CO2_{label}"]["coefficient_A2_per_s"][l]["median"] /
            max(coefficients[f"N2_{label}"]["coefficient_A2_per_s"][l]["median"], 1e-300) for l in range(len(TEMPERATURES))]
    if not quick:
        host = engine.context(-1)
        result["host_threads"] = int(pw._lib.load().pw_context_host_threads(host._h, 16))   # (sets, then reports)
        one, ew1 = RC.plan_charged_field(frames[:1], elements, lattice, "CO2", TEMPERATURES, charges=q, **kw)
        args1 = (ew1["jobs"], one[1], ew1["coef"], one[3], one[4], one[5], ew1["site_q"], ew1["cell"], ew1["kvecs"])
        t0 = time.perf_counter()
        ref = host.rigid_cell_ewald(*args1)
        result["host_path_16_threads_ms_one_frame_charged"] = (time.perf_counter() - t0) * 1e3
        dev = ctx.rigid_cell_ewald(*args1)
        result["device_equals_host_one_frame"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(dev, ref)))
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ewald_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/ewald_times.py" + (f" --frames {args.frames}" if args.frames else "") +
            (" --quick" if args.quick else ""), "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled; 2 warm-up calls, median of 7"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
