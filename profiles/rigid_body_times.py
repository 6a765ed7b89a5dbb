"""Times of pw_rigid_body_affinity for DESIGN.md ("Rigid non-linear guests"): writes profiles/rigid_body_times.json.

    python profiles/rigid_body_times.py [--out profiles/rigid_body_times.json]    # needs a gfx950 device
    python profiles/rigid_body_times.py --case cc3-1000 --quick                   # the CO2 comparison only

The case runs in a process of its own under a time limit.  The workload is that of profiles/rigid_times.py: 1000
synthetic CC3 frames (pywindow_amd.synth: the cage with Gaussian noise of 0.05 A an atom), each seeded at its optimised
pore centre in a box of half its maximum diameter at spacing 0.5 A and closed at planes through its own four windows; the
probe-0 cavities of all frames in ONE pw_rigid_body_affinity call (core2 = 0.25, no cutoff, no maps) at 298 K.

  guests      SF6 (seven sites, uncharged) and H2O (three sites, with synthetic framework charges that sum to zero) in the
              default rotation set.  device ms: HIP events from the first launch of a call to its last (the library's
              measurement hook), one warm-up call and the median of 3; public ms: perf_counter around
              pywindow_amd.rigid_body_affinity_batch, median of 3; host path: the public call on a device = -1 context with
              16 threads over the first HOST_FRAMES frames, once, and its bytes against the device's rows of those frames.
  comparison  whether the new kernel is sound: CO2 written as a pose table (p = t * d, the 64 default directions) through
              pw_rigid_body_affinity against CO2 through pw_rigid_affinity, the same frames and cavities, uncharged and
              charged.  The two alternate in one process, one warm-up call each, then five repeats each; median, min and
              max of the device ms of both, and whether the bytes agree.  The inner loop is the same arithmetic in the same
              instance shape (three sites, two poses a pass); only the way a pose's site positions reach the registers
              differs.
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
#: the frames the host path is timed on (the default set is 1024 rotations: all 1000 frames would take minutes)
HOST_FRAMES = 50


def spread(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def run_case(name, quick):
    import pywindow_amd as pw
    from pywindow_amd import engine, rigid, rigid_body, synth
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
    few = pw.cavity_grid_batch(frames[:HOST_FRAMES], radii, recs["pore_opt_c"][:HOST_FRAMES], probe=0.0, spacing=0.5,
                               half_widths=recs["maxd"][:HOST_FRAMES] / 2.0, planes=planes[:HOST_FRAMES], mask=True, device=0)
    n = len(elements)
    q = np.random.default_rng(11).uniform(-0.5, 0.5, n)
    q -= q.mean()                                                    # synthetic framework charges, net zero
    result = {"case": name, "frames": n_frames, "atoms": n, "temperature": 298.0, "spacing": 0.5,
              "voxels_median": float(np.median(cav.n_voxels)), "chunks_total": int(((cav.n_voxels + 63) // 64).sum())}

    # ---- CO2 as a pose table against CO2 through pw_rigid_affinity ----
    co2 = rigid.RIGID_GUESTS["CO2"]
    dirs = pw.sphere_directions(rigid.M_DEFAULT)
    rot = np.tile(np.eye(3), (len(dirs), 1, 1))
    rot[:, :, 2] = dirs                                              # (body_poses of a body on z: exactly t * d)
    as_body = pw.RigidBody("CO2-table", [(0.0, 0.0, t) for t in co2.offsets], co2.sigma, co2.eps_k, co2.charges)
    comparison = {"guest": "CO2", "sites": 3, "orientations": len(dirs), "repeats": 5, "warm_ups": 1}
    for kind, charges in (("uncharged", None), ("charged", q)):
        coef = rigid.rigid_coefficients(elements, co2, charges)
        linear = lambda ms: pw.rigid_guest_affinity_batch(frames, coef, co2, [298.0], cavity=cav, directions=dirs, device=0, kernel_ms=ms)
        table = lambda ms: pw.rigid_body_affinity_batch(frames, coef, as_body, [298.0], cavity=cav, rotations=rot, device=0, kernel_ms=ms)
        a, b = linear([]), table([])                                 # (the warm-up calls, and the bytes)
        ms_linear, ms_table = [], []
        for _ in range(5):
            linear(ms_linear)
            table(ms_table)
        terms = float(cav.n_voxels.sum()) * len(dirs) * 3 * n
        comparison[kind] = {"pair_terms": terms, "pw_rigid_affinity_device_ms": spread(ms_linear),
                            "pw_rigid_body_affinity_device_ms": spread(ms_table),
                            "table_over_linear": float(np.median(ms_table) / np.median(ms_linear)),
                            "same_bytes": bool(a.raw.tobytes() == b.raw.tobytes() and a.levels.tobytes() == b.levels.tobytes())}
    result["co2_as_a_table"] = comparison

    # ---- SF6 and H2O in the default rotation set ----
    if not quick:
        rotations = pw.rotation_set()
        result["rotations"] = [rigid_body.AXES_DEFAULT, rigid_body.SPINS_DEFAULT]
        for guest, charges in (("SF6", None), ("H2O", q)):
            body = pw.RIGID_BODIES[guest]
            S = len(body.sigma)
            coef = rigid.rigid_coefficients(elements, body, charges)
            call = lambda device, ms=None, x=frames, c=cav: pw.rigid_body_affinity_batch(x, coef, body, [298.0], cavity=c, rotations=rotations,
                                                                                         device=device, kernel_ms=ms)
            got = call(0)                                            # (the warm-up call)
            ms, times = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                call(0, ms)
                times.append((time.perf_counter() - t0) * 1e3)
            terms = float(cav.n_voxels.sum()) * len(rotations) * S * n
            r = {"sites": S, "charged": charges is not None, "poses": len(rotations), "pair_terms": terms, "device_ms": spread(ms),
                 "pair_terms_per_s": terms / (float(np.median(ms)) * 1e-3), "public_ms": spread(times),
                 "clamped_frames": int(np.asarray(got.clamped).sum()), "henry_median": float(np.median(got.henry[:, 0])),
                 "heat_median": float(np.median(got.heat[:, 0])), "min_energy_median": float(np.median(got.min_energy))}
            r["host_threads"] = int(pw._lib.load().pw_context_host_threads(engine.context(-1)._h, 16))   # (sets, then reports)
            t0 = time.perf_counter()
            ref = call(-1, None, frames[:HOST_FRAMES], few)
            r["host_path_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
            r["host_path_frames"] = HOST_FRAMES
            r["device_equals_host"] = bool(got.raw[:HOST_FRAMES].tobytes() == ref.raw.tobytes()
                                           and got.levels[:HOST_FRAMES].tobytes() == ref.levels.tobytes())
            result[guest] = r
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rigid_body_times.json"))
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
    meta = {"commit_parent": head or None, "command": "python profiles/rigid_body_times.py", "loadavg": list(os.getloadavg()),
            "note": "one MI355X of a shared machine, other tenants not controlled"}
    pathlib.Path(args.out).write_text(json.dumps({"meta": meta, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
