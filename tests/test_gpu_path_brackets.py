"""The bracketed path scans of the sampling stage (path_bracket_thread, pw_unit.hpp) on the device against the host
context (the same source for a one-lane team): every byte of every record, on small molecules chosen where the kernel
can take another way -- 4 and 5 atoms; ray-test survivor counts around the team's 256 threads (whole rounds against
left-over paths, the quarter-team rule); eight radii (grouped) and nine, ten and eleven (not grouped: the plain scan); a
per-atom batch and a template batch of CC3 frames; steps so long that a path has one step, or none, and so short that
it has more than sixteen points."""
import numpy as np
import pytest

from pywindow_amd import _lib, element_data as E, engine, synth

import _path_cases as PC

pytestmark = pytest.mark.gpu


def _same(host, dev):
    differ = {u: [k for k in host.dtype.names if host[u][k].tobytes() != dev[u][k].tobytes()]
              for u in range(len(host)) if host[u].tobytes() != dev[u].tobytes()}
    assert not differ, dict(list(differ.items())[:6])
    assert host.tobytes() == dev.tobytes()


def _molecules():
    mols = [PC.shell(s) for s in PC.SURVIVORS]
    mols += [PC.shell(11, n=4), PC.shell(12, n=5), PC.shell(13, n=4, n_elements=1), PC.shell(14, n=5, n_elements=2)]
    for k, n_el in enumerate((8, 10, 11, 12)):            # distinct radii: 8, 9, 10, 11 (S and P share one)
        mols += [PC.shell(100 + k, n=40 + k, n_elements=n_el), PC.shell(200 + k, n=23, n_elements=n_el)]
    mols += [PC.shell(s) for s in range(300, 321)]
    return mols


def test_per_atom_batch_is_the_host_batch(hip_ctx):
    mols = _molecules()
    assert len(mols) == 40 and all(4 <= len(el) <= 64 for el, _ in mols)
    host = engine.analyse(mols, stages=_lib.STAGE_ALL, device=-1)
    dev = engine.analyse(mols, stages=_lib.STAGE_ALL, device=0)
    for u, (cand, passed) in enumerate(PC.SURVIVORS.values()):
        assert host["n_survivors"][u] == passed, (u, cand, passed, host["n_survivors"][u])
    radii = [len(set(E.VDW[E.element_ids(el)])) for el, _ in mols]
    assert {8, 9, 10, 11} <= set(radii) and (host["n_survivors"] > 0).sum() >= 30
    _same(host, dev)


@pytest.mark.parametrize("steps", ["default", "one step", "many steps"])
def test_template_batch_of_cc3_frames_is_the_host_batch(hip_ctx, steps):
    elements, frames = synth.synthetic_units(6)
    ids = E.element_ids(elements)
    batch = _lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids])
    host_ctx = engine.context(-1)
    prm = None
    if steps != "default":
        r = host_ctx.analyse(batch)["sphere_r"]
        # one step: the smallest sphere's paths have one step (two points), where the spheres differ enough some have none;
        # many steps: more than sixteen points to every path
        prm = _lib.Params(increment=float(r.min()) / 1.5 if steps == "one step" else 0.3)
        assert steps == "one step" or r.min() / 0.3 > 16.0
    host = host_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    dev = hip_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    assert (host["n_survivors"] > 0).all()
    _same(host, dev)


def test_small_molecules_with_one_step_and_with_many(hip_ctx):
    mols = [PC.shell(s) for s in list(PC.SURVIVORS)[:3]] + [PC.shell(s) for s in range(400, 409)]
    r = engine.analyse(mols, stages=_lib.STAGE_ALL, device=-1)["sphere_r"]
    for inc in (float(np.median(r)) / 1.5, 0.3):          # (half of them: one step, the others none; then up to 30 points)
        prm = _lib.Params(increment=inc)
        host = engine.analyse(mols, stages=_lib.STAGE_ALL, device=-1, params=prm)
        dev = engine.analyse(mols, stages=_lib.STAGE_ALL, device=0, params=prm)
        assert (host["n_points"] > 0).all()
        _same(host, dev)
