"""The wave-level bracket scan (wave_path_bracket, pw_unit.hpp) in its two uses -- the refined path of every window and the
left-over paths of the sampling stage -- on the device against the host context (the same source for a one-lane team):
every byte of every record.  The forty small shells of test_gpu_path_brackets (4 to 64 atoms, 8 to 11 radii, ray-test
survivor counts around the team's 256 threads: 1, 15 and 1-after-two-rounds left-over paths) at three steps of the refined
path (0.1: some thirty points; 0.9: a handful; 0.02: more than a hundred, several passes of the plain walk), as a per-atom
batch and as template batches; shells of 65 and 129 atoms (a lane's second and third atom); CC3 frames; the units of the
cliffs fixture with dropped and negative windows; and the per-window rows of the stage capture (the neck's position new_z,
d0, the evaluation count) bit for bit."""
import numpy as np
import pytest

from pywindow_amd import _lib, element_data as E, engine, synth

import _path_cases as PC
from test_gpu_path_brackets import _molecules, _same

pytestmark = pytest.mark.gpu

INCREMENT2 = (0.1, 0.9, 0.02)


@pytest.fixture(scope="module")
def host_ctx():
    return engine.context(-1)


@pytest.mark.parametrize("inc2", INCREMENT2)
def test_per_atom_batch_of_small_shells_is_the_host_batch(hip_ctx, host_ctx, inc2):
    mols = _molecules() + [PC.shell(501, n=65), PC.shell(502, n=129)]
    assert len(mols) == 42 and all(4 <= len(el) <= 64 for el, _ in mols[:40])
    batch = engine.make_batch(mols)
    prm = _lib.Params(increment2=inc2)
    host = host_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    dev = hip_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    for u, (cand, passed) in enumerate(PC.SURVIVORS.values()):
        assert host["n_survivors"][u] == passed, (u, cand, passed, host["n_survivors"][u])
    radii = [len(set(E.VDW[E.element_ids(el)])) for el, _ in mols]
    assert {8, 9, 10, 11} <= set(radii) and (host["n_clusters"] > 0).sum() >= 30
    _same(host, dev)


@pytest.mark.parametrize("inc2", INCREMENT2)
def test_template_batches_of_small_shells_are_the_host_batches(hip_ctx, host_ctx, inc2):
    prm = _lib.Params(increment2=inc2)
    fitted = 0
    for el, xyz in _molecules():
        ids = E.element_ids(el)
        # (two frames of one composition: the shell and the shell turned a quarter about z)
        frames = np.stack([xyz, xyz[:, [1, 0, 2]] * np.array([-1.0, 1.0, 1.0])])
        batch = _lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids])
        host = host_ctx.analyse(batch, _lib.STAGE_ALL, prm)
        dev = hip_ctx.analyse(batch, _lib.STAGE_ALL, prm)
        fitted += int((host["n_windows"] > 0).sum())
        _same(host, dev)
    assert fitted >= 20


@pytest.mark.parametrize("inc2", INCREMENT2)
def test_cc3_frames_are_the_host_batch(hip_ctx, host_ctx, inc2):
    elements, frames = synth.synthetic_units(6)
    ids = E.element_ids(elements)
    batch = _lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids])
    prm = _lib.Params(increment2=inc2)
    host = host_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    dev = hip_ctx.analyse(batch, _lib.STAGE_ALL, prm)
    assert (host["n_windows"] == 4).all()
    _same(host, dev)


def test_units_with_dropped_and_negative_windows_are_the_host_records(hip_ctx, host_ctx):
    from test_cliffs import load_cliffs, params_of

    mols, calls = load_cliffs()
    dropped = negative = 0
    for call in calls:
        if not (call["dropped"] or call["negative"]):
            continue
        el, xyz = mols[call["mol"]]
        prm, stages = params_of(call)
        batch = engine.make_batch([(el, xyz)])
        host = host_ctx.analyse(batch, stages, prm)
        dev = hip_ctx.analyse(batch, stages, prm)
        assert bool(host["status"][0] & _lib.ST_WINDOW_DROPPED) == (call["dropped"] > 0)
        assert bool(host["status"][0] & _lib.ST_WINDOW_NEGATIVE) == (call["negative"] > 0)
        dropped += call["dropped"] > 0
        negative += call["negative"] > 0
        _same(host, dev)
    assert dropped == 3 and negative == 2


def _captures_agree(hip_ctx, host_ctx, batch):
    host, hdbg = host_ctx.analyse_debug(batch, _lib.STAGE_ALL)
    dev, ddbg = hip_ctx.analyse_debug(batch, _lib.STAGE_ALL)
    _same(host, dev)
    rows = 0
    for u in range(len(host)):
        k = min(max(int(host["n_clusters"][u]), 0), _lib.W_MAX)
        # (every column of every cluster's row: the chosen vector, the angles, new_z, d0, the optima, the evaluations)
        assert hdbg["win"][u][:k].tobytes() == ddbg["win"][u][:k].tobytes(), (u, hdbg["win"][u][:k], ddbg["win"][u][:k])
        assert hdbg["n_survivors"][u] == ddbg["n_survivors"][u] and hdbg["n_clusters"][u] == ddbg["n_clusters"][u]
        ns = min(int(hdbg["n_survivors"][u]), _lib.P_MAX)
        assert hdbg["gap2"][u][:ns].tobytes() == ddbg["gap2"][u][:ns].tobytes(), u
        rows += k
    return rows


def test_capture_rows_of_the_shells_are_the_host_rows(hip_ctx, host_ctx):
    mols = _molecules() + [PC.shell(501, n=65), PC.shell(502, n=129)]
    assert _captures_agree(hip_ctx, host_ctx, engine.make_batch(mols)) >= 40


def test_capture_rows_of_cc3_frames_are_the_host_rows(hip_ctx, host_ctx):
    elements, frames = synth.synthetic_units(6)
    ids = E.element_ids(elements)
    assert _captures_agree(hip_ctx, host_ctx, _lib.Batch.uniform(frames, E.VDW[ids], E.MASS[ids])) == 24
