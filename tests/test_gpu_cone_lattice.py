"""The ray tests' cone lattice on the device against the host context (the same source for a one-lane team): every byte
of every record, on molecules with atoms on the z axis through the centre, at azimuth +-pi and with a sphere that
nearly contains the centre, on CC3 frames and on random shells, at three settings of the adjust knobs -- from under 64
sampling vectors (every band shorter than one piece of the enumeration) to about 2000 (bands longer than three)."""
import numpy as np
import pytest

from pywindow_amd import _lib, engine, synth

import _cone_cases

pytestmark = pytest.mark.gpu


def _molecules():
    elements, frames = synth.synthetic_units(4)
    mols = [(elements, np.ascontiguousarray(f)) for f in frames] + _cone_cases.special_molecules(40, 7)
    rng = np.random.default_rng(11)
    pool = np.array(["C", "H", "N", "O", "S", "Br"])
    for n in [4, 5, 63, 64, 65, 127, 128, 129, 199, 200] + [int(v) for v in rng.integers(4, 201, size=10)]:
        p = rng.normal(size=(n, 3))
        p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(3.0, 12.0) + rng.normal(scale=0.4, size=(n, 3))
        mols.append((pool[rng.integers(0, len(pool), size=n)], np.ascontiguousarray(p - p.mean(axis=0))))
    return mols


@pytest.fixture(scope="module")
def molecules():
    return _molecules()


@pytest.mark.parametrize("adjust", [0.07, 1.0, 2.5])
def test_device_records_are_the_host_records(hip_ctx, molecules, adjust):
    assert len(molecules) == 64 and all(4 <= len(el) <= 200 for el, _ in molecules)
    prm = _lib.Params(adjust_windows=adjust, adjust_average=adjust)
    host = engine.analyse(molecules, stages=_lib.STAGE_ALL, device=-1, params=prm)
    dev = engine.analyse(molecules, stages=_lib.STAGE_ALL, device=0, params=prm)
    P = host["n_points"]
    print(f"adjust {adjust}: sampling vectors {P.min()} .. {P.max()}, statuses {dict(zip(*np.unique(host['status'], return_counts=True)))}")
    if adjust < 0.1:
        assert 0 < P[P > 0].min() < 64
    if adjust > 2.0:
        assert P.max() >= 1900
    differ = {u: [k for k in host.dtype.names if host[u][k].tobytes() != dev[u][k].tobytes()]
              for u in range(len(molecules)) if host[u].tobytes() != dev[u].tobytes()}
    assert not differ, dict(list(differ.items())[:6])
    assert host.tobytes() == dev.tobytes()
