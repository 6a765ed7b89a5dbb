"""pw_rigid_cell_ewald on the device: gfx950 against the host path (device = -1), as BYTES -- every sum of the definition
has its order written out (pywindow_amd/csrc/pw_ewald.hpp), so neither the launch geometry, how the jobs are gathered
into launches, what the workspace held before nor whether the skip is on may show.  tests/test_ewald_host.py holds the
host path to pw_rigid_cell, pw_rigid_affinity and a numpy restatement."""
import numpy as np
import pytest

import _ewald_cases as E
import _stat_edges as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1, host_threads=16)


@pytest.fixture(autouse=True)
def poison_off_afterwards():
    yield
    S.set_poison(False)


def jobs_of_the_host_tests():
    return [E.skew_job().replace(charged=0), E.skew_job(), E.skip_job(), E.wide_job()]


@pytest.mark.parametrize("k", range(4), ids=("uncharged", "charged", "skip", "K=65,M=5,n_cell=67"))
def test_the_device_is_the_host_path(hip_ctx, host, k):
    """The uncharged and the charged skew job, the job with atoms beyond every reach, and the job that crosses a wave of
    rows, the orientation tile and the 64 strided accumulators: out row, levels and maps byte for byte, with the skip on
    and off."""
    job = jobs_of_the_host_tests()[k]
    packed = E.pack([job], hole=2)
    want = E.run(host, packed)
    d = []
    got = E.run(hip_ctx, packed, diagnostics=d)
    assert E.same(got, want), (job.name, E.C.first_difference(got, want))
    assert E.same(E.run(hip_ctx, packed, skip=False), want)
    assert d[0][1] == 1 << (len(job.inputs.offsets) - 1) and np.isfinite(got[2]).any()


def test_two_launch_groups_are_one_at_a_time_calls(hip_ctx, host):
    """Six jobs on one set of inputs -- charged and not, with and without maps -- in one call with 20 kB of workspace a
    launch (the jobs need 1 kB to 45 kB each: three groups, one of them a job that is larger than the budget), with every job a
    launch of its own and with the default: each job's rows and maps are those of a call with that job alone, and the
    host path's."""
    jobs = E.shared_jobs()
    packed = E.pack(jobs)
    rec = packed[0]["cell"]
    want = E.run(host, packed)
    for workspace_bytes in (20_000, 1, 0):
        got = E.run(hip_ctx, packed, workspace_bytes=workspace_bytes)
        assert E.same(got, want), (workspace_bytes, E.C.first_difference(got, want))
    for k, job in enumerate(jobs):
        out, levels, maps = E.run(hip_ctx, E.pack([job]))
        L, first = len(job.betas), int(rec["level_first"][k])
        assert out[0].tobytes() == want[0][int(rec["out"][k])].tobytes() and levels.tobytes() == want[1][first:first + L].tobytes()
        if job.map:
            at = int(rec["map_first"][k])
            assert maps.tobytes() == want[2][at:at + (L + 1) * job.voxels].tobytes()


def test_pw_erfc_device_bits(hip_ctx, host):
    """pw_erfc on the sweep of the host test: the device's bits are the host build's."""
    x = E.erfc_sweep()
    assert hip_ctx.erfc(x).tobytes() == host.erfc(x).tobytes()


def test_poisoned_workspaces(hip_ctx, host):
    """The workspace and the compact result filled with 0xFF before the first kernel, right after a call of other shapes:
    the same bytes, and entries nobody owns untouched."""
    jobs = jobs_of_the_host_tests() + E.shared_jobs()
    packed = E.pack(jobs, hole=1)
    want = E.run(host, packed)
    for workspace_bytes in (20_000, 0):
        E.run(hip_ctx, E.pack([E.wide_job()]))
        S.set_poison(True)
        got = E.run(hip_ctx, packed, workspace_bytes=workspace_bytes)
        S.set_poison(False)
        assert E.same(got, want), (workspace_bytes, E.C.first_difference(got, want))
    rows = np.frombuffer(want[0].tobytes(), dtype=np.uint8).reshape(len(want[0]), -1)
    assert (rows == E.SENTINEL).all(axis=1).sum() == len(jobs)


def test_the_public_layer_on_the_device():
    """pw.ewald_potential of rock salt and the charged field of a made-up cell with CO2: the device's bytes are the host
    path's, through ewald_parameters' rows (242 and about 600 of them) and the Python plan."""
    import pywindow_amd as pw
    import test_ewald_host as H

    dev, ref = (H.rock_salt(5.0, 1e-6, device=d) for d in (0, -1))
    assert dev.phi.tobytes() == ref.phi.tobytes() and dev.n_k == ref.n_k > 100
    elements, xyz, lattice, q = H.made_up_cell()
    kw = dict(guest="CO2", temperatures=[250.0, 350.0], spacing=1.0, cutoff=6.0, directions=pw.sphere_directions(6), charges=q)
    dev, ref = (pw.rigid_guest_field(xyz, elements, lattice, device=d, **kw) for d in (0, -1))
    assert dev.raw.tobytes() == ref.raw.tobytes() and dev.levels.tobytes() == ref.levels.tobytes()
    assert dev.zbar.tobytes() == ref.zbar.tobytes() and dev.u_min_map.tobytes() == ref.u_min_map.tobytes()
