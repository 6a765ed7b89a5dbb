"""Shape and circumcircle kernels on the device at their edges (tests/_shape_cases.py): pw_shape_kernel and
pw_circumcircle_kernel on gfx950 against the host build of the same source (tests/hostsim/shape_probe.cpp,
both with -ffp-contract=off), BIT FOR BIT.  That equality carries tests/test_shape.py's results (tensors
equal to the oracle, eigenvalues against 50 digits) over to the device.  numpy only.

A NaN matches a NaN whatever its sign bit: IEEE 754 leaves the sign of an invalid operation's NaN open, so
x86 and gfx950 need not agree on it.  Every other bit is compared, the signs of zeros and infinities included.

The GPU time of each test (its device calls) is printed; the docstrings give what one MI355X measured."""
import ctypes
import time

import numpy as np
import pytest

import _shape_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hostsim):
    return ctypes.CDLL(str(hostsim / "libshapeprobe.so"))


def same_values(a, b):
    """Bit for bit, except that any NaN matches any NaN at the same place."""
    a = np.ascontiguousarray(a).reshape(-1).view(np.float64)
    b = np.ascontiguousarray(b).reshape(-1).view(np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return bool(np.array_equal(a.view(np.uint64)[keep], b.view(np.uint64)[keep]))


def device_shape(ctx, off, xyz, mass):
    from pywindow_amd import _lib

    t0 = time.perf_counter()
    out = ctx.shape(_lib.Batch(off, xyz, np.ones(len(mass)), mass))
    return out, time.perf_counter() - t0


def _device_host_oracle(ctx, L, mols):
    """One device call for `mols`: records equal to the host build's, tensors equal to the oracle's (block-wise
    above N = 8193).  Returns the device call's time."""
    from oracle import pw_shape as S

    packed = C.pack(mols)
    got, gpu_s = device_shape(ctx, *packed)
    want = C.host_shape(L, *packed)
    for u, (tag, x, m) in enumerate(mols):
        assert same_values(got[u:u + 1].view(np.float64), want[u:u + 1].view(np.float64)), tag
        inertia = S.inertia_tensor(x, m) if len(x) <= C.ORACLE_MAX_N else C.block_inertia(x, m)
        assert np.array_equal(got[u]["gyration"], S.gyration_tensor(x, m)), f"{tag}: gyration tensor"
        assert np.array_equal(got[u]["inertia"], inertia), f"{tag}: inertia tensor"
    return gpu_s


def test_hard_molecules_and_sizes_device_equals_host_and_oracle(hip_ctx, L):
    """Every hard molecule (one batch) and every size up to N = 8193 around numpy's blocks (one batch): the
    device's records equal the host build's, and the tensors equal the oracle's.  GPU time on one MI355X:
    1.46 s for the two calls, most of it the units of 8191 to 8193 atoms."""
    gpu_s = _device_host_oracle(hip_ctx, L, C.hard_molecules())
    gpu_s += _device_host_oracle(hip_ctx, L, C.sized_molecules(max_n=C.ORACLE_MAX_N))
    print(f"\ndevice calls: {gpu_s:.3f} s")


def test_largest_size_device_equals_host_and_oracle(hip_ctx, L):
    """The sizes above N = 8193 (N = 16411: 2.7e8 terms in each of the six inertia sums, one workgroup), on
    their own: the device's record equals the host build's, the tensors equal the block-wise oracle.  GPU
    time on one MI355X: 5.87 s for the call; the host build and the block-wise oracle take longer."""
    big = [m for m in C.sized_molecules() if len(m[1]) > C.ORACLE_MAX_N]
    assert big
    print(f"\ndevice call: {_device_host_oracle(hip_ctx, L, big):.3f} s")


def test_template_batches_equal_per_atom_masses(hip_ctx):
    """The hard molecules as template batches (one mass table per (shape, mass variant)) give the same bits
    as the same units sent with per-atom masses.  GPU time on one MI355X: 0.017 s for the 52 calls."""
    from pywindow_amd import _lib

    mols = C.hard_molecules()
    gpu_s = 0.0
    for tag, coords, mass, idx in C.template_groups(mols):
        t0 = time.perf_counter()
        tmpl = hip_ctx.shape(_lib.Batch.uniform(coords, np.ones(len(mass)), mass))
        gpu_s += time.perf_counter() - t0
        per_atom, s = device_shape(hip_ctx, *C.pack([mols[i] for i in idx]))
        gpu_s += s
        assert len(tmpl) == len(idx) >= C.ROTATIONS
        assert same_values(tmpl.view(np.float64), per_atom.view(np.float64)), tag
    print(f"\ndevice calls: {gpu_s:.3f} s")


def test_large_batch_device_equals_host_and_splits(hip_ctx, L):
    """LARGE_BATCH_UNITS (> 4096) units in one call: the grid strides, workgroups reuse their scratch.  Same
    bits as the host build, and as the same units sent in batches of at most 4096.  GPU time on one MI355X:
    0.008 s for the three calls."""
    off, xyz, mass = C.large_batch()
    assert len(off) - 1 > 4096
    got, gpu_s = device_shape(hip_ctx, off, xyz, mass)
    assert same_values(got.view(np.float64), C.host_shape(L, off, xyz, mass).view(np.float64))
    parts = []
    for u0, u1 in ((0, 4096), (4096, len(off) - 1)):
        o = off[u0:u1 + 1]
        part, s = device_shape(hip_ctx, o - o[0], xyz[o[0]:o[-1]], mass[o[0]:o[-1]])
        gpu_s += s
        parts.append(part)
    assert same_values(got.view(np.float64), np.concatenate(parts).view(np.float64))
    print(f"\ndevice calls: {gpu_s:.3f} s")


def test_circumcircle_triples_device_equals_host(hip_ctx, L):
    """N_TRIPLES triples in one call (not a multiple of the 64-lane block): diameters and centres equal the
    host build's, the places and signs of infinities and the places of NaNs included.  GPU time on one MI355X:
    0.002 s."""
    xyz, sets = C.circumcircle_triples()
    assert len(sets) >= 100_000 and len(sets) % 64
    t0 = time.perf_counter()
    d, c = hip_ctx.circumcircle(xyz, sets)
    gpu_s = time.perf_counter() - t0
    hd, hc = C.host_circumcircle(L, xyz, sets)
    assert np.isnan(hd).any() and np.isinf(hd).any() and np.isinf(hc).any()
    assert same_values(d, hd)
    assert same_values(c, hc)
    print(f"\ndevice call: {gpu_s:.3f} s, {np.isnan(d).sum()} NaN / {np.isinf(d).sum()} infinite diameters")


def test_refused_arguments_write_nothing(hip_ctx):
    """An empty unit, a unit of 46341 atoms, a template of another size than a unit, a triple index out of
    range: each returns PW_E_BAD_ARG and leaves the outputs as they were.  Nothing is launched but one
    three-atom circumcircle at the end."""
    from pywindow_amd import _lib

    lib = _lib.load()
    E_BAD_ARG = -2
    rng = np.random.default_rng(3)

    def shape_rc(batch):
        out = np.full(batch.n_units, np.nan, dtype=_lib.SHAPE_OUT_DTYPE)
        out.view(np.uint64)[:] = 0x7FF4DEADBEEF0001            # a signalling-NaN pattern nothing computes
        before = out.tobytes()
        rc = lib.pw_shape_batch(hip_ctx._h, ctypes.byref(batch.c), out.ctypes.data)
        return rc, out.tobytes() == before

    x3 = rng.normal(0.0, 3.0, (3, 3))
    empty = _lib.Batch(np.array([0, 3, 3, 6]), np.vstack([x3, x3]), np.ones(6), np.ones(6))
    big = _lib.Batch(np.array([0, 3, 3 + 46341]), rng.normal(0.0, 20.0, (3 + 46341, 3)), np.ones(46344), np.ones(46344))
    tmpl = _lib.Batch(np.array([0, 3, 6, 10]), rng.normal(0.0, 3.0, (10, 3)), np.ones(3), np.ones(3), template_atoms=3)
    for tag, batch in (("empty unit", empty), ("46341 atoms", big), ("template size", tmpl)):
        assert shape_rc(batch) == (E_BAD_ARG, True), tag

    xyz = np.ascontiguousarray(rng.normal(0.0, 3.0, (5, 3)))
    for bad in (5, -1):
        sets = np.ascontiguousarray(np.array([[0, 1, 2]] * 70 + [[0, bad, 2]], dtype=np.int32))
        d = np.full(len(sets), 7.0)
        c = np.full((len(sets), 3), 7.0)
        rc = lib.pw_circumcircle(hip_ctx._h, xyz.ctypes.data, len(xyz), sets.ctypes.data, len(sets),
                                 d.ctypes.data, c.ctypes.data)
        assert rc == E_BAD_ARG and (d == 7.0).all() and (c == 7.0).all(), bad
    # the context is still good
    d, _ = hip_ctx.circumcircle(xyz, [[0, 1, 2]])
    assert np.isfinite(d).all()
