"""The elementary functions of csrc/pw_math.hpp on gfx950 against the host path (device = -1), BIT FOR BIT, on the sets
of tests/_math_cases.py: every threshold of sin / cos, every entry of the device copies of SC_TAB, POW_LOG_TAB and
POW_EXP_TAB, every entry of the reciprocal-square-root table the context uploaded, the fall-backs of the wrappers, the
device's sqrt and division.  tests/test_math_edges.py holds the host path to the C library and numpy."""
import numpy as np
import pytest

import _math_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from pywindow_amd import _lib

    return _lib.Context(-1)


@pytest.mark.parametrize("name", M.SET_NAMES)
def test_device_equals_host_bit_for_bit(hip_ctx, host, name):
    which, x, y = M.sets()[name]
    dev = M.internal_math(hip_ctx, which, x, y)
    ref = M.internal_math(host, which, x, y)
    # the raw 64-bit patterns, for every argument; a NaN on one side needs a NaN on the other (payload not compared)
    same = (M.bits(dev) == M.bits(ref)) | (np.isnan(dev) & np.isnan(ref))
    if not same.all():
        k = int(np.flatnonzero(~same)[0])
        second = "" if y is None else f", y = {float(y[k]).hex()} (bits {int(M.bits(y)[k]):#018x})"
        raise AssertionError(
            f"{M.NAMES[which]} [{name}]: device and host differ on {int((~same).sum())} of {len(x)} arguments; first: "
            f"x = {float(x[k]).hex()} (bits {int(M.bits(x)[k]):#018x}){second}: device {int(M.bits(dev)[k]):#018x} "
            f"({dev[k]!r}), host {int(M.bits(ref)[k]):#018x} ({ref[k]!r})")
    again = M.internal_math(hip_ctx, which, x, y)
    assert again.tobytes() == dev.tobytes(), f"{M.NAMES[which]} [{name}]: a second identical call returned other bytes"


def test_empty_and_null_arrays_never_launch(hip_ctx):
    x = np.ones(4)
    out = np.full(4, -77.0)
    assert M.internal_math_rc(hip_ctx, M.SIN, None, None, 0, None) == 0
    assert M.internal_math_rc(hip_ctx, M.DIV, x, x, 0, out) == 0
    for rc in (M.internal_math_rc(hip_ctx, M.SIN, None, None, 4, out), M.internal_math_rc(hip_ctx, M.SIN, x, None, 4, None),
               M.internal_math_rc(hip_ctx, M.POW, x, None, 4, out), M.internal_math_rc(hip_ctx, M.DIV, x, None, 4, out),
               M.internal_math_rc(hip_ctx, 9, x, x, 4, out), M.internal_math_rc(hip_ctx, -1, x, x, 4, out),
               M.internal_math_rc(hip_ctx, M.SIN, x, None, -1, out)):
        assert rc == M.PW_E_BAD_ARG
    assert (out == -77.0).all()
    # a function of one argument ignores y
    assert M.internal_math(hip_ctx, M.SQRT, np.array([4.0, 9.0]), None).tolist() == [2.0, 3.0]
