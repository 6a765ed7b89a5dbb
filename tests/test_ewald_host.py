"""pw_rigid_cell_ewald on the host path (device = -1): the uncharged job is pw_rigid_cell's bytes, the alpha = 0, K = 0
job on an orthorhombic cell is charged pw_rigid_affinity's bytes, the charged job against a plain numpy restatement of
the definition, the Ewald potential of rock salt by its symmetries and against a converged sum, the skip, pw_erfc, the
refusals and the public layer.  tests/test_ewald_gpu.py holds the device to this path byte for byte."""
import math

import numpy as np
import pytest

import _ewald_cases as E
import _rigid_cell_cases as C

import pywindow_amd as pw
from pywindow_amd import _lib
from pywindow_amd.rigid import COULOMB

#: pw_erfc against the C library's erfc: the largest error measured over E.erfc_sweep() (pw_math.hpp records it)
ERFC_MEASURED_ULPS = 3.0


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=16)


def test_an_uncharged_job_is_pw_rigid_cell_byte_for_byte(host):
    """charged = 0 through the new entry, with a charge column, site charges, cell atoms, rows and an alpha that would all
    change the result: out row, levels and maps are pw_rigid_cell's bytes."""
    job = E.skew_job().replace(charged=0)
    got = E.run(host, E.pack([job]))
    rc, want = C.raw(host, C.pack([job.uncharged_case()]))
    assert rc == 0 and E.same(got, want), C.first_difference(got, want)
    assert not E.same(E.run(host, E.pack([E.skew_job()])), want)     # (and the charged job is another result)


def test_alpha_zero_without_rows_is_charged_pw_rigid_affinity(host):
    """step = (h, 0, h, 0, 0, h), alpha = 0, K = 0, charged = 1: erfc(0) is exactly 1 and (C * 1) / r == C / r, so the out row,
    the levels, and per voxel zbar at the map's level and the lowest pose energy are charged pw_rigid_affinity's bytes
    over the whole grid."""
    d, h = (6, 5, 7), 0.7
    inputs = E.make_inputs(25, 3, 4, d, C.ortho(h), 47, K=0, pad=1.5, origin=(0.2, -0.1, 0.3))
    job = E.Job("cage", inputs, d, origin=(0.2, -0.1, 0.3), step=C.ortho(h), core2=0.04, cutoff2=6.25, betas=(0.4, 0.9), alpha=0.0)
    out, levels, maps = E.run(host, E.pack([job]))
    rec = np.zeros(1, dtype=_lib.RIGID_JOB_DTYPE)
    rec[0] = (0, len(inputs.xyz), 0, -1, 0, 2, 0, 3, 0, 4, 0, 0, 0, job.origin, h, job.core2, job.cutoff2, *d, 1, 1, 0)
    w_out, w_levels, w_maps = host.rigid_affinity(rec, inputs.xyz, inputs.coef.reshape(-1, 3), inputs.offsets, inputs.dirs, job.betas,
                                                  maps=np.zeros(2 * job.voxels))
    assert out.tobytes() == w_out.tobytes() and levels.tobytes() == w_levels.tobytes()
    planes = maps.reshape(3, -1)
    assert planes[1].tobytes() == w_maps[0::2].tobytes() and planes[2].tobytes() == w_maps[1::2].tobytes()
    assert np.isfinite(planes[2]).any() and int(out["n_blocked_poses"][0]) > 0


def test_a_charged_job_against_numpy(host):
    """The charged skew job (40 listed atoms, 3 sites, 3 directions, 20 rows) against E.reference: every atom, no skip,
    math.erfc, the reciprocal sum by complex exponentials at the voxel centres.  Dead voxels and blocked poses are equal
    exactly.  The tolerance is measured, as the error of erfc and of the sines times the number of terms cannot be
    derived tighter: the largest difference on umin_v was 4.02e-16 and on zbar 3.45e-15 of the largest entry of the
    plane; the test allows ten times each."""
    job = E.skew_job()
    out, levels, maps = E.run(host, E.pack([job]))
    planes, n_blocked, n_dead, _ = E.reference(job)
    got = maps.reshape(planes.shape)
    assert int(out["n_blocked_poses"][0]) == n_blocked > 0 and int(out["n_dead"][0]) == n_dead > 0
    assert np.array_equal(np.isinf(got[-1]), np.isinf(planes[-1]))
    live = np.isfinite(planes[-1])
    rel_u = float((np.abs(got[-1][live] - planes[-1][live]) / np.abs(planes[-1][live]).max()).max())
    rel_z = float(max((np.abs(got[b] - planes[b]) / planes[b].max()).max() for b in range(len(job.betas))))
    print(f"charged job against numpy: umin_v {rel_u:.3g}, zbar {rel_z:.3g}")
    assert rel_u <= 10 * 4.02e-16 and rel_z <= 10 * 3.45e-15
    assert abs(float(out["u_min"][0]) - planes[-1].min()) <= 10 * 4.02e-16 * np.abs(planes[-1][live]).max()


A = 5.64
ROCK_SALT = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, .5]]) * A
ROCK_SALT_Q = np.array([1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0])


def rock_salt(cutoff, tolerance, device=-1):
    """The potential on the 8 x 8 x 8 grid of the cubic cell, an ion at the centre of voxel (0, 0, 0)."""
    h = A / 8
    return pw.ewald_potential(ROCK_SALT + 0.5 * h, ROCK_SALT_Q, np.eye(3) * A, spacing=h, cutoff=cutoff, tolerance=tolerance,
                              device=device)


def test_rock_salt_by_symmetry():
    """An 8-atom NaCl cell, a = 5.64, charges +-1, a real-space cutoff of 5 (no shell of neighbours of the points below is
    within 1e-3 of it).  (2, 2, 2) is the tetrahedral site, equally far from the two sublattices: the potential is zero
    by symmetry, both truncations are symmetric and only rounding remains -- a few hundred terms of order COULOMB / a at
    2^-53 each, against a bound of 1e-10 COULOMB / a.  Points that a symmetry of the crystal maps onto each other agree
    to the same bound: (4, 0, 0) and (0, 4, 0) are ions, (1, 2, 3) and (3, 2, 1) lie on a plane where the potential is
    zero, (1, 0, 3), (3, 0, 1) and (0, 1, 3) are general points."""
    P = rock_salt(5.0, 1e-6)
    assert tuple(P.shape) == (8, 8, 8) and P.n_k > 100
    bound = 1e-10 * COULOMB / A
    phi = P.phi                                                      # (nz, ny, nx)
    at = lambda i, j, l: float(phi[l, j, i])
    assert abs(at(2, 2, 2)) <= bound
    for a, b in (((4, 0, 0), (0, 4, 0)), ((1, 2, 3), (3, 2, 1)), ((1, 0, 3), (3, 0, 1)), ((1, 0, 3), (0, 1, 3))):
        assert at(*a) == at(*b) or abs(at(*a) - at(*b)) <= bound, (a, b, at(*a), at(*b))
    assert at(0, 0, 0) == np.inf and at(4, 0, 0) == np.inf           # (the ions themselves are inside the core)
    assert abs(at(1, 0, 3)) > 1.0 and abs(at(1, 0, 0) + at(5, 0, 0)) <= bound   # (a real potential; the ion swap flips its sign)
    assert np.abs(P.positions()[0, 0, 0] - 0.5 * A / 8).max() < 1e-12


def converged_rock_salt(points):
    """A plain numpy Ewald sum at tolerance 1e-14: alpha = 1.2, real space over the images within 5 cells, reciprocal space
    over the full lattice up to |index| 9."""
    alpha = 1.2
    erfc = np.vectorize(math.erfc)
    shifts = np.array([[i, j, k] for i in range(-5, 6) for j in range(-5, 6) for k in range(-5, 6)], dtype=np.float64) * A
    idx = np.array([[i, j, k] for i in range(-9, 10) for j in range(-9, 10) for k in range(-9, 10) if (i, j, k) != (0, 0, 0)])
    kv = 2.0 * math.pi * idx / A
    k2 = (kv * kv).sum(axis=1)
    w = COULOMB * (4.0 * math.pi / A ** 3) * np.exp(-k2 / (4.0 * alpha * alpha)) / k2
    rho = (ROCK_SALT_Q[None, :] * np.exp(1j * (kv @ ROCK_SALT.T))).sum(axis=1)
    out = []
    for p in points:
        r = np.linalg.norm(p[None, None, :] - ROCK_SALT[None, :, :] - shifts[:, None, :], axis=2)
        out.append(COULOMB * (ROCK_SALT_Q[None, :] * erfc(alpha * r) / r).sum() + (w * (rho * np.exp(-1j * (kv @ p))).real).sum())
    return np.array(out)


def test_the_potential_does_not_depend_on_alpha():
    """Rock salt at tolerance 1e-8 with the cutoffs 4.0 and 5.5 (alpha 1.07 and 0.78) at every voxel outside the cores,
    against a converged numpy Ewald sum at tolerance 1e-14.  Measured: the largest difference was 1.18e-6 kJ/mol/e at cutoff
    4.0 and 2.07e-7 at 5.5 (4.8e-9 and 8.4e-10 of COULOMB / a); the test allows ten times each, which is below the 1e-6
    COULOMB / a = 2.5e-4 that the parameter rule of ewald_parameters must meet."""
    h = A / 8
    measured = {4.0: 1.18e-6, 5.5: 2.07e-7}
    want = None
    for cutoff in (4.0, 5.5):
        P = rock_salt(cutoff, 1e-8)
        free = np.isfinite(P.phi)
        if want is None:
            l, j, i = np.nonzero(free)
            want = converged_rock_salt(np.stack([i, j, l], axis=1) * h)      # (relative to the ion at voxel (0, 0, 0))
        worst = float(np.abs(P.phi[free] - want).max())
        print(f"cutoff {cutoff}: alpha {P.alpha:.4f}, {P.n_k} rows, largest difference {worst:.3g}")
        assert free.sum() > 400 and worst <= 10 * measured[cutoff] <= 1e-6 * COULOMB / A


def test_the_skip_changes_no_byte(host):
    """The internal switch of pw_rigid_cell on a charged job whose listed atoms lie up to 5 beyond the cell at a cutoff of
    1.5: the same bytes with the skip on and off, and fewer pair terms with it."""
    packed = E.pack([E.skip_job()])
    on, off = [], []
    got = E.run(host, packed, diagnostics=on)
    assert E.same(got, E.run(host, packed, diagnostics=off, skip=False))
    assert 0 < on[0][0][0] < off[0][0][0] // 2 and np.isfinite(got[2]).any()


def test_pw_erfc(host):
    """Exactly 1.0 at 0, never NaN, non-increasing over the sweep (0, every piece boundary with both neighbours, the onset
    of the denormals, 2^21 and 10^5 log-spaced points), +0.0 or a denormal where the C library's value is below the
    normal numbers, and elsewhere within twice the measured largest error of 3.0 ulps of the C library's erfc."""
    x = E.erfc_sweep()
    got = host.erfc(x)
    assert got[0] == 1.0 and x[0] == 0.0 and not np.isnan(got).any() and not np.signbit(got).any()
    assert (np.diff(got) <= 0.0).all(), x[1:][np.diff(got) > 0.0][:5]
    worst, beyond = E.erfc_ulps(got, x)
    print(f"pw_erfc: largest error {worst:.3f} ulp")
    assert worst <= 2 * ERFC_MEASURED_ULPS
    assert beyond.sum() > 100 and (got[beyond] < 2.2250738585072014e-308).all() and got[-1] == 0.0 and x[-1] == 2.0 ** 21


def test_refusals(host):
    """Job 1 of two is refused, the message names it, and nothing is written."""
    jobs = [E.skew_job(), E.wide_job()]

    def refused(reason, field=None, value=None, edit=None, sizes=None):
        packed = list(E.pack(jobs))
        packed[0] = packed[0].copy()
        if field:
            (packed[0]["cell"] if field in _lib.RIGID_CELL_JOB_DTYPE.names else packed[0])[field][1] = value
        if edit:
            edit(packed)
        for q, n in (sizes or {}).items():
            packed[q] = packed[q][:n]
        out, levels, maps = C.blank(packed[11], packed[10], packed[9])
        blank = [a.copy() for a in (out, levels, maps)]
        with pytest.raises(ValueError, match=r"pw_rigid_cell_ewald: job 1: .*" + reason):
            host.rigid_cell_ewald(*packed[:9], out=out, levels=levels, maps=maps)
        assert E.same((out, levels, maps), blank)

    def kvec(column, value):
        def edit(p):
            p[8] = p[8].copy()
            p[8][int(p[0]["k_first"][1]) + 3, column] = value
        return edit

    refused("alpha is not finite", "alpha", np.nan)
    refused("alpha is not finite", "alpha", np.inf)
    refused("alpha < 0", "alpha", -0.1)
    refused("n_k outside 0 .. PW_EWALD_MAX_K", "n_k", E.MAX_K + 1)
    refused("n_k outside 0 .. PW_EWALD_MAX_K", "n_k", -1)
    refused("an index of a row is not an integer within", edit=kvec(1, E.MAX_INDEX + 1.0))
    refused("an index of a row is not an integer within", edit=kvec(0, 1.5))
    refused("an index of a row is not an integer within", edit=kvec(2, np.nan))
    refused("a weight is not finite", edit=kvec(3, np.inf))
    refused("cell atoms outside cell", "cell_first", -1)
    refused("cell atoms outside cell", sizes={7: len(E.skew_job().inputs.cell) + len(E.wide_job().inputs.cell) - 1})
    refused("rows outside kvecs", sizes={8: 20 + 65 - 1})
    refused("site charges outside site_q", sizes={6: 3})
    refused("charged is neither 0 nor 1", "charged", 2)
    refused("shares its row of out with an earlier job", "out", 0)
    refused("shares rows of levels with an earlier job", "level_first", 1)
    refused("shares maps with an earlier job", "map_first", 5)
    def charge_term(p):
        p[2] = p[2].copy()
        p[2][int(p[0]["cell"]["coef_first"][1]) + 1, 2] = np.nan

    refused("a charge term is not finite", edit=charge_term)
    refused("cutoff2 is 0", "cutoff2", 0.0)                         # (and what pw_rigid_cell refuses)
    # an uncharged job reads none of it
    packed = list(E.pack([j.replace(charged=0) for j in jobs]))
    packed[0] = packed[0].copy()
    packed[0]["alpha"], packed[0]["n_k"], packed[0]["cell_first"] = np.nan, 10 ** 6, -5
    assert np.isfinite(host.rigid_cell_ewald(*packed[:9])[1]["z"]).all()


def made_up_cell():
    """A 10 Angstrom cubic cell with six atoms along two rods, an open channel beside them; charges that sum to zero."""
    elements = ["C", "O", "C", "O", "N", "H"]
    xyz = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.5], [1.0, 1.0, 8.0], [6.0, 1.5, 2.0], [6.0, 1.5, 5.5], [6.0, 1.5, 9.0]])
    return elements, xyz, np.eye(3) * 10.0, np.array([0.6, -0.7, 0.5, -0.6, -0.3, 0.5])


def test_the_public_layer():
    """charges=None is the present call byte for byte; with charges the tensors are finite and other tensors; a framework
    that is not neutral and charges="qeq" are refused; ewald_parameters names the tolerance that fits."""
    elements, xyz, lattice, q = made_up_cell()
    kw = dict(guest="CO2", temperatures=[250.0, 350.0], spacing=1.0, cutoff=6.0, directions=pw.sphere_directions(6), device=-1)
    plain = pw.rigid_guest_diffusion(xyz, elements, lattice, **kw)
    again = pw.rigid_guest_diffusion(xyz, elements, lattice, charges=None, **kw)
    assert plain.tensor.tobytes() == again.tensor.tobytes() and plain.raw.tobytes() == again.raw.tobytes()
    charged = pw.rigid_guest_diffusion(xyz, elements, lattice, charges=q, **kw)
    assert np.isfinite(charged.tensor).all() and charged.tensor.shape == (2, 3, 3) and np.abs(charged.tensor).max() > 0.0
    assert not np.array_equal(charged.tensor, plain.tensor)
    field = pw.rigid_guest_field(xyz, elements, lattice, charges=q, **kw)
    rows = pw.rigid_guest_field(xyz[None], elements, lattice, charges=q[None], **kw)
    assert field.zbar.tobytes() == rows.zbar[0].tobytes()
    assert field.zbar.tobytes() != pw.rigid_guest_field(xyz, elements, lattice, **kw).zbar.tobytes()
    assert len(pw.rigid_guest_percolation(xyz, elements, lattice, charges=q, **kw)) == 2
    with pytest.raises(ValueError, match="not neutral"):
        pw.rigid_guest_field(xyz, elements, lattice, charges=q + 1e-6, **kw)
    with pytest.raises(ValueError, match="isolated-molecule model"):
        pw.rigid_guest_field(xyz, elements, lattice, charges="qeq", **kw)
    with pytest.raises(ValueError, match="one value per atom"):
        pw.rigid_guest_field(xyz, elements, lattice, charges=q[:5], **kw)
    alpha, kv = pw.ewald_parameters(lattice, 6.0, 1e-6)
    assert alpha == math.sqrt(-math.log(1e-6)) / 6.0 and len(kv) <= _lib.EWALD_MAX_K
    assert (kv[:, 0] >= 0).all() and len({tuple(r) for r in kv[:, :3]} | {tuple(-r) for r in kv[:, :3]}) == 2 * len(kv)
    assert [tuple(r) for r in kv[:, :3]] == sorted(tuple(r) for r in kv[:, :3])
    with pytest.raises(ValueError, match=r"the tolerance that fits is \d"):
        pw.ewald_parameters(np.eye(3) * 25.0, 8.0, 1e-8)
