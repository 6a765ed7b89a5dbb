"""Essential dynamics on the host path (device = -1): pywindow_amd.principal_modes, Modes and DLPOLY.essential_dynamics
against a trajectory with planted modes and against the same pipeline in numpy.  tests/test_gpu_cov.py holds the
device to the host path's bytes."""
import numpy as np
import pytest

import _cov_cases as C
import pywindow_amd as pw
from pywindow_amd import synth

LD = np.longdouble
U = 2.0 ** -53
F, N = 400, 12
SIGMA = 1e-6


def kabsch(x, y):
    """The proper rotation R and the centres with R (x - cx) + cy on y in the least-squares sense (numpy SVD)."""
    cx, cy = x.mean(axis=0), y.mean(axis=0)
    u, _, vt = np.linalg.svd((x - cx).T @ (y - cy))
    d = np.sign(np.linalg.det(u @ vt))
    return (u @ np.diag([1.0, 1.0, d]) @ vt).T, cx, cy


def planted():
    """A rigid base of 12 atoms, two orthonormal displacement fields and their amplitudes.  Both fields are orthogonal
    to the six rigid-body motions of the base, and sum_i u1_i x u2_i = 0.  Then, for every frame b + a1 u1 + a2 u2 and
    every target b + c1 u1 + c2 u2, the matrix sum_i (y_i - cy)(m_i - cm)^T is symmetric EXACTLY (b x b = 0, the terms
    linear in u vanish by the orthogonality, the term u1 x u2 by construction): the identity is the least-squares
    rotation whatever the amplitudes, not only to first order, and the superposition undoes the rotation a frame was
    given up to the noise alone."""
    rng = np.random.default_rng(11)
    base = 3.0 * rng.standard_normal((N, 3))
    base -= base.mean(axis=0)
    rigid = [np.tile(np.eye(3)[k], (N, 1)) for k in range(3)] + [np.cross(np.eye(3)[k], base) for k in range(3)]

    def field(extra):
        rows = np.array([r.reshape(-1) for r in rigid + extra])
        v = rng.standard_normal(3 * N)
        v -= np.linalg.pinv(rows) @ (rows @ v)              # out of the span of the rows
        return (v / np.linalg.norm(v)).reshape(N, 3)

    u1 = field([])
    # sum_i u1_i x u2_i = 0 is linear in u2: component k is sum_i (e_k x u1_i) . u2_i, up to sign
    u2 = field([u1] + [np.cross(np.eye(3)[k], u1) for k in range(3)])
    t = np.arange(F)
    a = np.stack([0.5 * np.sin(2 * np.pi * t / 17.3), 0.1 * np.cos(2 * np.pi * t / 7.1)], axis=1)
    noise = SIGMA * rng.standard_normal((F, N, 3))
    clean = base + a[:, 0, None, None] * u1 + a[:, 1, None, None] * u2
    coords = np.empty((F, N, 3))
    for f in range(F):
        coords[f] = (clean[f] + noise[f]) @ C.random_rotation(rng).T + rng.uniform(-20, 20, 3)
    return base, u1, u2, a, noise, coords


@pytest.fixture(scope="module")
def world():
    base, u1, u2, a, noise, coords = planted()
    return {"base": base, "u1": u1, "u2": u2, "a": a, "noise": noise, "coords": coords,
            "modes": pw.principal_modes(coords, n_modes=4, device=-1)}


def bars(world):
    """The bars of the planted test, from the noise-to-gap ratio.

    The sample covariance G (2 x 2) of the amplitudes has eigenvalues l1 > l2 and eigenvectors w_k; the ideal
    covariance of the superposed frames is sum_k l_k p_k p_k^T with p_k = w_k[0] u1 + w_k[1] u2 (in the orientation of
    the mean structure), of rank 2.  What is measured is the covariance of signal + N', N' the noise as the
    superposition leaves it: its rigid-body part removed (a projection, which does not lengthen it) and terms of second
    order in noise / size added, for which a factor 2 is kept: |N'|_2 <= 2 |N|_2.  So
        |E|_2 = |C - C_ideal|_2 <= (2 |S|_2 |N'|_2 + |N'|_2^2) / (F - 1),   |S|_2 = sqrt((F - 1) l1).
    Davis-Kahan (in the form of Yu, Wang and Samworth 2015): sin angle(v_k, p_k) <= 2 |E|_2 / gap_k with gap_1 =
    l1 - l2 and gap_2 = min(l1 - l2, l2); for unit vectors with v . p >= 0, |v - p| = 2 sin(angle / 2) <= sqrt(2) sin.
    The orientation of the mean structure is found in the test by a Kabsch fit of the ideal mean onto it; the mean
    of the N' over the frames is at most |N'|_2 / sqrt(F) long, and a displacement eta can pass for a rotation by at
    most |eta| / sqrt(I_min), I_min the smallest moment of inertia of the base (a rotation by phi about axis k moves
    the structure by phi sqrt(I_k)); a field of unit length rotated by phi moves by at most phi."""
    a, noise = world["a"], world["noise"].reshape(F, -1)
    lam, w = np.linalg.eigh(np.cov(a.T))
    lam, w = lam[::-1], w[:, ::-1]
    n2 = 2.0 * np.linalg.norm(noise - noise.mean(axis=0), 2)
    E = (2.0 * np.sqrt((F - 1) * lam[0]) * n2 + n2 * n2) / (F - 1)
    gaps = (lam[0] - lam[1], min(lam[0] - lam[1], lam[1]))
    second = np.linalg.eigvalsh(world["base"].T @ world["base"])
    phi = (n2 / np.sqrt(F)) / np.sqrt(second[0] + second[1])
    return lam, w, E, [np.sqrt(2.0) * 2.0 * E / g + phi for g in gaps], n2


def test_the_planted_modes_are_found(world):
    md, u1, u2, a = world["modes"], world["u1"], world["u2"], world["a"]
    lam, w, E, bar, n2 = bars(world)
    assert bar[0] < bar[1] < 1e-2                               # (the bars say something)
    ideal_mean = world["base"] + a[:, 0].mean() * u1 + a[:, 1].mean() * u2
    Q, cx, cy = kabsch(ideal_mean, md.mean_structure)
    for k in range(2):
        p = (w[0, k] * u1 + w[1, k] * u2) @ Q.T
        v = md.vectors[k]
        p = p if (p * v).sum() >= 0 else -p
        err = float(np.linalg.norm(v - p))
        print(f"mode {k}: |v - planted| {err:.3e}  bar {bar[k]:.3e}")
        assert err <= bar[k]
        # the projections follow the planted amplitudes: |z_t . (v - p)| + |N'_t . p| + the mean's share
        ideal = (a - a.mean(axis=0)) @ w[:, k] * (1.0 if (v * ((w[0, k] * u1 + w[1, k] * u2) @ Q.T)).sum() >= 0 else -1.0)
        slack = np.abs(a).sum(axis=1).max() * bar[k] + 2.0 * n2
        assert np.abs(md.projection[:, k] - ideal).max() <= slack
    # Weyl: the D - 2 eigenvalues the ideal has at 0 are at most |E|_2 each, the two leading ones at least l_k - |E|_2
    D = 3 * N
    assert 1.0 - md.explained[:2].sum() <= (D - 2) * E / (lam[0] + lam[1] - 2 * E)
    assert np.abs(md.eigenvalues[:2] - lam[:2]).max() <= E and md.eigenvalues[2] <= E
    assert md.eigenvalues.shape == (D,) and (np.diff(md.eigenvalues) <= 0).all() and abs(md.explained.sum() - 1.0) < 1e-12
    assert md.projection.shape == (F, 4) and md.vectors.shape == (4, N, 3) and np.array_equal(md.frames, np.arange(F))


def test_the_mean_iteration_stops_and_says_when(world):
    from pywindow_amd import modes as M
    from pywindow_amd import superposition as SP

    md, coords = world["modes"], world["coords"]
    assert 1 <= md.rounds < M.MEAN_ROUNDS
    # one more round does not move the mean by the tolerance
    rows = SP.superpose_onto(np.concatenate([coords, md.mean_structure[None]]), F, None, device=-1)[:F]
    again, _ = pw.covariance(coords.reshape(F, -1), rows, device=-1, scatter=False)
    m = md.mean_structure
    gyration = np.sqrt(((m - m.mean(axis=0)) ** 2).sum() / N)
    assert np.sqrt(((again.reshape(N, 3) - m) ** 2).sum() / N) < M.MEAN_TOLERANCE * gyration
    # a frame as the reference is one pass and no round; the cap holds for frames that share no structure
    one = pw.principal_modes(coords[:50], reference=3, n_modes=2, device=-1)
    assert one.rounds == 0 and np.abs(one.transforms["centre_target"][0] - coords[3].mean(axis=0)).max() < 1e-13
    wild = pw.principal_modes(np.random.default_rng(2).standard_normal((30, 9, 3)), n_modes=2, device=-1)
    assert 1 <= wild.rounds <= M.MEAN_ROUNDS


def test_eigenvalues_against_the_same_pipeline_in_numpy(world):
    """Align every frame onto frame 0 by numpy's SVD, np.cov, eigvalsh.  Weyl: |l_k - l'_k| <= |dC|_2 <= |dS|_F /
    (F - 1) <= D max|dS_ab| / (F - 1).  dS has two parts.  (1) What tests/test_cov.py allows between ours and reference
    (i) on the same aligned frames: ours within max(8 e_ref, 4 ulp(A_ab)) of the long-double truth and (i) within e_ref,
    e_ref measured here on this very matrix.  (2) The two alignments differ: tests/test_superpose.py holds every entry
    of a rotation within 2^-50 of the truth where the fit is well conditioned, the SVD's likewise, so two rotations
    differ by rho <= 3 * 2 * 2^-50 in the spectral norm; that moves a centred atom at distance <= r by rho r, its mean
    by as much, z by 2 rho r, and an entry of S by at most F (2 |z|_max (2 rho r) + (2 rho r)^2)."""
    coords = world["coords"]
    md = pw.principal_modes(coords, reference=0, n_modes=2, device=-1)
    aligned = np.empty_like(coords)
    for f in range(F):
        R, cx, cy = kabsch(coords[f], coords[0])
        aligned[f] = (coords[f] - cx) @ R.T + cy
    Y = aligned.reshape(F, -1)
    want = np.linalg.eigvalsh(np.cov(Y.T))[::-1]
    Z = Y - Y.mean(axis=0)
    Yt = Y.astype(LD)
    Zt = Yt - Yt.sum(axis=0) / LD(F)
    e_ref = float(np.abs(Z.T @ Z - Zt.T @ Zt).max())
    floor = float(4.0 * np.spacing(np.float64((np.abs(Zt).T @ np.abs(Zt)).max())))
    rho, zmax = 6.0 * 2.0 ** -50, float(np.abs(Z).max())
    r = float(np.linalg.norm(aligned - aligned.mean(axis=1, keepdims=True), axis=2).max())
    entry = max(8.0 * e_ref, floor) + e_ref + F * (2.0 * zmax * 2.0 * rho * r + (2.0 * rho * r) ** 2)
    bar = 3 * N * entry / (F - 1)
    err = float(np.abs(md.eigenvalues - want).max())
    print(f"eigenvalues: largest difference {err:.3e}  bar {bar:.3e}  leading {want[0]:.3e}")
    assert err <= bar and bar < 1e-9 * want[0]


def test_the_sign_rule():
    rng = np.random.default_rng(8)
    md = pw.principal_modes(rng.standard_normal((60, 7, 3)), reference=0, n_modes=21, device=-1)
    for v in md.vectors.reshape(21, -1):
        assert v[np.argmax(np.abs(v))] > 0.0 and abs(np.linalg.norm(v) - 1.0) < 1e-12
    from pywindow_amd.modes import _sign_rule

    assert np.array_equal(_sign_rule(np.array([0.5, -0.5, 0.1])), [0.5, -0.5, 0.1])       # the lowest index among equals
    assert np.array_equal(_sign_rule(np.array([-0.5, 0.5, 0.1])), [0.5, -0.5, -0.1])
    # vectors handed over are taken as they are
    given = pw.principal_modes(rng.standard_normal((60, 7, 3)), reference=0, vectors=-md.vectors[:2], device=-1)
    assert np.array_equal(given.vectors, -md.vectors[:2]) and given.n_modes == 2


def test_rmsf_and_cross_correlation_are_their_definitions(world):
    md = world["modes"]
    S = md.scatter
    trace = np.array([[S[3 * i, 3 * j] + S[3 * i + 1, 3 * j + 1] + S[3 * i + 2, 3 * j + 2] for j in range(N)] for i in range(N)])
    assert np.array_equal(md.rmsf, np.sqrt(np.diag(trace) / F))
    assert np.array_equal(md.cross_correlation, trace / np.sqrt(np.outer(np.diag(trace), np.diag(trace))))
    assert np.array_equal(np.diag(md.cross_correlation), np.ones(N)) and np.array_equal(md.cross_correlation, md.cross_correlation.T)
    assert np.abs(md.cross_correlation).max() <= 1.0 + 8 * U
    mean, scatter = pw.covariance(world["coords"].reshape(F, -1), md.transforms, device=-1)
    assert C.same(scatter, S) and C.same(mean.reshape(N, 3), md.mean_structure)
    assert C.same(md.projection, pw.project(world["coords"].reshape(F, -1), mean, md.vectors.reshape(4, -1), md.transforms, device=-1))


def test_frozen_atoms_give_zero_not_nan():
    """Four copies of one frame: the sums of four equal values and their quarter are exact, so z and S are exactly 0,
    every atom is frozen, and nothing divides 0 by 0."""
    frame = np.random.default_rng(1).standard_normal((5, 3))
    md = pw.principal_modes(np.stack([frame] * 4), n_modes=3, device=-1)
    assert not md.scatter.any() and not md.rmsf.any() and not md.cross_correlation.any() and not md.explained.any()
    assert not np.isnan(md.projection).any() and not md.projection.any() and md.vectors.shape == (3, 5, 3)


def test_series_feeds_the_module_level_functions(world):
    md = world["modes"]
    values, valid = md.series(0)
    assert values.dtype == np.float64 and valid.dtype == bool and valid.all() and np.array_equal(values, md.projection[:, 0])
    tc = pw.time_correlation(values, max_lag=40, valid_a=valid, device=-1)
    assert len(np.asarray(tc.lag)) == 41
    with pytest.raises(IndexError):
        md.series(4)


def test_python_layer_errors():
    x = np.random.default_rng(0).standard_normal((6, 4, 3))
    for bad in (dict(coords=x[:1]), dict(coords=x[:, :, :2]), dict(coords=x, n_modes=0), dict(coords=x, n_modes=13),
                dict(coords=x, reference="median"), dict(coords=x, reference=6), dict(coords=x, frames=[1, 2]),
                dict(coords=x, weights=np.ones(3))):
        with pytest.raises(ValueError):
            pw.principal_modes(device=-1, **bad)
    with pytest.raises(ValueError, match="atoms"):
        pw.principal_modes(np.zeros((2, 1025, 3)), device=-1)


def _history(tmp_path, cell=None):
    elements, base = synth.load_cc3_base()
    rng = np.random.default_rng(6)
    squeezed = base * np.array([1.0, 1.0, 1.06])                     # a second conformation: the cage stretched by 6 %
    frames = [(squeezed if t % 3 == 2 else base) + rng.normal(0.0, 0.005, base.shape) for t in range(9)]
    return pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=cell)), np.array(frames)


def test_essential_dynamics_of_a_trajectory(tmp_path):
    traj, frames = _history(tmp_path)
    md = traj.essential_dynamics(n_modes=3, device=-1)
    n = frames.shape[1]
    assert isinstance(md, pw.Modes) and md.vectors.shape == (3, n, 3) and md.projection.shape == (9, 3)
    assert np.array_equal(md.frames, np.arange(9)) and md.eigenvalues.shape == (3 * n,) and md.rounds >= 1
    # the stretch is the leading mode: it separates the frames t % 3 == 2 from the rest, and carries most of the trace
    side = md.projection[:, 0] > 0
    assert (side == side[2]).sum() == 3 and side[2] == side[5] == side[8] and md.explained[0] > 0.9
    from pywindow_amd.element_data import MASS, element_ids

    coords = traj._rigid_frames("all", "test")[1]
    same = pw.principal_modes(coords, MASS[element_ids(traj.elements(None, None))], n_modes=3, device=-1)
    assert C.same(same.scatter, md.scatter) and C.same(same.projection, md.projection)
    some = traj.essential_dynamics(frames=[1, 2, 5, 8], weights=None, reference=0, n_modes=2, device=-1)
    assert np.array_equal(some.frames, [1, 2, 5, 8]) and some.rounds == 0 and some.projection.shape == (4, 2)


def test_a_periodic_trajectory_is_refused(tmp_path):
    traj, _ = _history(tmp_path, cell=np.eye(3) * 40.0)
    with pytest.raises(ValueError, match="periodic or modular"):
        traj.essential_dynamics(device=-1)
