"""Shape descriptors and circumcircles (reference utilities.py:434-650,
1653-1691).  Golden values come from the reference itself (tests/golden/make_golden.py shape).

Bars: tensors, circumcircle diameters and centres bit-identical; eigenvalues (the reference:
LAPACK dgeev, here: Jacobi) within EIG_TOL of the largest eigenvalue; descriptors accordingly."""
import ctypes
import warnings

import numpy as np
import pytest

from _util import GOLDEN, group_batch
from pywindow_amd import _lib

EIG_TOL = 1e-12      # relative to the largest |eigenvalue| of the tensor


def load():
    g = np.load(GOLDEN / "shape.npz")
    return g, group_batch(g)


def check(out, g, where):
    for u in range(len(out)):
        assert np.array_equal(out[u]["gyration"], g["gyration"][u]), f"{where} u{u}: gyration tensor"
        assert np.array_equal(out[u]["inertia"], g["inertia"][u]), f"{where} u{u}: inertia tensor"
        scale = np.max(np.abs(g["eigenvalues"][u]))
        assert np.max(np.abs(out[u]["eigenvalues"] - g["eigenvalues"][u])) <= EIG_TOL * scale, f"{where} u{u}"
        a, b, k = g["descriptors"][u]
        assert abs(out[u]["asphericity"] - a) <= 2 * EIG_TOL * scale, f"{where} u{u}: asphericity"
        assert abs(out[u]["acylidricity"] - b) <= 2 * EIG_TOL * scale, f"{where} u{u}: acylidricity"
        assert abs(out[u]["relative_shape_anisotropy"] - k) <= 10 * EIG_TOL, f"{where} u{u}: anisotropy"


def test_oracle_shape_matches_reference():
    from oracle import pw_shape as S

    g, (off, xyz, _, mass) = load()
    for u in range(len(off) - 1):
        x, m = xyz[off[u]:off[u + 1]], mass[off[u]:off[u + 1]]
        inertia = S.inertia_tensor(x, m)
        assert np.array_equal(S.gyration_tensor(x, m), g["gyration"][u])
        assert np.array_equal(inertia, g["inertia"][u])
        eig = S.sorted_eigenvalues(inertia)
        assert np.array_equal(eig, g["eigenvalues"][u])
        assert np.array_equal(S.descriptors(eig), g["descriptors"][u])
        d, c = S.circumcircle(x, g["atom_sets"][u])
        assert np.array_equal(d, g["circum_d"][u]) and np.array_equal(np.array(c), g["circum_c"][u])


def test_host_team_shape_matches_reference(hostsim):
    g, (off, xyz, _, mass) = load()
    L = ctypes.CDLL(str(hostsim / "libshapeprobe.so"))
    vp = ctypes.c_void_p
    mass = np.ascontiguousarray(mass)
    out = np.zeros(len(off) - 1, dtype=_lib.SHAPE_OUT_DTYPE)
    assert L.hs_shape_batch(ctypes.c_long(len(out)), off.ctypes.data_as(vp), xyz.ctypes.data_as(vp),
                            mass.ctypes.data_as(vp), out.ctypes.data_as(vp)) == 0
    check(out, g, "hostsim")
    for u in range(len(out)):
        sets = np.ascontiguousarray(g["atom_sets"][u].astype(np.int32))
        x = np.ascontiguousarray(xyz[off[u]:off[u + 1]])
        d, c = np.zeros(len(sets)), np.zeros((len(sets), 3))
        L.hs_circumcircle(x.ctypes.data_as(vp), sets.ctypes.data_as(vp), ctypes.c_long(len(sets)),
                          d.ctypes.data_as(vp), c.ctypes.data_as(vp))
        assert np.array_equal(d, g["circum_d"][u]) and np.array_equal(c, g["circum_c"][u]), u


@pytest.mark.gpu
def test_hip_shape_matches_reference(hip_ctx):
    from pywindow_amd import utilities as U

    g, (off, xyz, vdw, mass) = load()
    out = hip_ctx.shape(_lib.Batch(off, xyz, vdw, mass))          # ragged batch, one launch
    check(out, g, "hip")
    for u in (0, 1, 5):
        el, x = g["elements"][off[u]:off[u + 1]], g["coordinates"][off[u]:off[u + 1]]
        assert np.array_equal(U.get_gyration_tensor(el, x), g["gyration"][u])
        assert np.array_equal(U.get_inertia_tensor(el, x), g["inertia"][u])
        assert U.calc_asphericity(el, x) == out[u]["asphericity"]
        assert U.calc_acylidricity(el, x) == out[u]["acylidricity"]
        assert U.calc_relative_shape_anisotropy(el, x) == out[u]["relative_shape_anisotropy"]
        d, c = U.circumcircle(x, g["atom_sets"][u])
        assert np.array_equal(d, g["circum_d"][u]) and np.array_equal(np.array(c), g["circum_c"][u])
        r, c0 = U.circumcircle_window(x, g["atom_sets"][u][0])
        assert 2 * r == g["circum_d"][u][0] and np.array_equal(c0, g["circum_c"][u][0])
        # Python's negative indices address the same atoms
        dn, _ = U.circumcircle(x, [g["atom_sets"][u][0] - len(x)])
        assert dn[0] == g["circum_d"][u][0]
    with pytest.raises(IndexError):
        U.circumcircle(x, [[0, 1, len(x)]])
    assert U.circumcircle(x, []) == ([], [])


@pytest.mark.gpu
def test_hip_shape_large_unit_matches_oracle(hip_ctx):
    """A 1008-atom unit: the inertia sums run over a million terms (124 numpy buffers)."""
    from oracle import pw_shape as S
    from pywindow_amd import element_data as E
    from pywindow_amd import synth

    el, frames = synth.synthetic_units(6)
    x = np.concatenate([frames[k] + np.array([30.0 * k, 0, 0]) for k in range(6)])
    ids = E.element_ids(list(el) * 6)
    out = hip_ctx.shape(_lib.Batch(np.array([0, len(x)]), x, E.VDW[ids], E.MASS[ids]))[0]
    assert np.array_equal(out["gyration"], S.gyration_tensor(x, E.MASS[ids]))
    inertia = S.inertia_tensor(x, E.MASS[ids])
    assert np.array_equal(out["inertia"], inertia)
    eig = S.sorted_eigenvalues(inertia)
    assert np.max(np.abs(out["eigenvalues"] - eig)) <= EIG_TOL * np.max(np.abs(eig))


def test_rotation_matrix_matches_reference():
    """rotation_matrix_arbitrary_axis / normalize_vector (reference utilities.py:539-591) are host
    arithmetic: 40 reference-generated matrices, bit for bit (axis rounded to four decimals included)."""
    from pywindow_amd import utilities as U

    g = np.load(GOLDEN / "axes.npz")
    for a, v, m in zip(g["rot_angles"], g["rot_axes"], g["rot_matrices"]):
        assert np.array_equal(U.rotation_matrix_arbitrary_axis(a, v), m)
    assert np.array_equal(U.normalize_vector(np.array([3.0, 4.0, 0.0])), [0.6, 0.8, 0.0])
    assert np.array_equal(U.normalize_vector(np.array([1.0, 1.0, 1.0])), [0.5774, 0.5774, 0.5774])


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:the matrix subclass")
def test_principal_axes_and_alignment_match_reference(hip_ctx):
    """principal_axes / align_principal_ax (reference utilities.py:532-623): inertia tensor from the GPU,
    eigenvector order and signs as LAPACK dgeev leaves them -- equal to the reference's on every
    fixture molecule; the aligned coordinates and the three rotation matrices likewise."""
    import pywindow_amd as pw
    from pywindow_amd import utilities as U

    g = np.load(GOLDEN / "axes.npz")
    off = g["atom_offset"]
    for u in range(len(off) - 1):
        el, xyz = g["elements"][off[u]:off[u + 1]], g["coordinates"][off[u]:off[u + 1]]
        assert np.array_equal(U.principal_axes(el, xyz), g["principal_axes"][u]), g["names"][u]
        moved, rots = U.align_principal_ax(el, xyz)
        assert np.array_equal(np.array([np.asarray(r) for r in rots]), g["rotations"][u]), g["names"][u]
        assert np.array_equal(moved, g["aligned"][off[u]:off[u + 1]]), g["names"][u]
        assert np.array_equal(xyz, g["coordinates"][off[u]:off[u + 1]])          # the input is not touched
    el, xyz = g["elements"][off[0]:off[1]], g["coordinates"][off[0]:off[1]]
    mol = pw.Molecule({"elements": el, "coordinates": xyz.copy()}, "cc3", 0)
    mol._align_to_principal_axes()
    assert mol.aligned_to_principal_axes is True


# ---- the edges (tests/_shape_cases.py): host build of pw_shape.hpp against the oracle and a 50-digit solver ----

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def edge_cases(hostsim):
    """[(tag, xyz, mass, host record)] of every shape case: the hard molecules, the sizes around numpy's
    blocks and the units of the large batch."""
    import _shape_cases as C

    L = ctypes.CDLL(str(hostsim / "libshapeprobe.so"))
    groups = [C.hard_molecules(), C.sized_molecules(), C.unpack(*C.large_batch())]
    cases = []
    for mols in groups:
        out = C.host_shape(L, *C.pack(mols))
        cases += [(tag, x, m, out[u]) for u, (tag, x, m) in enumerate(mols)]
    return cases


def test_block_inertia_restates_the_oracle():
    """The block-wise restatement used above ORACLE_MAX_N equals the oracle as written at N >= 8193."""
    import _shape_cases as C
    from oracle import pw_shape as S

    _, x, m = C.sized_molecule(C.ORACLE_MAX_N)
    assert np.array_equal(C.block_inertia(x, m), S.inertia_tensor(x, m))


def test_host_tensors_at_the_edges_match_oracle(edge_cases):
    """Gyration and inertia tensors of every edge case, bit for bit: the oracle as written up to N = 8193,
    its block-wise restatement above."""
    import _shape_cases as C
    from oracle import pw_shape as S

    assert len(edge_cases) == len(C.SHIFTS) * C.ROTATIONS * len(C.SHAPES) + len(C.SIZES) + C.LARGE_BATCH_UNITS
    for tag, x, m, rec in edge_cases:
        inertia = S.inertia_tensor(x, m) if len(x) <= C.ORACLE_MAX_N else C.block_inertia(x, m)
        assert np.array_equal(rec["gyration"], S.gyration_tensor(x, m)), f"{tag}: gyration tensor"
        assert np.array_equal(rec["inertia"], inertia), f"{tag}: inertia tensor"


def _exact(tensor):
    """Eigenvalues (descending) of the double tensor taken as exact, at 50 digits."""
    import mpmath

    with mpmath.workdps(50):
        ev = mpmath.eigsy(mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in tensor]), eigvals_only=True)
        return sorted((ev[i] for i in range(3)), reverse=True)


def _err(got, exact, scale):
    """|got - exact| in units of eps * scale (scale = max |exact eigenvalue|); a zero tensor must give zeros."""
    import mpmath

    with mpmath.workdps(50):
        d = max(abs(mpmath.mpf(float(g)) - e) for g, e in zip(got, exact))
        if scale == 0:
            return 0.0 if d == 0 else float("inf")
        return float(d / (scale * EPS))


def test_host_eigenvalues_and_descriptors_against_50_digits(edge_cases):
    """Eigenvalues of every edge case's inertia tensor against mpmath.eigsy at 50 digits, in units of
    eps * max|lambda|.  The bar is the worst error of the reference's own eigensolver (np.linalg.eigvals,
    LAPACK dgeev) over the same cases, measured in the same run: the Jacobi may not be less accurate.
    Every case is scored.  For a few spherical tops at the origin dgeev returns a complex pair; which ones
    depends on the BLAS kernels of the host.  The reference casts to float64 and so returns the real parts,
    and those are scored.  By Bauer-Fike, with orthogonal eigenvectors, each computed eigenvalue lies within
    dgeev's backward error of the spectrum, so the imaginary parts are held to the same bar.
    Measured over the 7095 cases (2080 hard molecules, 12 sizes, 5003 units): Jacobi 1.878, LAPACK 8.358, three
    complex pairs with imaginary parts up to 0.390 (OpenBLAS' own kernel choice on an AVX-512 host); with
    OPENBLAS_CORETYPE=Haswell, LAPACK 8.271 and three other complex pairs up to 0.794.
    Mutations: a Jacobi that stops at offd <= 1e-6 * diag fails with 5.6e9, one that stops at 1e-10 * diag with
    6.4e5 (on a top moved by 1e-3 A and shifted by 1000 A, where two eigenvalues lie close).

    Descriptors (utilities.py:434-446) against the descriptors of the 50-digit eigenvalues, with u = eps/2,
    M = max|lambda|, E = B * eps * M the eigenvalue bar (B the LAPACK worst):
      asphericity  a = l0 - (l1 + l2) / 2: propagated |d0| + (|d1| + |d2|) / 2 <= 2E; rounding: the sum
                   u * 2(M+E), the halving exact, the difference u * 2(M+E), the halved sum's error halved:
                   3u(M+E).  Bound 2E + 1.5 eps (M+E).
      acylidricity b = l1 - l2: propagated 2E, rounding u * 2(M+E).  Bound 2E + eps (M+E).
      anisotropy   k = 1 - 3 P / S^2, P = l0l1 + l0l2 + l1l2, S = l0 + l1 + l2: propagated
                   sum_a |dk/dl_a| E with dk/dl_a = -3 ((S - l_a) S - 2P) / S^3 at the exact eigenvalues;
                   rounding: P (three products, two additions) 3u Pabs (Pabs = sum of |products|), S 2u Sabs,
                   S^2 (pw_square_np: libm pow, within one ulp) relative 2(2u Sabs/|S|) + 2u, the quotient u:
                   |dq| <= 3u Pabs / S^2 + |q| (4u Sabs/|S| + 3u); then 3q (+ 3u|q|) and 1 - 3q (+ u|k|).
                   Bound sum |dk/dl_a| E + 3|dq| + 3u|q| + u|k|.
    Second-order terms are products of two of these relative errors (each below 1e3 eps): a factor
    1 + 1e-12 on every bound covers them.  A zero tensor (one atom at the origin) has k = 0/0: NaN in both."""
    import mpmath

    from oracle import pw_shape as S

    jac, lap, imag, scored, worst = [], [], [], 0, {}
    for tag, x, m, rec in edge_cases:
        w = np.linalg.eigvals(rec["inertia"])
        exact = _exact(rec["inertia"])
        scale = max(abs(e) for e in exact)
        with warnings.catch_warnings():
            # a complex pair: the reference's cast to float64 keeps the real parts, which are what it returns
            warnings.simplefilter("ignore", np.exceptions.ComplexWarning)
            ref = S.sorted_eigenvalues(rec["inertia"])
        jac.append(_err(rec["eigenvalues"], exact, scale))
        lap.append(_err(ref, exact, scale))
        if np.iscomplexobj(w) and np.any(np.imag(w) != 0):
            imag.append((float(np.max(np.abs(np.imag(w))) / (float(scale) * EPS)), tag))
        scored += 1
        worst["jac"] = max(worst.get("jac", (0.0, "")), (jac[-1], tag))
        worst["lap"] = max(worst.get("lap", (0.0, "")), (lap[-1], tag))
    print(f"\n{len(edge_cases)} cases, {len(edge_cases) - scored} left out; "
          f"{len(imag)} with a complex pair in np.linalg.eigvals, imaginary parts up to "
          f"{max(imag)[0] if imag else 0.0:.3f} eps * max|lambda| {[t for _, t in imag]}")
    print(f"worst eigenvalue error, eps * max|lambda|: Jacobi {worst['jac'][0]:.3f} ({worst['jac'][1]}), "
          f"LAPACK {worst['lap'][0]:.3f} ({worst['lap'][1]})")
    assert scored == len(edge_cases)
    B = max(lap)
    assert max(jac) <= B
    # a computed eigenvalue of the symmetric tensor lies within dgeev's backward error of the spectrum (Bauer-Fike,
    # orthogonal eigenvectors): its imaginary part is held to the same bar as the real parts' errors
    assert all(e <= B for e, _ in imag), imag
    u = EPS / 2
    slack = 1.0 + 1e-12
    for tag, x, m, rec in edge_cases:
        with mpmath.workdps(50):
            l0, l1, l2 = _exact(rec["inertia"])
            M = max(abs(l0), abs(l1), abs(l2))
            E = B * EPS * M
            mf = lambda v: mpmath.mpf(float(v))         # noqa: E731
            da = abs(mf(rec["asphericity"]) - (l0 - (l1 + l2) / 2))
            assert da <= (2 * E + 1.5 * EPS * (M + E)) * slack, f"{tag}: asphericity off by {float(da):.3e}"
            db = abs(mf(rec["acylidricity"]) - (l1 - l2))
            assert db <= (2 * E + EPS * (M + E)) * slack, f"{tag}: acylidricity off by {float(db):.3e}"
            Ssum, P = l0 + l1 + l2, l0 * l1 + l0 * l2 + l1 * l2
            k_got = float(rec["relative_shape_anisotropy"])
            if Ssum == 0:
                assert np.isnan(k_got), tag
                continue
            q = P / Ssum ** 2
            k = 1 - 3 * q
            Pabs, Sabs = abs(l0 * l1) + abs(l0 * l2) + abs(l1 * l2), abs(l0) + abs(l1) + abs(l2)
            dk = sum(abs(3 * ((Ssum - la) * Ssum - 2 * P) / Ssum ** 3) for la in (l0, l1, l2))
            dq = 3 * u * Pabs / Ssum ** 2 + abs(q) * (4 * u * Sabs / abs(Ssum) + 3 * u)
            bound = (dk * E + 3 * dq + 3 * u * abs(q) + u * abs(k)) * slack
            assert abs(mf(k_got) - k) <= bound, f"{tag}: anisotropy off by {float(abs(mf(k_got) - k)):.3e}"


def _same_pattern_and_values(got, want, tol, where):
    """NaN, +inf, -inf and finite at the same places; finite values bit for bit (tol == 0: -0.0 and 0.0
    differ too) or within tol relative."""
    got, want = np.asarray(got), np.asarray(want)
    for f in (np.isnan, np.isposinf, np.isneginf, np.isfinite):
        bad = np.nonzero(f(got) != f(want))[0]
        assert not len(bad), f"{where}: {f.__name__} differs at {bad[:10]}"
    fin = np.isfinite(want)
    if tol == 0.0:
        bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)) & ~np.isnan(want))[0]
        assert not len(bad), f"{where}: bits differ at {bad[:10]}"
    else:
        e = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
        assert (e <= tol).all(), f"{where}: rel err {e.max():.3e}"


def test_host_circumcircle_edges_match_oracle(hostsim):
    """N_TRIPLES triples in one call: bit for bit on the reference platform, LIVE_TOL_WINDOW relative
    elsewhere; the pattern of NaN, +inf, -inf and finite values identical either way."""
    import _shape_cases as C
    import _util
    from oracle import pw_shape as S

    L = ctypes.CDLL(str(hostsim / "libshapeprobe.so"))
    xyz, sets = C.circumcircle_triples()
    assert len(sets) >= 100_000 and len(sets) % 64
    d, c = C.host_circumcircle(L, xyz, sets)
    with np.errstate(all="ignore"):
        od, oc = S.circumcircle(xyz, sets)
    od, oc = np.array(od), np.array(oc)
    print(f"\n{len(sets)} triples: {np.isnan(od).sum()} NaN and {np.isinf(od).sum()} infinite diameters, "
          f"{np.isnan(oc).any(1).sum()} NaN and {np.isinf(oc).any(1).sum()} infinite centres")
    _same_pattern_and_values(d, od, _util.LIVE_TOL_WINDOW, "diameters")
    _same_pattern_and_values(c.reshape(-1), oc.reshape(-1), _util.LIVE_TOL_WINDOW, "centres")
