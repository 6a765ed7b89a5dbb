"""Periodic charge equilibration on the host path (device = -1): pw_charges_cell against the restatement of its definition
as bytes, against an independent dense model through numpy.linalg.solve, through the invariances that a missed image or
a wrong phase breaks, in the isolated limit against pw_charges, on the golden CC3 cell, at every refusal and through the
public layer (tests/_charges_cell_cases.py).  tests/test_gpu_charges_cell.py holds the device to the host path."""
import numpy as np
import pytest

import _charges_cell_cases as C

import pywindow_amd as pw
from pywindow_amd import _lib


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=16)


def test_the_case_list_covers_every_edge():
    names = [c.name for c in C.cases()]
    assert sorted(len(c.xyz) for c in C.cases()[:6]) == [1, 2, 63, 64, 65, 129]
    for wanted in ("skewed", "orthorhombic", "cutoff == the smallest width", "no pair", "on a face", "coincident", "r2 == cutoff2",
                   "r2 == shield_on2", "r2 == shield_off2", "alpha = 0, n_k = 0", "n_k = 64", "n_k = 65", "indices at the cap",
                   "tol 1e-14", "tol 1e-2", "max_iter 1"):
        assert any(wanted in n for n in names), wanted
    assert C.solved(C.breakdown_case())[1]["flags"] & C.BREAKDOWN


def test_the_host_path_is_the_restatement_byte_for_byte(host):
    """Job by job, and as one batch with holes and the outputs in reverse: charges and rows are the restatement's bytes, and
    what no job owns keeps the sentinel."""
    jobs = list(C.cases()) + [C.breakdown_case()]
    for c in jobs:
        packed = C.pack([c])
        rc, got = C.raw(host, packed)
        want = C.expected([c], packed)
        assert rc == 0 and C.same(got, want), (c.name, C.first_difference(got, want))
    packed = C.pack(jobs, hole=2, reverse=True, pad=3)
    rc, got = C.raw(host, packed)
    want = C.expected(jobs, packed)
    assert rc == 0 and C.same(got, want), C.first_difference(got, want)
    rows = got[1].view(np.uint8).reshape(len(got[1]), -1)
    assert (rows == C.SENTINEL).all(axis=1).sum() == 2 * len(jobs)


def test_no_pair_means_chi_and_J_alone_and_breakdown_is_a_result():
    lonely = [c for c in C.cases() if c.name.startswith("no pair")][0]
    q, row = C.solved(lonely)
    chi, J = lonely.params[:, 0], lonely.params[:, 1]
    mu = (chi / J).sum() / (1.0 / J).sum()
    assert np.allclose(q, (mu - chi) / J, rtol=0, atol=1e-14) and abs(row["mu"] - mu) < 1e-13 and abs(q.sum()) < 1e-14
    q, row = C.solved(C.breakdown_case())
    assert (q.view(np.uint64) == 0x7FF8000000000000).all() and row["iterations"] <= 4 and np.isnan(row["mu"])


def test_against_the_dense_model(host):
    """The matrix as a dense array from the formulas (math.erfc, G an explicit cosine matrix) and numpy.linalg.solve of the
    bordered system: at tol = 1e-10 the charges lie within 1e-7 e and mu within 1e-7 eV (the stopping rule times the
    condition number 370 with a decade to spare).  Measured: 8.1e-11 e and 2.7e-12 eV at worst over the list."""
    worst = [0.0, 0.0]
    checked = 0
    for c in C.cases():
        if not c.converges or c.tol != 1e-10:
            continue
        packed = C.pack([c])
        rc, (q, rows) = C.raw(host, packed)
        want_q, want_mu, A = C.dense_model(c)
        n = len(c.xyz)
        assert rc == 0 and rows["flags"][0] == 0 and abs(q[:n].sum()) < 1e-12
        worst = [max(worst[0], float(np.abs(q[:n] - want_q).max())), max(worst[1], abs(float(rows["mu"][0]) - want_mu))]
        checked += 1
    print(f"dense model: charges within {worst[0]:.3g} e, mu within {worst[1]:.3g} eV over {checked} cases")
    assert checked >= 8 and worst[0] <= 1e-7 and worst[1] <= 1e-7, worst


# ---- invariances ---------------------------------------------------------------------------------------------------
def both_ways(a, b, pick_a=lambda q: q, pick_b=lambda q: q, tol=1e-10):
    """(the largest charge difference of the dense model between the calls a and b, that of the library): a call is
    (xyz, elements, lattice, keywords); pick_a / pick_b choose the charges to compare."""
    model = [C.public_model(x, el, lat, **kw)[0] for x, el, lat, kw in (a, b)]
    made = [pw.equilibrate_cell_charges(x, el, lat, tol=tol, device=-1, **kw) for x, el, lat, kw in (a, b)]
    assert all(int(m.flags) == 0 for m in made)
    return (float(np.abs(pick_a(model[0]) - pick_b(model[1])).max()),
            float(np.abs(pick_a(made[0].charges) - pick_b(made[1].charges)).max()))


def held(name, d_model, d_library):
    """The library is allowed ten times the difference of the dense model, and never more than 1e-5 e."""
    print(f"{name}: dense model {d_model:.3g} e, library {d_library:.3g} e")
    assert d_library <= min(10.0 * d_model, 1e-5), (name, d_model, d_library)


def test_the_charges_do_not_depend_on_how_the_ewald_sum_is_split():
    """125 atoms in a 24.8 Angstrom cube: Ewald tolerance 1e-6 against 1e-8 (measured on the dense model: 3.7e-8 e; the CC3
    prototype had 4e-7) and cutoff 9 against 12 Angstrom (2.8e-8 e; 7e-7)."""
    el, x, lat = C.gas_system(125, 11, 24.8 * np.eye(3))
    held("tolerance 1e-6 / 1e-8", *both_ways((x, el, lat, dict(tolerance=1e-6)), (x, el, lat, dict(tolerance=1e-8))))
    held("cutoff 9 / 12", *both_ways((x, el, lat, dict(cutoff=9.0)), (x, el, lat, dict(cutoff=12.0))))


def test_the_charges_do_not_depend_on_how_the_crystal_is_described():
    """30 atoms in a skewed 12 Angstrom cell at cutoff 6 and shield (2, 3.5): the 2 x 1 x 1 supercell, all atoms shifted by
    an irrational vector and wrapped again, the lattice given as (a + b, b, c), the atoms permuted.  The model is exactly
    invariant, so its differences are rounding: 1.4e-15, 2.1e-15, 2.1e-15 and 1.2e-15 e measured; the library runs at tol =
    1e-14 so that its stopping rule is below that (4.0e-15, 1.2e-15, 9.7e-16 and 2.2e-15 e measured)."""
    lat = np.array([[12.0, 2.0, -1.5], [0.0, 11.0, 1.0], [0.0, 0.0, 12.5]])
    el, x, lat = C.gas_system(30, 5, lat)
    kw = dict(cutoff=6.0, shield=(2.0, 3.5))
    one = (x, el, lat, kw)
    sup = lat * np.array([2.0, 1.0, 1.0])[None, :]
    held("supercell", *both_ways(one, (np.concatenate([x, x + lat[:, 0]]), el + el, sup, kw), pick_b=lambda q: q[:30], tol=1e-14))
    shift = np.array([np.sqrt(2.0), np.pi, -np.e])
    held("shift", *both_ways(one, (x + shift, el, lat, kw), tol=1e-14))
    sheared = lat.copy()
    sheared[:, 0] = lat[:, 0] + lat[:, 1]
    held("(a + b, b, c)", *both_ways(one, (x, el, sheared, kw), tol=1e-14))
    perm = np.random.default_rng(3).permutation(30)
    held("permutation", *both_ways(one, (x[perm], [el[i] for i in perm], lat, kw), pick_a=lambda q: q[perm], tol=1e-14))


def test_the_isolated_limit_is_pw_charges():
    """Eight atoms under 9 Angstrom across with shield = (10, 11) -- every pair inside the cluster fully shielded -- in a 40
    Angstrom cube at cutoff 18: against pw.equilibrate_charges.  The dense periodic model against the dense vacuum model
    gives the expected difference d, the image dipoles of order 1 / L^3 (measured: d = 2.24e-4 e, and the library 2.24e-4 e from pw_charges); the library is within
    2 d + 1e-6."""
    rng = np.random.default_rng(21)
    el = ["C", "N", "O", "H", "C", "H", "N", "O"]
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
    x = 17.0 + 3.5 * corners + rng.uniform(-0.4, 0.4, (8, 3))
    assert np.sqrt(((x[:, None] - x[None]) ** 2).sum(axis=2)).max() < 9.0
    lat = 40.0 * np.eye(3)
    kw = dict(cutoff=18.0, shield=(10.0, 11.0))
    d = float(np.abs(C.public_model(x, el, lat, **kw)[0] - C.vacuum_model(x, el)[0]).max())
    cell = pw.equilibrate_cell_charges(x, el, lat, device=-1, **kw)
    vacuum = pw.equilibrate_charges(x, el, device=-1)
    got = float(np.abs(cell.charges - vacuum.charges).max())
    print(f"isolated limit: d = {d:.3g} e, library {got:.3g} e")
    assert bool(cell.converged) and bool(vacuum.converged) and got <= 2.0 * d + 1e-6, (d, got)


def test_the_cc3_cell_is_positive_definite_on_the_neutral_subspace():
    """One frame of the golden CC3 cell (1344 atoms, 24.8 Angstrom) at the defaults converges with no flag in fewer than 100
    steps (27; the numpy prototype, which stopped on the unprojected r.z, took 23)."""
    elements, xyz, lattice = C.cc3_cell()
    made = pw.equilibrate_cell_charges(xyz, elements, lattice, device=-1)
    print(f"CC3 cell: {int(made.iterations)} steps, charges {float(made.q_min):.4f} .. {float(made.q_max):.4f} e")
    assert bool(made.converged) and int(made.flags) == 0 and int(made.iterations) < 100
    assert abs(made.charges.sum()) < 1e-9 and made.charges.shape == (1344,)


def test_refusals(host):
    """Every refusal of the header: job 1 of two is refused, the message names it, nothing is written."""
    for packed, n_points, n_kvecs, what in C.bad_batches():
        rc, got = C.raw(host, packed, n_points=n_points, n_kvecs=n_kvecs)
        assert rc == -2 and C.same(got, C.blank(packed)), what
        message = _lib.load().pw_last_error().decode()
        assert message.startswith("pw_charges_cell: job 1: ") and what in message, (what, message)


# ---- the public layer ----------------------------------------------------------------------------------------------
def made_up_cell():
    lat = np.array([[10.5, 1.0, -0.5], [0.0, 10.0, 0.8], [0.0, 0.0, 11.0]])
    return C.gas_system(40, 77, lat)


def test_qeq_cell_is_the_two_step_call_byte_for_byte():
    el, x, lat = made_up_cell()
    kw = dict(guest="CO2", temperatures=[250.0, 350.0], spacing=1.0, cutoff=6.0, directions=pw.sphere_directions(6), device=-1)
    q = pw.equilibrate_cell_charges(x, el, lat, cutoff=6.0, device=-1)
    auto = pw.rigid_guest_field(x, el, lat, charges="qeq-cell", **kw)
    by_hand = pw.rigid_guest_field(x, el, lat, charges=q.charges, **kw)
    assert bool(q.converged) and bool(auto.charges_converged) and by_hand.charges_converged is None
    assert auto.raw.tobytes() == by_hand.raw.tobytes() and auto.levels.tobytes() == by_hand.levels.tobytes()
    assert auto.zbar.tobytes() == by_hand.zbar.tobytes() and auto.u_min_map.tobytes() == by_hand.u_min_map.tobytes()
    # a batch with a lattice a frame
    frames = np.stack([x, x * 1.01, x * 0.99])
    lats = np.stack([lat, lat * 1.01, lat * 0.99])
    qs = pw.equilibrate_cell_charges_batch(frames, el, lats, cutoff=6.0, device=-1)
    auto = pw.rigid_guest_field(frames, el, lats, charges="qeq-cell", **kw)
    by_hand = pw.rigid_guest_field(frames, el, lats, charges=qs.charges, **kw)
    assert qs.charges.shape == (3, 40) and qs.converged.all() and auto.charges_converged.all()
    assert auto.raw.tobytes() == by_hand.raw.tobytes() and auto.levels.tobytes() == by_hand.levels.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(auto.zbar, by_hand.zbar))
    assert qs.charges[0].tobytes() == q.charges.tobytes()            # (the grouping of the jobs does not show)
    diffusion = pw.rigid_guest_diffusion(x, el, lat, charges="qeq-cell", **kw)
    assert bool(diffusion.charges_converged)
    assert all(bool(p.charges_converged) for p in pw.rigid_guest_percolation(x, el, lat, charges="qeq-cell", **kw))


def test_what_the_public_layer_refuses():
    el, x, lat = made_up_cell()
    kw = dict(guest="CO2", temperatures=[250.0], spacing=1.0, cutoff=6.0, directions=pw.sphere_directions(4), device=-1)
    with pytest.raises(ValueError, match="isolated-molecule model"):
        pw.rigid_guest_field(x, el, lat, charges="qeq", **kw)
    rows = pw.rigid_coefficients(el, "CO2")[:, :, :2]
    with pytest.raises(ValueError, match="needs the elements"):
        pw.rigid_guest_field(x, rows, lat, charges="qeq-cell", **kw)
    with pytest.raises(KeyError, match="XX"):
        pw.equilibrate_cell_charges(x, ["XX"] + el[1:], lat, cutoff=6.0, device=-1)
    with pytest.raises(ValueError, match=r"the largest cutoff that fits is 9\.9"):
        pw.equilibrate_cell_charges(x, el, lat, cutoff=10.5, device=-1)
    with pytest.raises(ValueError, match="shield"):
        pw.equilibrate_cell_charges(x, el, lat, cutoff=5.0, shield=(4.0, 6.0), device=-1)


def test_series_and_the_molecular_system():
    el, x, lat = made_up_cell()
    frames = np.stack([x, x * 1.01])
    lats = np.stack([lat, lat * 1.01])
    made = pw.equilibrate_cell_charges_batch(frames, el, lats, cutoff=6.0, device=-1)
    for name in ("potential", "q_max", "q_min", "energy", ("charge", 3)):
        values, valid = made.series(name)
        assert values.shape == (2,) and valid.all()
    assert np.array_equal(made.series(("charge", 3))[0], made.charges[:, 3])
    with pytest.raises(KeyError):
        made.series("dipole_norm")
    short = pw.equilibrate_cell_charges_batch(frames, el, lats, cutoff=6.0, max_iter=1, device=-1)
    values, valid = short.series("q_max")
    assert np.isfinite(values).all() and not valid.any() and not short.converged.any() and (short.flags == 1).all()
    system = pw.MolecularSystem.load_system({"elements": np.array(el), "coordinates": x, "lattice": lat}, "gas")
    q = system.calculate_cell_charges(cutoff=6.0, device=-1)
    assert q.charges.tobytes() == made.charges[0].tobytes() and system.cell_charges is q
