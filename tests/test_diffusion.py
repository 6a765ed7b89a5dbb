"""The numpy layer of pywindow_amd/diffusion.py against closed forms, on the host path (device = -1): the tensor of
hand-made periodic hop networks (network_tensor), the merge (hop_network) and whole fields through diffusion_field.
Tolerance: relative 1e-9 -- the systems have at most a few dozen sites with rate ratios up to 1e6, so the least-squares
solve loses at most about ten digits of sixteen."""
import dataclasses
import math

import numpy as np
import pytest

import pywindow_amd as pw
from pywindow_amd import _lib
from pywindow_amd import diffusion as DF
from pywindow_amd.affinity import R

RTOL = 1e-9
E = np.eye(3, dtype=np.int64)


def close(got, want):
    want = np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    return np.abs(np.asarray(got) - want).max() <= RTOL * scale


def chain(k1, k2, l):
    """Two sites a cell along x, alternating rates: 0 -> 1 inside the cell at k1, 1 -> 0 of the next cell at k2."""
    i, j = [0, 0], [1, 1]
    cells = [[0, 0, 0], [-1, 0, 0]]
    vectors = [[l, 0.0, 0.0], [-l, 0.0, 0.0]]
    return [1.0, 1.0], i, j, vectors, [k1, k2], [k1, k2], cells


def test_simple_cubic():
    k, a = 3.5e9, 4.25
    D, trapped, rank = DF.network_tensor([2.0], [0, 0, 0], [0, 0, 0], a * np.eye(3), [k] * 3, [k] * 3, E)
    assert close(D, k * a * a * np.eye(3)) and trapped == 0.0 and rank == 3


def test_alternating_chain():
    for k1, k2 in ((1.0, 1.0), (2.0, 7.0), (1.0, 1e6)):
        l = 1.75
        D, trapped, rank = DF.network_tensor(*chain(k1, k2, l))
        want = np.zeros((3, 3))
        want[0, 0] = l * l / (0.5 * (1.0 / k1 + 1.0 / k2))
        assert close(D, want) and rank == 1 and trapped == 0.0


def test_a_dead_end_lowers_the_tensor_by_its_population_share():
    k, l = 2.0, 3.0
    base = DF.network_tensor([1.0], [0], [0], [[l, 0, 0]], [k], [k], [[1, 0, 0]])[0]
    assert close(base[0, 0], k * l * l)
    for share, ks in ((0.25, 5.0), (0.9, 1e-3), (1e-4, 1e3)):
        zs = share / (1.0 - share)                                   # the side site's population beside a site of 1
        D, trapped, rank = DF.network_tensor([1.0, zs], [0, 0], [0, 1], [[l, 0, 0], [0, 1.5, 0]], [k, ks * zs], [k, ks],
                                             [[1, 0, 0], [0, 0, 0]])
        assert close(D, base * (1.0 - share)) and trapped == 0.0 and rank == 1


def test_two_sublattices_and_a_pocket():
    a = 2.0
    Z = [1.0, 3.0]
    two = DF.network_tensor(Z, [0, 1, 1], [0, 1, 1], [[a, 0, 0], [a, 0, 0], [0, a, 0]], [4.0, 8.0, 2.0], [4.0, 8.0, 2.0],
                            [[1, 0, 0], [1, 0, 0], [0, 1, 0]])
    want = np.diag([(1.0 * 4.0 + 3.0 * 8.0) / 4.0 * a * a, 3.0 * 2.0 / 4.0 * a * a, 0.0])
    assert close(two[0], want) and two[1] == 0.0 and two[2] == 2
    # a pocket of two sites that hop between themselves only: it is trapped, and the tensor is that of the rest
    pocket = DF.network_tensor(Z + [0.5, 0.5], [0, 1, 1, 2], [0, 1, 1, 3], [[a, 0, 0], [a, 0, 0], [0, a, 0], [1.0, 1.0, 0.0]],
                               [4.0, 8.0, 2.0, 9.0], [4.0, 8.0, 2.0, 9.0], [[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]])
    assert close(pocket[0], want) and close(pocket[1], 1.0 / 5.0) and pocket[2] == 2
    # nothing winds: a zero tensor, everything trapped
    none = DF.network_tensor([1.0, 1.0], [0], [1], [[1.0, 0, 0]], [1.0], [1.0], [[0, 0, 0]])
    assert not none[0].any() and none[1] == 1.0 and none[2] == 0


def test_a_random_network_is_symmetric_and_positive():
    rng = np.random.default_rng(3)
    n, m = 24, 70
    Z = np.exp(rng.uniform(-3.0, 3.0, n))
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    cells = rng.integers(-1, 2, (m, 3))
    cells[i == j] = [1, 0, 0]
    pos = rng.uniform(0.0, 5.0, (n, 3))
    vectors = pos[j] + cells * 5.0 - pos[i]
    flux = np.exp(rng.uniform(-3.0, 3.0, m))
    D, trapped, rank = DF.network_tensor(Z, i, j, vectors, flux / Z[i], flux / Z[j], cells)
    assert np.abs(D - D.T).max() <= 1e-12 * np.abs(D).max() and np.linalg.eigvalsh(D).min() >= -1e-12 * np.abs(D).max()
    assert rank == 3 and 0.0 <= trapped < 1.0


def channel_field(barrier):
    """(nz, ny, nx) = (3, 3, 2): one row along a of a well at 0 and a saddle at `barrier`, everything else blocked."""
    f = np.full((3, 3, 2), np.inf)
    f[1, 1, :] = [0.0, barrier]
    return f


def test_a_one_barrier_channel_through_the_library():
    T = np.array([250.0, 300.0, 400.0])
    lattice = np.diag([4.0, 3.0, 3.0])
    got = pw.diffusion_field(channel_field(5.0), lattice, T, mass=131.293, merge=0.0, labels=True, device=-1)
    beta = 1.0 / (R * T)
    S, Z = np.exp(-beta * 5.0), 1.0 + np.exp(-beta * 5.0)
    k = DF._speed(T, 131.293) * 1.0 * S / (2.0 * Z)                  # a_x = 1, v = 2
    want = np.zeros((3, 3, 3))
    want[:, 0, 0] = k * 16.0
    assert got.tensor.shape == (3, 3, 3) and close(got.tensor, want)
    assert got.valid and not got.barrierless and got.winding_rank == 1 and got.n_basins == 1 and got.n_sites == 1
    assert close(got.coefficient, want[:, 0, 0] / 3.0) and close(got.axis_coefficient, np.stack([want[:, 0, 0], 0 * k, 0 * k], axis=1))
    assert close(got.principal[0][:, 2], want[:, 0, 0]) and close(got.free_energy[0], -(R * T) * np.log(Z * 2.0))
    assert got.hops["cell"].tolist() == [[1, 0, 0]] and close(got.hops["vector"], [[4.0, 0.0, 0.0]]) and got.hops["saddle"][0] == 5.0
    assert close(got.rates[0, :, 0], k) and close(got.rates[0, :, 1], k) and got.trapped_fraction.tolist() == [0.0] * 3
    assert got.labels["basin"][1, 1].tolist() == [0, 0] and got.labels["basin"][0, 0].tolist() == [-1, -1]
    values, valid = got.series("coefficient", level=1)
    assert close(values, [want[1, 0, 0] / 3.0]) and valid.tolist() == [True]
    assert close(got.series("axis_coefficient", level=2, axis=0)[0], [want[2, 0, 0]])
    with pytest.raises(KeyError):
        got.series("volume")
    with pytest.raises(ValueError, match="axis"):
        got.series("axis_coefficient")
    # the same channel without a barrier above the merge threshold: the guest runs free, and the frame says so
    free = pw.diffusion_field(channel_field(0.5), lattice, T, mass=131.293, device=-1)
    assert free.barrierless and not free.valid and free.series("coefficient")[1].tolist() == [False]
    with pytest.raises(ValueError, match=r"\(nz, ny, nx\)"):
        pw.diffusion_field(np.zeros((3, 3)), lattice, T, mass=1.0, device=-1)
    with pytest.raises(ValueError, match="temperatures"):
        pw.diffusion_field(channel_field(5.0), lattice, [], mass=1.0, device=-1)


def test_activation_energy_of_a_one_barrier_lattice_is_the_barrier():
    T = np.array([200.0, 250.0, 300.0, 500.0])
    barrier, a = 12.5, 3.0
    tensors = np.stack([DF.network_tensor([1.0], [0, 0, 0], [0, 0, 0], a * np.eye(3), [1e12 * math.exp(-barrier / (R * t))] * 3,
                                          [1e12 * math.exp(-barrier / (R * t))] * 3, E)[0] for t in T])
    base = pw.diffusion_field(channel_field(5.0), np.diag([4.0, 3.0, 3.0]), T, mass=40.0, merge=0.0, device=-1)
    made = dataclasses.replace(base, tensor=tensors)
    assert close(made.activation_energy(), barrier)
    with pytest.raises(ValueError, match="two temperatures"):
        pw.diffusion_field(channel_field(5.0), np.diag([4.0, 3.0, 3.0]), 300.0, mass=40.0, device=-1).activation_energy()


@pytest.fixture(scope="module")
def landscape():
    rng = np.random.default_rng(21)
    return rng.normal(0.0, 2.0, (5, 6, 7)), np.array([[7.0, 0.5, -0.3], [0.0, 6.5, 0.4], [0.0, 0.0, 5.5]])


def run(field, lattice, **kw):
    return pw.diffusion_field(field, lattice, [280.0, 350.0], mass=83.798, merge=0.0, device=-1, **kw)


def test_detailed_balance_symmetry_and_positivity(landscape):
    field, lattice = landscape
    got = run(field, lattice)
    assert got.valid and got.n_sites == got.n_basins and got.winding_rank == 3
    Z, i, j = got.populations, got.hops["i"], got.hops["j"]
    for l in range(2):
        assert close(Z[i, l] * got.rates[:, l, 0], Z[j, l] * got.rates[:, l, 1])
        D = got.tensor[l]
        assert np.abs(D - D.T).max() <= 1e-12 * np.abs(D).max() and np.linalg.eigvalsh(D).min() > 0.0
    assert (got.trapped_fraction == 0.0).all()
    assert close(got.free_energy, -(R * got.temperatures)[None, :] * np.log(Z * got.voxel_volume))


def test_invariances(landscape):
    field, lattice = landscape
    base = run(field, lattice).tensor
    # a cyclic shift of the field, an added constant
    for axis, by in ((2, 1), (1, -2), (0, 3)):
        assert close(run(np.roll(field, by, axis), lattice).tensor, base)
    assert close(run(field + 3.0, lattice).tensor, base)
    # the lattice turned in space: the tensor turns with it
    turn = np.linalg.qr(np.random.default_rng(4).normal(size=(3, 3)))[0]
    turn = turn * np.sign(np.linalg.det(turn))
    assert close(run(field, turn @ lattice).tensor, np.einsum("ab,lbc,dc->lad", turn, base, turn))
    # the cell tiled twice along a and along c
    twice = lattice.copy()
    twice[:, 0] *= 2.0
    assert close(run(np.concatenate([field, field], axis=2), twice).tensor, base)
    twice = lattice.copy()
    twice[:, 2] *= 2.0
    assert close(run(np.concatenate([field, field], axis=0), twice).tensor, base)


def test_the_merge():
    """Two wells at -2 and -1 over a saddle at 1 along a, walls blocked: below the threshold two sites and two hops (the
    saddle inside the cell, the one across its face); above it one site that keeps the higher saddle as a hop to its
    own image."""
    f = np.full((3, 3, 8), np.inf)
    f[1, 1, :] = [-2.0, 0.0, 1.0, 0.0, -1.0, 2.0, 4.0, 2.0]
    lattice = np.diag([8.0, 3.0, 3.0])
    two = pw.diffusion_field(f, lattice, 300.0, mass=40.0, merge=0.0, device=-1)
    assert two.n_basins == 2 and two.n_sites == 2 and two.winding_rank == 1 and len(two.hops) == 2
    assert sorted(two.hops["saddle"].tolist()) == [1.0, 4.0] and sorted(two.hops["cell"][:, 0].tolist()) == [-1, 0]
    one = pw.diffusion_field(f, lattice, 300.0, mass=40.0, merge=2.5, device=-1)      # 1 - (-1) = 2 <= 2.5
    assert one.n_basins == 2 and one.n_sites == 1 and len(one.hops) == 1 and one.hops["saddle"][0] == 4.0
    assert one.hops["cell"].tolist() == [[1, 0, 0]] and not one.barrierless and one.valid
    assert close(one.populations[0], two.populations.sum(axis=0))
    free = pw.diffusion_field(f, lattice, 300.0, mass=40.0, merge=6.0, device=-1)       # 4 - (-2) = 6: it runs free
    assert free.barrierless and not free.valid


def test_the_public_layer_on_a_crystal(tmp_path):
    """guest_diffusion, MolecularSystem.calculate_guest_diffusion and DLPOLY.diffusion on the CC3 cell at a coarse grid."""
    import _percolation_cases as P
    from pywindow_amd import synth

    elements, xyz, lattice = P.cc3_cell()
    kw = dict(guest="Xe", temperatures=[250.0, 350.0], spacing=2.0, cutoff=8.0)
    one = pw.guest_diffusion(xyz, elements, lattice, device=-1, maps=True, labels=True, **kw)
    assert one.tensor.shape == (2, 3, 3) and one.maps.shape == tuple(one.shape[::-1]) and one.labels.shape == one.maps.shape
    perc = pw.guest_percolation(xyz, elements, lattice, guest="Xe", spacing=2.0, cutoff=8.0, maps=True, device=-1)
    assert one.maps.tobytes() == perc.maps.tobytes()
    assert np.abs(one.tensor - np.swapaxes(one.tensor, 1, 2)).max() <= 1e-12 * max(np.abs(one.tensor).max(), 1e-300)
    system = pw.MolecularSystem.load_system({"elements": elements, "coordinates": xyz, "lattice": lattice})
    assert system.calculate_guest_diffusion(device=-1, **kw).tensor.tobytes() == one.tensor.tobytes()
    assert system.diffusion.raw.tobytes() == one.raw.tobytes()
    with pytest.raises(ValueError, match="no unit cell"):
        pw.MolecularSystem.load_system({"elements": elements, "coordinates": xyz}).calculate_guest_diffusion(device=-1)
    frames = [xyz + np.random.default_rng(40 + k).normal(0.0, 0.02, xyz.shape) for k in range(2)]
    traj = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY", elements, frames, cell=np.asarray(lattice).T))
    got = traj.diffusion(device=-1, **kw)
    assert got.tensor.shape == (2, 2, 3, 3) and got.frames.tolist() == [0, 1] and got.coefficient.shape == (2, 2)
    values, valid = got.series("trapped_fraction", level=1)
    assert values.shape == (2,) and valid.shape == (2,)
    assert traj.diffusion(frames=[1], device=-1, **kw).tensor[0].tobytes() == got.tensor[1].tobytes()
    flat = pw.DLPOLY(synth.write_history(tmp_path / "HISTORY_flat", elements, frames[:1]))
    with pytest.raises(ValueError, match="not periodic"):
        flat.diffusion(device=-1)
    with pytest.raises(ValueError, match="mass"):
        pw.guest_diffusion(xyz, pw.lj_coefficients(elements, "Xe"), lattice, guest=(4.1, 1.8), device=-1, spacing=2.0, cutoff=8.0)


def test_an_overflow_is_run_again(monkeypatch):
    rng = np.random.default_rng(8)
    field, lattice = rng.normal(0.0, 2.0, (6, 6, 6)), np.diag([6.0, 6.0, 6.0])
    want = run(field, lattice)
    monkeypatch.setattr(DF, "B_CAP", 3)
    monkeypatch.setattr(DF, "E_CAP", 5)
    got = run(field, lattice)
    assert want.n_basins > 3 and got.valid and not (got.raw["flags"] & _lib.BAS_OVERFLOW) and got.tensor.tobytes() == want.tensor.tobytes()
