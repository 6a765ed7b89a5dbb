"""``bench.py --dump-outputs DIR``: the records of the last timed step, one float64 ``.npy`` per field, and past the
byte budget a fixed, seeded sample of units -- so that two builds can be compared output for output."""
import importlib.util
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records(n):
    from pywindow_amd import _lib

    rec = np.zeros(n, dtype=_lib.UNIT_OUT_DTYPE)
    rec["n_atoms"] = 168
    rec["status"] = np.arange(n) % 3
    rec["pore_d"] = np.arange(n) * 1.5 + 1.0 / 3.0
    rec["n_windows"] = np.arange(n) % 5
    rec["win_c"][:, 2, 1] = -np.arange(n) * 0.25
    return rec


def test_dump_outputs_writes_every_field_as_float64(tmp_path):
    bench = _load_bench()
    rec = _records(7)
    bench.dump_outputs(str(tmp_path), rec)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([n + ".npy" for n in rec.dtype.names] + ["unit_index.npy"])
    for name in rec.dtype.names:
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == rec[name].shape, name
        assert np.array_equal(got, rec[name]), name
    assert np.array_equal(np.load(tmp_path / "unit_index.npy"), np.arange(7.0))


def test_dump_outputs_keeps_a_fixed_sample_within_the_budget(tmp_path):
    bench = _load_bench()
    rec = _records(5000)
    budget = 1 << 20
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), rec, budget=budget)
    index = np.load(tmp_path / "a" / "unit_index.npy")
    assert 0 < len(index) < len(rec) and np.all(np.diff(index) > 0)
    keep = index.astype(np.int64)
    total = 0
    for name in rec.dtype.names + ("unit_index",):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.tobytes() == b.tobytes(), name                     # the same sample every run
        if name != "unit_index":
            assert np.array_equal(a, rec[name][keep]), name
        total += a.nbytes
    assert total <= budget
