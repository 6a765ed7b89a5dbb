"""Spectra on the host path (device = -1): the sums of pw_dft_sums against the definition itself bit for bit, the
twiddles against mpmath, the sums against a long-double direct sum and the FFT within DERIVED bounds, the Lomb-Scargle
power against SciPy, batches, error paths and the route from the series of a record store.  tests/test_gpu_dft.py
holds the device to the host path bit for bit.

The bars are derived, not measured: a twiddle is within (3 pi + 1.1) 2^-53 of the truth; a sum within
(512 + chunks + 32) 2^-53 sum |a[t]|.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import _dft_cases as C
from pywindow_amd import _lib, records, spectra, synth
from pywindow_amd.trajectory import DLPOLY

EPS = C.EPS


@pytest.fixture(scope="module")
def host():
    return _lib.Context(-1, host_threads=8)


def fma(x, y, z):
    """Correctly rounded x * y + z (exact rational arithmetic, one rounding)."""
    return float(Fraction(x) * Fraction(y) + Fraction(z))


# ---- the definition ------------------------------------------------------------------------------------------

def definition(host, a, period, j):
    """pw_dft.hpp restated: twiddles from the library's hook, everything else in exact rational arithmetic."""
    n = len(a)
    starts = np.arange(0, n, C.CHUNK)
    cA, sA = C.twiddles(host, j, period, np.arange(min(n, C.CHUNK)))
    cB, sB = C.twiddles(host, j, period, starts)
    re = im = 0.0
    for ch, t0 in enumerate(starts.tolist()):
        pc = ps = 0.0
        for r in range(min(C.CHUNK, n - t0)):
            pc = fma(a[t0 + r], cA[r], pc)
            ps = fma(a[t0 + r], sA[r], ps)
        re = re + fma(cB[ch], pc, -(sB[ch] * ps))
        im = im + fma(sB[ch], pc, cB[ch] * ps)
    return re, im


@pytest.mark.parametrize("n", (1, 2, 511, 512, 513, 1025))
def test_the_definition_bit_for_bit(host, n):
    jobs = C.edge_jobs((n,))
    assert {j[1] for j in jobs} == {max(n, 2), 4 * n + 1, 1 << 31} and {j[3] for j in jobs} == {1, 2}
    got = host.dft_sums(*C.pack(jobs))
    at = 0
    for a, period, first, step, count in jobs:
        js = [first + q * step for q in range(count)]
        assert 0 in js or period - 1 in js
        for q, j in enumerate(js):
            re, im = definition(host, a.tolist(), period, j)
            want = np.array([re, im])
            have = np.array([got[at + q].real, got[at + q].imag])
            assert have.tobytes() == want.tobytes(), (n, period, j)
        at += count
    assert at == len(got)


# ---- twiddles ------------------------------------------------------------------------------------------------

def test_twiddles_against_mpmath(host):
    import mpmath

    mpmath.mp.dps = 50
    worst = 0.0
    for j, period, k in C.twiddle_cases():
        c, s = C.twiddles(host, j, period, k)
        for kk, cc, ss in zip(k.tolist(), c.tolist(), s.tolist()):
            ang = 2 * mpmath.pi * ((j * kk) % period) / period       # Python integers: the exact phase
            err = max(abs(mpmath.mpf(cc) - mpmath.cos(ang)), abs(mpmath.mpf(ss) - mpmath.sin(ang)))
            worst = max(worst, float(err) / EPS)
    print(f"DFT twiddles: worst error {worst:.2f} x 2^-53 (derived bound {C.TWIDDLE_BOUND:.2f})")
    assert worst <= C.TWIDDLE_BOUND


# ---- accuracy ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.accuracy_cases(), ids=lambda c: c[0])
def test_against_long_double(host, case):
    name, a, period, first, step, count = case
    got = host.dft_sums(*C.pack([case[1:]]))
    assert got.shape == (count,)
    j = first + step * np.arange(count)
    re, im = C.long_double_sums(a, period, j)
    bound = C.derived_bound(len(a), float(np.sum(np.abs(a).astype(C.LD))))
    err = np.maximum(np.abs(got.real.astype(C.LD) - re), np.abs(got.imag.astype(C.LD) - im)).astype(np.float64)
    print(f"DFT {name}: n={len(a)} x {count} worst error / bound = {err.max() / bound:.2e}")
    assert (err <= bound).all() and np.abs(got).max() > 0.0


@pytest.mark.parametrize("n", (1, 2, 511, 512, 513, 1025, 1300, 100_000))
def test_against_the_fft(host, n):
    a = np.random.default_rng(n).standard_normal(n)
    if n == 1:                                     # the smallest period is 2: only j = 0, against the sum itself
        got = host.dft_sums(*C.pack([(a, 2, 0, 1, 1)]))
        assert got[0] == a[0]
        return
    count = min(n // 2 + 1, 300)
    got = host.dft_sums(*C.pack([(a, n, 0, 1, count)]))
    want = np.fft.rfft(a)[:count]
    weight = float(np.sum(np.abs(a)))
    bound = C.derived_bound(n, weight) + math.log2(n) * EPS * weight
    err = np.maximum(np.abs(got.real - want.real), np.abs(-got.imag - want.imag))
    print(f"DFT fft n={n}: worst difference / bound = {err.max() / bound:.2e}")
    assert (err <= bound).all()


# ---- Lomb-Scargle against SciPy ------------------------------------------------------------------------------

def gls_long_double(y, ok, period, j):
    """The issue's formula evaluated in long double from long-double sums with exact integer phases."""
    n = C.LD(int(ok.sum()))
    mask = ok.astype(np.float64)
    yr, yi = C.long_double_sums(y, period, j)
    mr, mi = C.long_double_sums(mask, period, j)
    m2r, m2i = C.long_double_sums(mask, period, 2 * np.asarray(j))
    c, s, yc, ys = mr / n, mi / n, yr / n, yi / n
    yy = np.sum(y.astype(C.LD) ** 2) / n
    cc, ss, cs = (1 + m2r / n) / 2 - c * c, (1 - m2r / n) / 2 - s * s, m2i / (2 * n) - c * s
    d = cc * ss - cs * cs
    return (ss * yc * yc + cc * ys * ys - 2 * cs * yc * ys) / (yy * d), d


GLS_CASES = [(n, gaps, 0.5 if n <= 1300 else 0.0125) for n in (100, 1300, 20_000) for gaps in (0.0, 0.3, 0.9)]


@pytest.mark.parametrize("n,gaps,fmax", GLS_CASES)
def test_power_against_scipy(n, gaps, fmax):
    """E: the largest deviation from the long-double evaluation, relative to the peak power.  E_ours <= max(4 E_scipy,
    derived), derived = 24 (512 + chunks + 32) 2^-53 / (min D x peak); frequencies with D below 1e-6 of
    its maximum are left out (fewer than 1 % of the grid).  The truth is taken at up to 256 frequencies (n = 20 000: 64 of the
    1000) spread over the grid and the peak."""
    from scipy import signal

    rng = np.random.default_rng(n + int(100 * gaps))
    t = np.arange(n)
    v = 2.0 + np.cos(2.0 * np.pi * 0.0371 * t + 0.4) + 0.5 * C.ar1(n, 0.5, n)
    ok = rng.random(n) >= gaps
    sp = spectra.lomb_scargle(v, ok, max_frequency=fmax, device=-1)
    assert sp.period == 4 * n and sp.n_valid == ok.sum() and sp.j[0] == 1
    assert len(sp.j) == min(-(-sp.period // 2) - 1, math.floor(fmax * sp.period))
    theirs = signal.lombscargle(t[ok].astype(np.float64), v[ok], 2.0 * np.pi * sp.j / sp.period, normalize=True,
                                floating_mean=True)
    pick = np.unique(np.concatenate([np.linspace(0, len(sp.j) - 1, min(len(sp.j), 256 if n <= 1300 else 64)).astype(int),
                                     [int(np.nanargmax(sp.power))]]))
    y = np.where(ok, v - sp.mean, 0.0)
    truth, d = gls_long_double(y, ok, sp.period, sp.j[pick])
    d64 = d.astype(np.float64)
    keep = d64 >= 1e-6 * d64.max()
    assert (~keep).sum() < 0.01 * len(pick)
    peak = float(np.max(truth[keep]))
    e_ours = float(np.max(np.abs(sp.power[pick][keep].astype(C.LD) - truth[keep]))) / peak
    e_scipy = float(np.max(np.abs(theirs[pick][keep].astype(C.LD) - truth[keep]))) / peak
    derived = 24.0 * (C.CHUNK + -(-n // C.CHUNK) + C.K) * EPS / (float(d64[keep].min()) * peak)
    print(f"GLS n={n} gaps={gaps}: E_ours={e_ours:.2e} E_scipy={e_scipy:.2e} derived={derived:.2e} "
          f"D in {d64.min():.2e} .. {d64.max():.2e}, left out {(~keep).sum()} of {len(pick)}")
    assert e_ours <= max(4.0 * e_scipy, derived)


# ---- physics -------------------------------------------------------------------------------------------------

def test_the_peak_of_a_gapped_sinusoid():
    rng = np.random.default_rng(40)
    n, f = 3000, 0.01234
    t = np.arange(n)
    v = 7.0 + 0.8 * np.sin(2.0 * np.pi * f * t + 1.0) + 0.5 * rng.standard_normal(n)
    ok = rng.random(n) >= 0.4
    v[~ok] = np.nan                                # what a gap holds is ignored
    sp = spectra.lomb_scargle(v, ok, device=-1)
    assert abs(sp.peak_frequency - f) <= 1.0 / sp.period
    assert sp.peak_power == np.nanmax(sp.power) and sp.peak_period == 1.0 / sp.peak_frequency
    assert abs(sp.amplitude[np.nanargmax(sp.power)] - 0.8) < 0.05 and 0.0 < sp.peak_power <= 1.0
    scaled = spectra.lomb_scargle(v, ok, stride=5, dt=0.002, device=-1)       # frames of 5 steps of 0.002 ps
    assert np.allclose(scaled.frequency, sp.frequency / 0.01, rtol=1e-15) and scaled.power.tobytes() == sp.power.tobytes()


# ---- batches -------------------------------------------------------------------------------------------------

def test_a_batch_equals_its_jobs_one_at_a_time(host):
    jobs = C.mixed_batch()
    assert len(jobs) == 64 and any(len(j[0]) == 0 for j in jobs) and any(j[4] == 0 for j in jobs)
    rec, series = C.pack(jobs)
    batch = host.dft_sums(rec, series)
    for j, r in zip(jobs, rec):
        if len(j[0]) == 0 or j[4] == 0:
            continue
        alone = host.dft_sums(*C.pack([j]))
        assert alone.tobytes() == batch[int(r["out_first"]):int(r["out_first"] + r["n_freq"])].tobytes()
    for threads in (1, 3, 16):                     # the number of host threads takes no part
        assert batch.tobytes() == _lib.Context(-1, host_threads=threads).dft_sums(rec, series).tobytes()
    for budget in (1, 100_000, 1 << 30):           # nor does the budget of the workspace
        assert batch.tobytes() == C.internal_sums(host, rec, series, workspace_bytes=budget)[:len(batch)].tobytes()
    # frequencies of one job, and the Python wrappers
    a = jobs[12][0]
    whole = spectra.dft_sums(a, np.arange(3, 40), 4 * len(a) + 1, device=-1)
    each = spectra.dft_sums_batch([(a, [j], 4 * len(a) + 1) for j in range(3, 40)], device=-1)
    assert whole.tobytes() == np.concatenate(each).tobytes()
    assert spectra.dft_sums(a, [7, 3, 4], 100, device=-1).tobytes() == spectra.dft_sums(a, np.arange(3, 8), 100, device=-1)[[4, 0, 1]].tobytes()
    assert spectra.dft_sums_batch([], device=-1) == [] and spectra.dft_sums(a, [], 100, device=-1).shape == (0,)


# ---- bad arguments -------------------------------------------------------------------------------------------

def test_bad_arguments_write_nothing(host):
    good = (np.arange(5.0), 20, 1, 1, 3)
    x = np.arange(3.0)
    for bad, what in (((np.array([1.0, np.nan, 2.0]), 12, 1, 1, 2), "NaN"),
                      ((np.array([1.0, np.inf, 2.0]), 12, 1, 1, 2), "NaN or an infinity"),
                      ((x, 1, 0, 1, 1), "period"), ((x, (1 << 31) + 1, 0, 1, 1), "period"),
                      ((x, 12, 0, 0, 2), "j_step"), ((x, 12, 12, 1, 1), "j_first"), ((x, 12, -1, 1, 1), "j_first"),
                      ((x, 12, 10, 1, 3), "n_freq - 1"), ((x, 12, 8, 2, 3), "n_freq - 1"), ((x, 12, 0, 1, -1), "negative")):
        rec, series = C.pack([good, bad])
        with pytest.raises(ValueError, match="job 1: .*" + what):
            host.dft_sums(rec, series)
        rec["out_first"][1] = 3
        re, im = np.full(16, -7.0), np.full(16, -7.0)     # the raw entry with a sentinel in the result
        rc = _lib.load().pw_dft_sums(host._h, rec.ctypes.data, len(rec), series.ctypes.data, re.ctypes.data, im.ctypes.data)
        assert rc == -2 and (re == -7.0).all() and (im == -7.0).all()
        assert b"job 1" in _lib.load().pw_last_error()
    rec, series = C.pack([good])
    with pytest.raises(IndexError):
        host.dft_sums(rec, series[:4])
    assert host.dft_sums(rec[:0], series).shape == (0,)            # no job: nothing to do
    rec, series = C.pack([(np.zeros(0), 20, 1, 1, 3), (np.arange(4.0), 20, 1, 1, 0), (np.arange(5.0), 4, 0, 1, 2)])
    got = host.dft_sums(rec, series)                               # n == 0, n_freq == 0 write nothing
    assert got.shape == (2,) and got[0] == 10.0 and abs(got[1] - complex(2.0, -2.0)) < 1e-14


def test_error_paths_of_the_python_surface():
    x = np.arange(10.0)
    with pytest.raises(ValueError, match="constant"):
        spectra.lomb_scargle(np.full(10, 2.0), device=-1)
    with pytest.raises(ValueError, match="fewer than three valid"):
        spectra.lomb_scargle(x, np.arange(10) < 2, device=-1)
    with pytest.raises(ValueError, match="NaN"):
        spectra.lomb_scargle(np.array([1.0, np.nan, 3.0, 4.0]), device=-1)
    with pytest.raises(ValueError, match="max_frequency"):
        spectra.lomb_scargle(x, max_frequency=0.7, device=-1)
    with pytest.raises(ValueError, match="one flag"):
        spectra.lomb_scargle(x, np.ones(9, dtype=bool), device=-1)
    with pytest.raises(ValueError, match="integers"):
        spectra.dft_sums(x, [0.5], 10, device=-1)
    with pytest.raises(ValueError, match="outside"):
        spectra.dft_sums(x, [10], 10, device=-1)
    assert spectra.lomb_scargle_batch([], device=-1) == []
    sp = spectra.lomb_scargle(x + np.sin(x), device=-1)
    assert isinstance(sp, spectra.Spectrum) and sp.sums.shape == (3, len(sp.j)) and sp.sums.dtype == np.complex128
    with pytest.raises(Exception):
        sp.period = 3                              # frozen
    # singular fits are nan: three valid entries one period apart see the same phase at j = period / 4 ...
    ok = np.zeros(16, dtype=bool)
    ok[[0, 4, 8, 12]] = True
    sp = spectra.lomb_scargle(np.arange(16.0) ** 2, ok, oversample=1, device=-1)
    assert np.isnan(sp.power[3]) and np.isnan(sp.amplitude[3]) and np.isfinite(sp.power[0])


# ---- series of a store ---------------------------------------------------------------------------------------

def same_spectrum(a, b):
    for f in ("frequency", "j", "power", "amplitude", "sums"):
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False
    return (a.period, a.n_valid, a.mean, a.peak_frequency, a.peak_power, a.peak_period) == \
           (b.period, b.n_valid, b.mean, b.peak_frequency, b.peak_power, b.peak_period)


def test_trajectory_spectrum_and_per_molecule(tmp_path):
    path = synth.write_synthetic_history(tmp_path / "HISTORY", 20)
    traj = DLPOLY(path)
    order = [7, 2, 3] + [f for f in range(19, -1, -1) if f not in (7, 2, 3)]
    traj.analysis(frames=order, device=-1)
    store = traj.analysis_store
    frames, a, ok = store.series("windows_min")
    got = traj.spectrum("windows_min", device=-1)
    assert same_spectrum(got, spectra.lomb_scargle(a, ok, device=-1))
    assert got.period == 80 and got.j.tolist() == list(range(1, 40)) and got.n_valid == ok.sum()
    fine = traj.spectrum("maximum_diameter", oversample=8, max_frequency=0.25, dt=0.5, device=-1)
    assert same_spectrum(fine, spectra.lomb_scargle(store.series("maximum_diameter")[1], None, 8, 0.25, 1, 0.5, device=-1))
    assert fine.period == 160 and len(fine.j) == 40 and fine.frequency[-1] == 40 / (160 * 0.5)
    with pytest.raises(ValueError, match="modular"):
        store.spectrum("maximum_diameter", per_molecule=True, device=-1)
    # a modular store: two molecules a frame, frames 0, 2, 4, ...
    recs = np.concatenate([store.records, store.records[::-1]])
    pos = np.concatenate([np.arange(20), np.arange(20)])
    by = np.argsort(pos, kind="stable")
    modular = records.RecordStore(recs[by], 2 * pos[by], np.tile([0, 1], 20))
    each = modular.spectrum("pore_diameter", per_molecule=True, device=-1)
    assert sorted(each) == [0, 1]
    for m in (0, 1):
        only = records.RecordStore(modular.records[m::2], modular.unit_frame[m::2])
        assert same_spectrum(each[m], only.spectrum("pore_diameter", device=-1))
        assert same_spectrum(each[m], modular.spectrum("pore_diameter", molecule=m, device=-1))
        assert each[m].frequency[0] == 1 / (80 * 2.0)              # the stride of the frame axis is passed on
    assert each[0].sums.tobytes() != each[1].sums.tobytes()
    with pytest.raises(ValueError, match="molecule="):
        modular.spectrum("maximum_diameter", device=-1)
