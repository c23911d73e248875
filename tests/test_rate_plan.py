"""Output-rate conversion, host half (goofer_amd/rate.py and the library's goofer_host_rate_plan) against the numpy restatement
(tests/rate_ref.py): geometry, output offsets, the tap table, the capacity protocol and the refusals; then the quality of the
definition itself, through the float64 restatement on the library's table.  Pure host code: no GPU."""
import ctypes as C

import numpy as np
import pytest

import rate_ref as R
from goofer_amd import _lib
from goofer_amd import rate as RT


def _lengths(H):
    return [0, 1, 2, H - 1, H, 2047, 2048, 2049, 5000]


@pytest.fixture(scope="module")
def plans():
    return {pair: RT.plan(pair[0], pair[1], _lengths(R.geometry(*pair)[2])) for pair in R.PAIRS}


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: "%d-%d" % p)
def test_geometry_and_output_offsets(plans, pair):
    L, M, H = R.geometry(*pair)
    plan = plans[pair]
    assert (plan.L, plan.M, plan.H) == (L, M, H)
    lens = _lengths(H)
    assert np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lens)]))
    assert plan.out_off.dtype == np.int64 and np.array_equal(plan.out_off, R.out_offsets(lens, L, M))
    assert plan.taps.shape == (L, 2 * H) and plan.taps.dtype == np.float32
    assert plan.blob.nbytes == 2 * 8 * (len(lens) + 1) + 4 * L * 2 * H


def test_known_geometries():
    assert R.geometry(44100, 48000) == (160, 147, 32)
    assert R.geometry(48000, 44100) == (147, 160, 35)
    assert R.geometry(44100, 22050) == (1, 2, 64)
    assert R.geometry(44100, 8000) == (80, 441, 177)
    m, q, p = R.index(10, 160, 147)
    assert m == 11 and q.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9] and p[1] == 147 and p[2] == 134


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: "%d-%d" % p)
def test_taps_match_the_restatement(plans, pair):
    got, want64 = plans[pair].taps, R.taps64(*pair)
    want = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= np.maximum(ulp, 1e-12)), float(err.max())
    print(pair, "taps that differ from the restatement's:", int((got != want).sum()), "of", got.size)
    sums = got.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) <= 1e-7), float(np.abs(sums - 1.0).max())
    print(pair, "row sums within %.2e, max_p sum |h| %.3f" % (np.abs(sums - 1).max(), np.abs(got.astype(np.float64)).sum(axis=1).max()))


def _call(sr_in, sr_out, in_off, n, cap, taps=True, out=True, need=True, geo=True):
    lib = _lib.load()
    L, M, H, nd = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int64(-7)
    t = np.zeros(max(cap, 1), dtype=np.float32)
    o = np.full(n + 1, -7, dtype=np.int64)
    rc = lib.goofer_host_rate_plan(sr_in, sr_out, None if in_off is None else in_off.ctypes.data, n,
                                   C.byref(L) if geo else None, C.byref(M), C.byref(H), t.ctypes.data if taps else None, cap,
                                   C.byref(nd) if need else None, o.ctypes.data if out else None)
    return rc, (L.value, M.value, H.value), nd.value, t, o


def test_refusals_and_the_capacity_protocol():
    off = np.array([0, 100, 300], dtype=np.int64)
    assert _call(44100, 44100, off, 2, 100000)[0] == -1                    # equal rates
    assert _call(0, 48000, off, 2, 100000)[0] == -1                        # a rate of 0
    assert _call(44100, 0, off, 2, 100000)[0] == -1
    assert _call(44100, -5, off, 2, 100000)[0] == -1
    assert _call(11025, 96000, off, 2, 400000)[0] == -1                    # L = 1280
    assert _call(96000, 11025, off, 2, 400000)[0] == -1                    # M = 1280
    assert _call(44100, 48000, None, 2, 100000)[0] == -1                   # null pointers
    assert _call(44100, 48000, off, 2, 100000, taps=False)[0] == -1
    assert _call(44100, 48000, off, 2, 100000, out=False)[0] == -1
    assert _call(44100, 48000, off, 2, 100000, need=False)[0] == -1
    assert _call(44100, 48000, off, 2, 100000, geo=False)[0] == -1
    assert _call(44100, 48000, off, -1, 100000)[0] == -1
    assert _call(44100, 48000, off, 2, -1)[0] == -1
    assert _call(44100, 48000, np.array([0, 100, 50], dtype=np.int64), 2, 100000)[0] == -1            # offsets that decrease
    assert _call(44100, 48000, np.array([0, 1 << 31], dtype=np.int64), 1, 100000)[0] == -1            # 2^31 samples
    rc, geo, need, _, out = _call(44100, 48000, np.array([0, (1 << 31) - 1], dtype=np.int64), 1, 100000)
    assert rc == 0 and out[1] == (((1 << 31) - 1) * 160 + 146) // 147
    # a cap that is too small: 1, with need and the geometry; nothing else is promised
    rc, geo, need, _, _ = _call(44100, 48000, off, 2, 10239)
    assert rc == 1 and geo == (160, 147, 32) and need == 160 * 64
    rc, geo, need, _, _ = _call(44100, 48000, off, 2, 0, taps=False)       # the size query: no table to write to
    assert rc == 1 and need == 10240
    rc, geo, need, taps, out = _call(44100, 48000, off, 2, 10240)
    assert rc == 0 and need == 10240 and out.tolist() == [0, 109, 327]
    assert np.array_equal(taps, RT.plan(44100, 48000, [100, 200]).taps.ravel())
    rc, _, _, _, out = _call(44100, 48000, None, 0, 10240)                 # no signal: the table alone
    assert rc == 0 and out.tolist() == [0]
    for bad in ((44100, 44100), (0, 48000), (11025, 96000)):
        with pytest.raises(ValueError):
            RT.plan(bad[0], bad[1], [100])
    with pytest.raises(ValueError):
        RT.plan(44100, 48000, [100, -1])


def _sine_case(pair, frac, taps):
    """(y float64, analytic sine at the output instants, interior slice) of a unit sine at ``frac`` of the lower Nyquist rate"""
    sr_in, sr_out = pair
    L, M, H = R.geometry(*pair)
    f = frac * min(sr_in, sr_out) / 2.0
    n = 6000
    x = np.sin(2.0 * np.pi * f * np.arange(n, dtype=np.float64) / sr_in + 0.3).astype(np.float32)
    y, _ = R.convert(x, taps, L, M, H, np.float64)
    # the input is the fp32 sine: the analytic output is judged against the sine the converter was given, rounding included,
    # so its 2^-25 input rounding is inside the tolerance (the row sums bound its gain by 2.3)
    want = np.sin(2.0 * np.pi * f * np.arange(len(y), dtype=np.float64) / sr_out + 0.3)
    cut = R.margin(L, M, H)
    return x, y, want, slice(cut, len(y) - cut)


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: "%d-%d" % p)
def test_sines_come_out_as_sines(plans, pair):
    for frac in (0.02, 0.5, 0.8):
        _, y, want, mid = _sine_case(pair, frac, plans[pair].taps)
        assert mid.stop - mid.start > 100
        err = float(np.abs(y[mid] - want[mid]).max())
        print(pair, frac, "worst %.3e" % err)
        assert err <= 1e-6


# the down-conversions whose input can hold the tone at all: 1.12 of the new Nyquist rate lies below the old one (48 -> 44.1 kHz
# cannot: 24.7 kHz is no tone at 48 kHz)
@pytest.mark.parametrize("pair", [p for p in R.PAIRS if 1.12 * p[1] < p[0]], ids=lambda p: "%d-%d" % p)
def test_a_tone_above_the_new_nyquist_rate_is_removed(plans, pair):
    sr_in, sr_out = pair
    L, M, H = R.geometry(*pair)
    f = 1.12 * sr_out / 2.0
    x = np.sin(2.0 * np.pi * f * np.arange(6000, dtype=np.float64) / sr_in + 0.3).astype(np.float32)
    y, _ = R.convert(x, plans[pair].taps, L, M, H, np.float64)
    cut = R.margin(L, M, H)
    worst = float(np.abs(y[cut:len(y) - cut]).max())
    print(pair, "alias %.3e" % worst)
    assert len(y) - 2 * cut > 100 and worst <= 1e-6
