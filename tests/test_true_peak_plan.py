"""CPU: goofer_host_true_peak_plan against the numpy restatement (tests/true_peak_ref.py), the front ends' parsing, and the
properties the header's "true-peak detection" section states, measured on the float64 flavour of the restatement.

Property (c) is the reason for the feature: the limiter with true-peak detection keeps the 4-phase true peak of its output
within c (1 + delta_W), delta_W twice the worst value measured on exactly the inputs of ``true_peak_ref.property_inputs`` (the
quantity depends on the peaks a seed happens to make, hence the factor; the measured values stand in the header: 4.96e-3 at
W = 7, 9.85e-6 at W = 48, 7.9e-8 at W = 240).  The sample-peak limiter on the same inputs must miss: on each of the three noise
inputs it exceeds c by more than 1 dB in true peak at its worst setting (3.77, 1.54 and 3.69 dB measured; the noise low-passed
at half the Nyquist rate has little between its samples and stays at 0.6 dB at W = 240), and at every setting it misses the
bound the true-peak limiter keeps."""
import ctypes as C

import numpy as np
import pytest

import limit_ref as L
import true_peak_ref as TP
from goofer_amd import _lib
from goofer_amd import limit as LM

DELTA = {7: 2 * 4.96e-3, 48: 2 * 9.85e-6, 240: 2 * 7.9e-8}


def _call(sr, cap, args=3):
    lib = _lib.load()
    R, Z, need = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    taps = np.zeros(max(cap, 1), dtype=np.float32)
    rc = lib.goofer_host_true_peak_plan(sr, C.byref(R) if args & 1 else None, C.byref(Z) if args & 2 else None,
                                        taps.ctypes.data if cap else None, cap, C.byref(need))
    return rc, R.value, Z.value, need.value, taps[:cap]


@pytest.mark.parametrize("sr,R", [(8000, 4), (44100, 4), (48000, 4), (95999, 4), (96000, 2), (192000, 2)])
def test_table_word_for_word(sr, R):
    rc, r, z, need, _ = _call(sr, 0)
    assert (rc, r, z, need) == (1, R, TP.ZEROS, (R - 1) * 2 * TP.ZEROS) and TP.factor(sr) == R
    rc, r, z, need, taps = _call(sr, need)
    assert (rc, r, z) == (0, R, TP.ZEROS)
    want = TP.table32(R)
    assert np.array_equal(taps.view(np.int32), want.ravel().view(np.int32))
    sums = taps.astype(np.float64).reshape(R - 1, -1).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) <= 24 * 2.0 ** -25)          # 24 values of at most 1, each within half an fp32 ulp
    r2, z2, t2 = LM.true_peak_table(sr)
    assert (r2, z2) == (R, TP.ZEROS) and np.array_equal(t2, want)
    plan = LM.plan(sr, [100, 5000], 0.5, true_peak=True)
    assert plan.true_peak and plan.R == R and np.array_equal(plan.tp_taps, want) and plan.n_tiles == 3
    assert plan.blob.nbytes == plan.in_off.nbytes + plan.tiles.nbytes + plan.taps.nbytes + want.nbytes
    assert bytes(plan.blob[-want.nbytes:]) == want.tobytes()
    plain = LM.plan(sr, [100, 5000], 0.5)
    assert not plain.true_peak and plain.R == 0 and np.array_equal(plain.tiles, plan.tiles) and np.array_equal(plain.taps, plan.taps)
    meter = LM.true_peak_plan(sr, [100, 5000])
    assert meter.R == R and np.array_equal(meter.tiles, plan.tiles) and np.array_equal(meter.tp_taps, want)


def test_refusals():
    assert _call(7999, 72)[0] == -1 and _call(192001, 72)[0] == -1 and _call(0, 72)[0] == -1
    assert _call(48000, 72, args=2)[0] == -1 and _call(48000, 72, args=1)[0] == -1          # a null R, a null Z
    lib = _lib.load()
    R, Z = C.c_int(0), C.c_int(0)
    buf = np.zeros(72, np.float32)
    assert lib.goofer_host_true_peak_plan(48000, C.byref(R), C.byref(Z), buf.ctypes.data, 72, None) == -1
    assert lib.goofer_host_true_peak_plan(48000, C.byref(R), C.byref(Z), None, 72, C.byref(C.c_int64(0))) == -1
    assert lib.goofer_host_true_peak_plan(48000, C.byref(R), C.byref(Z), buf.ctypes.data, -1, C.byref(C.c_int64(0))) == -1
    rc, r, z, need, taps = _call(48000, 71)
    assert (rc, r, z, need) == (1, 4, 12, 72) and not taps.any()                            # too small: nothing written
    assert _call(96000, 23)[0] == 1 and _call(96000, 24)[0] == 0 and _call(96000, 72)[0] == 0
    for sr in (7999, 192001):
        with pytest.raises(ValueError):
            LM.true_peak_table(sr)
        with pytest.raises(ValueError):
            LM.plan(sr, [10], true_peak=True)
    with pytest.raises(ValueError):
        LM.true_peak_plan(44100.5, [10])


def test_parse_and_the_command_line(tmp_path, caplog):
    from goofer_amd import phrase as P
    assert LM.parse(0.5) == (0.5, 5.0) and LM.parse((0.25, 2)) == (0.25, 2.0)               # what they mean today
    assert LM.parse((0.25, 2, True)) == (0.25, 2.0, True) and LM.parse([0.25, 2, False]) == (0.25, 2.0, False)
    assert LM.parse(LM.Limiter(0.891, true_peak=True)) == (0.891, 5.0, True)
    assert LM.parse(LM.Limiter()) == (LM.CEILING, LM.LOOK_MS, False)
    for bad in ((0.5, 5.0, True, 1), (0.5,), (0.5, 5.0, 1.0)):
        with pytest.raises(ValueError):
            LM.parse(bad)
    assert LM.dbtp(1.0) == 0.0 and LM.dbtp(0.0) == -np.inf and abs(LM.dbtp(0.5) + 6.0206) < 1e-4
    job, out = tmp_path / "job.txt", tmp_path / "out.wav"
    job.write_text("R 240\n")
    assert P.main(["--true-peak", str(job), str(out)]) == 1                                 # the usage error: nothing is rendered
    assert "Usage" in caplog.text and "--true-peak" in caplog.text and not out.exists()
    caplog.clear()
    assert P.main(["--rate", "48000", "--true-peak", str(job), str(out)]) == 1
    assert "Usage" in caplog.text and not out.exists()


@pytest.mark.parametrize("R,under", [(4, -0.41), (2, -0.59)])
def test_properties_a_and_b(R, under):
    """(a) the meter on unit sines away from the ends reads between `under` dB (the grid of R points per sample itself: the
    reconstruction is sampled too) and +0.0005 dB (the rows are normalised at DC); (b) S = max_p sum_j |h_p[j]| is 2.2064."""
    got = TP.sine_readings(R)
    print(R, {f: ("%.4f" % lo, "%.5f" % hi) for f, (lo, hi) in got.items()})
    assert min(lo for lo, _ in got.values()) >= under and max(hi for _, hi in got.values()) <= 0.0005
    assert got[0.25][1] >= -0.001                                 # the quarter-rate sine at 45 degrees: sample peak -3.01 dBFS
    k = np.arange(512, dtype=np.float64)
    x = np.sin(0.5 * np.pi * k + 0.25 * np.pi)
    assert abs(float(TP.dbtp(np.abs(x).max())) + 3.0103) < 1e-3
    assert abs(float(TP.dbtp(TP.envelope(x, TP.table32(R), np.float64)[48:-48].max()))) < 0.001
    S = float(np.abs(TP.table32(R).astype(np.float64)).sum(axis=1).max())
    print("S", S)
    assert 2.2063 <= S <= 2.2064


@pytest.fixture(scope="module")
def inputs():
    xs = TP.property_inputs()
    assert [len(x) for x in xs] == [12000] * 5
    assert [round(float(np.abs(x).max()), 3) for x in xs] == [3.0, 1.5, 8.0, 0.95, 1.4]
    return xs


@pytest.mark.parametrize("W", TP.PROPERTY_LOOKS)
def test_property_c(inputs, W):
    t32, taps = TP.table32(4), L.table32(W)
    over = np.zeros((len(TP.PROPERTY_CEILINGS), len(inputs)))
    for k, c in enumerate(TP.PROPERTY_CEILINGS):
        got = TP.limit_batch(inputs, taps, W, c, t32, np.float64)
        plain = L.limit_batch(inputs, taps, W, c, np.float64)
        rel = [float(TP.true_peak(y, t32, np.float64)) / float(c) - 1.0 for y, *_ in got]
        over[k] = [float(TP.true_peak(y, t32, np.float64)) / float(c) for y, *_ in plain]
        print("W", W, "c %.4f" % c, "true peak / c - 1:", " ".join("%.2e" % v for v in rel), "| sample-peak limiter, dB over c:",
              " ".join("%.2f" % (20 * np.log10(v)) for v in over[k]))
        assert max(rel) <= DELTA[W], (W, float(c), rel)
        assert all(gm < 1.0 for *_, gm in got)
        assert np.all(over[k, :3] > 1.0 + DELTA[W])               # the sample-peak limiter misses the very bound


def test_the_sample_peak_limiter_misses_by_more_than_a_decibel(inputs):
    t32 = TP.table32(4)
    worst = np.zeros(3)
    for W in TP.PROPERTY_LOOKS:
        taps = L.table32(W)
        for c in TP.PROPERTY_CEILINGS:
            plain = L.limit_batch(inputs[:3], taps, W, c, np.float64)
            worst = np.maximum(worst, [20.0 * np.log10(float(TP.true_peak(y, t32, np.float64)) / float(c)) for y, *_ in plain])
    print("dB over c:", worst)
    assert np.all(worst > 1.0)
