"""CPU: the restatement of the convolution reverb (tests/reverb_ref.py) against np.convolve, the tolerance GOOFER_REVERB_TOL
measured on the model of the kernels' scheme, and ``synthetic_ir`` by property.

The tolerance is not chosen.  ``tiled``, the kernels' scheme in np.float32 / np.complex64, runs against the float64 restatement on
the cases of tests/test_gpu_reverb.py (the batch with every IR length, pre-delay and tail setting, the impulses at the block
edges, the two long IRs, the 70 partitions with a dead one); the worst max|err| / max|ref| per signal times 4, rounded up to a power of two, is the constant in
include/goofer_hip.h, goofer_amd/reverb.py and here.  Measured: worst 2^-21.73 (the batch, L = 2 B + 5); 2^-22.85 with 256
partitions.  The factor covers the kernels' other FFT factorisation and their fused multiply-adds, both absent from the model."""
import math

import numpy as np
import pytest

import reverb_ref as R
from goofer_amd import reverb as RV

TOL = 2.0 ** -19


def test_the_restatement_is_np_convolve():
    xs = R.signals()
    for L, pre, tail in [(1, 0, True), (5, 3, True), (R.B + 1, 0, False), (300, R.B + 3, True), (2 * R.B + 5, 1, False)]:
        h = R.ir(L)
        for x in xs:
            a, b = R.reference(x, h, pre, tail, R.DRY, R.WET), R.direct(x, h, pre, tail, R.DRY, R.WET)
            assert a.shape == b.shape == (R.n_out(len(x), L, pre, tail),)
            if len(a):
                assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))
    # by hand: x = [1, 2], h = [1, 10, 100], pre 2, dry 0.5, wet 2
    want = np.array([0.5, 1.0, 2.0, 24.0, 240.0, 400.0])
    assert np.allclose(R.reference([1, 2], [1, 10, 100], 2, True, 0.5, 2.0), want, atol=1e-12)
    assert np.allclose(R.reference([1, 2], [1, 10, 100], 2, False, 0.5, 2.0), want[:2], atol=1e-12)
    assert len(R.reference([], [1, 2, 3])) == 0


def test_the_tolerance_is_four_times_the_models_worst_error():
    assert TOL == R.TOL == RV.TOL
    worst, where = 0.0, None
    xs = R.signals()
    for L, pre, tail in R.batch_cases():
        h = R.ir(L)
        for i, x in enumerate(xs):
            e = R.error(R.tiled(x, h, pre, tail, R.DRY, R.WET), R.reference(x, h, pre, tail, R.DRY, R.WET))
            if e > worst:
                worst, where = e, ("batch", L, pre, tail, i)
    h = R.ir(R.IMPULSE_LEN)
    for pre in R.IMPULSE_PRE:
        for q in R.IMPULSE_AT:
            x = R.impulse(q)
            e = R.error(R.tiled(x, h, pre, True, 0.0, 1.0), R.reference(x, h, pre, True, 0.0, 1.0))
            if e > worst:
                worst, where = e, ("impulse", pre, q)
    for x, h in R.long_cases():
        e = R.error(R.tiled(x, h), R.reference(x, h))
        if e > worst:
            worst, where = e, ("long", len(h))
    xs, h = R.dead_case()
    for i, x in enumerate(xs):
        e = R.error(R.tiled(x, h, 2, True, R.DRY, R.WET), R.reference(x, h, 2, True, R.DRY, R.WET))
        if e > worst:
            worst, where = e, ("dead partition", i)
    print("worst max|err| / max|ref| of the model: %.3e = 2^%.2f at %r; the rule gives 2^%d" %
          (worst, math.log2(worst), where, round(math.log2(R.tolerance_rule(worst)))))
    assert R.tolerance_rule(worst) == TOL


def test_the_model_skips_dead_partitions_to_the_same_bits():
    h = R.ir(5 * R.B)
    h[R.B:2 * R.B] = 0.0
    h[3 * R.B:4 * R.B] = 0.0
    assert R.ir_spectra(h)[1].tolist() == [True, False, True, False, True]
    x = 0.3 * R.noise(6 * R.B + 9, 5)
    assert np.array_equal(R.words(R.tiled(x, h, skip=True)), R.words(R.tiled(x, h, skip=False)))


def test_a_wrong_block_index_breaks_the_bound():
    """the bound is tight enough to see the overlap-save indexing: the convolution shifted by one sample misses it"""
    x, h = R.signals()[5], R.ir(R.B + 1)
    ref = R.reference(x, h, 0, True, 0.0, 1.0)
    assert R.error(R.tiled(x, h, 0, True, 0.0, 1.0), ref) <= TOL / 4
    assert R.error(np.roll(R.tiled(x, h, 0, True, 0.0, 1.0), 1), ref) > 1000 * TOL


@pytest.mark.parametrize("sr, room", [(48000, RV.Room(0.5)), (44100, RV.Room(1.0, 3, 4000.0)), (8000, RV.Room(0.25, 9))])
def test_synthetic_ir_by_property(sr, room):
    h = RV.synthetic_ir(sr, room)
    assert h.dtype == np.float32 and h.shape == (math.ceil(room.rt60 * sr),)
    assert abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    assert np.array_equal(h, RV.synthetic_ir(sr, RV.Room(room.rt60, room.seed, room.damping_hz)))
    assert not np.array_equal(h, RV.synthetic_ir(sr, RV.Room(room.rt60, room.seed + 1, room.damping_hz)))
    # the energy decay curve (Schroeder's backward integral) falls by 60 dB per rt60: a line fitted from -5 to -35 dB
    edc = np.cumsum(h[::-1].astype(np.float64) ** 2)[::-1]
    db = 10.0 * np.log10(edc / edc[0])
    k = np.nonzero((db <= -5.0) & (db >= -35.0))[0]
    slope = np.polyfit(k / float(sr), db[k], 1)[0]
    print("%d Hz, rt60 %g s: decay %.2f dB/s (wanted %.2f)" % (sr, room.rt60, slope, -60.0 / room.rt60))
    assert abs(slope * room.rt60 + 60.0) <= 0.05 * 60.0


def test_synthetic_ir_refusals():
    for sr, room in ((7999, 0.5), (192001, 0.5), (48000.5, 0.5), (48000, 6.0), (48000, RV.Room(0.5, 0, 24000.0))):
        with pytest.raises(ValueError):
            RV.synthetic_ir(sr, room)
    for bad in (dict(rt60=0.0), dict(rt60=float("nan")), dict(rt60=-1.0), dict(rt60=1.0, seed=-1), dict(rt60=1.0, seed=0.5),
                dict(rt60=1.0, damping_hz=0.0), dict(rt60=1.0, damping_hz=float("inf"))):
        with pytest.raises(ValueError):
            RV.Room(**bad)
    assert len(RV.synthetic_ir(48000, 2.0 ** 18 / 48000.0)) == 2 ** 18
