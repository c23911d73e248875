"""The equaliser's restatement (tests/eq_ref.py) against itself: the three flavours of the arithmetic on the GPU tests' inputs,
the corner run that fixes the accepted ranges and the tolerance (include/goofer_hip.h, "Tolerance"), and wrong variants that the
GPU tests' bound would catch.  Pure host code: no GPU (the ``tiled`` flavour reads the planner's tables)."""
import math

import numpy as np
import pytest

import eq_ref as R
from goofer_amd import eq as EQ

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0])


def _tiled(x, sr, bands):
    plan = EQ.plan(sr, [len(x)], bands)
    return R.tiled(x, plan.coef, plan.section_mats, plan.carry_mats)


@pytest.mark.parametrize("sr", R.CORNER_RATES)
def test_corner_run(sr):
    """The measurement behind the ranges: on every corner of the accepted range the float64 model of the kernels' scheme is
    within TOL / 4 of the long-double truth (the factor 4: the kernel's sum order is not the model's, and other inputs will do
    somewhat worse), and TOL is at most 2^-26.  The corners (eq_ref.corners, 63 chains): single bands, eight equal bands,
    chains that cut and then boost or boost and then cut, inverse pairs, unequal splits, seeded random chains.  Measured
    worst: 2^-29.44 at 96 kHz (one notch, then seven peaks of +9 dB), 2^-29.51 at 192 kHz, 2^-29.95 at 48 kHz, 2^-30.20 at
    44.1 kHz, 2^-30.35 at 8 kHz.  The carry, not the format, spends the tolerance: sequential float64 on the one-band
    corners is at 2^-39 or better."""
    x = R.hazard_input(sr)
    assert len(x) == 16 * R.TILE
    cs = R.corners(sr)
    assert len(cs) == 63 and {len(c) for c in cs} == {1, 4, 8}
    assert all(b[1] * R.F_MIN_DIV >= sr and b[3] == (R.SHELF_Q_MAX if b[0] in R.SHELVES else R.Q_MAX) for c in cs for b in c)
    assert all(abs(b[2]) == (R.MAX_GAIN_DB if b[0] in R.GAINED else 0.0) for c in cs for b in c)
    coefs = []
    for bands in cs:
        c = R.cascade_coefficients(bands, sr)
        coefs.append(np.concatenate([c, np.tile(IDENTITY, (R.MAX_BANDS - len(c), 1))]))
    truth = R.cascade_many(x, np.array(coefs))
    worst = 0.0
    for bands, t in zip(cs, truth):
        e = R.carry_error(_tiled(x, sr, bands), t)
        print("%6d Hz  %-40s 2^%.2f" % (sr, " ".join("%s%+.0f" % (b[0][:2] + b[0][-1], b[2]) for b in ([bands[0]] if bands.count(bands[0]) == len(bands) else bands))
                                         + " x%d" % len(bands), math.log2(e)))
        worst = max(worst, e)
    print("%6d Hz  worst 2^%.2f, times 4: 2^%.2f (TOL 2^%.0f)" % (sr, math.log2(worst), math.log2(4.0 * worst), math.log2(R.TOL)))
    assert R.TOL <= 2.0 ** -26 and 4.0 * worst <= R.TOL


def test_cascade_many_is_cascade():
    sr = 48000
    x = R.hazard_input(sr)[:700]
    cs = [R.chain(sr, 8), R.chain(sr, 3), R.corners(sr)[0]]
    coefs = [np.concatenate([R.cascade_coefficients(b, sr), np.tile(IDENTITY, (8 - len(b), 1))]) for b in cs]
    many = R.cascade_many(x, np.array(coefs))
    for bands, got in zip(cs, many):
        want = R.cascade(x, R.cascade_coefficients(bands, sr))
        assert np.abs(got - want).max() <= 1e-17 * np.abs(want).max()           # (the sums associate alike; the identity sections are exact)
    taps = R.cascade(x, R.cascade_coefficients(R.chain(sr, 8), sr), taps=(1, 3, 8))
    assert np.array_equal(taps[3], R.cascade(x, R.cascade_coefficients(R.chain(sr, 3), sr)))


@pytest.mark.parametrize("sr", R.RATES)
def test_the_float64_flavours_on_the_gpu_tests_inputs(sr):
    """sequential float64 leaves the bound unspent by a factor of 100; the tiled model is within it on every signal and chain"""
    xs = R.batch(sr)
    assert [len(x) for x in xs] == list(R.lengths())
    for K in R.CHAINS:
        coef = R.cascade_coefficients(R.chain(sr, K), sr)
        assert len(coef) == K
        for x, t in zip(xs, R.reference(sr, K)):
            assert len(t) == len(x)
            if len(x) == 0:
                continue
            assert R.carry_error(R.cascade(x, coef, np.float64), t) <= R.TOL / 100.0
            e = R.error(_tiled(x, sr, R.chain(sr, K)).astype(np.float32), t)
            assert e <= R.TOL / 4.0, (sr, K, len(x), e)


def test_wrong_variants_break_the_bound():
    """what the GPU tests' tolerance is there to catch, on their own inputs: the state lost at a tile boundary, a section's input
    history lost there, an fp32 state"""
    sr, K = 48000, 3
    coef = R.cascade_coefficients(R.chain(sr, K), sr)
    i = R.lengths().index(2 * R.TILE + 1)
    x, t = R.batch(sr)[i], R.reference(sr, K)[i]
    good = R.cascade(x, coef, np.float64).astype(np.float32)
    assert R.error(good, t) <= 0.0                                      # the one fp32 rounding alone
    lost = np.concatenate([R.cascade(x[:R.TILE], coef, np.float64), R.cascade(x[R.TILE:], coef, np.float64)]).astype(np.float32)
    assert R.error(lost, t) > R.TOL
    assert R.error(lost[:R.TILE], t[:R.TILE]) <= 0.0
    # a first section carried rightly and the others from zero history
    head = R.cascade(x, coef[:1], np.float64)
    half = np.concatenate([R.cascade(head[:R.TILE], coef[1:], np.float64), R.cascade(head[R.TILE:], coef[1:], np.float64)]).astype(np.float32)
    assert R.error(half, t) > R.TOL
    u = x.astype(np.float32)
    for c in coef.astype(np.float32):
        y = np.zeros_like(u)
        h1 = h2 = s1 = s2 = np.float32(0.0)
        for j, xv in enumerate(u):
            v = c[0] * xv + c[1] * h1 + c[2] * h2 - c[3] * s1 - c[4] * s2
            h2, h1, s2, s1 = h1, xv, s1, v
            y[j] = v
        u = y
    assert R.error(u, t) > R.TOL


def test_error_measure():
    t = np.array([1.0, -0.5, 0.25], dtype=np.longdouble)
    assert R.error(t.astype(np.float32), t) <= 0.0
    assert abs(R.error(np.array([1.0, -0.5, 0.25 + 2.0 ** -20]), t) - (2.0 ** -20 - 2.0 ** -26)) <= 1e-12
    assert R.error(np.array([1.0, np.nan, 0.25]), t) == math.inf
    assert R.error(np.zeros(3), np.zeros(3, dtype=np.longdouble)) == 0.0
