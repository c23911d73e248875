"""The restatement of the stereo bus (tests/bus_ref.py) checked against the properties the header states (no GPU): the ceiling on
both channels, identity under the ceiling, a pair (x, x) against the mono limiter, the quiet channel beside a burst, the order
of the mix's sum, the linked loudness gate, and the interleaving."""
import numpy as np
import pytest

import bus_ref as R
import limit_ref as LR
import loudness_ref as LD
import true_peak_ref as TR


@pytest.fixture(scope="module")
def pair():
    return R.burst_pair()


@pytest.mark.parametrize("W", R.LOOKS)
@pytest.mark.parametrize("c", R.CEILINGS)
def test_ceiling_and_linked_gain(pair, W, c):
    L, Rq = pair
    (yl, yr), g, peak, gmin = R.limit_linked([L, Rq], LR.table32(W), W, c)
    bound = float(c) * (1.0 + 2.0 ** -22)
    assert np.abs(yl).max() <= bound and np.abs(yr).max() <= bound
    assert peak == np.float32(1.5) and gmin == g.min() and gmin < 1.0
    assert np.array_equal(LR.words(yl), LR.words(L * g)) and np.array_equal(LR.words(yr), LR.words(Rq * g))
    # the quiet channel beside the burst IS reduced, by the very gain of the loud one, on both sides of the tile boundary
    hit = np.flatnonzero(g < 1.0)
    assert hit.min() < 4096 <= hit.max() and np.abs(Rq).max() < c
    assert np.array_equal(yr[hit], Rq[hit] * g[hit]) and not np.array_equal(yr[hit], Rq[hit])
    far = np.ones(len(g), bool)
    far[max(0, 4090 - 2 * W):4100 + 2 * W + 1] = False
    assert np.array_equal(LR.words(yl[far]), LR.words(L[far])) and np.array_equal(LR.words(yr[far]), LR.words(Rq[far]))


@pytest.mark.parametrize("W", R.LOOKS)
@pytest.mark.parametrize("c", R.CEILINGS)
def test_identity_and_mono_pair(pair, W, c):
    taps = LR.table32(W)
    quiet = (pair[1] * np.float32(0.9)).astype(np.float32)     # |x| <= 0.27 < every ceiling
    (a, b), g, _, gmin = R.limit_linked([quiet, -quiet[::-1].copy()], taps, W, c)
    assert np.array_equal(LR.words(a), LR.words(quiet)) and np.array_equal(LR.words(b), LR.words(-quiet[::-1])) and gmin == 1.0 and (g == 1.0).all()
    x = pair[0]
    (a, b), g, peak, gmin = R.limit_linked([x, x], taps, W, c)
    y, g1, peak1, gmin1 = LR.limit(x, taps, W, c)
    assert np.array_equal(LR.words(a), LR.words(y)) and np.array_equal(LR.words(b), LR.words(y)) and (peak, gmin) == (peak1, gmin1)
    (a,), _, _, _ = R.limit_linked([x], taps, W, c)
    assert np.array_equal(LR.words(a), LR.words(y))


def test_true_peak_form():
    c, W = np.float32(0.891), 48
    tp = TR.table32(4)
    rng = np.random.default_rng(8)
    L = np.zeros(600, np.float32)
    L[300:300 + 36] = TR.burst(c)                               # samples under c, reconstruction above it
    Rq = (0.2 * rng.uniform(-1, 1, 600)).astype(np.float32)
    (yl, yr), g, peak, gmin = R.limit_linked([L, Rq], LR.table32(W), W, c, tp)
    assert np.abs(L).max() < c < peak and gmin < 1.0
    yt, gt, peak_t, _ = TR.limit(L, LR.table32(W), W, c, tp)     # R's envelope is under L's wherever it matters here
    assert peak == peak_t and np.array_equal(yr, Rq * g) and (yr[g < 1.0] != Rq[g < 1.0]).any()
    (m,), _, _, _ = R.limit_linked([L], LR.table32(W), W, c, tp)
    assert np.array_equal(LR.words(m), LR.words(yt))


def test_mix_order_and_edges():
    xs = [np.full(5, 1e8, np.float32), np.ones(5, np.float32), np.full(5, -1e8, np.float32)]
    one = np.float32(1.0)
    out = R.mix(xs, [(0, one, one)] * 3, 5)
    assert (out == 0.0).all()                                   # (1e8 + 1) - 1e8 in fp32: the 1 is lost
    out = R.mix([xs[0], xs[2], xs[1]], [(0, one, one)] * 3, 5)
    assert (out == 1.0).all()
    gl, gr = R.gains(-3.0, 0.3)
    x = np.arange(1, 8, dtype=np.float32)
    out = R.mix([x, x[:0]], [(3, gl, gr), (0, gl, gr)], 6)        # cut at total_out; a zero-length track
    assert np.array_equal(out[:6], np.concatenate([np.zeros(3, np.float32), gl * x[:3]])) and np.array_equal(out[6:], np.concatenate([np.zeros(3, np.float32), gr * x[:3]]))
    assert not np.signbit(out).any()
    assert len(R.mix([x], [(0, gl, gr)], 0)) == 0 and (R.mix([], [], 4) == 0).all()


def test_loud_linked():
    sr, S = 8000, 800
    x = LD._noisy(np.random.default_rng(4), 6 * S + 123, sr, 0.5)
    E = LD.seg_energy(LD.weighted_squares(x, sr)[0], S)
    z = LD.blocks(E, S)
    assert LD.gate_classes(z)[0][2].all()                       # every block above both gates
    L1, m1, _ = LD.stats(E, S)
    L2, m2, g2 = R.loud_linked(E, E, S, -16.0)
    assert abs(L2 - (L1 + 10.0 * np.log10(2.0))) < 1e-9 and abs(m2 - (m1 + 10.0 * np.log10(2.0))) < 1e-9
    assert g2 == np.float32(10.0 ** ((-16.0 - L2) / 20.0))
    L0, m0, _ = R.loud_linked(E, np.zeros_like(E), S)
    assert (L0, m0) == (L1, m1)
    assert R.loud_linked(E[:3], E[:3], S)[0] == -np.inf and R.loud_linked(E[:3], E[:3], S, -16.0)[2] == 1.0
    En = E.copy()
    En[2] = np.nan
    assert np.isnan(R.loud_linked(E, En, S, -16.0)).all()


def test_pcm16_planar():
    x = np.array([1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.0, 1.0 - 2.0 ** -15, -2.0, 2.5 / 32768], dtype=np.float32)
    out = R.pcm16_planar(x)
    assert out.shape == (4, 2) and out.dtype == np.dtype("<i2")
    assert out[:, 0].tolist() == [32767, -32768, 0, 2] and out[:, 1].tolist() == [32767, 32767, -32768, 2]
    assert np.array_equal(R.pcm16_planar(x, 1)[:, 0], LR.pcm16(x))
