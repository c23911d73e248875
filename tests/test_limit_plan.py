"""The look-ahead peak limiter, host half (goofer_amd/limit.py and the library's goofer_host_limit_plan) against the numpy
restatement (tests/limit_ref.py): the look-ahead, the table, the tile table, the capacity protocol and the refusals; then the
properties of the definition itself, through the restatement on the library's table.  Pure host code: no GPU."""
import ctypes as C

import numpy as np
import pytest

import limit_ref as R
from goofer_amd import _lib
from goofer_amd import limit as LM

TILE = 4096
CEILINGS = (R.CEILING, np.float32(0.891), np.float32(0.5))


def test_look_ahead_at_the_usual_rates():
    want = {8000: 40, 44100: 221, 48000: 240, 96000: 480, 192000: 960}     # 220.5 + 0.5 = 221.0: the floor of that
    for sr, W in want.items():
        plan = LM.plan(sr, [100])
        assert plan.W == W == R.look(sr) == LM.look_samples(sr), sr
        assert plan.taps.shape == (2 * W + 1,) and plan.taps.dtype == np.float32
        assert plan.ceiling == float(R.CEILING)
    assert LM.plan(1000, [5], 0.5, 7.0).W == 7 and LM.plan(1000, [5], 0.5, 7.49).W == 7 and LM.plan(1000, [5], 0.5, 7.5).W == 8


@pytest.mark.parametrize("W", [1, 7, 40, 220, 221, 240, 480, 960, 1024])
def test_table_matches_the_formula(W):
    got = LM.plan(1000, [], 1.0, float(W)).taps
    want64 = R.table64(W)
    want = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= ulp), float(err.max())
    print(W, "entries that differ from the restatement's:", int((got != want).sum()), "of", got.size)
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24
    assert np.all(got > 0) and np.array_equal(got, got[::-1]) and got.argmax() == W


def test_offsets_tiles_and_blob():
    lens = [0, 1, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 3, 0]
    plan = LM.plan(48000, lens)
    assert plan.n == len(lens) and plan.total == sum(lens)
    assert plan.in_off.dtype == np.int64 and np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lens)]))
    want = [(i, k) for i, n in enumerate(lens) for k in range(-(-n // TILE))]
    assert plan.tiles.dtype == np.int32 and plan.tiles.tolist() == [list(t) for t in want] and plan.n_tiles == 8
    assert plan.blob.nbytes == 8 * (len(lens) + 1) + 8 * len(want) + 4 * (2 * plan.W + 1)
    empty = LM.plan(48000, [])
    assert empty.n == 0 and empty.total == 0 and empty.n_tiles == 0 and empty.W == 240


def _call(sr, look_ms, c, in_off, n, taps_cap, tiles_cap, w=True, need=True, taps=True, tiles=True):
    lib = _lib.load()
    W, nd = C.c_int(-7), (C.c_int64 * 2)(-7, -7)
    t = np.full(max(taps_cap, 1), -7, dtype=np.float32)
    tl = np.full((max(tiles_cap, 1), 2), -7, dtype=np.int32)
    rc = lib.goofer_host_limit_plan(sr, look_ms, C.c_float(c), None if in_off is None else in_off.ctypes.data, n,
                                    C.byref(W) if w else None, t.ctypes.data if taps else None, taps_cap,
                                    tl.ctypes.data if tiles else None, tiles_cap, nd if need else None)
    return rc, W.value, (nd[0], nd[1]), t, tl


def test_refusals_and_the_capacity_protocol():
    off = np.array([0, 100, 5000], dtype=np.int64)
    ok = (48000, 5.0, 0.5, off, 2, 481, 3)
    assert _call(*ok)[0] == 0
    assert _call(1000, 0.4, 0.5, off, 2, 5000, 3)[0] == -1                  # W = 0
    assert _call(1000, 0.5, 0.5, off, 2, 5000, 3)[:2] == (0, 1)             # W = 1
    assert _call(1000, 1024.4, 0.5, off, 2, 5000, 3)[:2] == (0, 1024)
    assert _call(1000, 1024.5, 0.5, off, 2, 5000, 3)[0] == -1               # W = 1025
    assert _call(1000, -3.0, 0.5, off, 2, 5000, 3)[0] == -1
    assert _call(1000, float("nan"), 0.5, off, 2, 5000, 3)[0] == -1
    assert _call(1000, float("inf"), 0.5, off, 2, 5000, 3)[0] == -1
    for c in (0.0, -0.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 2.0, float("nan"), float("inf")):
        assert _call(48000, 5.0, c, off, 2, 481, 3)[0] == -1, c             # c of 0, above 1, NaN
    assert _call(48000, 5.0, 1.0, off, 2, 481, 3)[0] == 0
    assert _call(0, 5.0, 0.5, off, 2, 481, 3)[0] == -1                      # sr < 1
    assert _call(-48000, 5.0, 0.5, off, 2, 481, 3)[0] == -1
    assert _call(48000, 5.0, 0.5, np.array([0, 100, 50], dtype=np.int64), 2, 481, 3)[0] == -1      # a negative length
    assert _call(48000, 5.0, 0.5, np.array([0, 1 << 31], dtype=np.int64), 1, 481, 1 << 20)[0] == -1
    assert _call(48000, 5.0, 0.5, None, 2, 481, 3)[0] == -1                 # null pointers
    assert _call(48000, 5.0, 0.5, off, 2, 481, 3, w=False)[0] == -1
    assert _call(48000, 5.0, 0.5, off, 2, 481, 3, need=False)[0] == -1
    assert _call(48000, 5.0, 0.5, off, 2, 481, 3, taps=False)[0] == -1
    assert _call(48000, 5.0, 0.5, off, 2, 481, 3, tiles=False)[0] == -1
    assert _call(48000, 5.0, 0.5, off, -1, 481, 3)[0] == -1
    assert _call(48000, 5.0, 0.5, off, 2, -1, 3)[0] == -1
    assert _call(48000, 5.0, 0.5, off, 2, 481, -1)[0] == -1
    # a capacity that is too small: 1, with W and need; nothing else is promised
    for caps in ((480, 3), (481, 2), (0, 0)):
        rc, W, need, _, _ = _call(48000, 5.0, 0.5, off, 2, *caps, taps=caps[0] > 0, tiles=caps[1] > 0)
        assert (rc, W, need) == (1, 240, (481, 3)), caps
    rc, W, need, taps, tiles = _call(*ok)
    assert (rc, W, need) == (0, 240, (481, 3)) and tiles.tolist() == [[0, 0], [1, 0], [1, 1]]
    assert np.array_equal(taps, LM.plan(48000, [100, 4900], 0.5).taps)
    rc, W, need, _, _ = _call(48000, 5.0, 0.5, None, 0, 481, 0, tiles=False)      # no signal: the table alone
    assert (rc, W, need) == (0, 240, (481, 0))
    for bad in (dict(lookahead_ms=0.0), dict(lookahead_ms=21.4), dict(ceiling=0.0), dict(ceiling=1.5), dict(ceiling=float("nan"))):
        with pytest.raises(ValueError):
            LM.plan(48000, [100], **bad)
    with pytest.raises(ValueError):
        LM.plan(0, [100])
    with pytest.raises(ValueError):
        LM.plan(48000, [100, -1])
    assert LM.parse(0.5) == (0.5, 5.0) and LM.parse((0.25, 2)) == (0.25, 2.0)
    with pytest.raises(ValueError):
        LM.parse((0.5, 5.0, 1.0))


def _signal(rng, n, c, W, loud=True):
    """quiet noise below c with, where ``loud``, peaks of 1.5 to 40 c: single ones, two inside one window, a run of equal ones
    longer than the window, the first and the last sample"""
    x = (0.2 * float(c) * rng.standard_normal(n)).astype(np.float32)
    np.clip(x, -0.9 * float(c), 0.9 * float(c), out=x)
    if loud and n:
        amp = lambda k: (float(c) * rng.uniform(1.5, 40.0, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
        at = rng.integers(0, n, max(1, n // (6 * W + 7)))
        x[at] = amp(len(at))
        x[0], x[-1] = amp(2)
        p = int(rng.integers(0, n))
        x[p], x[min(n - 1, p + W)] = amp(2)
        q = int(rng.integers(0, n))
        x[q:q + 2 * W + 4] = amp(1)[0]
    return x


@pytest.fixture(scope="module", params=[1, 7, 220, 1024])
def case(request):
    W = request.param
    taps = LM.plan(1000, [], 1.0, float(W)).taps
    rng = np.random.default_rng(20261020 + W)
    return W, taps, rng


@pytest.mark.parametrize("c", CEILINGS, ids=lambda c: "%.3f" % c)
def test_ceiling_gain_and_statistics(case, c):
    W, taps, rng = case
    for n in (1, W, 2 * W + 1, 9 * W + 50):
        x = _signal(rng, n, c, W)
        y, g, peak, gmin = R.limit(x, taps, W, c)
        assert y.dtype == np.float32 and g.dtype == np.float32 and len(y) == n
        assert float(np.abs(x).max()) > 1.4 * float(c)
        worst = float(np.abs(y.astype(np.float64)).max()) / float(c)
        print(W, float(c), n, "worst |y| / c - 1 = %.3e" % (worst - 1.0))
        assert worst <= 1.0 + 2.0 ** -22
        assert np.all(g <= 1.0) and np.all(g >= 0.0)
        assert peak == np.abs(x).max() and gmin == g.min() and gmin < 1.0
        y64, g64, _, _ = R.limit(x, taps, W, c, np.float64)
        assert np.all(g64 <= 1.0) and np.all(np.abs(y.astype(np.float64) - y64) <= R.bound(x, W))
    y, g, peak, gmin = R.limit(np.zeros(0, np.float32), taps, W, c)
    assert len(y) == 0 and peak == 0.0 and gmin == 1.0


def test_at_the_default_ceiling_pcm16_never_clamps(case):
    W, taps, rng = case
    x = _signal(rng, 8 * W + 100, R.CEILING, W)
    y = R.limit(x, taps, W, R.CEILING)[0]
    assert np.array_equal(R.pcm16(y), np.round(y.astype(np.float64) * 32768.0).astype(np.int64))


@pytest.mark.parametrize("c", CEILINGS, ids=lambda c: "%.3f" % c)
def test_identity(case, c):
    """a <= c on [i - 2W, i + 2W]: g is exactly 1 and y is x's words; a signal that never exceeds c comes back bit for bit"""
    W, taps, rng = case
    x = _signal(rng, 10 * W + 30, c, W, loud=False)
    x[3], x[7] = np.float32(c), -np.float32(c)                  # at the ceiling is not above it
    x[5] = np.float32(-0.0)
    y, g, _, gmin = R.limit(x, taps, W, c)
    assert np.array_equal(R.words(y), R.words(x)) and np.all(g == 1.0) and gmin == 1.0
    at = 5 * W + 11
    x[at] = np.float32(3.0) * np.float32(c)
    y, g, _, _ = R.limit(x, taps, W, c)
    far = np.abs(np.arange(len(x)) - at) > 2 * W
    assert np.all(g[far] == 1.0) and np.array_equal(R.words(y[far]), R.words(x[far]))
    assert np.all(g[at - W:at + W + 1] < 1.0) and g[at] <= np.float32(c) / x[at]      # (tap 0 meets a d > 0 there)


def test_a_signal_alone_and_between_loud_neighbours(case):
    """Nothing in the definition reaches across a signal: the restatement of a batch is the restatement of each signal, and the
    quiet signal between two loud ones is its own words."""
    W, taps, rng = case
    c = np.float32(0.5)
    loud_a, quiet, loud_b = _signal(rng, 3 * W + 5, c, W), _signal(rng, 4 * W + 2, c, W, loud=False), _signal(rng, 2 * W, c, W)
    loud_a[-1], loud_b[0] = 20.0, -20.0
    alone = R.limit(quiet, taps, W, c)[0]
    batch = R.limit_batch([loud_a, quiet, loud_b], taps, W, c)
    assert np.array_equal(R.words(batch[1][0]), R.words(alone)) and np.array_equal(R.words(alone), R.words(quiet))
    mid = _signal(rng, 4 * W + 2, c, W)
    assert np.array_equal(R.words(R.limit_batch([loud_a, mid, loud_b], taps, W, c)[1][0]), R.words(R.limit(mid, taps, W, c)[0]))
    assert batch[0][3] < 1.0 and batch[2][3] < 1.0 and batch[1][3] == 1.0
