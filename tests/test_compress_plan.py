"""The dynamic range compressor, host half (goofer_amd/compress.py and the library's goofer_host_compress_plan) against the numpy
restatement (tests/compress_ref.py): coefficients, power tables, tile table, the capacity protocol and the refusals; then the
restatement itself: ``blocked`` against ``sequential`` in float64 and in long double on the fixtures of the GPU tests, the room
they leave under the GPU tests' bounds, and that wrong variants of the restatement break those bounds on those very fixtures.
Pure host code: no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import compress_ref as R
from goofer_amd import _lib
from goofer_amd import compress as CP

TILE = 4096


@pytest.mark.parametrize("sr", [8000, 11025, 44100, 48000, 96000, 192000])
@pytest.mark.parametrize("name", list(R.SETS))
def test_plan_against_numpy(sr, name):
    lens = [0, 1, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 3, 0]
    st = R.SETS[name]
    plan = CP.plan(sr, lens, CP.Compressor(*st))
    assert plan.n == len(lens) and plan.total == sum(lens) and plan.settings == CP.Compressor(*st)
    T, ratio, W, att, rel, M = st
    assert plan.coef.dtype == np.float64 and plan.coef.shape == (CP.COEF,)
    assert plan.coef[0] == T and plan.coef[1] == W and plan.coef[2] == 1.0 / ratio - 1.0 and plan.coef[3] == M
    assert -1.0 <= plan.coef[2] <= 0.0
    for got, ms in ((plan.coef[4], rel), (plan.coef[5], att)):
        want = R.coefficient(ms, sr)
        assert got == CP.coefficient(ms, sr) or abs(got - want) <= 2.0 * np.spacing(want)        # (exp of two libms)
        ld = np.exp(-np.longdouble(1.0) / (np.longdouble(ms) * np.longdouble(1e-3) * np.longdouble(sr))) if ms else np.longdouble(0.0)
        assert abs(np.longdouble(got) - ld) <= 2.0 * np.spacing(want)
        assert (got == 0.0) == (ms == 0) and 0.0 <= got < 1.0
    assert np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lens)]))
    tiles = [(i, k) for i, n in enumerate(lens) for k in range(-(-n // TILE))]
    assert plan.tiles.dtype == np.int32 and plan.tiles.tolist() == [list(t) for t in tiles] and plan.n_tiles == len(tiles)
    assert plan.blob.nbytes == 8 * (len(lens) + 1) + 8 * CP.COEF + 8 * 2 * CP.POWS + 8 * len(tiles)
    # a^(16 * 2^k), a the plan's own float64 coefficient: against long double and against float64
    assert plan.pows.shape == (2, CP.POWS)
    for row, a in ((0, plan.coef[4]), (1, plan.coef[5])):
        for k in range(CP.POWS):
            m = 16 * 2 ** k
            ld = np.power(np.longdouble(a), np.longdouble(m))
            got = plan.pows[row, k]
            assert abs(np.longdouble(got) - ld) <= np.spacing(max(float(ld), 5e-324)), (row, k)
            f64 = float(a) ** m
            assert abs(got - f64) <= 4.0 * np.spacing(max(f64, 5e-324)), (row, k, got, f64)
    assert CP.TILE == TILE == R.TILE and CP.RUN_TILES == R.RUN_TILES and CP.ROUND_TILES == R.ROUND_TILES == 256 * CP.RUN_TILES


def _call(sr=48000, st=R.SETS["defaults"], in_off=np.array([0, 100, 5000], dtype=np.int64), n=2, tiles_cap=3, coef=True, pows=True,
          tiles=True, need=True):
    lib = _lib.load()
    nd = (C.c_int64 * 1)(-7)
    co, pw = np.full(CP.COEF, -7.0), np.full(2 * CP.POWS, -7.0)
    tl = np.full((max(tiles_cap, 1), 2), -7, dtype=np.int32)
    rc = lib.goofer_host_compress_plan(sr, *st, None if in_off is None else in_off.ctypes.data, n, co.ctypes.data if coef else None,
                                       pw.ctypes.data if pows else None, tl.ctypes.data if tiles else None, tiles_cap, nd if need else None)
    return rc, nd[0], co, pw, tl


def test_refusals_and_the_capacity_protocol():
    assert _call()[0] == 0
    for sr in (7999, 192001, 0, -48000):
        assert _call(sr=sr)[0] == -1, sr
    assert _call(sr=8000)[0] == 0 and _call(sr=192000)[0] == 0
    d = R.SETS["defaults"]
    nan, inf = math.nan, math.inf
    edges = [(0, (-80.0, 0.0), (-80.1, 0.1, nan, -inf)), (1, (1.0, inf), (0.99, 0.0, -1.0, nan, -inf)), (2, (0.0, 40.0), (-0.1, 40.1, nan, inf)),
             (3, (0.0, 1000.0), (-0.1, 1000.1, nan, inf)), (4, (0.0, 5000.0), (-0.1, 5000.1, nan, inf)), (5, (-24.0, 24.0), (-24.1, 24.1, nan, inf))]
    for at, good, bad in edges:
        for v in good:
            assert _call(st=d[:at] + (v,) + d[at + 1:])[0] == 0, (at, v)
        for v in bad:
            assert _call(st=d[:at] + (v,) + d[at + 1:])[0] == -1, (at, v)
            with pytest.raises(ValueError):
                CP.Compressor(*(d[:at] + (v,) + d[at + 1:]))
    assert _call(in_off=np.array([0, 100, 50], dtype=np.int64))[0] == -1                       # offsets that decrease
    assert _call(in_off=np.array([0, 1 << 31], dtype=np.int64), n=1, tiles_cap=1 << 20)[0] == -1
    assert _call(in_off=np.array([0, (1 << 31) - 1], dtype=np.int64), n=1, tiles_cap=0, tiles=False)[:2] == (1, 1 << 19)
    assert _call(in_off=None)[0] == -1                                                          # null pointers
    for gone in ("coef", "pows", "tiles", "need"):
        assert _call(**{gone: False})[0] == -1, gone
    assert _call(n=-1)[0] == -1 and _call(tiles_cap=-1)[0] == -1
    for cap in (2, 0):                  # a capacity that is too small: 1, with need; nothing else is promised
        assert _call(tiles_cap=cap, tiles=cap > 0)[:2] == (1, 3), cap
    rc, need, coef, pows, tiles = _call()
    assert (rc, need) == (0, 3) and tiles.tolist() == [[0, 0], [1, 0], [1, 1]]
    assert np.array_equal(coef, CP.plan(48000, [100, 4900], CP.Compressor(*d)).coef) and np.array_equal(pows, CP.plan(48000, [], CP.Compressor(*d)).pows.ravel())
    assert _call(in_off=None, n=0, tiles_cap=0, tiles=False)[:2] == (0, 0)                      # no signal: the tables alone
    for bad in (7999, 192001, 44100.5):
        with pytest.raises(ValueError):
            CP.plan(bad, [100], CP.Compressor(*d))
    with pytest.raises(ValueError):
        CP.plan(48000, [100, -1], CP.Compressor(*d))


def test_parse():
    want = CP.Compressor(-18.0, 4.0)
    assert want.astuple() == (-18.0, 4.0, 6.0, 5.0, 100.0, 0.0)
    assert CP.parse("-18:4") == want == CP.parse((-18, 4)) == CP.parse(want)
    assert CP.parse("-18:4:2:50") == CP.Compressor(-18.0, 4.0, attack_ms=2.0, release_ms=50.0)
    assert CP.parse("-18:inf:2:50:0") == CP.Compressor(-18.0, math.inf, 0.0, 2.0, 50.0)
    assert CP.parse([-18, 4, 2, 50, 3, 1.5]) == CP.Compressor(-18.0, 4.0, 3.0, 2.0, 50.0, 1.5)
    for bad in ("-18", "-18:4:2", "-18:four", "", "-18:4:2:50:3:1:0", "1:4", "-18:0.5", (-18,), -18.0, None, "-18:nan"):
        with pytest.raises(ValueError):
            CP.parse(bad)


# ---- the restatement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_blocked_matches_sequential_and_the_long_double_flavour(sr, name):
    """2^-40 dB between the three on every fixture; the fp32 output of ``blocked`` within half the output bound of the
    long-double product — half is the fp32 rounding itself (2^-24, or 2^-150 absolute), to which the 2^-40 dB just shown add a
    relative 0.1152 * 2^-40 through the gain."""
    st = R.SETS[name]
    worst = worst_y = 0.0
    for i, x in enumerate(R.batch(sr)):
        y1, yl = R.reference(sr, name, i)
        l1, ll = R.reference(sr, name, i, "ld")
        b1, bl = R.blocked(x, sr, st)
        assert b1.dtype == bl.dtype == np.float64 and len(b1) == len(bl) == len(x) == len(yl) == len(ll)
        if not len(x):
            continue
        assert np.all(b1 >= 0.0) and np.all(bl >= 0.0)
        for a, b in ((bl, yl), (b1, y1), (bl, ll), (b1, l1), (yl, ll)):
            err = float(np.abs(a.astype(np.longdouble) - b).max())
            worst = max(worst, err)
            assert err <= 2.0 ** -40, (i, err)
        ok, ratio = R.within_output_bound(R.output(x, bl, st[5]), R.product(x, ll, st[5], np.longdouble), 0.5, 0.1152 * 2.0 ** -40)
        worst_y = max(worst_y, ratio)
        assert ok, (i, ratio)
    print(sr, name, "worst detector difference %.3e dB (bound %.3e), worst output error %.4f of its bound" % (worst, 2.0 ** -40, worst_y))
    assert R.max_reduction(R.reference(sr, name, R.LONG)[1]) > 4.0                  # the fixtures are compressed at all


def test_the_fixtures_are_what_the_tests_take_them_for():
    for sr in R.RATES:
        xs = R.batch(sr)
        assert tuple(len(x) for x in xs) == R.LENGTHS and len(xs[R.LONG]) > R.RUN_TILES * TILE
        for x in xs:
            assert x.dtype == np.float32 and np.all(np.isfinite(x)) and np.all(np.abs(x) < 1.0)
            assert not np.any((x != 0) & (np.abs(x) < 2.0 ** -100))
        x = xs[R.LONG]
        lv = 20.0 * np.log10(np.maximum(np.abs(x.astype(np.float64)), R.FLOOR))
        assert lv.max() > R.THRESHOLD + 12.0 and np.any(x == 0) and np.any(np.abs(x) == np.float32(2.0 ** -90))
        knee = np.abs(2.0 * (lv - R.THRESHOLD)) <= 6.0
        assert knee.mean() > 0.02 and (lv < R.THRESHOLD - 3.0).mean() > 0.2 and (lv > R.THRESHOLD + 3.0).mean() > 0.1
    q = R.quiet_signal()
    assert np.all(R.levels(q, R.SETS["defaults"]) == 0.0) and np.any(np.abs(q) > 10.0 ** (-23.1 / 20.0))
    assert R.words(R.output(q, R.sequential(q, 48000, R.SETS["defaults"])[1], 0.0)).tolist() == R.words(q).tolist()


# ---- wrong variants: each breaks a bound of tests/test_gpu_compress.py on that file's inputs -----------------------------------

WRONG_AT = 8                        # the fixture of 2 * 4096 + 5 samples: two tile boundaries


def _breaks(sr, name, i, yl_wrong):
    """whether the curve breaks the detector bound or the output bound against the float64 restatement of fixture i"""
    x, st = R.batch(sr)[i], R.SETS[name]
    yl = R.reference(sr, name, i)[1]
    if float(np.abs(np.asarray(yl_wrong, dtype=np.float64) - yl).max()) > R.TOL_DB:
        return True
    return not R.within_output_bound(R.output(x, yl_wrong, st[5]), R.product(x, yl, st[5]))[0]


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_wrong_fp32_state_breaks_the_bound(sr, name):
    yl = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], state_dtype=np.float32)[1]
    assert _breaks(sr, name, WRONG_AT, yl)


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_wrong_state_lost_at_a_tile_boundary_breaks_the_bound(sr, name):
    yl = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], zero_every=TILE)[1]
    assert _breaks(sr, name, WRONG_AT, yl)
    want = R.reference(sr, name, WRONG_AT)[1]
    assert np.array_equal(yl[:TILE], want[:TILE])               # ... behind the boundary, not in front of it


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_wrong_state_inherited_from_the_neighbour_breaks_the_bound(sr, name):
    y1, yl = R.reference(sr, name, WRONG_AT - 1)
    assert yl[-1] > 1e-3
    wrong = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], history=(y1[-1], yl[-1]))[1]
    assert _breaks(sr, name, WRONG_AT, wrong)


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", [k for k, v in R.SETS.items() if v[2] > 0])
def test_wrong_hard_knee_in_place_of_a_soft_one_breaks_the_bound(sr, name):
    yl = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], hard_knee=True)[1]
    assert _breaks(sr, name, WRONG_AT, yl)


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_wrong_attack_and_release_swapped_breaks_the_bound(sr, name):
    assert R.SETS[name][3] != R.SETS[name][4]
    yl = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], swap=True)[1]
    assert _breaks(sr, name, WRONG_AT, yl)


@pytest.mark.parametrize("sr", R.RATES)
@pytest.mark.parametrize("name", list(R.SETS))
def test_wrong_floor_after_the_logarithm_breaks_the_bound(sr, name):
    """1e-6 applied to the level in dB, max(20 log10 |x|, 1e-6), instead of to |x|: every sample counts as over full scale"""
    yl = R.sequential(R.batch(sr)[WRONG_AT], sr, R.SETS[name], floor_after_log=True)[1]
    assert _breaks(sr, name, WRONG_AT, yl)
