"""The equaliser, host half (goofer_amd/eq.py and the library's goofer_host_eq_plan) against the numpy restatement
(tests/eq_ref.py): coefficients, dropped bands, tile table, the matrix powers against exact ones, the frequency response's
textbook values, the capacity protocol and every refusal.  Pure host code: no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import eq_ref as R
from goofer_amd import _lib
from goofer_amd import eq as EQ

TILE = 4096
ALL_KINDS = [("highpass", 0.0), ("lowpass", 0.0), ("lowshelf", 6.0), ("lowshelf", -9.0), ("highshelf", 4.0), ("highshelf", -8.5),
             ("peak", 9.0), ("peak", -3.0), ("notch", 0.0)]


def test_constants_mirror_the_restatement():
    assert (EQ.MAX_BANDS, EQ.MIN_SR, EQ.MAX_SR, EQ.F_MIN_DIV, EQ.F_MAX_REL, EQ.Q_MIN, EQ.Q_MAX, EQ.SHELF_Q_MAX, EQ.MAX_GAIN_DB, EQ.TOL, EQ.TILE, EQ.SPT,
            EQ.LEVELS, EQ.RUN_TILES) == (R.MAX_BANDS, R.MIN_SR, R.MAX_SR, R.F_MIN_DIV, R.F_MAX_REL, R.Q_MIN, R.Q_MAX, R.SHELF_Q_MAX, R.MAX_GAIN_DB, R.TOL,
                                         R.TILE, R.SPT, R.LEVELS, R.RUN_TILES)
    assert EQ.KINDS == R.KINDS and EQ.TOL <= 2.0 ** -26


@pytest.mark.parametrize("sr", [8000, 44100, 48000, 192000])
def test_planner_coefficients_equal_the_restatements(sr):
    for f0, q in ((sr / 600.0 * 1.001, 8.0), (sr / 48.0, R.Q_DEFAULT), (0.45 * sr, 0.1)):
        bands = [(kind, f0, g, min(q, R.SHELF_Q_MAX) if kind in R.SHELVES else q) for kind, g in ALL_KINDS]
        for part in (bands[:8], bands[8:]):
            plan = EQ.plan(sr, [10], part)
            want = R.cascade_coefficients(part, sr)
            assert plan.K == len(part) and plan.coef.dtype == np.float64 and plan.coef.shape == (len(part), 5)
            assert np.array_equal(plan.coef, want), (sr, f0, np.abs(plan.coef - want).max())


@pytest.mark.parametrize("sr", [8000, 48000])
def test_plan_tables(sr):
    lens = [0, 1, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 3, 0]
    plan = EQ.plan(sr, lens, R.chain(sr, 3))
    assert plan.n == len(lens) and plan.total == sum(lens) and plan.K == 3 and plan.sr == sr
    assert np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lens)]))
    tiles = [(i, k) for i, n in enumerate(lens) for k in range(-(-n // TILE))]
    assert plan.tiles.dtype == np.int32 and plan.tiles.tolist() == [list(t) for t in tiles] and plan.n_tiles == len(tiles)
    assert plan.mats.shape == (EQ.n_mats(3),) == (32 * 3 + 36 * 9,)
    assert plan.section_mats.shape == (3, 8, 2, 2) and plan.carry_mats.shape == (9, 6, 6)
    assert plan.blob.nbytes == 8 * (len(lens) + 1) + 8 * 15 + 8 * EQ.n_mats(3) + 8 * len(tiles)
    # T^16 against numpy's own power of the restatement's matrix, in the coordinates (u[i-1], u[i-1] - u[i-2]) the planner stores
    # its powers in: the layout, loosely; the exact check is below
    T = np.array(R.transition(plan.coef))
    P = np.array(R.to_diff(np.linalg.matrix_power(T, 16).tolist()))
    for k in range(3):
        assert np.allclose(plan.section_mats[k, 0], P[2 * k:2 * k + 2, 2 * k:2 * k + 2], rtol=1e-9, atol=1e-12)
    assert np.allclose(plan.carry_mats[0], np.array(R.to_diff(np.linalg.matrix_power(T, TILE).tolist())), rtol=1e-6, atol=1e-9)
    assert np.all(np.triu(plan.carry_mats, 2) == 0.0)                       # block lower triangular: exact zeros above


@pytest.mark.parametrize("sr,K", [(48000, 1), (48000, 8), (192000, 8), (8000, 3)])
def test_matrix_powers_against_exact_ones(sr, K):
    """every matrix of the plan within 2^-50 of its largest entry of the power computed exactly from the plan's coefficients, in
    the coordinates (u[i-1], u[i-1] - u[i-2]) per section"""
    mp = pytest.importorskip("mpmath")
    bands = R.chain(sr, K) if sr != 192000 else R.corners(sr)[1][:K]           # (eight high-passes at the lowest f0, q 8)
    plan = EQ.plan(sr, [100], bands)
    with mp.workprec(600):
        P = mp.matrix(R.transition(plan.coef, mp.mpf)) ** 16

        def err(got, rows, cols):
            Pd = R.to_diff([[P[a, b] for b in range(2 * plan.K)] for a in range(2 * plan.K)])
            want = [[Pd[a][b] for b in cols] for a in rows]
            top = max(abs(v) for r in want for v in r)
            worst = max(abs(mp.mpf(float(got[i][j])) - want[i][j]) for i in range(len(rows)) for j in range(len(cols)))
            if worst <= mp.mpf(2) ** -1074:                     # (a power that has decayed under float64's smallest number: 0.0 is right)
                return 0.0
            return float(worst / top)
        for j in range(EQ.LEVELS):
            for k in range(plan.K):
                e = err(plan.section_mats[k, j], (2 * k, 2 * k + 1), (2 * k, 2 * k + 1))
                assert e <= 2.0 ** -50, ("section", k, j, e)
            P = P * P
        D = range(2 * plan.K)
        assert err(plan.carry_mats[0], D, D) <= 2.0 ** -50
        P = P ** 16
        for j in range(EQ.LEVELS):
            e = err(plan.carry_mats[1 + j], D, D)
            assert e <= 2.0 ** -50, ("carry", j, e)
            P = P * P


def _db(h):
    return 20.0 * math.log10(abs(complex(h)))


@pytest.mark.parametrize("sr", [8000, 44100, 48000, 192000])
def test_response_has_the_textbook_values(sr):
    f0 = sr / 40.0
    lo, hi = f0 / 1000.0, 0.499 * sr
    for g in (6.0, -9.0):
        assert abs(_db(EQ.response([("peak", f0, g, 2.0)], sr, f0)) - g) <= 1e-9
        for f in (lo, hi):
            assert abs(_db(EQ.response([("peak", f0, g, 2.0)], sr, f))) <= 0.01
        assert abs(_db(EQ.response([("lowshelf", f0, g)], sr, lo)) - g) <= 0.01 and abs(_db(EQ.response([("lowshelf", f0, g)], sr, hi))) <= 0.01
        assert abs(_db(EQ.response([("highshelf", f0, g)], sr, hi)) - g) <= 0.01 and abs(_db(EQ.response([("highshelf", f0, g)], sr, lo))) <= 0.01
    for kind, passed, stopped in (("highpass", hi, lo), ("lowpass", lo, hi)):
        assert abs(_db(EQ.response([(kind, f0)], sr, f0)) + 3.0103) <= 1e-3           # q = sqrt(1/2): -3.01 dB at f0
        assert abs(_db(EQ.response([(kind, f0)], sr, passed))) <= 0.01 and _db(EQ.response([(kind, f0)], sr, stopped)) < -60.0
    assert abs(complex(EQ.response([("notch", f0, 0.0, 4.0)], sr, f0))) <= 1e-12
    assert abs(_db(EQ.response([("notch", f0, 0.0, 4.0)], sr, lo))) <= 0.01
    # a cascade multiplies, a string is the same bands, an array of frequencies keeps its shape
    f = np.array([[lo, f0], [2.0 * f0, hi]])
    both = EQ.response("hp:%r,peak:%r:3:1" % (f0, 2.0 * f0), sr, f)
    assert both.shape == (2, 2) and both.dtype == np.complex128
    assert np.allclose(both, EQ.response([("highpass", f0)], sr, f) * EQ.response([EQ.Band("peak", 2.0 * f0, 3.0, 1.0)], sr, f), rtol=1e-14)


def test_zero_gain_bands_are_dropped():
    plan = EQ.plan(48000, [10], [("peak", 1000.0, 0.0, 2.0), ("highpass", 100.0), ("lowshelf", 200.0, 0.0), ("highshelf", 8000.0, 0.0),
                                ("peak", 3000.0, 1.0, 1.0), ("notch", 50.0 * 2)])
    assert plan.K == 3 and len(plan.bands) == 6 and [b.identity for b in plan.bands] == [True, False, True, True, False, False]
    want = R.cascade_coefficients([("highpass", 100.0, 0.0, R.Q_DEFAULT), ("peak", 3000.0, 1.0, 1.0), ("notch", 100.0, 0.0, R.Q_DEFAULT)], 48000)
    assert np.array_equal(plan.coef, want)
    none = EQ.plan(48000, [10, 5000], [("peak", 1000.0, 0.0, 2.0), ("lowshelf", 200.0, 0.0)])
    assert none.K == 0 and none.coef.shape == (0, 5) and none.mats.size == 0 and none.n_tiles == 3
    assert EQ.plan(48000, [10], []).K == 0


def test_parse():
    want = (EQ.Band("highpass", 80.0), EQ.Band("peak", 3000.0, 3.0, 1.0), EQ.Band("highshelf", 10000.0, 4.0))
    assert EQ.parse("hp:80,peak:3000:3:1,hs:10000:4") == want
    assert EQ.parse([("hp", 80), ("peak", 3000, 3, 1), EQ.Band("hs", 10000, 4)]) == want
    assert want[0].q == math.sqrt(0.5) and want[2].q == math.sqrt(0.5) and want[0].gain_db == 0.0
    assert [EQ.Band(k, 100.0).kind for k in ("hp", "lp", "ls", "hs", "peak", "notch")] == list(EQ.KINDS[:4]) + ["peak", "notch"]
    assert EQ.parse(()) == () and EQ.parse(EQ.Band("lp", 5000.0)) == (EQ.Band("lowpass", 5000.0),)
    nan, inf = float("nan"), float("inf")
    for bad in ("", "hp", "hp:", "hp:80:0:1:2", "bell:100", "hp:abc", "hp:80;lp:100", "hp:80,,lp:9000", 80.0, None, [("hp",)], [(80.0, "hp")],
                [("hp", nan)], [("hp", inf)], [("hp", 0.0)], [("hp", -80.0)], [("hp", 80.0, 1.0)], [("lp", 80.0, -0.5)], [("notch", 80.0, 3.0)],
                [("peak", 100.0, 9.5)], [("peak", 100.0, -9.5)], [("ls", 100.0, 3.0, 2.5)], [("hs", 100.0, 3.0, 8.0)], [("peak", 100.0, nan)], [("ls", 100.0, inf)], [("hs", 100.0, 3.0, 0.09)],
                [("hs", 100.0, 3.0, 8.5)], [("hs", 100.0, 3.0, nan)], [("hp", 100.0)] * 9, "hp:100," * 8 + "hp:100"):
        with pytest.raises(ValueError):
            EQ.parse(bad)


def _call(sr, bands, in_off, n, tiles_cap, gone=()):
    lib = _lib.load()
    K, nd = C.c_int(-7), (C.c_int64 * 1)(-7)
    kind = np.array([b[0] for b in bands], dtype=np.int32)
    f0, g, q = (np.array([b[j] for b in bands], dtype=np.float64) for j in (1, 2, 3))
    co, ma = np.full(5 * EQ.MAX_BANDS, -7.0), np.full(EQ.n_mats(EQ.MAX_BANDS), -7.0)
    tl = np.full((max(tiles_cap, 1), 2), -7, dtype=np.int32)
    ptr = {"kind": kind, "f0": f0, "gain": g, "q": q, "coef": co, "mats": ma, "tiles": tl}
    a = {k: (None if k in gone else v.ctypes.data) for k, v in ptr.items()}
    rc = lib.goofer_host_eq_plan(sr, a["kind"], a["f0"], a["gain"], a["q"], len(bands), None if in_off is None else in_off.ctypes.data, n,
                                 None if "K" in gone else C.byref(K), a["coef"], a["mats"], a["tiles"], tiles_cap, None if "need" in gone else nd)
    return rc, K.value, nd[0], co, tl


def test_refusals_and_the_capacity_protocol():
    off = np.array([0, 100, 5000], dtype=np.int64)
    hp, peak = (0, 100.0, 0.0, 1.0), (4, 1000.0, 6.0, 2.0)
    assert _call(48000, [hp, peak], off, 2, 3)[:3] == (0, 2, 3)
    nan, inf = float("nan"), float("inf")
    for sr in (7999, 192001, 0, -48000):
        assert _call(sr, [hp], off, 2, 3)[0] == -1, sr
    # the ranges: f0 in [sr / 600, 0.45 sr], q in [0.1, 8], (shelves: 2), |gain| <= 9, gain == 0 where it is ignored, a kind that exists
    assert _call(48000, [(0, 80.0, 0.0, 1.0)], off, 2, 3)[0] == 0 and _call(48000, [(0, 0.45 * 48000, 0.0, 1.0)], off, 2, 3)[0] == 0
    assert _call(48000, [(4, 100.0, 9.0, 8.0)], off, 2, 3)[0] == 0 and _call(48000, [(2, 100.0, -9.0, 2.0)], off, 2, 3)[0] == 0
    for bad in ((0, 79.99, 0.0, 1.0), (0, 0.4501 * 48000, 0.0, 1.0), (0, nan, 0.0, 1.0), (0, inf, 0.0, 1.0), (0, -100.0, 0.0, 1.0),
                (0, 100.0, 0.0, 0.0999), (0, 100.0, 0.0, 8.001), (0, 100.0, 0.0, nan), (0, 100.0, 0.0, inf),
                (4, 100.0, 9.001, 1.0), (2, 100.0, -9.001, 1.0), (2, 100.0, 3.0, 2.001), (3, 100.0, -3.0, 8.0), (3, 100.0, nan, 1.0), (4, 100.0, inf, 1.0),
                (0, 100.0, 1.0, 1.0), (1, 100.0, -1.0, 1.0), (5, 100.0, 0.5, 1.0), (0, 100.0, nan, 1.0),
                (6, 100.0, 0.0, 1.0), (-1, 100.0, 0.0, 1.0)):
        assert _call(48000, [hp, bad], off, 2, 3)[0] == -1, bad
    assert _call(192000, [(0, 319.0, 0.0, 1.0)], off, 2, 3)[0] == -1 and _call(192000, [(0, 320.0, 0.0, 1.0)], off, 2, 3)[0] == 0
    assert _call(48000, [hp] * 8, off, 2, 3)[:2] == (0, 8) and _call(48000, [hp] * 9, off, 2, 3)[0] == -1
    assert _call(48000, [hp], np.array([0, 100, 50], dtype=np.int64), 2, 3)[0] == -1            # offsets that decrease
    assert _call(48000, [hp], np.array([0, 1 << 31], dtype=np.int64), 1, 1 << 20)[0] == -1      # a signal of 2^31 samples
    assert _call(48000, [hp], None, 2, 3)[0] == -1                                              # null pointers
    for gone in ("kind", "f0", "gain", "q", "coef", "mats", "tiles", "K", "need"):
        assert _call(48000, [hp], off, 2, 3, gone=(gone,))[0] == -1, gone
    assert _call(48000, [hp], off, -1, 3)[0] == -1 and _call(48000, [hp], off, 2, -1)[0] == -1
    # a capacity that is too small: 1, with K and need; then 0
    for cap in (2, 0):
        assert _call(48000, [hp, (4, 1000.0, 0.0, 1.0)], off, 2, cap, gone=() if cap else ("tiles",))[:3] == (1, 1, 3), cap
    rc, K, need, coef, tiles = _call(48000, [hp, peak], off, 2, 3)
    assert (rc, K, need) == (0, 2, 3) and tiles.tolist() == [[0, 0], [1, 0], [1, 1]]
    assert np.array_equal(coef[:10].reshape(2, 5), EQ.plan(48000, [100, 4900], [("hp", 100.0, 0.0, 1.0), ("peak", 1000.0, 6.0, 2.0)]).coef)
    assert _call(48000, [], None, 0, 0, gone=("kind", "f0", "gain", "q", "tiles"))[:3] == (0, 0, 0)      # no band, no signal
    # ... and through Python: ValueError before anything is launched
    for sr, bands in ((7999, "hp:100"), (192001, "hp:500"), (44100.5, "hp:100"), (48000, "hp:79"), (48000, "lp:21700"), (192000, "hp:80"),
                      (8000, "peak:3000:3:1,hs:10000:4")):
        with pytest.raises(ValueError):
            EQ.plan(sr, [100], bands)
    with pytest.raises(ValueError):
        EQ.plan(48000, [100, -1], "hp:100")
    with pytest.raises(ValueError):
        EQ.plan(48000, [1 << 31], "hp:100")
