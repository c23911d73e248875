"""Loudness metering, host half (goofer_amd/loudness.py and the library's goofer_host_loudness_plan) against the numpy
restatement (tests/loudness_ref.py): coefficients, segment length and CSR, tile table, matrix powers, the capacity protocol and
the refusals; then the restatement itself (the standard's table and its 997 Hz figure), the headroom the float64 flavour leaves
under the GPU tests' bound, the gating fixtures, and that wrong variants of the restatement would break the GPU tests' bounds
on the inputs those tests use.  Pure host code: no GPU."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as R
from goofer_amd import _lib
from goofer_amd import loudness as LD

TILE = 4096


def test_coefficients_match_the_standards_table_at_48_khz():
    got = LD.plan(48000, []).coef
    assert got.dtype == np.float64 and got.shape == (10,)
    assert np.all(np.abs(got - np.array(R.BS1770_48K)) <= 1e-14), np.abs(got - np.array(R.BS1770_48K)).max()
    assert np.all(np.abs(R.coefficients(48000) - np.array(R.BS1770_48K)) <= 1e-14)


@pytest.mark.parametrize("sr", [8000, 11025, 44100, 48000, 96000, 192000])
def test_plan_against_numpy(sr):
    lens = [0, 1, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 3, 5 * R.seg_len(sr) - 1, 0]
    plan = LD.plan(sr, lens)
    S = R.seg_len(sr)
    assert plan.S == S == LD.seg_samples(sr) and plan.n == len(lens) and plan.total == sum(lens)
    want = R.coefficients(sr)
    assert np.all(np.abs(plan.coef - want) <= 4.0 * np.spacing(np.abs(want))), np.abs(plan.coef - want).max()      # (tan, pow of two libms)
    assert np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lens)]))
    assert plan.seg_off.dtype == np.int64 and np.array_equal(plan.seg_off, np.concatenate([[0], np.cumsum([n // S for n in lens])]))
    tiles = [(i, k) for i, n in enumerate(lens) for k in range(-(-n // TILE))]
    assert plan.tiles.dtype == np.int32 and plan.tiles.tolist() == [list(t) for t in tiles] and plan.n_tiles == len(tiles)
    assert plan.blob.nbytes == 16 * (len(lens) + 1) + 80 + 8 * 16 * LD.MATS + 8 * len(tiles)
    # A^(16 * 2^k): the same squaring in numpy's long double from the plan's own coefficients.  Both round a value that is good
    # to about 2^-60 of the matrix's largest entry to float64, so they agree within an ulp or two of that entry.
    c = plan.coef.astype(np.longdouble)
    A = np.zeros((4, 4), dtype=np.longdouble)
    A[0, 0], A[0, 1], A[1, 0], A[3, 2] = -c[3], -c[4], 1.0, 1.0
    A[2] = [c[6] - c[5] * c[3], c[7] - c[5] * c[4], -c[8], -c[9]]
    assert np.allclose(A.astype(np.float64), R.transition(sr), rtol=1e-15, atol=0.0)
    P = A
    for _ in range(4):
        P = P @ P
    assert plan.mats.shape == (LD.MATS, 4, 4)
    assert np.abs(plan.mats[0] - np.linalg.matrix_power(R.transition(sr), 16)).max() <= 1e-12 * np.abs(plan.mats[0]).max()
    for k in range(LD.MATS):
        top = float(np.abs(P).max())
        err = float(np.abs(plan.mats[k].astype(np.longdouble) - P).max())
        assert err <= 2.0 ** -50 * top, (k, err / top)
        P = P @ P


def test_a_full_scale_997_hz_sine_measures_minus_3_01_lufs():
    t = np.arange(48000) / 48000.0
    x = np.sin(2.0 * np.pi * 997.0 * t).astype(np.float32)
    for dtype in (np.float64, np.longdouble):
        E, L, mm, g = R.measure(x, 48000, dtype=dtype)
        assert len(E) == 10 and abs(float(L) + 3.01) <= 0.01 and abs(float(mm) + 3.01) <= 0.01 and g == 1.0, (L, mm)
    assert R.measure(x, 48000, target=-23.0)[3] == np.float32(10.0 ** ((-23.0 - R.measure(x, 48000)[1]) / 20.0))


def _call(sr, in_off, n, tiles_cap, s=True, coef=True, mats=True, seg=True, tiles=True, need=True):
    lib = _lib.load()
    S, nd = C.c_int(-7), (C.c_int64 * 1)(-7)
    co, ma, so = np.full(10, -7.0), np.full(16 * LD.MATS, -7.0), np.full(max(n, 0) + 1, -7, dtype=np.int64)
    tl = np.full((max(tiles_cap, 1), 2), -7, dtype=np.int32)
    rc = lib.goofer_host_loudness_plan(sr, None if in_off is None else in_off.ctypes.data, n, C.byref(S) if s else None,
                                       co.ctypes.data if coef else None, ma.ctypes.data if mats else None,
                                       so.ctypes.data if seg else None, tl.ctypes.data if tiles else None, tiles_cap, nd if need else None)
    return rc, S.value, nd[0], co, so, tl


def test_refusals_and_the_capacity_protocol():
    off = np.array([0, 100, 5000], dtype=np.int64)
    assert _call(48000, off, 2, 3)[0] == 0
    for sr in (7999, 192001, 0, -48000):
        assert _call(sr, off, 2, 3)[0] == -1, sr
    assert _call(8000, off, 2, 3)[:2] == (0, 800) and _call(192000, off, 2, 3)[:2] == (0, 19200)
    assert _call(48000, np.array([0, 100, 50], dtype=np.int64), 2, 3)[0] == -1                # offsets that decrease
    assert _call(48000, np.array([0, 1 << 31], dtype=np.int64), 1, 1 << 20)[0] == -1
    assert _call(48000, None, 2, 3)[0] == -1                                                  # null pointers
    for gone in ("s", "coef", "mats", "seg", "tiles", "need"):
        assert _call(48000, off, 2, 3, **{gone: False})[0] == -1, gone
    assert _call(48000, off, -1, 3)[0] == -1 and _call(48000, off, 2, -1)[0] == -1
    # a capacity that is too small: 1, with S and need; nothing else is promised
    for cap in (2, 0):
        assert _call(48000, off, 2, cap, tiles=cap > 0)[:3] == (1, 4800, 3), cap
    rc, S, need, coef, seg, tiles = _call(48000, off, 2, 3)
    assert (rc, S, need) == (0, 4800, 3) and tiles.tolist() == [[0, 0], [1, 0], [1, 1]] and seg.tolist() == [0, 0, 1]
    assert np.array_equal(coef, LD.plan(48000, [100, 4900]).coef)
    assert _call(48000, None, 0, 0, tiles=False)[:3] == (0, 4800, 0)                            # no signal: the tables alone
    for bad in (7999, 192001, 44100.5):
        with pytest.raises(ValueError):
            LD.plan(bad, [100])
    with pytest.raises(ValueError):
        LD.plan(48000, [100, -1])
    assert LD.parse(-16) == (-16.0, 20.0) and LD.parse((-23, 6)) == (-23.0, 6.0) and LD.parse((-23.0, 0)) == (-23.0, 0.0)
    for bad in (float("nan"), float("inf"), -float("inf"), (-16.0, -0.1), (-16.0, 60.1), (-16.0, float("nan")), (-16.0, 20.0, 1.0)):
        with pytest.raises(ValueError):
            LD.parse(bad)


def test_the_float64_flavour_leaves_the_bound_unspent():
    """On every input of the GPU tests the float64 restatement is within 2^-26 max E of the long-double one: far within."""
    worst = 0.0
    for key, sr, x in R.all_inputs():
        ld, f64 = R.reference(key, "ld")[0], R.reference(key, "f64")[0]
        ok = ~np.isnan(ld)
        assert np.array_equal(ok, ~np.isnan(f64)), key
        if ok.any():
            top = np.abs(ld[ok]).max()
            err = float(np.abs(f64[ok].astype(np.longdouble) - ld[ok]).max())
            assert err <= R.TOL * float(top), (key, err / float(top))
            if top > 0:
                worst = max(worst, err / float(top))
    print("float64 against long double, worst error / max E = %.3e (bound %.3e)" % (worst, R.TOL))
    assert worst <= R.TOL / 100.0


def test_gating_fixtures_have_blocks_in_every_class_and_none_on_a_threshold():
    sr, xs = R.gating_fixtures()
    S = R.seg_len(sr)
    for k in range(len(xs)):
        E, L, _ = R.reference(("gate", k), "ld")
        z = R.blocks(E.astype(np.float64), S)
        classes, thresholds = R.gate_classes(z)
        assert all(c.any() for c in classes), (k, [int(c.sum()) for c in classes])
        for th in thresholds:
            assert np.all(np.abs(z - th) > 1e-6 * th), k
        assert abs(L - R.ungated(E.astype(np.float64), S)) > 1.0, k
    sr, x = R.under_gate_signal()
    E, L, mm = R.reference(("under",), "ld")
    assert len(E) == 10 and L == -np.inf and np.isfinite(mm) and mm < -70.0


# ---- wrong variants: each breaks a bound of tests/test_gpu_loudness.py on that file's inputs ------------------------------

def _breaks_energy(wrong, key):
    E = R.reference(key, "ld")[0]
    return len(wrong) != len(E) or bool(np.any(np.abs(wrong.astype(np.longdouble) - E) > R.TOL * np.abs(E).max()))


def _long(sr):
    """the signal over four tiles and its key"""
    b, i = R.trio(sr)
    return R.batch(sr)[b][i], (sr, b, i)


@pytest.mark.parametrize("sr", R.RATES)
def test_wrong_fp32_state_breaks_the_energy_bound(sr):
    x, key = _long(sr)
    wrong = R.seg_energy(R.weighted_squares(x, sr, state_dtype=np.float32)[0], R.seg_len(sr))
    assert _breaks_energy(wrong, key)


@pytest.mark.parametrize("sr", R.RATES)
def test_wrong_state_zeroed_at_a_tile_boundary_breaks_the_energy_bound(sr):
    x, key = _long(sr)
    wrong = R.seg_energy(R.weighted_squares(x, sr, zero_every=TILE)[0], R.seg_len(sr))
    assert _breaks_energy(wrong, key)


def test_wrong_state_zeroed_between_two_runs_of_tiles_breaks_the_energy_bound():
    """the state lost where one thread's 16 tiles end and the next thread's begin"""
    sr, b, i = R.runs_signal()
    x = R.batch(sr)[b][i]
    assert len(x) > R.RUN_TILES * TILE and i > 0
    wrong = R.seg_energy(R.weighted_squares(x, sr, zero_every=R.RUN_TILES * TILE)[0], R.seg_len(sr))
    assert _breaks_energy(wrong, (sr, b, i))
    k = R.RUN_TILES * TILE // R.seg_len(sr)                             # ... and it is the segments behind the boundary that break
    E = R.reference((sr, b, i))[0]
    bad = np.abs(wrong.astype(np.longdouble) - E) > R.TOL * np.abs(E).max()
    assert not bad[:k].any() and bad[k]


def test_wrong_state_zeroed_between_two_rounds_of_tiles_breaks_the_window_bound():
    """the GPU test's window around tile 4096 of the long signal, with the state lost at that tile's first sample"""
    sr, x = R.long_signal()
    S, at = R.seg_len(sr), 4096 * TILE
    kr = at // S
    want = R.window_energy(x, sr, kr - 4, kr + 12)
    a = (kr - 14) * S                                                   # (window_energy's own start: one multiple of at - a inside)
    wrong = R.seg_energy(R.weighted_squares(x[a:(kr + 12) * S], sr, zero_every=at - a)[0], S)[10:]
    bad = np.abs(wrong.astype(np.longdouble) - want) > R.TOL * want.max()
    assert len(wrong) == len(want) == 16 and not bad[:4].any() and bad[4]


def test_window_energy_is_the_whole_restatement():
    sr, b, i = R.runs_signal()
    x, E = R.batch(sr)[b][i], R.reference((sr, b, i))[0]
    got = R.window_energy(x, sr, 60, 80)
    assert len(got) == 20 and np.all(np.abs(got - E[60:80]) <= 1e-3 * R.TOL * np.abs(E).max())


@pytest.mark.parametrize("sr", R.RATES)
def test_wrong_history_from_the_previous_signal_breaks_the_zero_signal(sr):
    b, i = R.trio(sr)
    xs = R.batch(sr)[b]
    _, last = R.weighted_squares(xs[i + 1], sr)
    wrong = R.seg_energy(R.weighted_squares(xs[i + 2], sr, history=last)[0], R.seg_len(sr))
    assert np.any(wrong != 0.0)                                       # the GPU test wants exactly 0.0 there
    wrong = R.seg_energy(R.weighted_squares(xs[i], sr, history=last)[0], R.seg_len(sr))
    assert _breaks_energy(wrong, (sr, b, i))


@pytest.mark.parametrize("sr", R.RATES)
def test_wrong_trailing_partial_segment_breaks_the_count_and_the_loudness(sr):
    S = R.seg_len(sr)
    x = next(v for xs in R.batch(sr) for v in xs if len(v) == 4 * S - 1)                    # no block by the definition
    wrong = R.seg_energy(R.weighted_squares(x, sr)[0], S, partial=True)
    assert len(wrong) == 4 and R.stats(wrong, S)[0] > -np.inf          # the GPU test wants 3 segments, -inf and gain 1


def test_wrong_gates_break_the_loudness_bound():
    sr, xs = R.gating_fixtures()
    S = R.seg_len(sr)
    for k in range(len(xs)):
        E, L, _ = R.reference(("gate", k), "ld")
        assert abs(R.stats(E, S, rel_factor=10.0 ** -0.8)[0] - L) > 1e-6, k        # the relative gate at -8 LU
    E = R.reference(("under",), "ld")[0]
    assert np.isfinite(R.stats(E, S, abs_gate=False)[0])                              # no absolute gate: a loudness where -inf belongs
