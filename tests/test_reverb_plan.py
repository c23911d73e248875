"""CPU: the convolution reverb's settings (goofer_amd.reverb: ``Reverb``, ``Room``, ``parse``) and the library's host planner
(goofer_host_reverb_plan) against the numpy restatement of its tables (tests/reverb_ref.py), with the capacity protocol."""
import ctypes as C
import math
import wave

import numpy as np
import pytest

import reverb_ref as R
from goofer_amd import _lib
from goofer_amd import reverb as RV

B = R.B


def _wav(path, y, sr, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(np.asarray(y) * 32767.0).astype("<i2").tobytes())


def test_parse_takes_every_form(tmp_path):
    h = R.ir(300)
    rv = RV.Reverb(h)
    assert RV.parse(rv) is rv
    assert (rv.wet_db, rv.dry_db, rv.predelay_ms, rv.tail, rv.ir_sr) == (-12.0, 0.0, 0.0, True, None)
    assert rv.ir.dtype == np.float32 and np.array_equal(rv.ir, h) and abs(rv.wet - 10.0 ** (-12.0 / 20.0)) < 1e-15 and rv.dry == 1.0
    t = RV.parse((h.astype(np.float64), -6, -3, 12.5, False))
    assert (t.wet_db, t.dry_db, t.predelay_ms, t.tail) == (-6.0, -3.0, 12.5, False) and np.array_equal(t.ir, h)
    assert RV.parse([list(h[:4])]).ir.tolist() == h[:4].tolist()
    room = RV.Room(0.3, 7)
    assert RV.parse(room).ir == room and RV.parse((room, -20)).wet_db == -20.0
    for spec, want in (("room:0.3", (RV.Room(0.3), -12.0, 0.0)), ("room:0.3:-10", (RV.Room(0.3), -10.0, 0.0)),
                       ("room:0.3:-10:5", (RV.Room(0.3), -10.0, 5.0)), ("room:0.3:-10:5:7", (room, -10.0, 5.0)),
                       ("room:1.5:-inf", (RV.Room(1.5), -math.inf, 0.0))):
        p = RV.parse(spec)
        assert (p.ir, p.wet_db, p.predelay_ms) == want and p.dry_db == 0.0 and p.tail
    assert RV.parse("room:1:-inf").wet == 0.0 and RV.Reverb(h, dry_db=-math.inf).dry == 0.0
    # a mono wav, read by the standard-library reader; its rate is remembered
    path = tmp_path / "hall:1.wav"                               # (a colon of the path's own)
    _wav(path, h * 0.5, 44100)
    for spec, wet, pre in ((f"ir:{path}", -12.0, 0.0), (f"ir:{path}:-9", -9.0, 0.0), (f"ir:{path}:-9:20", -9.0, 20.0)):
        p = RV.parse(spec)
        assert (p.wet_db, p.predelay_ms, p.ir_sr) == (wet, pre, 44100) and p.ir.shape == (300,)
        assert np.max(np.abs(p.ir - h * 0.5)) <= 1.0 / 32768.0
    assert RV.plan(44100, [10], f"ir:{path}").L == 300
    with pytest.raises(ValueError, match="recorded at 44100"):
        RV.plan(48000, [10], f"ir:{path}")                       # a wav at another rate than the stage's
    # the pre-delay in whole samples, rounded half up; a room's IR at the plan's rate
    assert RV.Reverb(h, predelay_ms=10.0).predelay(44100) == 441 and RV.Reverb(h, predelay_ms=0.0113).predelay(44100) == 0
    assert RV.Reverb(h, predelay_ms=0.0114).predelay(44100) == 1
    assert RV.plan(48000, [], "room:0.3").L == 14400 and RV.plan(8000, [], "room:0.3").L == 2400


def test_parse_refuses(tmp_path):
    h = R.ir(10)
    stereo = tmp_path / "stereo.wav"
    _wav(stereo, np.zeros(20), 48000, channels=2)
    for bad in ("", "room", "room:", "room:fast", "room:0.3:-10:5:7:1", "room:0.3:-10:5:1.5", "room:0:-10", "room:-1", "room:nan", "hall:0.3",
                "ir", "ir:", f"ir:{tmp_path}/missing.wav", f"ir:{stereo}", "room:0.3:nan", "room:0.3:inf", "room:0.3:-10:-1", None, 3.0, (),
                (h, 1, 2, 3, True, 5), ("room:0.3",), (np.zeros((2, 3)),), {"ir": h}):
        with pytest.raises(ValueError):
            RV.parse(bad)
    for bad in (dict(ir=np.zeros(0)), dict(ir=np.zeros((2, 2))), dict(ir=np.array([1.0, np.nan])), dict(ir=np.array([np.inf])),
                dict(ir=np.zeros(RV.MAX_TAPS + 1)), dict(ir="hall"), dict(ir=h, wet_db=math.nan), dict(ir=h, wet_db=math.inf),
                dict(ir=h, wet_db=800.0), dict(ir=h, dry_db=math.nan), dict(ir=h, dry_db=math.inf), dict(ir=h, predelay_ms=-0.1),
                dict(ir=h, predelay_ms=math.nan), dict(ir=h, predelay_ms=math.inf), dict(ir=h, wet_db="loud"), dict(ir=h, ir_sr=100)):
        with pytest.raises(ValueError):
            RV.Reverb(**bad)
    assert len(RV.Reverb(np.zeros(RV.MAX_TAPS)).ir) == RV.MAX_TAPS
    # what only the plan can see: the rate, the pre-delay in samples, the room's length, the lengths
    for sr, lengths, rv in ((7999, [10], (h,)), (192001, [10], (h,)), (48000.5, [10], (h,)), (48000, [-1], (h,)),
                            (48000, [10], RV.Reverb(h, predelay_ms=1000.0 * (2 ** 16 + 1) / 48000)), (48000, [10], "room:6"),
                            (48000, [2 ** 31 - 9], (h,)), (48000, [2 ** 31 - 1 - 9 - 5], RV.Reverb(h, predelay_ms=1000.0 * 6 / 48000))):
        with pytest.raises(ValueError):
            RV.plan(sr, lengths, rv)
    assert RV.plan(48000, [10], RV.Reverb(h, predelay_ms=1000.0 * 2 ** 16 / 48000)).pre == 2 ** 16
    assert RV.plan(48000, [2 ** 31 - 1 - 9 - 5], RV.Reverb(h, predelay_ms=1000.0 * 5 / 48000)).total_out == 2 ** 31 - 1
    assert RV.plan(48000, [2 ** 31 - 1], RV.Reverb(h, tail=False)).total_out == 2 ** 31 - 1


@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("L, pre", [(1, 0), (B, 1), (B + 1, B - 1), (2 * B + 5, B + 3), (40 * B + 3, 0), (300, 5000)])
def test_the_planner_against_the_restatement(L, pre, tail):
    lengths = R.LENGTHS + [0, 33 * B, 32 * B - pre - L + 1 if 32 * B - pre - L + 1 > 0 else 5, 64 * B + 1, 3]     # n = 0 and pre > n too
    rv = RV.Reverb(np.ones(L, np.float32), predelay_ms=1000.0 * pre / 48000.0, tail=tail)
    plan = RV.plan(48000, lengths, rv)
    out_off, blk_off, runs = R.tables(lengths, L, pre, tail)
    assert (plan.L, plan.pre, plan.tail, plan.n) == (L, pre, tail, len(lengths))
    assert plan.out_off.dtype == np.int64 and np.array_equal(plan.out_off, out_off)
    assert plan.blk_off.dtype == np.int64 and np.array_equal(plan.blk_off, blk_off)
    assert plan.runs.dtype == np.int32 and plan.runs.shape == runs.shape and np.array_equal(plan.runs, runs)
    assert np.array_equal(plan.in_off, np.concatenate([[0], np.cumsum(lengths)]))
    assert plan.total_out == out_off[-1] and plan.total_blocks == blk_off[-1] and plan.n_runs == len(runs)
    assert plan.added == (pre + L - 1 if tail else 0)
    n_out = np.diff(plan.out_off)
    assert all(m == (0 if n == 0 else n + plan.added) for n, m in zip(lengths, n_out))
    # every block of every signal in exactly one run, no run longer than 32 blocks
    seen = np.zeros(plan.total_blocks, dtype=np.int32)
    for s, first, count in plan.runs:
        assert 1 <= count <= R.RUN and first % R.RUN == 0
        seen[plan.blk_off[s] + first:plan.blk_off[s] + first + count] += 1
        assert first + count <= plan.blk_off[s + 1] - plan.blk_off[s]
    assert np.all(seen == 1)
    # the blob: the four tables back to back
    assert plan.blob.nbytes == 3 * 8 * (plan.n + 1) + 12 * plan.n_runs
    assert np.array_equal(plan.blob[24 * (plan.n + 1):].view(np.int32).reshape(-1, 3), runs)


def test_no_signal_and_signals_without_a_sample():
    for lengths in ([], [0], [0, 0, 0]):
        plan = RV.plan(48000, lengths, (R.ir(100), -6))
        assert plan.total == plan.total_out == plan.total_blocks == plan.n_runs == 0 and plan.runs.shape == (0, 3)
        assert plan.out_off.tolist() == [0] * (len(lengths) + 1)


def test_the_capacity_protocol():
    lib = _lib.load()
    in_off = np.array([0, 5, 5, 40 * B], dtype=np.int64)
    out_off, blk_off, need = np.full(4, -1, np.int64), np.full(4, -1, np.int64), (C.c_int64 * 1)(-1)
    want_out, want_blk, want_runs = R.tables([5, 0, 40 * B - 5], 3 * B, 7, True)

    def call(runs, cap, sr=48000, n=3, L=3 * B, pre=7, off=in_off.ctypes.data, out=out_off.ctypes.data, blk=blk_off.ctypes.data,
             need_p=need):
        return lib.goofer_host_reverb_plan(sr, off, n, L, pre, 1, out, blk, None if runs is None else runs.ctypes.data, cap, need_p)
    assert call(None, 0) == 1 and need[0] == len(want_runs) == 3                 # the query: only need is valid
    short = np.full((2, 3), -1, np.int32)
    assert call(short, 2) == 1 and need[0] == 3 and np.all(short == -1)          # too short: nothing written
    runs = np.full((5, 3), -1, np.int32)
    assert call(runs, 5) == 0 and need[0] == 3
    assert np.array_equal(runs[:3], want_runs) and np.all(runs[3:] == -1)
    assert np.array_equal(out_off, want_out) and np.array_equal(blk_off, want_blk)
    for bad in (dict(sr=7999), dict(sr=192001), dict(L=0), dict(L=R.MAX_TAPS + 1), dict(pre=-1), dict(pre=R.MAX_PREDELAY + 1), dict(n=-1),
                dict(off=None), dict(out=None), dict(blk=None), dict(need_p=None)):
        assert call(runs, 5, **bad) == -1, bad
    assert call(None, 5) == -1 and call(runs, -1) == -1
    assert call(np.zeros((64, 3), np.int32), 64, L=R.MAX_TAPS, pre=R.MAX_PREDELAY) == 0   # the ends of the ranges are inside
    down = np.array([0, 5, 4, 10], dtype=np.int64)
    assert call(runs, 5, off=down.ctypes.data) == -1                             # offsets that decrease
    assert call(None, 0, n=0, off=None) == 0 and need[0] == 0                    # no signal: nothing to write but the zeros
