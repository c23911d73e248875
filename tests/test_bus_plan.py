"""The host half of the stereo bus (no GPU): the pan law, goofer_host_bus_plan against a brute-force cover, its capacity protocol
and every refusal, the Python plan, the song-file parser, the two-channel wav, and the limiter plan's ``channels``."""
import ctypes as C
import math
import wave

import numpy as np
import pytest

import bus_ref as R
from goofer_amd import _lib
from goofer_amd import bus as B
from goofer_amd import limit as LM

EINVAL = -1


def test_pan_law_exact_positions():
    for db in (0.0, -6.0, 24.0, -144.0, 3.3):
        g = 10.0 ** (db / 20.0)
        gl, gr = B.gains(db, -1.0)
        assert gl == np.float32(g) and gr == 0.0 and not np.signbit(gr)
        gl, gr = B.gains(db, 1.0)
        assert gr == np.float32(g) and gl == 0.0 and not np.signbit(gl)
        gl, gr = B.gains(db, 0.0)
        assert gl == gr == np.float32(g * math.sqrt(0.5))
        assert gl.dtype == np.float32 and gr.dtype == np.float32


def test_pan_law_constant_power_and_restatement():
    for db in np.linspace(-144.0, 24.0, 29):
        g = 10.0 ** (db / 20.0)
        for pan in np.linspace(-1.0, 1.0, 41):
            gl, gr = B.gains(db, pan)
            assert (gl, gr) == R.gains(db, pan)
            assert abs(float(gl) ** 2 + float(gr) ** 2 - g * g) <= 2.0 ** -22 * g * g
    left = [float(B.gains(0.0, p)[0]) for p in np.linspace(-1.0, 1.0, 41)]
    assert all(a >= b for a, b in zip(left, left[1:]))


@pytest.mark.parametrize("db, pan", [(math.nan, 0.0), (math.inf, 0.0), (-144.5, 0.0), (24.5, 0.0), (0.0, 1.0001), (0.0, -1.5), (0.0, math.nan)])
def test_pan_law_refusals(db, pan):
    with pytest.raises(ValueError):
        B.gains(db, pan)


def _records(starts, lens, ptr=4096):
    rec = np.zeros(len(starts), dtype=_lib.BUS_TRACK)
    rec["x"], rec["len"], rec["start"], rec["gl"], rec["gr"] = ptr, lens, starts, 0.5, 0.25
    return rec


def test_record_layout():
    assert _lib.BUS_TRACK.itemsize == 32
    assert [_lib.BUS_TRACK.fields[k][1] for k in ("x", "len", "start", "gl", "gr")] == [0, 8, 16, 24, 28]


def test_planner_against_brute_force():
    rng = np.random.default_rng(20261021)
    for trial in range(40):
        n = int(rng.integers(0, 9))
        total = int(rng.choice([0, 1, 2047, 2048, 2049, 5000, 20000]))
        starts = rng.integers(0, 12000, n)
        lens = rng.choice([0, 1, 7, 2048, 3000, 9000], n)
        if trial % 5 == 0 and n:
            starts[0], lens[0] = 2048, 2048                     # exactly one tile
        tile_off, tile_tracks = B.cover(_records(starts, lens), total)
        want_off, want = R.cover(starts, lens, total)
        assert np.array_equal(tile_off, want_off) and np.array_equal(tile_tracks, want)
        for t in range(len(want_off) - 1):
            assert list(want[want_off[t]:want_off[t + 1]]) == sorted(want[want_off[t]:want_off[t + 1]])


def test_planner_capacity_protocol():
    lib = _lib.load()
    rec = _records([0, 100, 5000], [6000, 10, 3000])
    total = 9000
    want_off, want = R.cover(rec["start"], rec["len"], total)
    tile_off = np.zeros(len(want_off), dtype=np.int64)
    need = C.c_int64(-1)
    small = np.full(len(want) - 1, -7, dtype=np.int32)
    assert lib.goofer_host_bus_plan(rec.ctypes.data, 3, total, tile_off.ctypes.data, small.ctypes.data, len(small), C.byref(need)) == 1
    assert need.value == len(want) and (small == -7).all()
    assert lib.goofer_host_bus_plan(rec.ctypes.data, 3, total, tile_off.ctypes.data, None, 0, C.byref(need)) == 1 and need.value == len(want)
    full = np.zeros(len(want), dtype=np.int32)
    assert lib.goofer_host_bus_plan(rec.ctypes.data, 3, total, tile_off.ctypes.data, full.ctypes.data, len(full), C.byref(need)) == 0
    assert np.array_equal(full, want) and np.array_equal(tile_off, want_off)
    # no track, no sample: a table of one zero
    assert lib.goofer_host_bus_plan(None, 0, 0, tile_off.ctypes.data, None, 0, C.byref(need)) == 0 and need.value == 0 and tile_off[0] == 0


def test_planner_refusals():
    lib = _lib.load()
    rec = _records([0, 10], [100, 100])
    tile_off, tt, need = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int32), C.c_int64(0)

    def call(r=rec, n=2, total=300, off=tile_off, tracks=tt, cap=8, nd=need):
        return lib.goofer_host_bus_plan(None if r is None else r.ctypes.data, n, total, None if off is None else off.ctypes.data,
                                        None if tracks is None else tracks.ctypes.data, cap, None if nd is None else C.byref(nd))
    assert call() == 0
    assert call(r=None) == EINVAL and call(off=None) == EINVAL and call(tracks=None) == EINVAL and call(nd=None) == EINVAL
    assert call(n=-1) == EINVAL and call(total=-1) == EINVAL and call(cap=-1) == EINVAL
    assert call(total=2048 * (1 << 31)) == EINVAL               # 2^31 tiles; nothing of that size is touched
    for field, bad in (("len", -1), ("start", -1), ("gl", np.nan), ("gr", np.inf), ("gl", -np.inf), ("x", 0), ("x", 4098)):
        r = rec.copy()
        r[field][1] = bad
        assert call(r=r) == EINVAL, (field, bad)
    r = rec.copy()
    r["x"][1], r["len"][1] = 0, 0                               # no sample: no pointer needed
    assert call(r=r) == 0
    with pytest.raises(ValueError):
        B.cover(_records([0], [-1]), 10)


def test_python_plan():
    tracks = [B.Track(-3.0, -0.5), B.Track(0.0, 0.5, start_ms=100.0), B.Track(mute=True), B.Track(-6.0, 1.0, start_ms=0.0)]
    p = B.plan([4096, 8192, 0, 12288], [1000, 500, 77, 0], tracks, 48000)
    assert p.n == 3 and list(p.index) == [0, 1, 3] and p.total_out == 4800 + 500 and p.sr == 48000
    assert list(p.tracks["start"]) == [0, 4800, 0] and list(p.tracks["len"]) == [1000, 500, 0]
    assert (p.tracks["gl"][0], p.tracks["gr"][0]) == R.gains(-3.0, -0.5) and p.tracks["gl"][2] == 0.0
    assert np.array_equal(p.in_off, [0, 5300, 10600])
    want_off, want = R.cover(p.tracks["start"], p.tracks["len"], p.total_out)
    assert np.array_equal(p.tile_off, want_off) and np.array_equal(p.tile_tracks, want)
    assert len(p.blob) == p.tracks.nbytes + p.tile_off.nbytes + p.tile_tracks.nbytes + 4
    assert B.plan([4096], [1000], [B.Track()], 8000, total_out=300).total_out == 300
    assert B.plan([], [], [], 8000).total_out == 0 and B.plan([0], [5], [B.Track(mute=True)], 8000).n == 0
    assert B.samples(100.0, 44100) == 4410 and B.samples(0.011, 44100) == 0 and B.samples(0.012, 44100) == 1
    for bad in (dict(tracks=[B.Track(start_ms=-1.0)]), dict(tracks=[B.Track(pan=2.0)]), dict(tracks=[B.Track(gain_db=30.0)]),
                dict(lengths=[-1]), dict(sr=44100.5), dict(tracks=[]), dict(tracks=[B.Track(start_ms=math.nan)])):
        kw = dict(ptrs_or_tensors=[4096], lengths=[10], tracks=[B.Track()], sr=8000)
        kw.update(bad)
        with pytest.raises(ValueError):
            B.plan(**kw)


def test_song_file(tmp_path):
    job, t = B.parse_line("lead.txt")
    assert job == "lead.txt" and t == B.Track()
    job, t = B.parse_line("sub/harm.txt -6 -0.5 250 eq=hp:120 reverb=room:1.2:-10 mute")
    assert job == "sub/harm.txt" and (t.gain_db, t.pan, t.start_ms, t.mute) == (-6.0, -0.5, 250.0, True)
    assert t.eq[0].kind == "highpass" and t.eq[0].f0_hz == 120.0 and t.reverb is not None and t.compress is None
    _, t = B.parse_line("a.txt 3 compress=-20:4")
    assert (t.gain_db, t.pan, t.start_ms) == (3.0, 0.0, 0.0) and t.compress.ratio == 4.0
    for bad in ("", "a.txt 0 0 0 0", "a.txt mute 3", "a.txt eq=hp:120 -3", "a.txt 0 2", "a.txt 30", "a.txt 0 0 -5", "a.txt x", "a.txt eq=",
                "a.txt eq=hp:120 eq=hp:80", "a.txt eq=nonsense"):
        with pytest.raises(ValueError):
            B.parse_line(bad)
    song = tmp_path / "song.txt"
    song.write_text("# a song\n\nlead.txt 0 0\n  sub/harm.txt -6 0.5 100\n/abs/choir.txt -9 mute\n")
    lines = B.read_song(song)
    assert [p for p, _ in lines] == [str(tmp_path / "lead.txt"), str(tmp_path / "sub/harm.txt"), "/abs/choir.txt"]
    assert [t.mute for _, t in lines] == [False, False, True] and lines[1][1].start_ms == 100.0
    song.write_text("lead.txt 0 0\nharm.txt 0 7\n")
    with pytest.raises(ValueError, match="song.txt:2"):
        B.read_song(song)
    assert B.main(["--true-peak", str(song), str(tmp_path / "o.wav")]) == 1     # --true-peak without --limit: the usage line
    assert B.main([str(song)]) == 1


def test_write_wav_stereo(tmp_path):
    from goofer_amd.render import write_wav
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.2, 1.2, (37, 2)).astype(np.float32)
    x[0], x[1] = (1.0, -1.0), (0.5 / 32768.0, 1.5 / 32768.0)
    want = R.pcm16_planar(np.concatenate([x[:, 0], x[:, 1]]))
    for k, data in enumerate((x, want)):
        path = tmp_path / f"s{k}.wav"
        write_wav(path, data, 48000)
        with wave.open(str(path), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, 48000, 37)
            assert w.readframes(37) == want.astype("<i2").tobytes()
    write_wav(tmp_path / "m.wav", x[:, 0], 8000)                # 1-D input: one channel, as before
    with wave.open(str(tmp_path / "m.wav"), "rb") as w:
        assert (w.getnchannels(), w.getnframes()) == (1, 37) and w.readframes(37) == want[:, 0].astype("<i2").tobytes()
    with pytest.raises(ValueError):
        write_wav(tmp_path / "bad.wav", np.zeros((4, 3), np.float32), 8000)


def test_limit_plan_channels():
    one = LM.plan(48000, [9000, 9000, 100, 100])
    two = LM.plan(48000, [9000, 9000, 100, 100], channels=2)
    grp = LM.plan(48000, [9000, 100])
    assert one.channels == 1 and two.channels == 2 and two.n == 4 and np.array_equal(two.in_off, one.in_off)
    assert np.array_equal(two.tiles, grp.tiles) and two.W == one.W and np.array_equal(two.taps, one.taps)
    assert len(one.tiles) == 2 * len(grp.tiles) and LM.plan(48000, [], channels=2).n == 0
    for bad in ([9000, 8999], [10, 10, 10]):
        with pytest.raises(ValueError):
            LM.plan(48000, bad, channels=2)
    with pytest.raises(ValueError):
        LM.plan(48000, [10, 10], channels=3)
