"""Phrase assembly, host half (goofer_amd/phrase.py and the library's goofer_host_phrase_plan): wavtool's arguments to note
records, placement, the cover table against a brute-force cover, the capacity protocol and the refusals.  Pure host code: no
GPU."""
import ctypes as C

import numpy as np
import pytest

import phrase_ref as R
from goofer_amd import _lib
from goofer_amd import phrase as P

SR = 44100


def test_parse_length():
    assert P.parse_length("480@120+15.5") == 480 / 480 * 60000 / 120 + 15.5 == 515.5
    assert P.parse_length("240@90-3") == 240 / 480 * 60000 / 90 - 3
    assert P.parse_length("500") == 500.0
    assert P.parse_length("240@120") == 250.0
    assert P.parse_length(12.5) == 12.5
    with pytest.raises(ValueError):
        P.parse_length("abc")


def _knots_ms(pos, sr=SR):
    return pos.astype(np.float64) * 1000.0 / sr


def test_envelope_knots_short_form():
    L = 500.0
    pos, val = P.envelope_knots("5 35 40 10 100 90 20".split(), L, SR)
    take = P.samples(L, SR)
    assert take == 22050 and pos.dtype == val.dtype == np.float32
    # p4 = 0, no p5 / v5: knot 3 repeats knot 2
    want = np.array([0, 5, 40, 40, 460, 500, 500], dtype=np.float64) * SR / 1000
    assert np.array_equal(pos, want.astype(np.float32))
    assert pos[0] == 0 and pos[6] == np.float32(take)
    assert np.array_equal(val, np.array([0, 0.1, 1.0, 1.0, 0.9, 0.2, 0], dtype=np.float32))
    assert P.envelope_overlap("5 35 40 10 100 90 20".split()) == 0.0


def test_envelope_knots_full_form_and_missing_p5():
    L = 400.0
    args = "10 20 30 50 100 80 40 25 15 60 120".split()        # p1 p2 p3 v1 v2 v3 v4 ovr p4 p5 v5
    pos, val = P.envelope_knots(args, L, SR)
    want = np.array([0, 10, 30, 90, 355, 385, 400], dtype=np.float64) * SR / 1000
    assert np.array_equal(pos, want.astype(np.float32))
    assert np.array_equal(val, (np.array([0, 50, 100, 120, 80, 40, 0], dtype=np.float64) / 100).astype(np.float32))
    assert P.envelope_overlap(args) == 25.0
    # without p5 / v5 (nine values: ovr and p4 given)
    pos9, val9 = P.envelope_knots(args[:9], L, SR)
    assert np.array_equal(pos9, (np.array([0, 10, 30, 30, 355, 385, 400], dtype=np.float64) * SR / 1000).astype(np.float32))
    assert val9[3] == val9[2] == np.float32(1.0)
    for bad in (args[:6], args[:10], args + ["1"]):
        with pytest.raises(ValueError):
            P.envelope_knots(bad, L, SR)


def test_envelope_knots_of_a_note_too_short_for_its_envelope():
    # p1 + p2 = 80 ms > L - p4 - p3 = 30.3 - 5 - 20: the running maximum keeps the knots in order, the clamp inside the note
    L = 30.3
    pos, val = P.envelope_knots("30 50 20 100 100 100 100 0 5".split(), L, SR)
    take = P.samples(L, SR)
    assert take == 1336                                         # 1336.23 samples: take lies below L * sr / 1000
    assert np.all(np.diff(pos) >= 0) and pos[0] == 0 and pos[6] == np.float32(take)
    assert pos.max() <= np.float32(take)
    ms = _knots_ms(pos)
    assert abs(ms[1] - 30.0) < 1e-3 and np.all(ms[2:6] >= 30.0)
    # and the library takes the record
    notes = np.zeros(1, dtype=_lib.PHRASE_NOTE)
    notes[0] = (0, 0, take, pos, val)
    P.cover(notes, [take], take)


def test_placement():
    # positive overlap: the second note starts before the first ends
    s = P.place([500.0, 500.0, 250.0], [0.0, 30.0, 0.0], SR)
    assert s.dtype == np.int64
    assert s.tolist() == [0, P.samples(470.0, SR), P.samples(970.0, SR)]
    # negative overlap: a gap
    s = P.place([500.0, 500.0], [0.0, -12.5], SR)
    assert s.tolist() == [0, P.samples(512.5, SR)]
    # a first overlap puts start_0 below 0
    s = P.place([500.0, 100.0], [20.0, 10.0], SR)
    assert s.tolist() == [-882, P.samples(470.0, SR)]
    # rounding is floor(x + 0.5) of the float64 position, negative ones included
    assert P.place([10.0], [0.0113378684807], SR).tolist() == [int(np.floor(-0.0113378684807 * SR / 1000 + 0.5))]


def _note(start, skip, take, knots=None, vals=None):
    r = np.zeros((), dtype=_lib.PHRASE_NOTE)
    r["start"], r["skip"], r["take"] = start, skip, take
    r["pos"] = np.linspace(0, take, 7).astype(np.float32) if knots is None else knots
    r["pos"][6] = np.float32(take)
    r["val"] = [0, 1, 1, 1, 1, 1, 0] if vals is None else vals
    return r


def _check_cover(notes, lens, total_out):
    notes = np.array(notes, dtype=_lib.PHRASE_NOTE)
    off, lst = P.cover(notes, lens, total_out)
    woff, wlst = R.cover(notes, lens, total_out)
    assert np.array_equal(off, woff) and np.array_equal(lst, wlst)
    assert off.dtype == np.int64 and lst.dtype == np.int32
    return off, lst


def test_cover_one_long_note_spanning_five_short_ones():
    notes = [_note(100, 0, 10000)] + [_note(700 + 1800 * k, 0, 300 + 150 * k) for k in range(5)]
    off, lst = _check_cover(notes, [10000] + [900] * 5, 10100)
    assert len(off) == 6 and lst[0] == 0                       # ascending note index inside every tile
    for t in range(5):
        assert np.all(np.diff(lst[off[t]:off[t + 1]]) > 0)


def test_cover_rest_longer_than_a_tile_and_notes_ending_on_tile_edges():
    # note 0 ends exactly at 2048, note 1 starts at 2048 + 5000 (a rest of 5000 samples) and ends exactly at 4 * 2048
    notes = [_note(0, 0, 2048), _note(7048, 0, 8192 - 7048), _note(4096, 10, 2048)]
    off, lst = _check_cover(notes, [2048, 5000, 2058], 8192)
    assert off.tolist() == [0, 1, 1, 2, 3] and lst.tolist() == [0, 2, 1]      # tile 1 is empty; note 2 ends on the edge 6144, note 1 on 8192
    # the same with the track cut inside a tile, and with a start below 0 ending exactly on the first edge
    _check_cover(notes, [2048, 5000, 2058], 7100)
    _check_cover([_note(-100, 0, 2148)], [3000], 5000)


def test_cover_skips_notes_without_an_effective_range():
    notes = [_note(10, 500, 400), _note(20, 0, 0), _note(30, 0, 100), _note(-500, 0, 500), _note(6000, 0, 50), _note(40, 100, 300)]
    lens = [500, 100, 0, 500, 50, 250]                         # skip >= len, take 0, len 0, ends at 0, starts at total_out; the last one plays
    off, lst = _check_cover(notes, lens, 6000)
    assert lst.tolist() == [5]
    # starts at the ends of int64 do not overflow
    _check_cover([_note(2 ** 63 - 1, 0, 100), _note(-2 ** 63, 0, 100), _note(5, 0, 100)], [100, 100, 100], 4096)


def test_planner_against_brute_force():
    """The twin of test_bus_plan.test_planner_against_brute_force: seeded random records, starts in front of the track included."""
    rng = np.random.default_rng(20261021)
    for trial in range(40):
        n = int(rng.integers(0, 9))
        total = int(rng.choice([0, 1, 2047, 2048, 2049, 5000, 20000]))
        starts = rng.integers(-3000, 12000, n)
        skips = rng.choice([0, 1, 500], n)
        takes = rng.choice([0, 1, 7, 2048, 3000, 9000], n)
        lens = rng.choice([0, 1, 7, 2048, 3000, 9000], n)
        if trial % 5 == 0 and n:
            starts[0], skips[0], takes[0], lens[0] = 2048, 0, 2048, 2048     # exactly tile 1
        off, lst = _check_cover([_note(int(s), int(k), int(t)) for s, k, t in zip(starts, skips, takes)], lens, total)
        for t in range(len(off) - 1):
            assert list(lst[off[t]:off[t + 1]]) == sorted(lst[off[t]:off[t + 1]])


def test_cover_capacity_protocol():
    lib = _lib.load()
    notes = np.array([_note(0, 0, 5000), _note(1000, 0, 3000)], dtype=_lib.PHRASE_NOTE)
    lens = np.array([5000, 3000], dtype=np.int64)
    off = np.zeros(4, dtype=np.int64)
    lst = np.full(5, -7, dtype=np.int32)
    need = C.c_int64(-1)
    args = (notes.ctypes.data, lens.ctypes.data, 2, 5000, off.ctypes.data)
    assert lib.goofer_host_phrase_plan(*args, lst.ctypes.data, 4, C.byref(need)) == 1
    assert need.value == 5 and np.all(lst == -7)               # too small: the count only
    assert lib.goofer_host_phrase_plan(*args, None, 0, C.byref(need)) == 1 and need.value == 5
    assert lib.goofer_host_phrase_plan(*args, lst.ctypes.data, 5, C.byref(need)) == 0
    assert off.tolist() == [0, 2, 4, 5] and lst.tolist() == [0, 1, 0, 1, 0]
    # an empty track: one offset, no entry
    assert lib.goofer_host_phrase_plan(notes.ctypes.data, lens.ctypes.data, 2, 0, off.ctypes.data, None, 0, C.byref(need)) == 0
    assert need.value == 0 and off[0] == 0


@pytest.mark.parametrize("what", ["decreasing", "nan_pos", "inf_val", "pos0", "pos6", "take_neg", "take_big", "skip_neg", "len_neg",
                                  "total_neg"])
def test_plan_refuses(what):
    r = _note(0, 0, 1000)
    lens, total = [1000], 1000
    if what == "decreasing":
        r["pos"][3] = r["pos"][2] - 1
    elif what == "nan_pos":
        r["pos"][2] = np.nan
    elif what == "inf_val":
        r["val"][4] = np.inf
    elif what == "pos0":
        r["pos"][0] = 1.0
    elif what == "pos6":
        r["pos"][6] = 999.0
    elif what == "take_neg":
        r["take"] = -1
        r["pos"][:] = 0
        r["pos"][6] = -1.0
    elif what == "take_big":
        r["take"] = (1 << 24) + 1
        r["pos"][6] = np.float32((1 << 24) + 1)
    elif what == "skip_neg":
        r["skip"] = -1
    elif what == "len_neg":
        lens = [-1]
    elif what == "total_neg":
        total = -1
    with pytest.raises(ValueError):
        P.cover(np.array([r], dtype=_lib.PHRASE_NOTE), lens, total)
    lib = _lib.load()
    notes = np.array([r], dtype=_lib.PHRASE_NOTE)
    ln = np.array(lens, dtype=np.int64)
    off, lst, need = np.zeros(4, dtype=np.int64), np.zeros(8, dtype=np.int32), C.c_int64(0)
    assert lib.goofer_host_phrase_plan(notes.ctypes.data, ln.ctypes.data, 1, total, off.ctypes.data, lst.ctypes.data, 8, C.byref(need)) == -1


def test_plan_takes_the_largest_note():
    r = _note(0, 0, 1 << 24)
    P.cover(np.array([r], dtype=_lib.PHRASE_NOTE), [1 << 24], 4096)


def test_plan_phrase_records_rests_and_track_length():
    entries = ["0 500 5 35 40 0 100 100 0", "R 250", "12.5 240@120 5 35 40 0 100 100 0 30", P.Entry(100.0, rest=True)]
    plan = P.plan_phrase(entries, [22050 + 300, 12000], SR)
    assert plan.n == 2 and plan.notes.dtype == _lib.PHRASE_NOTE and plan.sr == SR
    assert plan.notes["start"].tolist() == [0, P.samples(500.0 + 250.0 - 30.0, SR)]
    assert plan.notes["skip"].tolist() == [0, P.samples(12.5, SR)]
    assert plan.notes["take"].tolist() == [22050, 11025]
    # the track ends where the last rest ends: the cursor after note 1 is 720 + 250 ms
    assert plan.total_out == P.samples(720.0 + 250.0, SR) + P.samples(100.0, SR)
    woff, wlst = R.cover(plan.notes, plan.note_len, plan.total_out)
    assert np.array_equal(plan.tile_off, woff) and np.array_equal(plan.tile_notes, wlst)
    # the blob is the three tables back to back
    a, b = plan.notes.nbytes, plan.notes.nbytes + plan.tile_off.nbytes
    assert plan.blob[:a].tobytes() == plan.notes.tobytes() and plan.blob[a:b].tobytes() == plan.tile_off.tobytes()
    assert plan.blob[b:b + plan.tile_notes.nbytes].tobytes() == plan.tile_notes.tobytes()
    # explicit starts and track length
    plan2 = P.plan_phrase(entries, [22350, 12000], SR, starts=[-100, 777], total_out=9000)
    assert plan2.notes["start"].tolist() == [-100, 777] and plan2.total_out == 9000
    with pytest.raises(ValueError):
        P.plan_phrase(entries, [22350], SR)
    # nothing but rests: a silent track of their length; nothing at all: an empty one
    assert P.plan_phrase(["R 100", "R 50.5"], [], SR).total_out == P.samples(100.0, SR) + P.samples(50.5, SR) - 0
    assert P.plan_phrase([], [], SR).total_out == 0


def test_binding_record_matches_the_library():
    lib = _lib.load()
    assert _lib.PHRASE_NOTE.itemsize == lib.goofer_sizeof(11) == 72
    assert [_lib.PHRASE_NOTE.fields[k][1] for k in ("start", "skip", "take", "pos", "val")] == [0, 8, 12, 16, 44]
    assert _lib.PHRASE_TILE == R.TILE == 2048


def test_read_job(tmp_path):
    job = tmp_path / "job.txt"
    job.write_text("# a phrase\n"
                   "voice bank/a.wav out/a.wav C4 100 g-5 30 600 80 50 100 0 !120 AA | 0 480@120+20 5 35 40 0 100 100 0 20\n"
                   "\n"
                   "R 240@120\n")
    lines = P.read_job(job)
    assert len(lines) == 2 and lines[1][0] is None and lines[1][1].rest and lines[1][1].length == 250.0
    args, e = lines[0]
    assert len(args) == 13 and args[2:] == ["C4", "100", "g-5", "30", "600", "80", "50", "100", "0", "!120", "AA"]
    assert e.length == 520.0 and e.stp == 0.0 and e.overlap == 20.0 and not e.rest
    job.write_text("a.wav b.wav C4 100 g-5 30 600 80 50 100 0 !120 AA\n")
    with pytest.raises(ValueError, match="job.txt:1"):
        P.read_job(job)
