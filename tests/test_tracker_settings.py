"""CPU: the native tracker's settings — the ``native:key=value`` names, every validation bound, the minimum length and its
refusal, and the library's frame layout under settings against the numpy restatement at the same settings."""
import numpy as np
import pytest

import tracker_cases as C
import tracker_settings_ref as S
from goofer_amd import trackers
from goofer_amd.trackers import TrackerSettings


def test_defaults_match_the_restatement_and_the_library():
    import ctypes
    from goofer_amd import _lib
    d = TrackerSettings()
    assert {k: getattr(d, k) for k in S.FIELDS} == S.DEFAULTS
    st = _lib.TrackSettings()
    lib = _lib.load()
    lib.goofer_track_settings_default(ctypes.byref(st))
    assert [getattr(st, k) for k, _ in _lib.TrackSettings._fields_] == [S.DEFAULTS[k] for k in S.FIELDS]
    assert ctypes.sizeof(_lib.TrackSettings) == lib.goofer_sizeof(10)


def test_native_names_parse_into_bound_trackers(monkeypatch):
    t = trackers.get("native:pitch_floor=40,pitch_ceiling=1200,max_formant=5000")
    assert isinstance(t, trackers.NativeTracker)
    assert t.settings == TrackerSettings(pitch_floor=40, pitch_ceiling=1200.0, max_formant=5000)
    assert isinstance(t.settings.pitch_floor, int) and isinstance(t.settings.max_formant, int)
    assert trackers.native_settings(t) == (True, t.settings)
    assert trackers.native_settings(trackers.native_tracker) == (True, None)
    assert trackers.native_settings(trackers.praat_tracker) == (False, None)
    assert trackers.get("native") is trackers.native_tracker is trackers.native(None)
    assert trackers.get(" native: n_formants = 4 , voicing_threshold=0.6".strip()).settings == TrackerSettings(n_formants=4, voicing_threshold=0.6)
    monkeypatch.setenv("GOOFER_TRACKER", "native:pitch_floor=40")
    assert trackers.get().settings == TrackerSettings(pitch_floor=40)
    assert trackers.get(t) is t


@pytest.mark.parametrize("name", ("native:", "native:pitch_floor", "native:floor=40", "native:pitch_floor=forty", "native:pitch_floor=40,,",
                                  "native:pitch_floor=40,pitch_floor=50", "native:pitch_floor=40.5", "native:n_formants=6"))
def test_bad_native_names_are_value_errors(name):
    with pytest.raises(ValueError):
        trackers.get(name)


BAD = (("pitch_floor", 19), ("pitch_floor", 601), ("pitch_floor", 75.5), ("pitch_ceiling", 75.0), ("pitch_ceiling", 20000.5),
       ("pitch_ceiling", float("nan")), ("silence_threshold", -0.01), ("silence_threshold", float("inf")), ("voicing_threshold", 0.0),
       ("voicing_threshold", 1.0), ("octave_cost", -1.0), ("octave_cost", float("nan")), ("octave_jump_cost", -1e-9),
       ("octave_jump_cost", float("inf")), ("voiced_unvoiced_cost", -0.14), ("max_formant", 2499), ("max_formant", 8001),
       ("max_formant", 5000.5), ("n_formants", 2), ("n_formants", 6), ("n_formants", "five"), ("pitch_floor", None))
GOOD = (("pitch_floor", 20), ("pitch_floor", 600), ("pitch_ceiling", 20000.0), ("silence_threshold", 0.0), ("voicing_threshold", 1e-9),
        ("voicing_threshold", 1 - 1e-9), ("octave_cost", 0.0), ("octave_jump_cost", 0.0), ("voiced_unvoiced_cost", 0.0),
        ("max_formant", 2500), ("max_formant", 8000), ("n_formants", 3), ("n_formants", 4), ("pitch_floor", 40.0))


@pytest.mark.parametrize("field,value", BAD)
def test_every_bound_refuses_naming_the_field(field, value):
    with pytest.raises(ValueError, match=field):
        TrackerSettings(**({"pitch_ceiling": 950.0, field: value} if field != "pitch_floor" else {"pitch_ceiling": 20000.0, field: value}))


def test_the_bounds_themselves_are_admitted_and_the_library_agrees():
    from goofer_amd.device import GooferError, track_frame_offsets
    for field, value in GOOD:
        s = TrackerSettings(**{"pitch_ceiling": 20000.0 if field == "pitch_floor" else 950.0, field: value})
        track_frame_offsets([48000], 48000, 256, s)                            # goofer_track_layout validates as _configure does

    class Raw:                                                                 # past the dataclass, to the library's own check
        pass
    for field, value in BAD:
        if isinstance(value, (str, type(None))) or (field in ("pitch_floor", "max_formant") and value != int(value)):
            continue
        r = Raw()
        for k, v in S.DEFAULTS.items():
            setattr(r, k, v)
        setattr(r, field, value)
        with pytest.raises(GooferError):
            track_frame_offsets([48000], 48000, 256, r)
    with pytest.raises(ValueError, match="pitch_ceiling"):
        TrackerSettings(pitch_floor=600, pitch_ceiling=600.0)
    with pytest.raises(dataclasses_error()):
        TrackerSettings().pitch_floor = 40                                     # frozen


def dataclasses_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


@pytest.mark.parametrize("floor", (20, 40, 150))
def test_min_length_and_refusal_follow_the_floor(floor):
    s = TrackerSettings(pitch_floor=floor, pitch_ceiling=950.0)
    M = S.load(s)
    for sr in C.RATES:
        n = trackers.native_min_length(sr, s)
        assert n == M.min_length(sr) == -(-3 * sr // floor)
        assert trackers.native_refusal(n, sr, s) is None
        e = trackers.native_refusal(n - 1, sr, s)
        assert isinstance(e, ValueError) and f"{n} samples" in str(e) and f"({3000 / floor:g} ms)" in str(e)
    assert trackers.native_min_length(44100) == 1764 and "(40 ms)" in str(trackers.native_refusal(10, 44100))
    assert "outside" in str(trackers.native_refusal(10 ** 6, 7999, s))


def test_a_tenth_of_a_second_at_96k_is_short_of_the_floor_20_window():
    e = trackers.native_refusal(9600, 96000, TrackerSettings(pitch_floor=20))
    assert isinstance(e, ValueError) and "14400" in str(e)
    with pytest.raises(ValueError, match="14400"):                             # before any device is asked for
        trackers.native_tracker(np.zeros(9600), 96000, 512, 10, settings=TrackerSettings(pitch_floor=20))
    with pytest.raises(ValueError, match="14400"):
        trackers.native(TrackerSettings(pitch_floor=20))(np.zeros(9600), 96000, 512, 10)


@pytest.mark.parametrize("settings", [st for st, *_ in S.SETTINGS] + [{}], ids=lambda s: ",".join(f"{k}={v:g}" for k, v in s.items()) or "defaults")
def test_frame_offsets_match_the_restatement(settings):
    from goofer_amd.device import GooferError, track_frame_offsets
    s = TrackerSettings(**settings)
    M = S.load(s)
    for sr in C.RATES:
        for hop in C.HOPS[sr]:
            n0, nw = M.min_length(sr), -(-M.FORMANT_WIN * sr // M.FORMANT_SR)
            lengths = sorted({n0, n0 + 1, n0 + hop - 1, n0 + hop, max(n0, nw - 1), max(n0, nw), max(n0, nw) + hop, int(0.37 * sr), sr + 17})
            p_off, f_off = track_frame_offsets(lengths, sr, hop, s if settings else None)
            assert np.diff(p_off).tolist() == [M.pitch_frames(n, sr, hop) for n in lengths], (sr, hop)
            assert np.diff(f_off).tolist() == [M.formant_frames(n, sr, hop) for n in lengths], (sr, hop)
            with pytest.raises(GooferError):
                track_frame_offsets([n0 - 1], sr, hop, s)


def test_the_helpers_long_window_correlate_is_numpys():
    """The lag-by-lag sums the helper uses above LONG_WINDOW samples against numpy's correlate, where numpy's is quick."""
    rng = np.random.default_rng(3)
    for W in (160, 1200, 7200):
        x = rng.standard_normal(W) * np.hanning(W)
        assert np.array_equal(S.long_correlate(x, x, "full")[W - 1:], np.correlate(x, x, mode="full")[W - 1:])
    M = S.load({"pitch_floor": 20})
    assert M.np.correlate is not np.correlate and M.np.pi == np.pi
    assert np.array_equal(M.np.correlate(x, x, mode="full"), np.correlate(x, x, mode="full"))
