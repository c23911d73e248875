"""CPU: the batched cold-cache analysis' host logic — the device-pass planner and the files it refuses before any device work."""
import logging
import wave

import numpy as np
import pytest

from goofer_amd import trackers


def _wav(path, y, sr, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
    return path


def test_planner_groups_by_rate_in_input_order_within_budget():
    entries = [("a", 44100, 30), ("b", 48000, 10), ("c", 44100, 50), ("d", 44100, 30), ("e", 48000, 95), ("f", 44100, 1)]
    passes = trackers.plan_passes(entries, frame_budget=100)
    assert passes == [(44100, ["a", "c"]), (44100, ["d", "f"]), (48000, ["b"]), (48000, ["e"])]
    frames = {k: f for k, _, f in entries}
    for _, keys in passes:
        assert sum(frames[k] for k in keys) <= 100


def test_planner_gives_an_oversized_signal_a_pass_of_its_own_and_dedupes():
    entries = [("a", 22050, 5), ("big", 22050, 500), ("b", 22050, 5), ("a", 22050, 5), ("big", 22050, 500)]
    passes = trackers.plan_passes(entries, frame_budget=64)
    assert passes == [(22050, ["a"]), (22050, ["big"]), (22050, ["b"])]
    keys = [k for _, ks in passes for k in ks]
    assert len(keys) == len(set(keys)) == 3
    assert trackers.plan_passes([], 10) == []
    with pytest.raises(ValueError):
        trackers.plan_passes(entries, frame_budget=0)


def test_planner_holds_every_signal_exactly_once_on_random_input():
    rng = np.random.default_rng(7)
    entries = [(f"s{i}", int(rng.choice([22050, 44100, 48000])), int(rng.integers(1, 400))) for i in range(300)]
    passes = trackers.plan_passes(entries, frame_budget=1000)
    by_key = {k: (sr, f) for k, sr, f in entries}
    seen = [k for _, ks in passes for k in ks]
    assert sorted(seen) == sorted(by_key)
    for sr, ks in passes:
        assert all(by_key[k][0] == sr for k in ks)
        assert sum(by_key[k][1] for k in ks) <= 1000
        idx = [int(k[1:]) for k in ks]
        assert idx == sorted(idx)                                 # input order inside a pass


def _alone_error(fn):
    with pytest.raises(Exception) as info:
        fn()
    return info.value


def test_refusals_carry_the_per_file_exception(tmp_path):
    """Too short for the native tracker, a sample rate it does not take, an unreadable and a missing file: each fails up front,
    before any device work, with the type and message the tracker or ensure_features on that file alone raises for it."""
    short = _wav(tmp_path / "short.wav", np.zeros(100), 44100)
    slow = _wav(tmp_path / "slow.wav", np.zeros(4000), 4000)
    junk = tmp_path / "junk.wav"
    junk.write_bytes(b"this is not a wav file at all")
    missing = tmp_path / "missing.wav"
    got = trackers.ensure_features_batch([short, slow, junk, missing, short], tracker="native")
    assert list(got) == [short, slow, junk, missing]
    expect = {
        short: _alone_error(lambda: trackers.native_tracker(np.zeros(100), 44100, 256, 1)),
        slow: _alone_error(lambda: trackers.native_tracker(np.zeros(4000), 4000, 256, 16)),
        junk: _alone_error(lambda: trackers.ensure_features(junk, tracker="native")),
        missing: _alone_error(lambda: trackers.ensure_features(missing, tracker="native")),
    }
    for path, err in expect.items():
        assert type(got[path]) is type(err) and str(got[path]) == str(err), path
    assert not list(tmp_path.glob("*.goofy")) and not list(tmp_path.glob("*.tmp*"))


def test_existing_cache_is_returned_untouched(tmp_path):
    wav = _wav(tmp_path / "a.wav", np.zeros(44100), 44100)
    feat = trackers.features_path(wav)
    feat.write_bytes(b"old")
    before = feat.stat().st_mtime_ns
    got = trackers.ensure_features_batch([wav], tracker="native")
    assert got == {wav: feat} and feat.read_bytes() == b"old" and feat.stat().st_mtime_ns == before


def test_folder_mode_tallies_refused_files(tmp_path, caplog):
    _wav(tmp_path / "short.wav", np.zeros(10), 44100)
    (tmp_path / "junk.wav").write_bytes(b"RIFF....")
    _wav(tmp_path / "done.wav", np.zeros(10), 44100)
    trackers.features_path(tmp_path / "done.wav").write_bytes(b"old")
    with caplog.at_level(logging.INFO):
        tally = trackers.extract_folder(tmp_path, tracker="native")
    assert tally == {"extracted": 0, "skipped": 1, "failed": 2}
    text = caplog.text
    assert "[SKIP] done_features.goofy already exists" in text
    assert text.count("[EXTRACT]") == 2 and text.count("[ERROR] Failed to extract") == 2
    assert "[DONE] Extracted features from 3 files." in text


def test_pool_size_is_a_fixed_default():
    assert trackers.WORKERS == 8 and trackers.FRAME_BUDGET >= 1 << 12
