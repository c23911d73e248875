"""CPU: the native f0 / formant tracker's registration, frame layout and input checks, and its algorithm (the numpy
restatement in tracker_ref.py) against ground-truth signals (tracker_truth.py)."""
import numpy as np
import pytest

import tracker_ref as R
import tracker_truth as T

from goofer_amd import trackers

RATES = (22050, 44100, 48000, 96000)
HOP = 256


def test_native_is_registered_and_selectable(monkeypatch):
    assert trackers.get("native") is trackers.native_tracker
    monkeypatch.setenv("GOOFER_TRACKER", "native")
    assert trackers.get() is trackers.native_tracker


def test_native_is_not_the_default(monkeypatch):
    monkeypatch.delenv("GOOFER_TRACKER", raising=False)
    try:
        import parselmouth  # noqa: F401
    except ImportError:
        with pytest.raises(trackers.TrackerUnavailable):
            trackers.get()


@pytest.mark.parametrize("sr", RATES)
def test_frame_layout(sr):
    """floor((dur - 40 ms) / dt) + 1 pitch frames and floor((dur' - 50 ms) / dt) + 1 formant frames, from the library's own
    geometry, the restatement's and the plain float formula."""
    from goofer_amd.device import track_frame_offsets
    win = R.min_length(sr)
    lengths = [win, win + 1, win + HOP - 1, win + HOP, sr, 3 * sr + 17, 6000 * sr // 11000, 6000 * sr // 11000 - 1]
    p_off, f_off = track_frame_offsets(lengths, sr, HOP)
    dt = HOP / sr
    for k, n in enumerate(lengths):
        np_ = int(np.floor((n / sr - 0.04) / dt + 1e-9)) + 1
        assert p_off[k + 1] - p_off[k] == R.pitch_frames(n, sr, HOP) == np_, (n, np_)
        m = n * 11000 // sr
        nf = 0 if m < 550 else int(np.floor((m / 11000 - 0.05) / dt + 1e-9)) + 1
        assert f_off[k + 1] - f_off[k] == R.formant_frames(n, sr, HOP) == nf, (n, nf)
    starts = R.pitch_starts(sr, sr, HOP)                       # centred: equal margins to within a sample
    head, tail = starts[0], sr - (starts[-1] + R.pitch_window(sr))
    assert abs(head - tail) <= 1


def test_short_signal_is_refused_with_the_minimum_length():
    sr = 44100
    n = R.min_length(sr)
    with pytest.raises(ValueError, match=str(n)):
        trackers.native_tracker(np.zeros(n - 1), sr, HOP, 10)
    with pytest.raises(ValueError, match=str(n)):
        R.track_pitch(np.zeros(n - 1), sr, HOP)
    from goofer_amd.device import GooferError, track_frame_offsets
    with pytest.raises(GooferError):
        track_frame_offsets([n - 1], sr, HOP)
    assert track_frame_offsets([n], sr, HOP)[0][-1] == 1


@pytest.mark.parametrize("sr", RATES)
def test_restatement_meets_ground_truth(sr):
    y, f0, kind = T.synth(sr)
    s = T.score(R.track_pitch(y, sr, HOP), R.track_formants(y, sr, HOP), f0, kind, sr, HOP)
    T.assert_meets_bars(s)


def test_restatement_edge_cases():
    sr = 22050
    n = R.min_length(sr)
    t = np.arange(sr // 2) / sr
    cases = {
        "zeros": np.zeros(sr // 2),
        "dc": np.full(sr // 2, 0.3),
        "square": np.clip(4.0 * np.sign(np.sin(2 * np.pi * 150 * t)), -1, 1),
        "one_window": T.synth(sr)[0][sr // 4:sr // 4 + n],
    }
    for name, y in cases.items():
        f0, forms = R.track(y, sr, HOP)
        assert np.isfinite(f0).all() and np.isfinite(forms).all(), name
        if name in ("zeros", "dc"):
            assert not f0.any(), name
    assert not R.track_formants(cases["zeros"], sr, HOP).any()
    f0, _ = R.track(cases["square"], sr, HOP)
    assert np.all(np.abs(f0[2:-2] / 150.0 - 1.0) < 0.01)
