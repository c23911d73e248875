"""GPU: the native tracker (csrc/tracker.hip) against its numpy restatement frame by frame, against ground truth, batch
against one-signal calls bit for bit, on edge cases, and end to end from a bare wav to a rendered note."""
import os
import wave

import numpy as np
import pytest

import tracker_ref as R
import tracker_truth as T

from goofer_amd import trackers

pytestmark = pytest.mark.gpu

RATES = (22050, 44100, 48000, 96000)
HOP = 256


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _track(ctx, signals, sr):
    import torch
    y = torch.as_tensor(np.concatenate(signals).astype(np.float64)).to(ctx.device)
    f0, p_off, forms, f_off = ctx.track(y, [len(s) for s in signals], sr, HOP)
    f0, forms = f0.cpu().numpy(), forms.cpu().numpy()
    return [(f0[p_off[k]:p_off[k + 1]], forms[f_off[k]:f_off[k + 1]]) for k in range(len(signals))]


def _compare(gpu, ref):
    (gf0, gfm), (rf0, rfm) = gpu, ref
    assert gf0.shape == rf0.shape and gfm.shape == rfm.shape
    assert np.isfinite(gf0).all() and np.isfinite(gfm).all()
    assert np.mean((gf0 > 0) == (rf0 > 0)) >= 0.995
    both = (gf0 > 0) & (rf0 > 0)
    assert np.all(np.abs(gf0[both] / rf0[both] - 1.0) <= 1e-4)
    defined = (gfm > 0) & (rfm > 0)
    assert np.all(np.abs(gfm[defined] - rfm[defined]) <= 0.5)
    assert np.mean((gfm > 0) == (rfm > 0)) >= 0.995


@pytest.mark.parametrize("sr", RATES)
def test_gpu_matches_restatement_and_ground_truth(ctx, sr):
    y, f0, kind = T.synth(sr)
    (got,) = _track(ctx, [y], sr)
    _compare(got, (R.track_pitch(y, sr, HOP), R.track_formants(y, sr, HOP)))
    T.assert_meets_bars(T.score(got[0], got[1], f0, kind, sr, HOP))


def test_batch_equals_single_calls_bit_for_bit(ctx):
    sr = 44100
    y, _, _ = T.synth(sr)
    rng = np.random.default_rng(3)
    signals = [y[:R.min_length(sr)], y[5000:5000 + sr // 3], 0.2 * rng.standard_normal(sr // 5), y, np.zeros(sr // 7),
               y[::-1][:sr // 2 + 77]]
    batch = _track(ctx, signals, sr)
    for k, s in enumerate(signals):
        (one,) = _track(ctx, [s], sr)
        assert np.array_equal(one[0], batch[k][0]) and np.array_equal(one[1], batch[k][1]), k


def test_edge_cases(ctx):
    sr = 22050
    n = R.min_length(sr)
    t = np.arange(sr // 2) / sr
    cases = {
        "zeros": np.zeros(sr // 2),
        "dc": np.full(sr // 2, 0.3),
        "square": np.clip(4.0 * np.sign(np.sin(2 * np.pi * 150 * t)), -1, 1),
        "one_window": T.synth(sr)[0][sr // 4:sr // 4 + n],
    }
    got = dict(zip(cases, _track(ctx, list(cases.values()), sr)))
    for name, (f0, forms) in got.items():
        assert np.isfinite(f0).all() and np.isfinite(forms).all(), name
        assert len(f0) == R.pitch_frames(len(cases[name]), sr, HOP), name
    assert not got["zeros"][0].any() and not got["zeros"][1].any() and not got["dc"][0].any()
    assert len(got["one_window"][0]) == 1
    sq = got["square"][0]
    assert np.all(np.abs(sq[2:-2] / 150.0 - 1.0) < 0.01)
    with pytest.raises(ValueError, match=str(n)):
        trackers.native_tracker(np.zeros(n - 1), sr, HOP, 10, ctx=ctx)
    f0, forms = trackers.native_tracker(cases["one_window"], sr, HOP, 1 + n // HOP, ctx=ctx)
    assert len(f0) == 1 and all(len(v) == 1 + n // HOP for v in forms.values())


def test_bare_wav_to_render_and_folder_mode(tmp_path, monkeypatch):
    from goofer_amd import core
    from goofer_amd import synthetic as syn
    from goofer_amd.device import Context
    from goofer_amd.render import GooferResampler, Renderer
    sr = 44100
    y, _, _ = T.synth(sr)
    bank = tmp_path / "bank"
    bank.mkdir()
    wav = bank / "voice.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
    ctx = Context(0)
    try:
        r = Renderer(ctx)
        req = syn.make_request(2000, "t0g0", length_ms=300)
        a = GooferResampler(str(wav), str(tmp_path / "o1.wav"), *syn.request_args(req), renderer=r, seed=5, tracker="native")
        feat = trackers.features_path(wav)
        assert feat.exists() and not list(bank.glob("*.tmp*"))
        env, f0, mask, forms, sr2, ylen = core.load_features(feat)
        assert sr2 == sr and ylen == len(y) and env["mode"] == "knots" and env["knot_vals_log"].shape[1] == 1 + len(y) // 256
        assert f0.shape == (len(y),) and mask.shape == (len(y),) and 0.3 < mask.mean() < 0.95
        assert all(len(v) == 1 + len(y) // 256 for v in forms.values())
        assert np.isfinite(a.out).all() and np.abs(a.out).max() > 0.01
        monkeypatch.setitem(trackers._REGISTRY, "native", lambda *args: pytest.fail("the cache was not used"))
        b = GooferResampler(str(wav), str(tmp_path / "o2.wav"), *syn.request_args(req), renderer=r, seed=5, tracker="native")
        assert np.array_equal(a.out, b.out)
        monkeypatch.undo()
        os.link(wav, bank / "second.wav")
        tally = trackers.extract_folder(bank, tracker="native", ctx=ctx)
        assert tally == {"extracted": 1, "skipped": 1, "failed": 0} and trackers.features_path(bank / "second.wav").exists()
    finally:
        ctx.close()
