"""GPU: the native tracker at other settings than the defaults (goofer_track_configure, trackers.TrackerSettings) against
the numpy restatement at the same settings (tracker_settings_ref.py), stage by stage as test_gpu_tracker_oracle.py does it —
candidates, the path on the GPU's candidates, the resampled signal, formant frames on the GPU's resampled signal, the
compositions — then defaults and handle state, what a user gets through core.extract_features, the batched paths and the
refusals.  Bounds are that file's (1e-9, 1e-9, 1e-9, 1e-12, 1e-6), the first three times max(1, W / 3840) for a pitch
window of W samples.

At the floor 20 Hz row (96 kHz, a 14400-sample window) the restatement's autocorrelation is summed lag by lag by the helper
(tracker_settings_ref._Numpy): numpy's correlate needs more than a minute per call at that length.

Measured worst on the MI355X, divided by that scale where it applies (bound in brackets): candidate frequencies 5.5e-14
relative (1e-9); candidate and unvoiced strengths 7.2e-15 absolute (1e-9); f0 of unflagged signals 1.4e-14 relative (1e-9);
the resampled signal 1.4e-15 x the signal's peak (1e-12); formants 3.3e-8 relative (1e-6).  Unflagged by the restatement
alone: 1124 of 1124 pitch frames, 1165 of 1177 formant frames, 43 of 45 signals.
"""
import numpy as np
import pytest

import tracker_cases as C
import tracker_settings_ref as S

pytestmark = pytest.mark.gpu

F_REL, S_ABS, F0_REL, X11_REL, FORM_REL = 1e-9, 1e-9, 1e-9, 1e-12, 1e-6
RESTATED = list(S.SETTINGS)
WORST = {}


def _worst(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def _settings(d):
    from goofer_amd.trackers import TrackerSettings
    return TrackerSettings(**d)


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()
    print("\ntracker settings worst:", {k: f"{v:.2e}" for k, v in sorted(WORST.items())})


def _dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(ctx.device)


@pytest.fixture(scope="module")
def ref():
    cases = [(st, sr, hop, name, y) for st, sr, hop, dur in RESTATED for name, y in S.signals(st, sr, hop, dur).items()]
    return cases, [S.restate(c) for c in cases]


@pytest.fixture(scope="module")
def gpu(ctx, ref):
    """Per case the GPU's stages, each settings row as ragged batches: the pitch stages over the signals of a pitch window or
    more, the formant stages over all."""
    cases, _ = ref
    out = [dict() for _ in cases]
    for row in RESTATED:
        st, sr, hop, _ = row
        s, M = _settings(st), S.load(st)
        idx = [k for k, c in enumerate(cases) if c[0] is st and c[1] == sr and c[2] == hop]
        allx = [cases[k][4] for k in idx]
        x11, x_off = ctx.track_resample(_dev(ctx, np.concatenate(allx)), [len(y) for y in allx], sr, settings=s)
        forms, m_off = ctx.track_formant_frames(x11, np.diff(x_off), sr, hop, settings=s)
        x11, forms = x11.cpu().numpy(), forms.cpu().numpy()
        for j, k in enumerate(idx):
            out[k].update(x11=x11[x_off[j]:x_off[j + 1]], forms_stage=forms[m_off[j]:m_off[j + 1]])
        pidx = [k for k in idx if len(cases[k][4]) >= M.min_length(sr)]
        ys = [cases[k][4] for k in pidx]
        lengths = [len(y) for y in ys]
        y = _dev(ctx, np.concatenate(ys))
        cf, cs, cn, p_off = ctx.track_candidates(y, lengths, sr, hop, settings=s)
        f0_path = ctx.track_path(cf, cs, cn, p_off, sr, hop, settings=s).cpu().numpy()
        f0, p_off2, forms2, m_off2 = ctx.track(y, lengths, sr, hop, settings=s)
        assert np.array_equal(p_off, p_off2)
        cf, cs, cn, f0, forms2 = cf.cpu().numpy(), cs.cpu().numpy(), cn.cpu().numpy(), f0.cpu().numpy(), forms2.cpu().numpy()
        for j, k in enumerate(pidx):
            a, b = p_off[j], p_off[j + 1]
            out[k].update(cf=cf[a:b], cs=cs[a:b], cn=cn[a:b], f0_path=f0_path[a:b], f0=f0[a:b], forms=forms2[m_off2[j]:m_off2[j + 1]])
    return out


def _scale(st, sr):
    return max(1.0, (3 * sr // S.as_dict(st)["pitch_floor"]) / 3840.0)


def test_compositions_equal_their_stages(gpu):
    for g in gpu:
        if "f0" in g:
            assert np.array_equal(g["f0"], g["f0_path"])
            assert np.array_equal(g["forms"], g["forms_stage"])


def test_candidates_match_restatement(ref, gpu):
    cases, refs = ref
    n_frames = n_unflagged = 0
    for (st, sr, hop, name, _), r, g in zip(cases, refs, gpu):
        if not r["pitch"]:
            continue
        k = _scale(st, sr)
        assert len(g["cn"]) == len(r["cands"]), (st, sr, name)
        for i, (f, s) in enumerate(r["cands"]):
            n_frames += 1
            if r["cand_fragile"][i]:
                continue
            n_unflagged += 1
            n = g["cn"][i]
            assert n == len(f), (st, sr, name, i, n, len(f))
            gf, gs = g["cf"][i, :n], g["cs"][i, :n]
            assert gf[0] == 0.0
            if n > 1:
                _worst("cand_f_rel / scale", np.max(np.abs(gf[1:] / f[1:] - 1.0)) / k)
            _worst("cand_s_abs / scale", np.max(np.abs(gs - s)) / k)
            assert np.all(np.abs(gf[1:] - f[1:]) <= k * F_REL * f[1:]), (st, sr, name, i)
            assert np.all(np.abs(gs - s) <= k * S_ABS), (st, sr, name, i)
    assert n_unflagged >= 0.95 * n_frames, (n_unflagged, n_frames)


def test_path_on_gpu_candidates_matches_restatement(ref, gpu):
    cases, refs = ref
    for (st, sr, hop, name, _), r, g in zip(cases, refs, gpu):
        if not r["pitch"]:
            continue
        cands = [(g["cf"][i, :g["cn"][i]].copy(), g["cs"][i, :g["cn"][i]].copy()) for i in range(len(g["cn"]))]
        f0, _, fragile = S.load(st).viterbi_diag(cands, 0.01 * sr / hop)
        assert np.array_equal(g["f0_path"][~fragile], f0[~fragile]), (st, sr, name)


def test_resample_matches_restatement(ref, gpu):
    cases, refs = ref
    for (st, sr, hop, name, y), r, g in zip(cases, refs, gpu):
        assert g["x11"].shape == r["x11"].shape, (st, sr, name)
        peak = np.abs(y).max()
        _worst("x11_rel_peak", np.max(np.abs(g["x11"] - r["x11"])) / peak)
        assert np.all(np.abs(g["x11"] - r["x11"]) <= X11_REL * peak), (st, sr, name)


def _close_formants(got, want, n):
    assert got.shape == (len(want), 5) and not got[:, n:].any()
    got = got[:, :n]
    assert np.array_equal(got == 0, want == 0)
    on = want != 0
    if on.any():
        err = np.max(np.abs(got[on] / want[on] - 1.0))
        _worst("formant_rel", err)
        assert err <= FORM_REL, err


def test_formant_frames_on_gpu_resample_match_restatement(ref, gpu):
    cases, _ = ref
    n_frames = n_unflagged = 0
    for (st, sr, hop, name, _), g in zip(cases, gpu):
        M = S.load(st)
        forms, fragile = M.formants_of_11k(g["x11"], sr, hop)
        assert len(g["forms_stage"]) == len(forms), (st, sr, name)
        n_frames += len(fragile)
        n_unflagged += int((~fragile).sum())
        _close_formants(g["forms_stage"][~fragile], forms[~fragile], M.N_FORMANTS)
    assert n_unflagged >= 0.95 * n_frames, (n_unflagged, n_frames)


def test_end_to_end_matches_restatement(ref, gpu):
    cases, refs = ref
    unflagged = total = 0
    for (st, sr, hop, name, _), r, g in zip(cases, refs, gpu):
        if not r["pitch"]:
            continue
        total += 1
        if r["cand_fragile"].any() or r["path_fragile"].any() or r["formant_fragile"].any():
            continue
        unflagged += 1
        rf0, k = r["f0"], _scale(st, sr)
        assert np.array_equal(g["f0"] > 0, rf0 > 0), (st, sr, name)
        v = rf0 > 0
        if v.any():
            _worst("f0_rel / scale", np.max(np.abs(g["f0"][v] / rf0[v] - 1.0)) / k)
        assert np.all(np.abs(g["f0"][v] - rf0[v]) <= k * F0_REL * rf0[v]), (st, sr, name)
        _close_formants(g["forms"], r["formants"], S.load(st).N_FORMANTS)
    assert unflagged >= 0.9 * total, (unflagged, total)


def _tracks(ctx, ys, sr, hop, settings):
    f0, p_off, forms, f_off = ctx.track(_dev(ctx, np.concatenate(ys)), [len(y) for y in ys], sr, hop, settings=settings)
    f0, forms = f0.cpu().numpy(), forms.cpu().numpy()
    return [(f0[p_off[k]:p_off[k + 1]], forms[f_off[k]:f_off[k + 1]]) for k in range(len(ys))]


def test_floor_20_at_96k_launches_and_tracks_30_hz(ctx):
    sr, hop, s = 96000, 512, _settings({"pitch_floor": 20})
    sig = S.signals({"pitch_floor": 20}, sr, hop, 0.3)
    low = C.harmonic(sr, np.full(int(0.3 * sr), 30.0), 5)
    ys = [sig["voice"], low, sig["len_min"], sig["glide"]]
    batch = _tracks(ctx, ys, sr, hop, s)
    M = S.load({"pitch_floor": 20})
    for k, y in enumerate(ys):
        (one,) = _tracks(ctx, [y], sr, hop, s)
        assert len(one[0]) == M.pitch_frames(len(y), sr, hop) and len(one[1]) == M.formant_frames(len(y), sr, hop)
        assert np.array_equal(one[0], batch[k][0]) and np.array_equal(one[1], batch[k][1]), k
    y = _dev(ctx, low)
    cf, cs, cn, off = ctx.track_candidates(y, [len(low)], sr, hop, settings=s)
    assert np.array_equal(ctx.track_path(cf, cs, cn, off, sr, hop, settings=s).cpu().numpy(), batch[1][0])
    assert np.all(np.abs(batch[1][0] - 30.0) <= 0.005 * 30.0)


# -- defaults and state ---------------------------------------------------------------------------------------------
def test_default_settings_equal_no_settings_and_state_does_not_leak(ctx):
    from goofer_amd.device import Context
    from goofer_amd.trackers import TrackerSettings
    sr, hop = 16000, 128
    ys = [C.voice(sr, 0.4, 3), C.harmonic(sr, np.full(6000, 55.0), 2), C.voice(sr, 0.3, 4)[:1300]]
    s40 = TrackerSettings(pitch_floor=40, max_formant=5000)
    first = _tracks(ctx, ys, sr, hop, s40)
    none = _tracks(ctx, ys, sr, hop, None)
    third = _tracks(ctx, ys, sr, hop, s40)
    explicit = _tracks(ctx, ys, sr, hop, TrackerSettings())
    fresh = Context(0)
    try:
        want = _tracks(fresh, ys, sr, hop, None)
    finally:
        fresh.close()
    for k in range(len(ys)):
        for a, b in ((first, third), (none, want), (explicit, none)):
            assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), k
    assert not np.array_equal(first[1][0], none[1][0])


# -- what the user gets ---------------------------------------------------------------------------------------------
def test_low_and_high_voices_through_extract_features(ctx):
    from goofer_amd import core
    sr, hop = 16000, 128
    n = int(0.4 * sr)
    low = C.harmonic(sr, np.full(n, 55.0), 1)
    high = 0.5 * np.sin(2 * np.pi * 1200.0 * np.arange(n) / sr)

    def feats(y, tracker):
        _, f0, mask, _, _ = core.extract_features(y, sr, 1024, hop, pitch_tracker=tracker, ctx=ctx)
        return np.asarray(f0), np.asarray(mask)
    f0, mask = feats(low, "native")
    assert not mask.any()
    f0, mask = feats(low, "native:pitch_floor=40")
    assert mask.all() and np.all(np.abs(f0 - 55.0) <= 0.005 * 55.0)
    f0, mask = feats(high, "native")
    assert np.all(f0[mask > 0] < 600.0)
    f0, mask = feats(high, "native:pitch_ceiling=1500")
    assert mask.all() and np.all(np.abs(f0 - 1200.0) <= 0.005 * 1200.0)


# -- batched paths --------------------------------------------------------------------------------------------------
NAME = "native:pitch_floor=40,max_formant=5000"


def _ragged(sr):
    return [C.voice(sr, 0.4, 1), C.harmonic(sr, np.full(int(0.31 * sr), 55.0), 2), C.voice(sr, 0.25, 3), C.voice(sr, 0.4, 4)[:1201],
            0.3 * np.sin(2 * np.pi * 440.0 * np.arange(int(0.2 * sr)) / sr), C.voice(sr, 0.33, 5)]


def test_analyse_batch_equals_single_calls_with_one_track_call(ctx, monkeypatch):
    from goofer_amd import trackers
    from goofer_amd.device import Context
    sr, hop = 16000, 128
    ys = _ragged(sr)
    s = trackers.get(NAME).settings
    calls = []
    real = Context.track

    def counted(self, *a, **kw):
        calls.append(kw.get("settings"))
        return real(self, *a, **kw)
    monkeypatch.setattr(Context, "track", counted)
    res = trackers.analyse_batch(ys, sr, 1024, hop, tracker=NAME, ctx=ctx, want_env=False)
    assert calls == [s]
    monkeypatch.setattr(Context, "track", real)
    fifth = False                                                              # max_formant alone leaves five formants
    for y, r in zip(ys, res):
        _, f0, mask, forms, _ = r
        T = 1 + len(y) // hop
        f0_track, forms_one = trackers.native_tracker(y, sr, hop, T, ctx=ctx, settings=s)
        want_f0, want_mask = trackers.per_sample_f0(f0_track, len(y), sr, f0_min=40)   # f0_min follows a lower floor
        assert np.array_equal(f0, want_f0) and np.array_equal(mask, want_mask)
        assert forms == forms_one
        fifth = fifth or any(forms[5])
    assert fifth
    short = trackers.analyse_batch([ys[0][:1199], ys[0]], sr, 1024, hop, tracker=NAME, ctx=ctx, want_env=False)
    assert isinstance(short[0], ValueError) and "1200 samples" in str(short[0]) and not isinstance(short[1], BaseException)


def test_ensure_features_batch_writes_caches_with_those_tracks(ctx, tmp_path):
    import wave
    from goofer_amd import core, trackers
    sr, hop = 16000, 128
    ys = _ragged(sr)[:3]
    paths = []
    for k, y in enumerate(ys):
        p = tmp_path / f"s{k}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
            w.writeframes((np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
        paths.append(p)
    out = trackers.ensure_features_batch(paths, 1024, hop, tracker=NAME, ctx=ctx)
    for p in paths:
        assert not isinstance(out[p], BaseException), out[p]
        y, _ = trackers.read_audio(p)
        (want,) = trackers.analyse_batch([y], sr, 1024, hop, tracker=NAME, ctx=ctx, want_env=False)
        got = core.load_features(out[p])
        f0, mask, forms = got[1], got[2], got[3]
        assert np.array_equal(np.asarray(f0), np.asarray(want[1]).astype(np.float16).astype(np.asarray(f0).dtype))
        assert np.array_equal(np.asarray(mask) > 0, np.asarray(want[2]) > 0)
        assert len(forms) >= 4                                                 # the cache keeps the formants the synthesis reads
        assert {int(k): list(map(float, v)) for k, v in forms.items()} == {int(k): list(map(float, want[3][int(k)])) for k in forms}
    assert np.asarray(core.load_features(out[paths[1]])[2]).all()              # the 55 Hz harmonic is voiced under floor 40


# -- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(ctx):
    import ctypes
    from goofer_amd import _lib, trackers
    from goofer_amd.device import GooferError
    with pytest.raises(ValueError, match="14400"):
        trackers.native_tracker(np.zeros(9600), 96000, 512, 10, ctx=ctx, settings=_settings({"pitch_floor": 20}))
    with pytest.raises(GooferError, match="14400"):
        ctx.track(_dev(ctx, np.zeros(9600)), [9600], 96000, 512, settings=_settings({"pitch_floor": 20}))
    for field, value in (("pitch_floor", 10), ("pitch_ceiling", 75.0), ("max_formant", 9000), ("n_formants", 6)):
        st = _lib.TrackSettings()
        ctx.lib.goofer_track_settings_default(ctypes.byref(st))
        setattr(st, field, value)
        assert ctx.lib.goofer_track_configure(ctx.h, ctypes.byref(st)) != 0
        assert field in ctx.lib.goofer_last_error(ctx.h).decode()
    sr, hop, y = 16000, 128, C.voice(16000, 0.3, 2)                            # a refused configure leaves the handle's settings
    assert np.array_equal(_tracks(ctx, [y], sr, hop, None)[0][0], _tracks(ctx, [y], sr, hop, _settings({}))[0][0])
