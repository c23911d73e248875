"""GPU: the cold-cache analysis of one signal alone against the same signal inside a many-signal pass, bit for bit —
envelopes and knots (Context.envelope_knots), whole features (core.extract_features_batch), folder mode and the HTTP
collector — and what the single-signal calls refuse."""
import shutil
import wave

import numpy as np
import pytest

from goofer_amd import core, trackers

pytestmark = pytest.mark.gpu

SR = 44100


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _wav(path, y, sr, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
    return path


def _voiced(rng, n, sr):
    t = np.arange(n) / sr
    f0 = rng.uniform(110, 330) * (1 + 0.02 * np.sin(2 * np.pi * 5 * t))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = sum(np.sin(k * ph) / k for k in range(1, 12))
    return 0.3 * y / np.max(np.abs(y)) + 0.003 * rng.standard_normal(n)


def _bursts(rng, n):
    """White noise whose level jumps by 40 dB every 2000 samples: an envelope no knot count below 192 fits."""
    level = np.repeat(rng.choice([0.005, 0.5], size=n // 2000 + 1), 2000)[:n]
    return level * rng.standard_normal(n)


def _signals(seed, count, sr):
    rng = np.random.default_rng(seed)
    sigs = [np.zeros(sr // 3), _bursts(rng, sr), np.zeros(700), 0.5 * rng.standard_normal(300)]
    click = np.zeros(sr // 2)
    click[::4410] = 0.8
    sigs.append(click)
    for r, f in ((0.7, 9000.0), (0.8, 9000.0)):                   # one resonant click: envelopes that need 64 or 80 knots
        y, state = np.zeros(8000), np.zeros(2)
        th = 2 * np.pi * f / 44100
        for i in range(4000, 8000):
            y[i] = (0.5 if i == 4000 else 0.0) + 2 * r * np.cos(th) * state[0] - r * r * state[1]
            state = (y[i], state[0])
        sigs.append(y)
    while len(sigs) < count:
        n = int(rng.integers(200, 3 * sr))
        kind = rng.integers(3)
        sigs.append(_voiced(rng, n, sr) if kind == 0 else _bursts(rng, n) if kind == 1 else 0.1 * rng.standard_normal(n))
    return [s.astype(np.float32) for s in sigs]


def _batch(ctx, sigs, sr, want_env):
    import torch
    ctx.plan(sr, 1024, 256)
    y = torch.from_numpy(np.concatenate(sigs)).to(ctx.device)
    knots, K, f_off, env = ctx.envelope_knots(y, [len(s) for s in sigs], want_env=want_env)
    knots, K = knots.cpu().numpy(), K.cpu().numpy()
    env = env.cpu().numpy() if want_env else None
    out = []
    for i in range(len(sigs)):
        a, b = int(f_off[i]), int(f_off[i + 1])
        assert b - a == 1 + len(sigs[i]) // 256
        vals = knots[a:b].reshape(-1)[:(b - a) * int(K[i])].reshape(b - a, int(K[i]))
        out.append((int(K[i]), vals, None if env is None else env[a:b]))
    return out


@pytest.mark.parametrize("sr,count", [(SR, 44), (48000, 8), (22050, 8)])
def test_envelope_knots_bit_equal_to_per_file_path(ctx, sr, count):
    sigs = _signals(11 + sr, count, sr)
    refs = [core.envelope_features(s, sr, 1024, 256, ctx=ctx) for s in sigs]
    whole = _batch(ctx, sigs, sr, want_env=True)
    seen_K = set()
    for (K, vals, env), (env_ref, knots_ref) in zip(whole, refs):
        ref = knots_ref["knot_vals_log"]
        assert K == ref.shape[0] and np.array_equal(vals.T, ref)
        assert np.array_equal(env.T, env_ref)
        seen_K.add(K)
    if sr == SR:
        assert {32, 192} <= seen_K and len(seen_K) >= 3, seen_K
    # the same batch cut into passes of at most a quarter of its frames (a larger signal alone)
    frames = [(i, sr, 1 + len(s) // 256) for i, s in enumerate(sigs)]
    passes = trackers.plan_passes(frames, frame_budget=sum(f for _, _, f in frames) // 4)
    assert len(passes) > 2
    for _, idx in passes:
        for i, (K, vals, env) in zip(idx, _batch(ctx, [sigs[i] for i in idx], sr, want_env=False)):
            assert env is None and K == whole[i][0] and np.array_equal(vals, whole[i][1])


def _same_features(got, ref):
    env, f0, vm, forms, knots = got
    env_r, f0_r, vm_r, forms_r, knots_r = ref
    assert np.array_equal(env, env_r) and np.array_equal(f0, f0_r) and np.array_equal(vm, vm_r)
    assert list(forms) == list(forms_r) and all(np.array_equal(forms[k], forms_r[k]) for k in forms)
    assert set(knots) == set(knots_r)
    for k in knots:
        assert np.array_equal(np.asarray(knots[k]), np.asarray(knots_r[k])), k


def test_extract_features_batch_native_bit_equal(ctx):
    rng = np.random.default_rng(5)
    sigs = [_voiced(rng, int(n), SR) for n in rng.integers(2000, 2 * SR, size=10)] + [np.zeros(SR // 4), np.zeros(500)]
    got = core.extract_features_batch(sigs, SR, pitch_tracker="native", ctx=ctx)
    for y, g in zip(sigs, got):
        try:
            ref = core.extract_features(y, SR, pitch_tracker="native", ctx=ctx)
        except ValueError as e:
            assert isinstance(g, ValueError) and str(g) == str(e)
            continue
        _same_features(g, ref)
    assert isinstance(got[-1], ValueError)


def test_extract_features_batch_calls_another_tracker_per_signal(ctx):
    calls = []

    def fake(y, sr, hop, n_frames):
        calls.append(len(y))
        frames = np.abs(np.asarray(y, dtype=np.float64))[: (len(y) // hop) * hop].reshape(-1, hop).mean(axis=1)
        f0 = np.where(frames > 0.05, 100.0 + 1000.0 * frames, 0.0)
        return f0, {k: list(100.0 * k + frames[:n_frames]) for k in range(1, 6)}

    rng = np.random.default_rng(9)
    sigs = [_voiced(rng, int(n), SR) for n in rng.integers(3000, SR, size=6)]
    got = core.extract_features_batch(sigs, SR, pitch_tracker=fake, ctx=ctx)
    assert calls == [len(s) for s in sigs]
    for y, g in zip(sigs, got):
        _same_features(g, core.extract_features(y, SR, pitch_tracker=fake, ctx=ctx))


def test_single_signal_calls_refuse_empty_and_non_mono(ctx):
    """envelope_features / extract_features are the batch of one: an empty or a 2-D signal is the ValueError a pass gives it,
    and the pass's other signals are unaffected."""
    calls = []

    def fake(y, sr, hop, n_frames):
        calls.append(y)
        return np.full(n_frames + 2, 150.0), {k: [500.0 * k] * n_frames for k in range(1, 6)}

    good = _voiced(np.random.default_rng(3), 6000, SR)
    for y in (np.zeros(0), np.zeros((2, 4096)), np.zeros((4096, 1))):
        with pytest.raises(ValueError):
            core.envelope_features(y, SR, ctx=ctx)
        with pytest.raises(ValueError):
            core.extract_features(y, SR, pitch_tracker=fake, ctx=ctx)
        with pytest.raises(ValueError):
            core.extract_features(y, SR, pitch_tracker="native", ctx=ctx)
        bad, ok = core.extract_features_batch([y, good], SR, pitch_tracker=fake, ctx=ctx)
        assert isinstance(bad, ValueError)
        _same_features(ok, core.extract_features(good, SR, pitch_tracker=fake, ctx=ctx))
    assert len(calls) == 6 and all(c is good for c in calls)


def test_single_call_raises_the_host_trackers_exception(ctx):
    """A host tracker is called once, with the signal itself, and its exception is what extract_features raises."""
    err = RuntimeError("no tracks for this one")
    calls = []

    def failing(y, sr, hop, n_frames):
        calls.append((y, sr, hop, n_frames))
        raise err

    y = _voiced(np.random.default_rng(4), 9000, SR)
    with pytest.raises(RuntimeError) as info:
        core.extract_features(y, SR, pitch_tracker=failing, ctx=ctx)
    assert info.value is err
    assert len(calls) == 1 and calls[0][0] is y and calls[0][1:] == (SR, 256, 1 + len(y) // 256)


def test_folder_mode_batched(ctx, tmp_path):
    rng = np.random.default_rng(21)
    bank, ref_dir = tmp_path / "bank", tmp_path / "ref"
    bank.mkdir()
    ref_dir.mkdir()
    names = []
    for i in range(26):
        sr = (22050, 44100, 48000)[i % 3]
        names.append(_wav(bank / f"s{i:02d}.wav", _voiced(rng, int(rng.integers(sr // 5, sr)), sr), sr))
    y2 = _voiced(rng, 30000, SR)
    names.append(_wav(bank / "stereo.wav", np.stack([y2, 0.5 * y2], axis=1).reshape(-1), SR, channels=2))
    _wav(bank / "short.wav", np.zeros(300), SR)
    (bank / "garbage.wav").write_bytes(b"not audio")
    cached = []
    for name in ("c0", "c1"):
        _wav(bank / f"{name}.wav", _voiced(rng, 20000, SR), SR)
        feat = trackers.features_path(bank / f"{name}.wav")
        feat.write_bytes(b"pre-existing " + name.encode())
        cached.append((feat, feat.read_bytes(), feat.stat().st_mtime_ns))
    tally = trackers.extract_folder(bank, tracker="native", ctx=ctx)
    assert tally == {"extracted": 27, "skipped": 2, "failed": 2}
    for feat, data, mtime in cached:
        assert feat.read_bytes() == data and feat.stat().st_mtime_ns == mtime
    assert not trackers.features_path(bank / "short.wav").exists() and not list(bank.glob("*.tmp*"))
    for wav in names:
        copy = shutil.copy(wav, ref_dir / wav.name)
        got = core.load_features(trackers.features_path(wav))
        ref = core.load_features(trackers.ensure_features(copy, tracker="native", ctx=ctx))
        env, env_r = got[0], ref[0]
        assert set(env) == set(env_r) and all(np.array_equal(np.asarray(env[k]), np.asarray(env_r[k])) for k in env)
        for a, b in zip(got[1:3], ref[1:3]):
            assert np.array_equal(a, b)
        assert list(got[3]) == list(ref[3]) and all(np.array_equal(got[3][k], ref[3][k]) for k in got[3])
        assert got[4:] == ref[4:]


def test_http_collector_analyses_cold_samples_once(ctx, tmp_path, monkeypatch):
    from goofer_amd import cli
    from goofer_amd import synthetic as syn
    from goofer_amd.render import GooferResampler, Renderer
    rng = np.random.default_rng(33)
    bank = tmp_path / "bank"
    bank.mkdir()
    good = [_wav(bank / "ka.wav", _voiced(rng, SR, SR), SR), _wav(bank / "sa.wav", _voiced(rng, SR + 5000, SR), SR)]
    short = _wav(bank / "n.wav", np.zeros(400), SR)
    wavs = [good[0], good[1], short, good[0], short, good[1], good[0], good[1]]
    req = syn.make_request(4, "", length_ms=250)
    entered = []
    real = trackers.ensure_features_batch

    def spy(paths, *a, **kw):
        entered.append(list(paths))
        return real(paths, *a, **kw)

    monkeypatch.setattr(trackers, "ensure_features_batch", spy)
    renderer = Renderer(ctx)
    col = cli.BatchCollector(renderer=renderer, tracker="native")
    try:
        batch = [cli._Pending([str(w), str(tmp_path / f"o{i}.wav"), *syn.request_args(req)]) for i, w in enumerate(wavs)]
        col._render(batch)
    finally:
        col.close()
    assert len(entered) == 1 and sorted(map(str, entered[0])) == sorted(map(str, [good[0], good[1], short]))
    assert sorted(bank.glob("*.goofy")) == sorted(trackers.features_path(w) for w in good)
    expect = {}
    for w in good:
        expect[w] = len(GooferResampler(str(w), str(tmp_path / f"ref_{w.stem}.wav"), *syn.request_args(req), renderer=renderer,
                                         seed=1, tracker="native").out)
    short_err = trackers.native_refusal(400, SR)
    for i, (w, p) in enumerate(zip(wavs, batch)):
        assert p.done.is_set()
        if w == short:
            assert isinstance(p.error, ValueError) and str(p.error) == str(short_err)
            assert not (tmp_path / f"o{i}.wav").exists()
        else:
            assert p.error is None
            with wave.open(str(tmp_path / f"o{i}.wav"), "rb") as r:
                assert r.getnframes() == expect[w] > 0
