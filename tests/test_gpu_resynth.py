"""GPU: wav-to-wav resynthesis — Context.per_sample_f0 against trackers.per_sample_f0 and the reference's pinned data,
core.resynthesize_batch against the sequential extract_features -> synthesize calls (bit for bit, and the legacy np.random
state after them), its device residency, analyse_batch with the kernel against analyse, and the command line end to end."""
import wave

import numpy as np
import pytest

from goofer_amd import core, trackers

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _voiced(rng, n, sr, gaps=True):
    """A harmonic tone with a vibrato and (``gaps``) a few short silences: f0 tracks with interior unvoiced runs."""
    t = np.arange(n) / sr
    f0 = rng.uniform(110, 330) * (1 + 0.02 * np.sin(2 * np.pi * 5 * t))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    y = sum(np.sin(k * ph) / k for k in range(1, 12))
    y = 0.3 * y / np.max(np.abs(y)) + 0.003 * rng.standard_normal(n)
    if gaps:
        for _ in range(3):
            a = int(rng.integers(0, max(1, n - sr // 20)))
            y[a:a + int(rng.integers(sr // 200, sr // 25))] = 0.0
    return y


# -- kernel ----------------------------------------------------------------------------------------------------------
def test_per_sample_f0_kernel_matches_reference_fixture(ctx, gold):
    g = gold("cold_cache")
    sr = int(g["sr"][0])
    tracks = [g["pitch_track"], g["y2_pitch_track"]]
    f0, mask = ctx.per_sample_f0(ctx.tensor(np.concatenate(tracks)), [t.size for t in tracks], [len(g["y"]), 3000], sr)
    f0, mask = f0.cpu().numpy(), mask.cpu().numpy()
    n = len(g["y"])
    assert np.array_equal(f0[:n], g["f0_interp"]) and np.array_equal(mask[:n], g["voicing_mask"])
    assert np.array_equal(f0[n:], g["y2_f0_interp"]) and np.array_equal(mask[n:], g["y2_voicing_mask"])


def _random_track(rng, L):
    tr = rng.uniform(60, 600, L)
    kind = rng.integers(6)
    for _ in range(int(rng.integers(1, 5))):                    # zero runs of 1-6 frames, anywhere (ends included)
        a = int(rng.integers(0, L))
        tr[a:a + int(rng.integers(1, 7))] = 0.0
    if kind == 0:
        tr[:int(rng.integers(1, 4))] = 0.0                       # a run touching the start
    if kind == 1:
        tr[-int(rng.integers(1, 4)):] = 0.0                      # ... the end
    if rng.random() < 0.4:
        tr[rng.integers(0, L, int(rng.integers(1, 4)))] = np.nan
    if rng.random() < 0.3:                                      # equal neighbours
        a = int(rng.integers(0, L - 1))
        tr[a + 1] = tr[a]
    return tr


def test_per_sample_f0_kernel_matches_host_function(ctx):
    rng = np.random.default_rng(7)
    for sr in (8000, 22050, 44100, 48000, 96000):
        for f0_min in (75, 120):
            for gap in (0, 2, 4):
                tracks, lens = [], []
                for k in range(40):
                    L = 2 if k < 4 else int(rng.integers(3, 400))
                    n = int(rng.integers(1, L)) if k % 7 == 0 else int(rng.integers(1, 40000))   # some with more frames than samples
                    n = 1 if k == 5 else 2 if k == 6 else n
                    tracks.append(_random_track(rng, L))
                    lens.append(n)
                f0, mask = ctx.per_sample_f0(ctx.tensor(np.concatenate(tracks)), [t.size for t in tracks], lens, sr, f0_min, gap)
                f0, mask = f0.cpu().numpy(), mask.cpu().numpy()
                off = np.concatenate([[0], np.cumsum(lens)])
                for k, (tr, n) in enumerate(zip(tracks, lens)):
                    ref_f0, ref_m = trackers.per_sample_f0(tr, n, sr, f0_min, gap)
                    s = slice(off[k], off[k + 1])
                    assert np.array_equal(f0[s], ref_f0) and np.array_equal(mask[s], ref_m), (sr, f0_min, gap, k, tr.size, n)


def test_per_sample_f0_kernel_refuses_bad_batches(ctx):
    t = ctx.tensor(np.ones(10))
    with pytest.raises(ValueError):
        ctx.per_sample_f0(t, [5, 4], [100, 100], 44100)            # lengths do not cover the tensor
    with pytest.raises(ValueError):
        ctx.per_sample_f0(t, [9, 1], [100, 100], 44100)            # a one-frame track
    with pytest.raises(ValueError):
        ctx.per_sample_f0(t, [5, 5], [100, -1], 44100)             # a negative length
    with pytest.raises(ValueError):
        ctx.per_sample_f0(t, [5, 5], [100], 44100)                 # tracks and signals disagree
    with pytest.raises(ValueError):
        ctx.per_sample_f0(t.float(), [5, 5], [100, 100], 44100)    # not fp64


# -- resynthesize_batch ----------------------------------------------------------------------------------------------
def _sequential(signals, sr, n_fft, hop, variants, seeds, phis, tracker, synth_kw):
    out = []
    for i, y in enumerate(signals):
        try:
            env, f0, mask, forms, _ = core.extract_features(y, sr, n_fft, hop, pitch_tracker=tracker)
        except Exception as e:                                    # noqa: BLE001
            out.append(type(e))
            continue
        res = []
        for v, var in enumerate(variants or [{}]):
            k = i * len(variants or [{}]) + v
            kw = {"formants": forms, **synth_kw, **var}
            try:
                res.append(core.synthesize(env, f0, mask, y, sr, n_fft, hop, **kw, seed=seeds[k], phi=phis[k]))
            except Exception as e:                                # noqa: BLE001
                res.append(type(e))
        out.append(res if variants is not None else res[0])
    return out


def _same(a, b):
    if isinstance(b, type):
        assert isinstance(a, b), (a, b)
        return
    assert len(a) == 4 and all(np.array_equal(x, y) for x, y in zip(a, b))


def _compare(got, want, variants):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, type):
            assert isinstance(g, w), (g, w)
        elif variants is None:
            _same(g, w)
        else:
            assert len(g) == len(w)
            for gv, wv in zip(g, w):
                _same(gv, wv)


def _check(ctx, signals, sr, n_fft, hop, variants=None, tracker="native", phis=None, **synth_kw):
    V = 1 if variants is None else len(variants)
    seeds = [1000 + k for k in range(len(signals) * V)]
    phis = phis or [None] * (len(signals) * V)
    np.random.seed(3)
    want = _sequential(signals, sr, n_fft, hop, variants, seeds, phis, tracker, synth_kw)
    state = np.random.get_state()
    np.random.seed(3)
    got = core.resynthesize_batch(signals, sr, n_fft, hop, pitch_tracker=tracker, variants=variants, seeds=seeds, phis=phis, ctx=ctx,
                                  **synth_kw)
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    _compare(got, want, variants)
    return got


@pytest.mark.parametrize("n_fft,hop,sr", [(1024, 256, 44100), (2048, 512, 44100), (1024, 256, 48000)])
def test_resynthesize_batch_equals_sequential_calls(ctx, n_fft, hop, sr):
    rng = np.random.default_rng(n_fft + sr)
    signals = [_voiced(rng, int(rng.integers(sr // 4, sr)), sr) for _ in range(4)]
    signals.insert(2, 0.1 * rng.standard_normal(500))           # shorter than one pitch window: its ValueError, the rest render
    variants = [{"pitch_shift": 1.3, "formant_shift": 0.9, "F2_shift": 1.1},
                {"volume_jitter": True, "volume_jitter_strength_harm": 0.5, "volume_jitter_strength_breath": 1.0}]
    got = _check(ctx, signals, sr, n_fft, hop, variants=variants)
    assert isinstance(got[2], ValueError) and all(isinstance(g, list) for k, g in enumerate(got) if k != 2)


def test_resynthesize_batch_stretch_with_jitter_and_subharmonics(ctx):
    rng = np.random.default_rng(11)
    sr = 44100
    signals = [_voiced(rng, int(rng.integers(sr // 3, sr)), sr) for _ in range(3)]
    variants = [{"stretch_factor": 1.4, "f0_jitter": True, "f0_jitter_strength": 0.5},
                {"stretch_factor": 0.8, "add_subharm": True, "subharm_weight": 0.6, "pitch_shift": 1.1},
                {"stretch_factor": 1.2, "start_sec": 0.05, "end_sec": 0.2}]
    _check(ctx, signals, sr, 1024, 256, variants=variants)


def test_resynthesize_batch_one_variant_phis_and_keywords(ctx):
    rng = np.random.default_rng(12)
    sr = 44100
    signals = [_voiced(rng, int(rng.integers(sr // 4, sr // 2)), sr) for _ in range(3)]
    nb = 1024 // 2 + 1
    phis = [rng.uniform(-np.pi, np.pi, (nb, 1 + len(y) // 256)) for y in signals]
    got = _check(ctx, signals, sr, 1024, 256, phis=phis, pitch_shift=0.8, breath_strength=0.3)
    assert all(isinstance(g, tuple) for g in got)


def test_resynthesize_batch_host_tracker(ctx):
    """A host pitch_tracker= callable: its tracks are uploaded and go through the same kernel."""
    def tracker(y, sr, hop, n_frames):
        L = max(1, (len(y) - 400) // hop)
        t = np.arange(L)
        f0 = 150 + 20 * np.sin(t / 5.0)
        f0[(t % 17) < 3] = 0.0                                   # interior gaps of three frames
        f0[t % 23 == 4] = np.nan
        return f0, {k: list(500.0 * k + t[:n_frames]) for k in range(1, 6)}
    rng = np.random.default_rng(13)
    sr = 44100
    signals = [_voiced(rng, int(rng.integers(sr // 4, sr // 2)), sr) for _ in range(3)] + [rng.standard_normal(650)]   # 1 frame
    _check(ctx, signals, sr, 1024, 256, variants=[{}, {"pitch_shift": 1.2}], tracker=tracker)


def test_resynthesize_keeps_features_on_the_device(ctx, monkeypatch):
    """Native tracker, no stretch: nothing fp64 per sample or per bin comes to the host — only the formant tracks
    ([frames, 5] fp64) and the four fp32 stems of each synthesis pass."""
    rng = np.random.default_rng(14)
    sr = 44100
    signals = [_voiced(rng, int(rng.integers(sr // 4, sr)), sr) for _ in range(3)]
    core.resynthesize_batch(signals[:1], sr, ctx=ctx, pitch_tracker="native", seeds=[1])          # warm-up outside the spy
    seen = []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def cpu(self, *a, **k):
        if self.is_cuda:
            seen.append((self.dtype, tuple(self.shape)))
        return real_cpu(self, *a, **k)

    def to(self, *a, **k):
        dev = k.get("device", a[0] if a else None)
        if self.is_cuda and (dev == "cpu" or (isinstance(dev, torch.device) and dev.type == "cpu")):
            seen.append((self.dtype, tuple(self.shape)))
        return real_to(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "to", to)
    res = core.resynthesize_batch(signals, sr, ctx=ctx, pitch_tracker="native", variants=[{}, {"pitch_shift": 1.5}],
                                  seeds=list(range(6)))
    monkeypatch.undo()
    total = sum(len(y) for y in signals) * 2
    assert all(isinstance(r, list) for r in res)
    formants = [s for s in seen if s[0] == torch.float64]
    stems = [s for s in seen if s[0] == torch.float32]
    assert len(formants) == 1 and len(formants[0][1]) == 2 and formants[0][1][1] == 5, seen
    assert stems == [(torch.float32, (total,))] * 4, seen
    assert len(seen) == 5, seen


# -- analyse_batch with the kernel ------------------------------------------------------------------------------------
def test_analyse_batch_with_kernel_equals_extract_features(ctx, tmp_path):
    """Each signal of a six-signal pass against the same signal alone (core.extract_features), bit for bit, .goofy bytes too."""
    rng = np.random.default_rng(15)
    sr = 44100
    signals = [_voiced(rng, int(rng.integers(sr // 4, 2 * sr)), sr) for _ in range(6)]
    batch = trackers.analyse_batch(signals, sr, tracker="native", ctx=ctx)
    for k, (y, b) in enumerate(zip(signals, batch)):
        one = core.extract_features(y, sr, pitch_tracker="native", ctx=ctx)
        for x, z in zip(one[:3], b[:3]):
            assert np.array_equal(x, z)
        assert one[3] == b[3]
        for key in ("knot_vals_log", "hz_knots"):
            assert np.array_equal(one[4][key], b[4][key])
        p1, p2 = tmp_path / f"one{k}.goofy", tmp_path / f"batch{k}.goofy"
        core.save_features(p1, one[4], one[1], one[2], one[3], sr, len(y))
        core.save_features(p2, b[4], b[1], b[2], b[3], sr, len(y))
        assert p1.read_bytes() == p2.read_bytes()


# -- command line -----------------------------------------------------------------------------------------------------
def _wav(path, y, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())


def test_cli_writes_what_the_library_renders(ctx, tmp_path):
    from goofer_amd import resynth
    from goofer_amd.render import write_wav
    rng = np.random.default_rng(16)
    src = tmp_path / "in"
    (src / "sub").mkdir(parents=True)
    files = [src / "a.wav", src / "sub" / "b.wav", src / "c.wav"]
    for f, sr in zip(files, (44100, 44100, 48000)):
        _wav(f, _voiced(rng, int(rng.integers(sr // 4, sr // 2)), sr), sr)
    _wav(src / "short.wav", 0.1 * rng.standard_normal(300), 44100)          # refused by the tracker: logged, exit 1
    out = tmp_path / "out"
    variants = [{"pitch_shift": 1.2}, {"formant_shift": 0.9, "breath_strength": 0.2}]
    rc = resynth.main([str(src), "--out", str(out), "--tracker", "native", "--stems", "--seed", "5", "--set", "uv_strength=0.5",
                       "--variant", "pitch_shift=1.2", "--variant", "formant_shift=0.9,breath_strength=0.2"])
    assert rc == 1
    assert not list(out.rglob("short_*"))
    order = sorted(files + [src / "short.wav"])                 # collect_inputs' order: the seeds' file index
    for f in files:
        y, sr = trackers.read_audio(f)
        k = order.index(f)
        np.random.seed(5)
        res = core.resynthesize_batch([y], sr, 1024, 256, pitch_tracker="native", variants=variants, seeds=[5 + 2 * k, 5 + 2 * k + 1],
                                      uv_strength=0.5, ctx=ctx)[0]
        for stems, paths in zip(res, resynth.output_paths(f, src, out, 2, True)):
            assert set(paths) == {"reconstruct", "harmonic", "breathiness", "unvoiced"}
            for name, idx in resynth.STEM_NAMES:
                ref = tmp_path / "ref.wav"
                write_wav(ref, stems[idx], sr)
                assert paths[name].read_bytes() == ref.read_bytes(), (f, name)
