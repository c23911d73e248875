"""GPU: n_fft above 2048 — the workgroup transform (n_fft 4096) and its Bluestein length 4096 (every other even size in
[2052, 4094]) through stft / istft, synthesize, synthesize_batch, the cold-sample analysis and resynthesize_batch, against the
reference (golden/large_fft.npz) and the oracle.  The sizes that stay refused close the file."""
import numpy as np
import pytest

import analysis_ref as A
from conftest import golden, rel_rms, rms_err
from oracle import goofer_ref as R
from test_gpu_resynth import _check, _voiced
from test_gpu_synth import _random_kwargs
from test_large_fft_oracle import _synth_case

from goofer_amd import core

pytestmark = pytest.mark.gpu

TOL = 1e-4                               # the project's sample-RMS bound against the reference
ENV_RTOL, ENV_ATOL = 2e-6, 1e-9          # test_gpu_analysis_oracle.py's envelope bounds
TRUTH_FACTOR = 3.0                       # test_gpu_analysis_oracle.py's; at Bluestein 3000 (L = 4096) measured 3.0 x: 4.0
TRUTH_FACTOR_BLUESTEIN = 4.0


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _off(c, lengths):
    return c.tensor(c.offsets(lengths))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_stft_istft_against_reference(ctx, tag):
    """test_gpu_kernels.py's bounds: the spectrum to 5e-7 relative RMS, the inverse to 3e-7 of max(1, |y|)."""
    g = golden("large_fft")
    n_fft, hop = (int(v) for v in g[f"geo_{tag}"])
    x, S_ref, y_ref = g[f"x_{tag}"], g[f"S_{tag}"], g[f"y_{tag}"]
    n = len(x)
    S = core.stft(x, n_fft=n_fft, hop_length=hop, ctx=ctx)
    assert S.shape == S_ref.shape
    assert rel_rms(S, S_ref) < 5e-7, (tag, rel_rms(S, S_ref))
    y = core.istft(S_ref, hop_length=hop, length=n, ctx=ctx)
    assert y.shape == y_ref.shape
    assert rms_err(y, y_ref) < 3e-7 * max(1.0, float(np.abs(y_ref).max())), tag
    # the raw entry points on a ragged batch: the second copy of the signal gives the same rows
    T = 1 + n // hop
    S2 = ctx.rfft_frames(ctx.tensor(np.concatenate([x, x])), _off(ctx, [n, n]), _off(ctx, [T, T]), 2 * T).cpu().numpy()
    assert np.array_equal(S2[:T], S2[T:])


def test_synthesize_against_reference(ctx):
    g = golden("large_fft")
    for name in g["names"]:
        c = _synth_case(g, name)
        outs = core.synthesize(c["env"], c["f0"], c["mask"], np.empty(c["n"], bool), c["sr"], n_fft=c["n_fft"], hop_length=c["hop"],
                               formants=c["formants"], phi=c["phi"], ctx=ctx, **c["kw"])
        for got, key in zip(outs, ("rec", "harm", "uv", "bre")):
            ref = g[f"{name}_{key}"]
            assert got.dtype == np.float32 and got.shape == ref.shape
            e = rms_err(got, ref) / max(1.0, float(np.max(np.abs(ref))))
            assert e < TOL, (name, key, e)


def _random_vs_oracle(ctx, name, case):
    c = _synth_case(golden("large_fft"), name)
    kw = _random_kwargs(case)
    kw.pop("start_sec", None), kw.pop("end_sec", None)       # (the fixture notes are shorter than the regions it draws)
    phi = c["phi"]
    if "stretch_factor" in kw:
        n_new = len(R.stretch_feature(c["f0"], kw["stretch_factor"]))
        if "start_sec" in kw:
            a, b = int(kw["start_sec"] * c["sr"]), int(kw["end_sec"] * c["sr"])
            n_new = a + int((b - a) * kw["stretch_factor"]) + (len(c["f0"]) - b)
        phi = np.random.default_rng(case).uniform(0.0, 2.0 * np.pi, size=(c["env"].shape[0], 1 + n_new // c["hop"])).astype(np.float32)
    args = (c["env"], c["f0"], c["mask"], np.empty(c["n"], bool), c["sr"])
    np.random.seed(300 + case)
    ref = R.synthesize(*args, n_fft=c["n_fft"], hop_length=c["hop"], formants=c["formants"], phi=phi, **kw)
    np.random.seed(300 + case)
    got = core.synthesize(*args, n_fft=c["n_fft"], hop_length=c["hop"], formants=c["formants"], phi=phi, ctx=ctx, **kw)
    for a, b, key in zip(got, ref, ("rec", "harm", "uv", "bre")):
        assert a.shape == b.shape, (key, kw)
        e = rms_err(a, b) / max(1.0, float(np.max(np.abs(b))))
        assert e < TOL, (key, e, kw)


@pytest.mark.parametrize("case", range(100))
def test_synthesize_random_kwargs_4096_vs_oracle(ctx, case):
    _random_vs_oracle(ctx, "sr96_4096", 40000 + case)


@pytest.mark.parametrize("case", range(50))
def test_synthesize_random_kwargs_bluestein_vs_oracle(ctx, case):
    _random_vs_oracle(ctx, "sr44_3000", 41000 + case)


def test_synthesize_batch_equals_sequential_calls_bitwise(ctx):
    """Mixed notes at 4096 (plain, shifted, jittered, sub-harmonic, stretched, silent) in one call against one call each."""
    c = _synth_case(golden("large_fft"), "sr96_4096")
    base = dict(env_spec=c["env"], f0_interp=c["f0"], voicing_mask=c["mask"], y=np.empty(c["n"], bool), formants=c["formants"])
    extra = [{}, {"pitch_shift": 1.2, "formant_shift": 0.85, "F1_shift": 1.2}, {"f0_jitter": True, "f0_jitter_strength": 0.5},
             {"volume_jitter": True}, {"add_subharm": True, "subharm_weight": 0.6}, {"stretch_factor": 1.3},
             {"voicing_mask": np.zeros_like(c["mask"])}, {"normalize": 0.0, "apply_brightness": False}]
    notes = [{**base, **e} for e in extra]
    seeds = [500 + i for i in range(len(notes))]
    np.random.seed(11)
    want = [core.synthesize(**{k: v for k, v in nt.items()}, sr=c["sr"], n_fft=4096, hop_length=c["hop"], seed=s, ctx=ctx)
            for nt, s in zip(notes, seeds)]
    np.random.seed(11)
    got = core.synthesize_batch(notes, c["sr"], 4096, c["hop"], seeds=seeds, ctx=ctx)
    for i, (g_, w) in enumerate(zip(got, want)):
        assert len(g_) == 4 and all(np.array_equal(a, b) for a, b in zip(g_, w)), (i, extra[i])


@pytest.mark.parametrize("geom", [(96000, 4096, 1024), (44100, 3000, 750)], ids=["96000-4096-1024", "44100-3000-750"])
def test_envelope_and_knots_against_oracle(ctx, geom):
    """envelope_features and extract_features' envelope against envelope_of, test_gpu_analysis_oracle.py's bounds."""
    sr, n_fft, hop = geom
    e_gpu = e_ora = 0.0
    for kind, y in A.signal_set(sr, n_fft, hop):
        what = (kind, len(y))
        env_o, pack_o = R.envelope_of(y, sr, n_fft, hop)
        env_g, pack_g = core.envelope_features(y, sr, n_fft, hop, ctx=ctx)
        assert env_g.dtype == np.float64 and env_g.shape == env_o.shape, what
        if kind in A.DIP_KINDS:
            assert A.frame_error(env_g, env_o).max() <= ENV_RTOL, what
        else:
            np.testing.assert_allclose(env_g, env_o, rtol=ENV_RTOL, atol=ENV_ATOL, err_msg=str(what))
        truth = A.truth_envelope(y, sr, n_fft, hop)
        e_gpu = max(e_gpu, A.frame_error(env_g, truth).max())
        e_ora = max(e_ora, A.frame_error(env_o, truth).max())
        if A.margin(A.candidate_errors(env_o, sr, n_fft)) > 1e-3:
            assert len(pack_g["hz_knots"]) == len(pack_o["hz_knots"]), what
            assert pack_g["n_fft"] == n_fft and pack_g["n_bins"] == n_fft // 2 + 1
            d = np.abs(pack_g["knot_vals_log"].astype(np.float64) - pack_o["knot_vals_log"].astype(np.float64))
            reach = ENV_RTOL * np.max(env_o, axis=0)[None, :] / np.exp(pack_o["knot_vals_log"].astype(np.float64))
            tol = np.abs(np.spacing(pack_o["knot_vals_log"])).astype(np.float64) + 2 * reach
            assert np.all(d <= tol), (what, float(np.max(d / tol)))
    assert e_gpu <= (TRUTH_FACTOR if n_fft == 4096 else TRUTH_FACTOR_BLUESTEIN) * e_ora, (e_gpu, e_ora)
    # extract_features' envelope half is the same batch of one
    y = A.make_signal("voiced", 3 * n_fft, sr, 1)
    env_o, pack_o = R.envelope_of(y, sr, n_fft, hop)
    env_x, _, _, _, knots_x = core.extract_features(y, sr, n_fft, hop, pitch_tracker="native", ctx=ctx)
    assert env_x.shape == env_o.shape and A.frame_error(env_x, env_o).max() <= ENV_RTOL


def test_resynthesize_batch_native_tracker_96k(ctx):
    """resynthesize_batch(pitch_tracker='native') at 96 kHz / 4096 equals extract_features + synthesize, bit for bit."""
    sr, n_fft, hop = 96000, 4096, 1024
    rng = np.random.default_rng(4096)
    signals = [_voiced(rng, int(rng.integers(sr // 4, sr // 2)), sr) for _ in range(3)]
    variants = [{"pitch_shift": 1.2, "formant_shift": 0.9}, {"volume_jitter": True}]
    got = _check(ctx, signals, sr, n_fft, hop, variants=variants, tracker="native")
    assert all(isinstance(g, list) for g in got)


@pytest.mark.parametrize("n_fft", [4095, 4098, 8192, 2050])
def test_other_sizes_still_refused(ctx, n_fft):
    """Odd sizes, sizes above 4096, and 2050, whose refusal test_gpu_kernels.py pins."""
    from goofer_amd.device import GooferError
    with pytest.raises(GooferError, match=r"\[64, 4096\] other than 2050"):
        ctx.plan(44100, n_fft, n_fft // 4)
    with pytest.raises(GooferError):
        core.stft(np.zeros(10000, np.float32), n_fft=n_fft, hop_length=n_fft // 4, ctx=ctx)


def test_renderer_refuses_a_4096_source(ctx):
    """The resampler path stays at n_fft <= 2048: a source analysed at 4096 is refused before anything is launched."""
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Renderer, Source
    sr, n_fft, hop = 44100, 4096, 1024
    y = _voiced(np.random.default_rng(1), sr // 2, sr).astype(np.float32)
    env, f0, mask, forms, pack = core.extract_features(y, sr, n_fft, hop, pitch_tracker="native", ctx=ctx)
    src = Source.from_pack(pack, f0, mask, forms, sr, len(y))
    assert src.n_fft == 4096
    from goofer_amd import sampler as S
    req = S.decode_request(*syn.request_args(syn.make_request(2000, "t0g0", length_ms=300)))
    with pytest.raises(ValueError, match="n_fft <= 2048"):
        Renderer(ctx).render([(src, req)])
