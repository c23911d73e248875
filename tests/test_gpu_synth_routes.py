"""GPU: goofer_synth_batch's routes (stem walkers, spectra in HBM with one / three stems per overlap-add, separate kernels) as
seen from outside — the stage names each route reports to the profiler, and the onset view a batch with the 'sg' layer leaves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_HEAD = ["setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place"]
_TAIL = ["env_edit", "env_rows", "sample_assemble"]
STEMS = _HEAD + ["mask_short", "noise_stems", "", "harm_stem", "", "", "", "note_finish", ""] + _TAIL
OLA = _HEAD + ["rfft_frames", "harm_shape", "", "noise_spectra", "", "", "mask_short", "irfft_ola3", "apply_gain"] + _TAIL
SEPARATE = _HEAD + ["rfft_frames", "harm_shape", "irfft_harm", "noise_spectra", "irfft_breath", "irfft_unvoiced", "mask_short",
                    "ola3_gains", "apply_gain"] + _TAIL


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _batch(ctx, sr, n_fft, hop, lens, seed, subharm_weight=None, fixed_f0=None):
    from goofer_amd.device import default_params
    ctx.plan(sr, n_fft, hop)
    rng = np.random.default_rng(seed)
    nb = n_fft // 2 + 1
    envs, f0s, masks, env_len = [], [], [], []
    for n in lens:
        T = 1 + n // hop
        envs.append((1.0 + rng.random((T, nb))).astype(np.float32))
        env_len.append(T)
        m = (rng.random(n) > 0.2).astype(np.float32)
        m[n // 4:n // 2] = 1.0
        masks.append(m)
        f0s.append((150.0 + 100.0 * rng.random(n)).astype(np.float32) * m)
    for k, hz in (fixed_f0 or {}).items():                     # note k: voiced throughout at a constant f0
        masks[k][:] = 1.0
        f0s[k][:] = hz
    par = default_params(len(lens))
    if subharm_weight is not None:
        par["subharm_weight"] = subharm_weight
    args = (ctx.rows_from(np.concatenate(envs)), env_len, ctx.tensor(np.concatenate(f0s)), ctx.tensor(np.concatenate(masks)), lens, par)
    return args, f0s, masks


# (geometry, options, sub-harmonic layer, the names the route reports)
ROUTES = {
    "walkers": ((44100, 1024, 256), {}, False, STEMS),
    "stems=0": ((44100, 1024, 256), {"stems": 0}, False, OLA),
    "fused_ola=0": ((44100, 1024, 256), {"fused_ola": 0}, False, SEPARATE),
    "sg": ((44100, 1024, 256), {}, True, OLA),
    "ola_split": ((96000, 2048, 96), {}, False, OLA),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_profile_stage_names_per_route(ctx, route):
    """Each route reports the stage table bench.py keys its kernel names and roofline on — the one-stem overlap-add of
    96 kHz / 2048 / 96 included, which reports k_irfft_ola1 as irfft_ola3 and k_note_finish as apply_gain."""
    (sr, n_fft, hop), opts, sg, names = ROUTES[route]
    args, _, _ = _batch(ctx, sr, n_fft, hop, [3000, 5000, 7000], 3, 0.5 if sg else None)
    sub = dict(semitones=-12) if sg else None
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.profile_begin(4)
        out = ctx.synth_batch(*args, seed=5, subharm=sub)
        res = ctx.profile_end()
        got = ctx.profile_stage_names()
    finally:
        ctx.set_option("stems", 1)
        ctx.set_option("fused_ola", 1)
        ctx.plan(44100, 1024, 256)
    assert res["steps"] == 1
    assert got == names
    assert np.isfinite(out["mix"].cpu().numpy()).all()


def _sub_onsets(f0, mask, sr, ratio):
    """k_subharm_inc + k_pulse_onsets_wrap without vibrato: fp64 increments f0 * ratio / sr where voiced, one sequential phase
    walk; an onset wherever the phase reaches 1."""
    f = f0.astype(np.float64)
    sub = f * ratio
    inc = np.where((mask > 0) & (f > 0) & ~(sub < 1e-2), sub / sr, 0.0)
    out, ph = [], 0.0
    for i, a in enumerate(inc.tolist()):
        ph += a
        if ph >= 1.0:
            out.append(i)
            ph -= 1.0
    return np.array(out, dtype=np.int32)


def test_onset_view_after_a_subharmonic_batch(ctx):
    """After a batch with the 'sg' layer the onset slots hold the sub-harmonic trackers' onsets (k_pulse_onsets_wrap runs last),
    n + 16 per note: the view covers every carved slot, and note k's onsets start at sample_off[k] + 16 k.

    The second batch has lengths at the edges of a walk block (16 samples) and of a chunk (512), a workgroup whose last wave has
    no note (nine notes, four per workgroup), and a note whose sub-harmonic increment 3000 * 16 / 44100 is above 1 throughout:
    the tracker fires on every sample, 512 events per chunk, so its 64-entry queue is flushed from inside the walk."""
    lens = [4000, 9000, 2500, 12000, 6000]
    weight = np.array([0.5, 0.0, 0.8, 0.5, 0.3], dtype=np.float32)
    args, f0s, masks = _batch(ctx, 44100, 1024, 256, lens, 11, weight)
    ctx.synth_batch(*args, seed=2, subharm=dict(semitones=-12))
    cnt = ctx.debug_fetch("onset_cnt")
    idx = ctx.debug_fetch("onset_idx")
    N, n = sum(lens), len(lens)
    assert cnt.size == n
    assert idx.size == N + 16 * n + 16
    off = np.concatenate([[0], np.cumsum(lens)])
    for k in range(n):
        want = _sub_onsets(f0s[k], masks[k], 44100, 0.5) if weight[k] > 0 else np.zeros(0, np.int32)
        assert want.size > 0 or weight[k] == 0
        assert cnt[k] == want.size, k
        assert np.array_equal(idx[off[k] + 16 * k: off[k] + 16 * k + cnt[k]], want), k
    lens = [1, 15, 16, 17, 511, 512, 513, 1025, 1500]
    args, f0s, masks = _batch(ctx, 44100, 1024, 256, lens, 12, np.full(len(lens), 0.5, dtype=np.float32), fixed_f0={8: 3000.0})
    ctx.synth_batch(*args, seed=2, subharm=dict(semitones=48))
    cnt = ctx.debug_fetch("onset_cnt")
    idx = ctx.debug_fetch("onset_idx")
    N, n = sum(lens), len(lens)
    assert cnt.size == n
    assert idx.size == N + 16 * n + 16
    off = np.concatenate([[0], np.cumsum(lens)])
    for k in range(n):
        want = _sub_onsets(f0s[k], masks[k], 44100, 16.0)
        assert want.size <= lens[k] + 16, k
        assert cnt[k] == want.size, k
        assert np.array_equal(idx[off[k] + 16 * k: off[k] + 16 * k + cnt[k]], want), k
    assert cnt[8] == lens[8]
