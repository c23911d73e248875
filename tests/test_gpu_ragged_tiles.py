"""GPU: a note gets the same bits whether its workgroups lie inside it (rendered alone) or straddle its neighbours (rendered in a
batch) — the property csrc/ragged.h's sample_tile and note_reduce exist to provide, through every entry point that reaches a
kernel built on them.

One batch of nine notes whose boundaries fall at offsets 0, 1, 255 and mid-tile of the 256-sample tiles, inside the 1024-sample
tiles of the four-samples-per-thread kernels (k_apply_gain, k_scale_f0), on odd samples (k_normal_fill's pairs), with a total
that is no multiple of 1024.  The batch and each note alone, every output compared as int32 words.

The one exception: k_note_sumsq adds the float64 partial sums of a note's workgroups with atomics, so the sum of a note longer
than one workgroup has no fixed order, in a batch or alone.  The post-chain outputs of notes with tension != 0 and more than 256
samples are therefore held to tests/test_gpu_post_chain.py's judge (both renderings) instead of to each other's bits.
"""
import numpy as np
import pytest

import post_ref as P
import synth_ref as SR
from test_gpu_post_chain import judge, run_post

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
LENGTHS = [256, 1, 254, 257, 1023, 1025, 700, 2048, 3]
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
SYNTH_OPTIONS = {"stems": 1}                                  # what the tests here change, with the library's defaults
SR_HZ = 16000                                                 # the 0.1 s vibrato fade-in (1600 samples) ends inside the 2048-sample note


def test_the_batch_puts_note_boundaries_where_the_tiles_differ():
    inner = OFFSETS[1:-1]
    assert {0, 1, 255} <= set(int(v) for v in inner % 256) and any(1 < v < 255 for v in inner % 256)
    assert any(v % 1024 and not v % 256 for v in inner) and any(v % 1024 and v % 256 for v in inner)
    assert any(v % 2 for v in inner) and OFFSETS[-1] % 1024 and OFFSETS[-1] % 2
    assert max(LENGTHS) > 1024 and OFFSETS[-1] < 7000


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype.itemsize == 4 else a.view(np.int64)


def _same_bits(what, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(_words(got) != _words(want))[0]
    assert bad.size == 0, "%s: %d of %d samples differ, first at %d (%r alone, %r in the batch)" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------
# Context.synth_batch on the spectra routes
# ---------------------------------------------------------------------------------------------
JITTER = dict(f0_jitter=True, f0_jitter_strength=0.7, volume_jitter=True, volume_jitter_strength_harm=0.8, volume_jitter_strength_breath=1.6)
VARIANTS = {
    "plain": (lambda k: {}, {}),
    "jitter": (lambda k: JITTER if k % 2 else {}, dict(noise=True)),
    "vibrato": (lambda k: JITTER if k % 2 else {}, dict(volume_vibrato=True, vol_jitter_speed=9.0)),
    "subharm": (lambda k: dict(add_subharm=True, subharm_weight=0.7) if k % 2 else {},
                dict(subharm=dict(semitones=[-12, 7], vibrato=True, rate=40.0, depth=0.2, delay=0.01))),
}


def synth_cases(geo, variant):
    """The nine notes for one geometry: a pitch_shift != 1 on every third note (k_scale_f0), the variant's keywords on every second."""
    per_note = VARIANTS[variant][0]
    return [SR.make_case(geo, 7000 + geo[1] + k, n, "n%d" % n, mask="blocks",
                         kw=dict(per_note(k), **({"pitch_shift": SR.f32(1.0 + 0.1 * (k % 3))} if k % 3 else {})))
            for k, n in enumerate(LENGTHS)]


def synth_noise(cases):
    """The caller's draws of the jitter flags: (noise_f0, noise_vol_h, noise_vol_b), float64 per sample of the batch."""
    rng = np.random.default_rng(99)
    return [rng.standard_normal(sum(c["n"] for c in cases)) for _ in range(3)]


def run_synth(ctx, geo, cases, call, noise=None):
    """One goofer_synth_batch over ``cases``: {output name: host array}."""
    from goofer_amd.core import note_params_from_kwargs
    ctx.plan(*geo)
    par = np.concatenate([note_params_from_kwargs(1, **c["kw"]) for c in cases])
    par["seed"][:, 0] = [c["n"] for c in cases]
    kw = dict(call)
    if kw.pop("noise", False):
        kw.update(noise_f0=ctx.tensor(noise[0]), noise_vol=(ctx.tensor(noise[1]), ctx.tensor(noise[2])))
    out = ctx.synth_batch(ctx.rows_from(np.concatenate([c["env"].T for c in cases])), [c["env"].shape[1] for c in cases],
                          ctx.tensor(np.concatenate([c["f0"] for c in cases])), ctx.tensor(np.concatenate([c["mask"] for c in cases])),
                          [c["n"] for c in cases], par, phi=ctx.rows_from(np.concatenate([c["phi"].T for c in cases])), seed=5, **kw)
    ctx.check()
    return {k: out[k].cpu().numpy() for k in ("harm", "uv", "bre", "rec", "mix")}


_plain = {}                                                   # geometry: the plain batch's outputs


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("geo", [(SR_HZ, 1024, 256), (SR_HZ, 768, 192)], ids=["ola3", "frames"])
def test_synth_batch_notes_alone_and_in_the_batch(ctx, geo, variant):
    """n_fft 1024 / hop 256: k_irfft_ola3 + k_apply_gain; n_fft 768 / hop 192: k_irfft_frames + k_ola3_gains.  plain; the four
    jitter kernels and k_stem_peak; the vibrato envelope; the k_subharm_* kernels.  (No length is refused by the synthesis.)"""
    cases = synth_cases(geo, variant)
    call = VARIANTS[variant][1]
    noise = synth_noise(cases) if call.get("noise") else None
    assert int(0.1 * SR_HZ) < max(LENGTHS)
    try:
        ctx.set_option("stems", 0)
        batch = run_synth(ctx, geo, cases, call, noise)
        assert all(np.any(batch[name]) for name in batch)
        if geo not in _plain:
            _plain[geo] = batch if variant == "plain" else run_synth(ctx, geo, synth_cases(geo, "plain"), {})
        plain = _plain[geo]
        for k, c in enumerate(cases):
            sl = slice(int(OFFSETS[k]), int(OFFSETS[k + 1]))
            if variant != "plain" and k % 2 and c["n"] > 1:           # the variant's kernels ran: its notes are not the plain ones
                assert np.any(batch["mix"][sl] != plain["mix"][sl]), (k, c["n"])
            alone = run_synth(ctx, geo, [c], call, [v[sl] for v in noise] if noise else None)
            for name, v in alone.items():
                _same_bits("%s of note %d (%d samples)" % (name, k, c["n"]), v, batch[name][sl])
    finally:
        for name, v in SYNTH_OPTIONS.items():
            ctx.set_option(name, v)
        ctx.plan(44100, 1024, 256)


# ---------------------------------------------------------------------------------------------
# Renderer._post_chain's call (goofer_post_batch)
# ---------------------------------------------------------------------------------------------
SR_POST = SR_HZ
EVERY_LAYER = dict(layers=("su", "sj", "sa"), su_gain=0.4, sj_mix=0.3, sa_mix=0.2, sd_strength=30.0, tension=0.375, pitch_dyn=-0.5,
                   mix_harm=0.9, mix_breath=1.1, mix_unvoiced=0.9, volume=0.8)


def post_notes(tension=True):
    """Every layer on for alternating notes (``tension`` False: all but st, so that every note is compared by bits)."""
    notes = []
    for k, n in enumerate(LENGTHS):
        kw = {}
        if k % 2 == 0:
            kw = dict(EVERY_LAYER, fry_a=n // 5, fry_b=n - n // 7, fry_fade=int(0.01 * SR_POST))
            if not tension:
                kw["tension"] = 0.0
        notes.append(P.make_note(800 + k, n, SR_POST, **kw))
    return notes


@pytest.mark.parametrize("tension", [False, True], ids=["all_but_st", "every_layer"])
def test_post_chain_notes_alone_and_in_the_batch(ctx, tension):
    ctx.plan(SR_POST, 1024, 256)
    notes = post_notes(tension)
    batch = run_post(ctx, notes)
    alone = [run_post(ctx, [c])[0] for c in notes]
    open_sum = [k for k, c in enumerate(notes) if c["tension"] != 0 and c["n"] > 256]
    assert bool(open_sum) == tension
    for k, c in enumerate(notes):
        if k in open_sum:
            continue
        # (the mix of a note without a flag is not written: it keeps run_post's fill pattern, which goes by position in the batch)
        for name, a, b in zip(("harm", "bre", "mix") if P.flagged(c) else ("harm", "bre"), alone[k], batch[k]):
            _same_bits("%s of note %d (%d samples)" % (name, k, c["n"]), a, b)
    if open_sum:
        sub = [notes[k] for k in open_sum]
        judge("ragged tiles st, batch", sub, [batch[k] for k in open_sum], SR_POST)
        judge("ragged tiles st, alone", sub, [alone[k] for k in open_sum], SR_POST)


# ---------------------------------------------------------------------------------------------
# single-kernel entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [0, 4])
def test_normal_fill_notes_alone_and_in_the_batch(ctx, tag):
    """k_normal_fill: pairs that straddle the alignment in the notes that start on an odd sample; note_on off for every third note,
    whose samples keep what the buffer held."""
    from goofer_amd.device import default_params
    n = len(LENGTHS)
    par = default_params(n)
    par["seed"][:, 0] = np.arange(n) + 11
    on = np.array([k % 3 != 1 for k in range(n)], dtype=np.uint8)
    growl = np.linspace(0.1, 0.9, n) if tag == 4 else None
    total = int(OFFSETS[-1])
    keep = -7.25
    batch = ctx.normal_fill(2026, par, LENGTHS, tag, note_on=on, growl_scale=growl,
                            out=torch.full((total,), keep, dtype=torch.float64, device=ctx.device)).cpu().numpy()
    for k, ln in enumerate(LENGTHS):
        sl = slice(int(OFFSETS[k]), int(OFFSETS[k + 1]))
        alone = ctx.normal_fill(2026, par[k:k + 1], [ln], tag, note_on=on[k:k + 1], growl_scale=None if growl is None else growl[k:k + 1],
                                out=torch.full((ln,), keep, dtype=torch.float64, device=ctx.device)).cpu().numpy()
        _same_bits("note %d (%d samples)" % (k, ln), alone, batch[sl])
        assert np.all(alone == keep) if not on[k] else not np.any(alone == keep)


@pytest.mark.parametrize("fast_interp", [False, True])
def test_smooth_mask_ds_notes_alone_and_in_the_batch(ctx, fast_interp):
    ctx.plan(44100, 1024, 256)
    rng = np.random.default_rng(31)
    masks = [np.repeat(rng.random(n // 37 + 1) > 0.4, 37)[:n].astype(F32) for n in LENGTHS]
    batch = ctx.smooth_mask_ds(ctx.tensor(np.concatenate(masks)), LENGTHS, sigma=100.0, fast_interp=fast_interp).cpu().numpy()
    for k, m in enumerate(masks):
        alone = ctx.smooth_mask_ds(ctx.tensor(m), [len(m)], sigma=100.0, fast_interp=fast_interp).cpu().numpy()
        _same_bits("note %d (%d samples)" % (k, len(m)), alone, batch[int(OFFSETS[k]):int(OFFSETS[k + 1])])


def test_irfft_ola_notes_alone_and_in_the_batch(ctx):
    """k_ola_gather behind the framewise inverse transform."""
    from goofer_amd.device import spec_stride
    geo = (44100, 1024, 256)
    ctx.plan(*geo)
    nb = geo[1] // 2 + 1
    frames = ctx.frame_counts(LENGTHS)
    f_off = ctx.offsets(frames)
    rng = np.random.default_rng(57)
    S = np.zeros((int(f_off[-1]), spec_stride(nb)), dtype=np.complex64)
    S[:, :nb] = (rng.standard_normal((int(f_off[-1]), nb)) + 1j * rng.standard_normal((int(f_off[-1]), nb))).astype(np.complex64)
    batch = ctx.irfft_ola(ctx.tensor(S), ctx.tensor(OFFSETS.astype(np.int64)), ctx.tensor(f_off), int(OFFSETS[-1])).cpu().numpy()
    for k, ln in enumerate(LENGTHS):
        rows = S[int(f_off[k]):int(f_off[k + 1])]
        alone = ctx.irfft_ola(ctx.tensor(rows), ctx.tensor(np.array([0, ln], dtype=np.int64)),
                              ctx.tensor(np.array([0, frames[k]], dtype=np.int64)), ln).cpu().numpy()
        _same_bits("note %d (%d samples)" % (k, ln), alone, batch[int(OFFSETS[k]):int(OFFSETS[k + 1])])
