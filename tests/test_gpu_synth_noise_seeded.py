"""GPU: ``synthesize(noise_seed=)`` / ``synthesize_batch(noise_seeds=)`` / ``resynthesize_batch(noise_seeds=)`` — a note renders what
a reference process produces that calls ``np.random.seed(s)`` immediately before ``gf.synthesize``, with every legacy draw (f0,
sub-harmonic f0, harmonic and breath volume jitter; the roughness noises) made on the device by goofer_legacy_normal_jobs.

Geometry: sr 44100, n_fft 1024, hop 256; six notes of 1501 to 4001 samples.  Every Gaussian stays inside its note: the jitter
sigmas are sr / (6 * speed) = 73.5 (f0, speed 100) and 49 (volume, speed 150) samples, the roughness smoothing 20 ms -> sigma
147, radius 4 sigma = 588 < 1501.

The bound is the keyword cases' of tests/test_gpu_synth.py: 2e-5 sample-RMS against the oracle.  The device's normals differ
from the host's by the last place of ``log`` (1e-14 relative, tests/test_gpu_legacy_jobs.py), which is nothing beside the fp32
synthesis; so the same bound holds against this library's own host-draw path."""
import numpy as np
import pytest

from conftest import rms_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SR, N_FFT, HOP = 44100, 1024, 256
LENGTHS = [1501, 2048, 2750, 3333, 3500, 4001]
ROUGH = dict(roughness_on=True, rough_k_list=(2, 3), rough_noise_smooth_ms=20.0, rough_alpha_slew_ms=20.0)
KW = [
    dict(f0_jitter=True, f0_jitter_strength=1.2),
    dict(volume_jitter=True, volume_jitter_strength_harm=0.8, volume_jitter_strength_breath=1.6),
    dict(volume_jitter=True, volume_vibrato=True, volume_jitter_speed=9.0, volume_jitter_strength_harm=0.8,
         volume_jitter_strength_breath=1.6),                                       # the sinusoid: draws nothing
    dict(add_subharm=True, subharm_f0_jitter=0.8, f0_jitter=True, f0_jitter_strength=0.5, volume_jitter=True,
         volume_jitter_strength_harm=0.4, volume_jitter_strength_breath=0.7),      # all four streams, odd n: the cache carries
    dict(stretch_factor=1.3, f0_jitter=True, f0_jitter_strength=0.7),              # n is the stretched length
    dict(f0_jitter=True, f0_jitter_strength=0.6, **ROUGH),
]
LEGACY = [4027, 0, 7, 2 ** 32 - 1, 99, 123456789]
PHI = [6001, 6002, 6003, 6004, 6005, 2 ** 70 + 5]
STEMS = ("rec", "harm", "uv", "bre")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _note(i, n):
    from goofer_amd import synthetic as syn
    from oracle import goofer_ref as R
    src = syn.make_source(60 + i, seconds=(n + 0.25) / SR)
    assert src["y_len"] == n
    env = np.ascontiguousarray(R.decode_env_from_knots(src["env_pack"]), dtype=np.float32)
    f0 = ((170.0 + 25.0 * i) * src["mask"]).astype(np.float32)
    return {"env_spec": env, "f0_interp": f0, "voicing_mask": src["mask"].copy(), "y": np.empty(n, bool), "formants": src["formants"]}


@pytest.fixture(scope="module")
def notes():
    return [_note(i, n) for i, n in enumerate(LENGTHS)]


def _single(ctx, note, kw, phi_seed, noise_seed=None):
    from goofer_amd import core
    return core.synthesize(note["env_spec"], note["f0_interp"], note["voicing_mask"], note["y"], SR, N_FFT, HOP,
                           formants=note["formants"], phi_seed=phi_seed, noise_seed=noise_seed, ctx=ctx, **kw)


@pytest.fixture(scope="module")
def rendered(ctx, notes):
    """per note: the oracle after np.random.seed(s), this library's host-draw path after np.random.seed(s) (the parent's
    behaviour) and the seeded call; the global generator is put back"""
    from oracle import goofer_ref as R
    state = np.random.get_state()
    out = []
    try:
        for note, kw, s, ps in zip(notes, KW, LEGACY, PHI):
            n = len(note["y"])
            n_out = int(n * kw["stretch_factor"]) if "stretch_factor" in kw else n
            phi = np.random.default_rng(ps).uniform(0.0, 2.0 * np.pi, size=(N_FFT // 2 + 1, 1 + n_out // HOP)).astype(np.float32)
            np.random.seed(s)
            ref = R.synthesize(note["env_spec"].copy(), note["f0_interp"].copy(), note["voicing_mask"].copy(), note["y"], SR, n_fft=N_FFT,
                               hop_length=HOP, formants=note["formants"], phi=phi, **kw)
            np.random.seed(s)
            parent = _single(ctx, note, kw, ps)
            np.random.seed(12345)
            before = np.random.get_state()
            seeded = _single(ctx, note, kw, ps, s)
            after = np.random.get_state()
            assert before[2:] == after[2:] and np.array_equal(before[1], after[1])       # neither read nor advanced
            out.append({"ref": ref, "parent": parent, "seeded": seeded})
    finally:
        np.random.set_state(state)
    return out


@pytest.mark.parametrize("i", range(6))
def test_seeded_note_matches_the_oracle_seeded_the_same_way(rendered, i):
    r = rendered[i]
    for a, b, key in zip(r["seeded"], r["ref"], STEMS):
        assert a.dtype == np.float32 and a.shape == b.shape, key
        e = rms_err(a, b)
        print(f"note {i} {key}: sample-RMS against the oracle {e:.3e}")
        assert e < 2e-5, (i, key, e)


@pytest.mark.parametrize("i", range(6))
def test_seeded_note_matches_the_host_draws_of_the_same_seed(rendered, i):
    r = rendered[i]
    for a, b, key in zip(r["seeded"], r["parent"], STEMS):
        assert a.shape == b.shape, key
        e = rms_err(a, b)
        print(f"note {i} {key}: sample-RMS against the host-draw path {e:.3e}")
        assert e < 2e-5, (i, key, e)


def test_another_seed_renders_another_note(ctx, notes, rendered):
    other = _single(ctx, notes[0], KW[0], PHI[0], LEGACY[0] + 1)
    assert rms_err(other[1], rendered[0]["seeded"][1]) > 1e-3


def _batch_notes(notes, idxs=range(6)):
    return [{**notes[i], **KW[i]} for i in idxs]


def test_batch_equals_the_single_calls_bit_for_bit(ctx, notes, rendered):
    from goofer_amd import core
    before = np.random.get_state()
    got = core.synthesize_batch(_batch_notes(notes), SR, N_FFT, HOP, phi_seeds=PHI, noise_seeds=LEGACY, ctx=ctx)
    after = np.random.get_state()
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])
    for i, (g, r) in enumerate(zip(got, rendered)):
        assert not isinstance(g, BaseException), g
        for a, b, key in zip(g, r["seeded"], STEMS):
            assert np.array_equal(a, b), (i, key)


def test_mixed_list_leaves_the_state_the_unseeded_notes_leave(ctx, notes):
    """seeded and unseeded notes in shared passes (pairs of one keyword set): the seeded ones are their single calls, the
    unseeded ones and the global generator are what the unseeded notes alone give"""
    from goofer_amd import core
    order = [(0, 0), (3, 0), (1, 1), (2, 1), (5, 5), (4, 5)]                       # (note, keyword set): three shared passes
    batch = [{**notes[i], **KW[k]} for i, k in order]
    phi = [PHI[i] for i, _ in order]
    seeds = [LEGACY[0], None, None, LEGACY[2], LEGACY[5], None]
    unseeded = [q for q, s in enumerate(seeds) if s is None]
    state = np.random.get_state()
    try:
        np.random.seed(5)
        alone = core.synthesize_batch([batch[q] for q in unseeded], SR, N_FFT, HOP, phi_seeds=[phi[q] for q in unseeded], ctx=ctx)
        want = np.random.get_state()
        np.random.seed(5)
        got = core.synthesize_batch(batch, SR, N_FFT, HOP, phi_seeds=phi, noise_seeds=seeds, ctx=ctx)
        have = np.random.get_state()
    finally:
        np.random.set_state(state)
    assert have[0] == want[0] and np.array_equal(have[1], want[1]) and have[2:] == want[2:]
    for q, a in zip(unseeded, alone):
        assert all(np.array_equal(x, y) for x, y in zip(got[q], a)), q
    for q, s in enumerate(seeds):
        if s is not None:
            i, k = order[q]
            one = _single(ctx, notes[i], KW[k], phi[q], s)
            assert all(np.array_equal(x, y) for x, y in zip(got[q], one)), q


def test_all_seeded_call_uploads_no_per_sample_noise(ctx, notes, monkeypatch):
    from goofer_amd import core
    uploads, jobs = [], []
    real_noise, real_rough, real_jobs = core._noise, core._rough_noise, ctx.legacy_normal_jobs

    def noise(*a, **k):
        uploads.append(real_noise(*a, **k))
        return uploads[-1]

    def rough(c, host, lens, n_k):
        uploads.extend(h for h in host if h is not None)
        return real_rough(c, host, lens, n_k)

    def spy_jobs(table, **k):
        jobs.extend(table)
        return real_jobs(table, **k)
    monkeypatch.setattr(core, "_noise", noise)
    monkeypatch.setattr(core, "_rough_noise", rough)
    monkeypatch.setattr(ctx, "legacy_normal_jobs", spy_jobs)
    monkeypatch.setattr(np.random, "randn", lambda *a: pytest.fail("a host draw"))
    before = np.random.get_state()
    got = core.synthesize_batch(_batch_notes(notes), SR, N_FFT, HOP, phi_seeds=PHI, noise_seeds=LEGACY, ctx=ctx)
    after = np.random.get_state()
    monkeypatch.undo()
    assert all(not isinstance(g, BaseException) for g in got)
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])
    assert uploads and all(u is None for u in uploads)                             # asked for every stream, uploaded none
    # one job per drawing note (its streams in order) and one float32 job per roughness partial
    shapes = sorted((s, n, len(d), f) for s, n, d, f in jobs)
    assert shapes == sorted([(LEGACY[0], 1501, 1, False), (LEGACY[1], 2048, 2, False), (LEGACY[3], 3333, 4, False),
                             (LEGACY[4], int(3500 * 1.3), 1, False), (LEGACY[5], 4001, 1, False), (1337, 4001, 1, True),
                             (1338, 4001, 1, True)])


def test_resynthesize_batch_variants_are_each_seeded_afresh(ctx):
    from goofer_amd import core
    rng = np.random.default_rng(21)
    t = np.arange(12000) / SR
    ph = 2 * np.pi * np.cumsum(200.0 * (1 + 0.02 * np.sin(2 * np.pi * 5 * t))) / SR
    y = sum(np.sin(k * ph) / k for k in range(1, 12))
    y = 0.3 * y / np.max(np.abs(y)) + 0.003 * rng.standard_normal(t.size)
    variants = [dict(KW[3]), dict(KW[5])]
    before = np.random.get_state()
    got = core.resynthesize_batch([y], SR, N_FFT, HOP, pitch_tracker="native", variants=variants, seeds=[1, 2], phi_seeds=[11, 12],
                                  noise_seeds=[4027], ctx=ctx)[0]
    one = core.resynthesize(y, SR, N_FFT, HOP, pitch_tracker="native", variants=variants, seeds=[1, 2], phi_seeds=[11, 12],
                            noise_seed=4027, ctx=ctx)
    after = np.random.get_state()
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])
    env, f0, mask, forms, _ = core.extract_features(y, SR, N_FFT, HOP, pitch_tracker="native", ctx=ctx)
    for v, var in enumerate(variants):
        want = core.synthesize(env, f0, mask, y, SR, N_FFT, HOP, formants=forms, seed=1 + v, phi_seed=11 + v, noise_seed=4027, ctx=ctx,
                               **var)
        assert not isinstance(got[v], BaseException), got[v]
        for a, b, c2, key in zip(got[v], want, one[v], STEMS):
            assert np.array_equal(a, b) and np.array_equal(c2, b), (v, key)
    # the variants do not share one stream: variant 1 alone renders what it renders behind variant 0
    alone = core.resynthesize_batch([y], SR, N_FFT, HOP, pitch_tracker="native", variants=variants[1:], seeds=[2], phi_seeds=[12],
                                    noise_seeds=[4027], ctx=ctx)[0]
    assert all(np.array_equal(a, b) for a, b in zip(alone[0], got[1]))


def test_bad_seeds_raise_and_nothing_is_launched(ctx, notes, monkeypatch):
    from goofer_amd import core
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("goofer_"):
                return fn

            def wrapped(*a):
                called.append(name)
                return fn(*a)
            return wrapped
    ctx.plan(SR, N_FFT, HOP)
    monkeypatch.setattr(ctx, "lib", Spy(ctx.lib))
    monkeypatch.setattr(np.random, "randn", lambda *a: pytest.fail("a host draw"))
    batch = _batch_notes(notes)
    for bad in (LEGACY[:5], LEGACY + [1], [-1] + LEGACY[1:], [2 ** 32] + LEGACY[1:], LEGACY[:5] + [1.5], [True] + LEGACY[1:]):
        with pytest.raises(ValueError):
            core.synthesize_batch(batch, SR, N_FFT, HOP, phi_seeds=PHI, noise_seeds=bad, ctx=ctx)
    for bad in (-1, 2 ** 32, 2.0, True):
        with pytest.raises(ValueError):
            _single(ctx, notes[0], KW[0], PHI[0], bad)
    with pytest.raises(ValueError):
        core.resynthesize_batch([np.zeros(12000)], SR, N_FFT, HOP, pitch_tracker="native", noise_seeds=[1, 2], ctx=ctx)
    assert called == [], called
