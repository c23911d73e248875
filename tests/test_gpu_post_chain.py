"""GPU: the sample-domain post chain (csrc/post.hip, and the chunked-tap path of k_gauss_samples in csrc/jitter.hip) stage by
stage and sample by sample against tests/post_ref.py.

goofer_post_batch takes its stems as plain device pointers and edits harm / bre in place, so every stage is observable with
synthetic stems and one flag at a time; k_onepole_cascade and k_gauss_samples also have entry points of their own.

THE JUDGEMENT, the same everywhere: per sample, no RMS, no sample left out.  With ``peak`` the largest absolute truth value of
the note, ``e_ref = max|ref32 - truth| / peak`` (post_ref in the reference arithmetic) and ``e_gpu = max|gpu - truth| / peak``,

    e_gpu <= 3 e_ref + 2^-23

- the project's own factor (test_gpu_analysis_oracle.py) plus one fp32 rounding of the stored result, which covers the stages
where the reference arithmetic is exact.  Samples of notes without a post flag must be bit-unchanged in harm and bre, and their
mix samples (pre-filled with a pattern) untouched.  Every stage of goofer_post_batch holds the bound as it stands.  The
cascade kernel on its own needed two decisions, explained at test_cascade_seams: its seam windows are held to the note's bound,
and notes shorter than 64 samples get the factor 6 (measured: 3.8), because the reference error of a handful of samples is not
a level.

MEASURED on an MI355X, worst note of each test, e_ref / e_gpu (for the chain: of harm, bre and mix the one with the largest e_gpu):

    cascade, per setting (order, f0 mode, cutoff factor): note e_ref / e_gpu; worst e_gpu in the seam windows 8 | 512 | 2048
      high-pass  1  0  0.05    7.97e-07 / 6.86e-07    6.86e-07 | 5.54e-07 | 2.05e-07
      high-pass  4  0  1       2.50e-06 / 2.13e-06    2.13e-06 | 1.53e-06 | 9.43e-08
      high-pass  6  2  200     2.64e-06 / 1.93e-06    1.93e-06 | 1.81e-06 | 1.68e-06
      high-pass 12  1  1       2.13e-06 / 1.18e-06    1.18e-06 | 8.26e-07 | 3.81e-07
      high-pass  4  0  400     1.16e-06 / 6.45e-07    6.45e-07 | 5.18e-07 | 1.34e-07
      high-pass  6  1  0.01    2.24e-06 / 2.06e-06    2.06e-06 | 1.81e-06 | 1.15e-06
      high-pass 12  2  30000   3.60e-07 / 4.03e-07    4.03e-07 | 2.87e-07 | 1.94e-07
      low-pass   1  0  0.1     2.37e-07 / 7.85e-08    7.85e-08 | 6.45e-08 | 5.34e-08
      low-pass   4  0  1.25    2.03e-07 / 3.02e-07    3.02e-07 | 9.67e-08 | 5.59e-08
      low-pass   6  0  3       5.12e-07 / 4.50e-07    4.50e-07 | 1.02e-07 | 8.02e-08
      low-pass  12  1  2       9.14e-07 / 8.36e-07    8.36e-07 | 1.47e-07 | 1.28e-07
      low-pass   6  2  1000    2.90e-07 / 9.00e-08    9.00e-08 | 6.88e-08 | 6.66e-08
      low-pass   4  2  1e6     1.75e-07 / 1.75e-07    1.75e-07 | 1.12e-07 | 9.65e-08
      low-pass  12  0  0.2     5.70e-07 / 5.70e-07    5.70e-07 | 3.10e-07 | 8.62e-08
      worst (e_gpu - 2^-23) / e_ref: 1.18 over the notes of 511 samples and more, 3.81 over the notes of 1 to 9 samples;
      the worst seam error is 2.13e-06 of the note's peak (order-4 high-pass, where e_ref is 2.50e-06).
      In all 14 launches every one of the 22 045 device samples equals the numpy emulation of the kernel's documented
      arithmetic (post_ref.dynamic_filter_batch_device) bit for bit; the test prints the count and does not assert it.
    note boundaries   su 1.13e-07 / 1.02e-07   sj 8.86e-08 / 1.06e-07   sa 1.41e-07 / 1.41e-07   fry 1.95e-07 / 1.69e-07
                      sd 9.98e-08 / 9.98e-08   st > 0 1.20e-06 / 1.17e-06   st < 0 6.27e-07 / 2.99e-07
                      pd > 0 8.15e-08 / 1.01e-07   pd < 0 1.21e-07 / 1.35e-07   all together 1.89e-06 / 1.04e-06
    fry ramps         5.49e-07 / 5.74e-07
    sd fade-in        44.1 kHz 9.79e-08 / 9.79e-08   22.05 kHz 8.72e-08 / 8.72e-08
    st gain           3.05e-06 / 2.20e-06          st leak  5.65e-07 / 4.44e-07
    pd level          44.1 kHz 8.58e-08 / 1.10e-07   22.05 kHz 1.58e-07 / 1.11e-07
    long Gaussians    max |device - oracle|: sigma 441 3.8e-15, sigma 960 8.9e-16, sigma 1920 3.6e-15 (single = ragged)
"""
import ctypes as C

import numpy as np
import pytest

import post_ref as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
GEOMETRIES = [(44100, 1024, 256), (22050, 512, 128)]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def run_post(ctx, notes):
    """goofer_post_batch over the ragged batch ``notes`` (post_ref.make_note dicts), set up the way Renderer._post_chain does it.
    Returns per note (harm, bre, mix) as the device left them; checks that notes without a flag were left alone."""
    from goofer_amd import _lib
    n = len(notes)
    off = ctx.offsets([c["n"] for c in notes])
    total = int(off[-1])
    host = {k: np.concatenate([np.asarray(c[k], dtype=F32) for c in notes]) for k in ("harm", "uv", "bre", "f0", "mask", "bend")}
    host["mix"] = ((np.arange(total) % 251) * 0.5 - 60.0).astype(F32)
    dev = {k: ctx.tensor(v) for k, v in host.items()}
    post = np.zeros(n, dtype=_lib.POST_NOTE)
    post["su_off"] = post["sj_off"] = post["sa_off"] = -1
    for f in P.NOTE_FIELDS:
        post[f] = [c[f] for c in notes]
    layers = {}
    for key, names in (("su", ("su_harm",)), ("sj", ("sj_harm",)), ("sa", ("sa_uv", "sa_bre"))):
        o, parts = 0, {nm: [] for nm in names}
        for i, c in enumerate(notes):
            if c[names[0]] is not None and c["n"] > 0:
                post[key + "_off"][i] = o
                o += c["n"]
                for nm in names:
                    parts[nm].append(np.asarray(c[nm], dtype=F32))
        for nm in names:
            layers[nm] = ctx.tensor(np.concatenate(parts[nm])) if parts[nm] else None
    par = np.zeros(n, dtype=_lib.NOTE_PARAMS)
    for f in P.MIX_FIELDS:
        par[f] = [c[f] for c in notes]
    d_off, d_par = ctx.tensor(off), ctx.tensor(par.view(np.uint8))
    ptr = lambda t: t.data_ptr() if t is not None else None
    desc = _lib.Post(n_notes=n, total_samples=total, sample_off=d_off.data_ptr(), sample_off_host=off.ctypes.data,
                     params=d_par.data_ptr(), notes=post.ctypes.data, f0=dev["f0"].data_ptr(), mask=dev["mask"].data_ptr(),
                     bend=dev["bend"].data_ptr(), harm=dev["harm"].data_ptr(), uv=dev["uv"].data_ptr(), bre=dev["bre"].data_ptr(),
                     su_harm=ptr(layers["su_harm"]), sj_harm=ptr(layers["sj_harm"]), sa_uv=ptr(layers["sa_uv"]),
                     sa_bre=ptr(layers["sa_bre"]), mix=dev["mix"].data_ptr())
    ctx._check(ctx.lib.goofer_post_batch(ctx.h, C.byref(desc), ctx._stream()))
    got = {k: dev[k].cpu().numpy() for k in ("harm", "bre", "mix")}
    for k in ("uv", "f0", "mask", "bend"):
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(host[k])), k
    outs = []
    for i, c in enumerate(notes):
        sl = slice(int(off[i]), int(off[i + 1]))
        outs.append(tuple(got[k][sl] for k in ("harm", "bre", "mix")))
        if not P.flagged(c):
            for k in ("harm", "bre", "mix"):
                assert np.array_equal(_bits(got[k][sl]), _bits(host[k][sl])), ("a note without a flag was written", i, k)
    return outs


def judge(label, notes, outs, sr):
    """Every flagged note of the batch against the truth; prints and returns the worst (e_ref, e_gpu) per output."""
    worst = {k: (0.0, 0.0) for k in ("harm", "bre", "mix")}
    bad = []
    for i, (c, out) in enumerate(zip(notes, outs)):
        if not P.flagged(c):
            continue
        ref, truth = P.chain(c, sr), P.chain(c, sr, exact=True)
        for k, g_, r_, t_ in zip(("harm", "bre", "mix"), out, ref, truth):
            assert g_.dtype == F32 and g_.shape == t_.shape
            e_ref, e_gpu = P.errors(g_, r_, t_)
            if e_gpu >= worst[k][1]:
                worst[k] = (e_ref, e_gpu)
            if not P.within(e_ref, e_gpu):
                bad.append((i, c.get("name", c["n"]), k, e_ref, e_gpu))
    print("%-28s" % label + "  ".join("%s e_ref %.2e e_gpu %.2e" % (k, *worst[k]) for k in worst))
    assert not bad, bad
    return worst


# ---------------------------------------------------------------------------------------------
# 1. the cascade's seams
# ---------------------------------------------------------------------------------------------
SHORT_NOTE, SHORT_NOTE_FACTOR = 64, 6.0


@pytest.mark.parametrize("order,btype,f0_mode,cf", P.CASCADE_SETTINGS,
                         ids=["%s%d_mode%d_cf%g" % (s[1][:2], s[0], s[2], s[3]) for s in P.CASCADE_SETTINGS])
def test_cascade_seams(ctx, order, btype, f0_mode, cf):
    """k_onepole_cascade, one ragged launch per setting: note lengths on both sides of the 8-sample lane seam, the 512-sample
    wave seam and the 2048-sample tile, f0 with unvoiced stretches that begin and end on those seams.  Besides the whole
    note, the note's bound is held on the 16 samples around every multiple of 8, 512 and 2048 on their own and the worst
    seam error is reported: a broken carry shows there and nowhere else.

    Two things the measurements decided (docs/HISTORY.md has the figures):
    - the seam windows are held to the NOTE's bound, 3 e_ref(note) + 2^-23.  With e_ref taken over the 9 to 16 samples of the
      window as well, the reference arithmetic's error there is the maximum of a handful of roundings and falls to a
      fraction of its level by chance (3.7e-8 in a window of a note whose e_ref is 8e-7, where both arithmetics carry the
      same 3e-7 from the fp32 alpha): two windows of two settings then fail on device values that equal, in every digit
      printed, the numpy emulation of the kernel's documented arithmetic.
    - notes shorter than SHORT_NOTE samples get the factor SHORT_NOTE_FACTOR for the same reason: the 8-sample note of the
      order-12 high-pass at the 0.45 sr ceiling has e_ref 5.3e-8 where the setting's longer notes have 3.6e-7, and the
      device's 3.2e-7 (again the emulation's value) is 3.8 e_ref + 2^-23.  Notes of 511 samples and more keep the factor 3."""
    sr = 44100
    ctx.plan(sr, 1024, 256)
    xs, f0s = P.cascade_inputs()
    lens = [len(x) for x in xs]
    y = ctx.onepole_cascade(ctx.tensor(np.concatenate(xs)), ctx.tensor(np.concatenate(f0s)), cf, order, btype, f0_mode=f0_mode,
                            lengths=lens).cpu().numpy()
    assert y.dtype == F32
    ref = P.dynamic_filter_batch(xs, f0s, sr, cf, order, btype, f0_mode)
    truth = P.dynamic_filter_batch(xs, f0s, sr, cf, order, btype, f0_mode, exact=True)
    emu = P.dynamic_filter_batch_device(xs, f0s, sr, cf, order, btype, f0_mode)
    off = np.concatenate([[0], np.cumsum(lens)])
    worst, worst_seam, worst_ratio, bad, differ = (0.0, 0.0), {8: (0.0, 0.0), 512: (0.0, 0.0), 2048: (0.0, 0.0)}, {}, [], 0
    for i, n in enumerate(lens):
        g_ = y[off[i]:off[i + 1]]
        factor = 3.0 if n >= SHORT_NOTE else SHORT_NOTE_FACTOR
        e = P.errors(g_, ref[i], truth[i])
        worst = max(worst, e, key=lambda v: v[1])
        differ += int(np.count_nonzero(g_ != emu[i]))
        if e[0] > 0.0:
            k = "short" if n < SHORT_NOTE else "long"
            worst_ratio[k] = max(worst_ratio.get(k, 0.0), (e[1] - P.EPS32) / e[0])
        if not P.within(*e, factor):
            bad.append((n, "note", e))
        for period in (8, 512, 2048):
            es = (e[0], P.errors(g_, ref[i], truth[i], where=P.seam_indices(n, period))[1])
            worst_seam[period] = max(worst_seam[period], es, key=lambda v: v[1])
            if not P.within(*es, factor):
                bad.append((n, period, es))
    print("cascade %s order %2d mode %d cf %-8g note e_ref %.2e e_gpu %.2e  seams " % (btype, order, f0_mode, cf, *worst) +
          "  ".join("%d: %.2e" % (p, worst_seam[p][1]) for p in worst_seam) +
          "  (e_gpu - 2^-23) / e_ref: " + " ".join("%s %.2f" % kv for kv in sorted(worst_ratio.items())) +
          "  samples off the emulated device arithmetic: %d of %d" % (differ, sum(lens)))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 2. note boundaries of the elementwise kernels
# ---------------------------------------------------------------------------------------------
BOUNDARY_NOTES = [(100, 1), (0, 0), (1, 1), (300, 0), (0, 1), (157, 1), (0, 0), (411, 1), (1, 0), (256, 1), (90, 0), (513, 1)]
KINDS = {
    "su": dict(layers=("su",), su_gain=0.5),
    "sj": dict(layers=("sj",), sj_mix=0.3),
    "sa": dict(layers=("sa",), sa_mix=0.3, mix_harm=0.9, mix_breath=1.1, mix_unvoiced=0.9, volume=0.8),
    "fry": dict(fry=True),
    "sd": dict(sd_strength=30.0),
    "st_pos": dict(tension=0.5),
    "st_neg": dict(tension=-0.5),
    "pd_pos": dict(pitch_dyn=0.5),
    "pd_neg": dict(pitch_dyn=-0.5),
    "all": dict(layers=("su", "sj", "sa"), su_gain=0.4, sj_mix=0.3, sa_mix=0.2, fry=True, sd_strength=30.0, tension=0.375,
                pitch_dyn=-0.5, mix_harm=0.9, mix_breath=1.1, mix_unvoiced=0.9, volume=0.8),
}


def _boundary_batch(kind, sr):
    notes = []
    for k, (n, on) in enumerate(BOUNDARY_NOTES):
        kw = dict(KINDS[kind]) if on else {}
        if kw.pop("fry", False):
            kw.update(fry_a=n // 5, fry_b=n - n // 7, fry_fade=int(0.01 * sr))
        notes.append(P.make_note(100 + k, n, sr, **kw))
    return notes


@pytest.mark.parametrize("kind", list(KINDS))
def test_note_boundaries(ctx, kind):
    """Note edges inside a 256-sample block, zero-length notes between others, notes of one sample, flagged and unflagged notes
    alternating inside one block: one flag at a time, then all together."""
    sr = 44100
    ctx.plan(sr, 1024, 256)
    notes = _boundary_batch(kind, sr)
    assert sum(P.flagged(c) for c in notes) == 6
    judge("boundaries " + kind, notes, run_post(ctx, notes), sr)


# ---------------------------------------------------------------------------------------------
# 3. fry ramps
# ---------------------------------------------------------------------------------------------
def test_fry_ramps(ctx):
    """b - a of 1, 2, fade - 1, fade, fade + 1, 2 fade - 1, 2 fade, 2 fade + 1 (one-point ramps, overlapping ramps, ramps that just
    touch), a = 0 and b = n."""
    sr = 44100
    ctx.plan(sr, 1024, 256)
    notes = P.fry_cases(sr)
    judge("fry ramps", notes, run_post(ctx, notes), sr)


# ---------------------------------------------------------------------------------------------
# 4. the sd fade-in
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_fft,hop", GEOMETRIES)
def test_sd_fade_in(ctx, sr, n_fft, hop):
    """The vibrato fades in only when the note is longer than int(0.1 sr): lengths one below, at and one above; a strength at
    which the [0.5, 1.5] clip engages."""
    ctx.plan(sr, n_fft, hop)
    fade = int(0.1 * sr)
    notes = [P.make_note(400 + k, n, sr, sd_strength=s) for k, (n, s) in
             enumerate(((fade - 1, 30.0), (fade, 30.0), (fade + 1, 30.0), (fade + 1, 150.0), (fade - 1, 150.0)))]
    assert np.any(P.vibrato_curve(fade + 1, sr, 150.0, 150.0 / 200.0) == 1.5)
    judge("sd fade-in %d" % sr, notes, run_post(ctx, notes), sr)


# ---------------------------------------------------------------------------------------------
# 5. the st gain
# ---------------------------------------------------------------------------------------------
def test_st_gain(ctx):
    """Tensions whose low-pass order 1 + 4 t lands on 1.5, 2.5 and 3.5 (round half to even), both signs, up to +-1; a silent note
    (both sums zero: gain 1)."""
    sr = 44100
    ctx.plan(sr, 1024, 256)
    notes = [P.make_note(500 + k, 600 + 7 * k, sr, tension=t)
             for k, t in enumerate((0.125, -0.125, 0.375, -0.375, 0.5, -0.5, 0.625, -0.625, 1.0, -1.0))]
    silent = P.make_note(520, 300, sr, amp=0.0, tension=0.5)
    notes.append(silent)
    outs = run_post(ctx, notes)
    assert not np.any(outs[-1][0]) and not np.any(outs[-1][1]) and not np.any(outs[-1][2])
    judge("st gain", notes, outs, sr)


def test_st_sums_do_not_leak_between_notes(ctx):
    """A tension note of 700 samples that starts inside a block, between two unflagged notes 10^3 times louder, another tension
    note sharing its first block: k_note_sumsq reduces the blocks inside the note one way and the blocks it shares another,
    and a sample counted for the wrong note in either moves the gain by orders of magnitude."""
    sr = 44100
    ctx.plan(sr, 1024, 256)
    notes = [P.make_note(530, 300, sr, amp=1000.0), P.make_note(531, 130, sr, tension=0.5),
             P.make_note(532, 700, sr, tension=-0.5), P.make_note(533, 400, sr, amp=1000.0)]
    off = np.cumsum([0] + [c["n"] for c in notes])
    assert off[2] % 256 and off[1] // 256 == off[2] // 256 and (off[3] - 1) // 256 - off[2] // 256 >= 3
    judge("st leak", notes, run_post(ctx, notes), sr)


# ---------------------------------------------------------------------------------------------
# 6. the pd reference level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n_fft,hop", GEOMETRIES)
def test_pd_reference_level(ctx, sr, n_fft, hop):
    """np.percentile(|bend_s|, 95) read through the result: with mask = 1 and pitch_dyn = +-1 the mix is the pre-pd mix times
    the fp32 gain 10^(12 v / 20).  A slow ramp plus noise with the 95 % point a fraction 0.05, 0.3 and 0.8 between two order
    statistics, a plateau that ties them, n = 21 (0.95 * 20 = 19), tiny and block-sized notes, an all-zero and an
    all-negative bend."""
    ctx.plan(sr, n_fft, hop)
    notes = P.pd_cases(sr)
    names = [c["name"] for c in notes]
    assert notes[names.index("plateau_tie")]["level_shift"] == 0.0 and notes[names.index("ramp_frac_0.8")]["level_shift"] > 1e-5
    outs = run_post(ctx, notes)
    zero = notes[names.index("all_zero")]
    assert np.array_equal(outs[names.index("all_zero")][2], P.stage_mix(zero["harm"], zero["uv"], zero["bre"], zero))   # gain 1
    judge("pd level %d" % sr, notes, outs, sr)


# ---------------------------------------------------------------------------------------------
# 7. long Gaussian filters: the chunked taps of k_gauss_samples
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [441.0, 960.0, 1920.0])
def test_long_gaussian_filters(ctx, sigma):
    """More than 2048 taps (two to eight chunks), notes shorter than the radius (several reflections) and longer; each length on
    its own through core.gaussian_filter1d and all as one ragged batch, where the blocks inside a note and the blocks across
    notes take different paths."""
    from goofer_amd import core
    from oracle import goofer_ref as R
    rng = np.random.default_rng(int(sigma))
    lens = [1, 7, 300, 1763, 1764, 1765, 4097, 20000]
    xs = [rng.standard_normal(n) for n in lens]
    refs = [R.gauss1d(x, sigma) for x in xs]
    assert 2 * int(4.0 * sigma + 0.5) + 1 > 2048
    worst = 0.0
    for x, ref in zip(xs, refs):
        got = core.gaussian_filter1d(x, sigma, ctx=ctx)
        assert got.dtype == np.float64 and got.shape == ref.shape
        worst = max(worst, float(np.max(np.abs(got - ref))))
    rag = ctx.gauss_rows_f64(ctx.tensor(np.concatenate(xs)), core.gaussian_taps(sigma, 4.0), lengths=lens).cpu().numpy()
    worst_rag = float(np.max(np.abs(rag - np.concatenate(refs))))
    print("gauss sigma %g: single %.2e  ragged %.2e" % (sigma, worst, worst_rag))
    assert worst < 1e-13 and worst_rag < 1e-13
