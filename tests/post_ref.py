"""The sample-domain post chain of one note (csrc/post.hip: the su / sj layers, the vf fry blend, sd, st, the V/B/U mix, the sa
blend and the pd gain) restated in plain numpy, one function per stage, in two arithmetics.  TEST INFRASTRUCTURE ONLY.

Written from this project's own oracle: ``oracle/sampler_ref.py`` (``dynamic_filter``, the ``fry_mask`` and ``dyn_gain`` blocks
of ``assemble``, the post part of ``render``) and ``oracle/goofer_ref.py`` (``rms``, ``gauss1d``, ``volume_jitter_curve``).

Every function takes ``exact``:

``exact=False``  the REFERENCE ARITHMETIC: fp32 wherever the reference holds fp32.  The cascade's ``alpha`` is rounded to fp32 and
    every step of its recurrence is an fp32 operation (so each section's output is an fp32 array), the 5-tap box runs on fp32,
    the fry mask is an fp32 array multiplied by fp64 ramps, ``np.mean(np.square(fp32))`` is what numpy makes of it, the ``dyn``
    curve is fp64.  ``post_chain(exact=False)`` equals ``oracle.sampler_ref.render`` bit for bit in every stage
    (tests/test_post_ref.py); no stage needed the one-ulp allowance.  Scalars are used as they are handed in, which matters
    under numpy >= 2: an fp32 array times an ``np.float64`` scalar is an fp64 array there, times a Python float an fp32 one.
    The oracle carries V / su / sj / sa as ``np.float64`` (``np.clip(..) / 100.0``), so tests/test_post_ref.py hands over the
    oracle's own objects and follows it either way; tests/test_gpu_post_chain.py hands over Python floats, which keeps these
    products in fp32: the arithmetic of the reference under value-based casting, and the one the kernels implement.
``exact=True``   the TRUTH: the same fp32 inputs, every operation after them in float64 with no intermediate rounding
    (``alpha``, the sections' outputs, the fry mask, the pd gain all stay fp64); ``np.percentile`` stays the definition.

The recurrences are numpy loops over time, vectorised ACROSS notes (``cascade``): a ragged batch of notes costs what its longest
note costs, which is what keeps the GPU tests that are judged against the truth quick.
"""
import numpy as np

F32, F64 = np.float32, np.float64

NOTE_FIELDS = ("su_gain", "sj_mix", "sa_mix", "sd_strength", "tension", "pitch_dyn", "fry_a", "fry_b", "fry_fade")
MIX_FIELDS = ("mix_harm", "mix_breath", "mix_unvoiced", "volume")


def _dt(exact):
    return F64 if exact else F32


def _arr(x, exact):
    """The truth starts from the fp32 inputs in float64; the reference arithmetic keeps every array as numpy made it."""
    return np.asarray(x, dtype=F64) if exact else np.asarray(x)


# ---------------------------------------------------------------------------------------------
# dynamic_butter_filter: cascades of time-varying one-pole sections
# ---------------------------------------------------------------------------------------------
def f0_reference(f0, f0_mode):
    """What the cascade kernel reads as f0: 0 the note's f0, 1 max(f0, 120) (the su / sj layers), 2 all ones (the fry)."""
    f0 = np.asarray(f0, dtype=F32)
    return f0 if f0_mode == 0 else (np.maximum(f0, F32(120.0)) if f0_mode == 1 else np.ones_like(f0))


def section_alpha(f0, sr, cutoff_factor, btype, exact=False):
    """Per-sample coefficient of every section: cutoff_factor * (5-tap box over the edge-padded f0), the bare factor where that
    is not positive, clamped to [60 Hz low-pass | 20 Hz high-pass, 0.45 sr]."""
    dt = _dt(exact)
    f0 = np.asarray(f0, dtype=F32).astype(dt)
    if np.any(f0 > 0):
        f0s = np.convolve(np.pad(f0, (2, 2), mode="edge"), np.ones(5, dtype=dt) / 5, mode="valid")
    else:
        f0s = f0
    f0s = np.asarray(f0s, dtype=dt)
    cf = dt(cutoff_factor)
    fc = np.where(f0s > 0.0, f0s * cf, cf).astype(dt)
    fc = np.maximum(fc, dt(60.0 if btype == "lowpass" else 20.0))
    fc = np.minimum(fc, dt(0.45 * sr))
    w = (2.0 * np.pi) * fc.astype(F64)
    return ((w / (w + sr)) if btype == "lowpass" else (sr / (w + sr))).astype(dt)


def cascade(xs, alphas, orders, btype, exact=False):
    """``orders[r]`` one-pole sections over note ``xs[r]`` with coefficients ``alphas[r]``, all notes side by side.
    low-pass:  y_i = y_{i-1} + a_i (x_i - y_{i-1});  high-pass:  y_i = a_i ((y_{i-1} + x_i) - x_{i-1}),  y_{-1} = 0 and, for the
    high-pass, x_{-1} = x_0: the first difference of every section is zero."""
    dt = _dt(exact)
    R = len(xs)
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    L = int(lens.max()) if R else 0
    Y = np.zeros((L, R), dtype=dt)
    A = np.zeros((L, R), dtype=dt)
    for r in range(R):
        Y[:lens[r], r] = np.asarray(xs[r], dtype=dt)
        A[:lens[r], r] = np.asarray(alphas[r], dtype=dt)
    orders = np.maximum(1, np.asarray(orders, dtype=np.int64))
    hp = btype != "lowpass"
    for s in range(int(orders.max()) if R else 0):
        live = orders > s
        X = Y.copy()
        yp = np.zeros(R, dtype=dt)
        prev = X[0].copy()
        for i in range(L):
            a, xp = A[i], X[i]
            if hp:
                yp = a * ((yp + xp) - prev)
                prev = xp
            else:
                yp = yp + a * (xp - yp)
            Y[i] = yp
        Y[:, ~live] = X[:, ~live]
    return [Y[:lens[r], r].copy() for r in range(R)]


def dynamic_filter(signal, f0, sr, cutoff_factor, order=4, btype="lowpass", exact=False):
    x = np.asarray(signal, dtype=_dt(exact))
    if len(x) == 0:
        return x
    alpha = section_alpha(f0, sr, cutoff_factor, btype, exact)
    return cascade([x], [alpha], [order], btype, exact)[0]


def dynamic_filter_batch(signals, f0s, sr, cutoff_factor, order, btype, f0_mode=0, exact=False):
    """One cascade setting over a ragged batch (what one launch of the cascade kernel does)."""
    alphas = [section_alpha(f0_reference(f, f0_mode), sr, cutoff_factor, btype, exact) for f in f0s]
    return cascade(signals, alphas, [order] * len(signals), btype, exact)


def dynamic_filter_batch_device(signals, f0s, sr, cutoff_factor, order, btype, f0_mode=0):
    """The arithmetic k_onepole_cascade documents, emulated: the reference's fp32 alpha, every section's recurrence in fp64,
    every section's output rounded to fp32.  (The kernel composes the steps of a tile as a scan, not in sequence, so a
    rounding may fall the other way now and then: the tests print how far the device is from this, they do not assert it.)"""
    alphas = [section_alpha(f0_reference(f, f0_mode), sr, cutoff_factor, btype).astype(F64) for f in f0s]
    ys = [np.asarray(x, dtype=F32) for x in signals]
    for _ in range(max(1, int(order))):
        ys = [y.astype(F32) for y in cascade(ys, alphas, [1] * len(ys), btype, exact=True)]
    return ys


# ---------------------------------------------------------------------------------------------
# small pieces
# ---------------------------------------------------------------------------------------------
def rms(x):
    return float(np.sqrt(np.mean(np.square(x)) + 1e-12))


def gauss_taps(sigma, truncate=4.0):
    r = int(truncate * sigma + 0.5)
    if r <= 0:
        return None, 0
    t = np.arange(-r, r + 1)
    k = np.exp(-0.5 * (t / sigma) ** 2)
    return k / k.sum(), r


def gauss1d(a, sigma):
    """1-D Gaussian FIR with numpy 'reflect' padding, fp64 whatever the input (the same in both arithmetics)."""
    a = np.asarray(a)
    k, r = gauss_taps(sigma) if sigma > 0.0 else (None, 0)
    if a.size == 0 or k is None:
        return a.copy()
    pad = np.pad(a, (r, r), mode="reflect")
    if k.size > 64:
        return np.convolve(pad, k, mode="valid")
    out = np.zeros(a.shape, dtype=F64)
    for j in range(k.size):
        out += k[j] * pad[j:j + a.size]
    return out


def ramp(start, stop, m):
    """The fades of the fry mask: both ends included."""
    return np.linspace(start, stop, m, endpoint=True)


def fry_mask(n, a, b, fade, exact=False):
    """1 on [a, b), 0 elsewhere, a linear fade of ``fade`` samples in at ``a`` and out at ``b`` (the two overlap on short ranges)."""
    if not b > a:
        return None
    m = np.zeros(n, dtype=_dt(exact))
    m[a:b] = 1.0
    if fade > 0:
        a1 = min(b, a + fade)
        if a1 > a:
            m[a:a1] *= ramp(0.0, 1.0, a1 - a)
        b0 = max(a, b - fade)
        if b > b0:
            m[b0:b] *= ramp(1.0, 0.0, b - b0)
    return m


def vibrato_curve(n, sr, speed, strength):
    """volume_jitter_curve(vibrato=True): zero-phase sinusoid, 0.1 s fade-in when the note is longer than that, clip [0.5, 1.5]."""
    t = np.arange(n) / sr
    z = np.sin(2 * np.pi * speed * t + 0)
    fade = int(0.1 * sr)
    if fade < n:
        z[:fade] *= np.linspace(0, 1, fade)
    return np.clip(1.0 + z * strength, 0.5, 1.5)


def percentile95(x):
    """The pd reference level: linear interpolation between the two order statistics around 0.95 (n - 1)."""
    return float(np.percentile(x, 95))


def dyn_gain(bend, mask, pitch_dyn, sr, exact=False):
    """pd: 10^(12 |pd| clip(bend_s / ref, -1, 1) / 20), fp32 and clipped in the reference, blended in by the smoothed mask."""
    bend_s = gauss1d(np.asarray(bend, dtype=F32), max(1, int(0.010 * sr)))
    ref = percentile95(np.abs(bend_s)) + 1e-8
    v = np.clip(bend_s / ref, -1.0, 1.0)
    db = (12.0 * abs(pitch_dyn)) * (v if pitch_dyn > 0 else -v)
    g = np.clip(np.power(10.0, db / 20.0).astype(_dt(exact)), 1e-3, 1e3)
    return 1.0 + (g - 1.0) * gauss1d(np.asarray(mask, dtype=F32), int(0.01 * sr))


# ---------------------------------------------------------------------------------------------
# the stages, in the reference's order
# ---------------------------------------------------------------------------------------------
def stage_layers(harm, su_harm, sj_harm, f0, su_gain, sj_mix, sr, exact=False):
    harm = _arr(harm, exact).copy()
    ref_f0 = f0_reference(f0, 1)

    def hp_pair(x):
        x = dynamic_filter(x, ref_f0, sr, 1.0, 6, "highpass", exact)
        return dynamic_filter(x, ref_f0, sr, 1.0, 6, "highpass", exact)

    if su_harm is not None:
        harm += hp_pair(su_harm) * su_gain
    if sj_harm is not None:
        harm = (1.0 - sj_mix) * harm + sj_mix * hp_pair(sj_harm)
    return harm


def stage_fry(harm, bre, a, b, fade, sr, exact=False):
    harm, bre = _arr(harm, exact), _arr(bre, exact)
    fmk = fry_mask(len(harm), a, b, fade, exact)
    if fmk is None:
        return harm, bre
    ones = np.ones(len(harm), dtype=F32)
    h_hp = dynamic_filter(harm, ones, sr, 200, 6, "highpass", exact)
    b_hp = dynamic_filter(bre, ones, sr, 200, 6, "highpass", exact)
    return harm * (1.0 - fmk) + h_hp * fmk, bre * (1.0 - fmk) + b_hp * fmk


def stage_sd(bre, mask, sd_strength, sr, exact=False):
    bre = _arr(bre, exact).copy()
    if sd_strength > 0:
        j = vibrato_curve(len(bre), sr, 150.0, sd_strength / 200.0)
        bre *= 1.0 + (j - 1.0) * gauss1d(np.asarray(mask, dtype=F32).astype(float), 20)
        bre *= 1.0 + (sd_strength / 100.0) * 10
    return bre


def stage_tension(harm, bre, f0, tension, sr, exact=False):
    harm, bre = _arr(harm, exact).copy(), _arr(bre, exact).copy()
    if tension == 0:
        return harm, bre
    before = rms(harm + bre)
    t = abs(tension)
    if tension < 0:
        order = np.clip(int(np.round(1 + (t * 4))), 1, 6)
        harm = dynamic_filter(harm, f0, sr, 2.0 - t * 0.75, order, "lowpass", exact)
        bre = dynamic_filter(bre, f0, sr, t, 4, "highpass", exact)
    else:
        hi = dynamic_filter(harm, f0, sr, t * 4, 4, "highpass", exact)
        harm += hi * (1.0 + t * 20.0)
        bre = dynamic_filter(bre, f0, sr, (2.0 - t) / 0.5, 6, "lowpass", exact)
        bre *= (1.0 - t)
    after = rms(harm + bre)
    if after > 0:
        harm *= before / after
        bre *= before / after
    return harm, bre


def stage_mix(harm, uv, bre, mix, sa_uv=None, sa_bre=None, sa_mix=0.0, dyn=None, exact=False):
    harm, uv, bre = (_arr(v, exact) for v in (harm, uv, bre))
    out = ((harm * mix["mix_harm"] + bre * mix["mix_breath"]) + uv * mix["mix_unvoiced"]) * mix["volume"]
    if sa_uv is not None:
        out = out * (1.0 - sa_mix) + ((_arr(sa_uv, exact) + _arr(sa_bre, exact)) * mix["volume"]) * sa_mix
    if dyn is not None:
        out = out * dyn
    return out


def post_chain(harm, uv, bre, f0, mask, bend, note, mix, sr, su_harm=None, sj_harm=None, sa_uv=None, sa_bre=None, exact=False):
    """One note through the whole chain.  ``note``: the goofer_post_note fields (NOTE_FIELDS), ``mix``: MIX_FIELDS; a layer is on
    when its stem is given.  Returns (harm', bre', mix): fp32 arrays in the reference arithmetic, except that the pd gain makes
    the mix fp64 like the reference's; fp64 arrays in the exact one."""
    harm = stage_layers(harm, su_harm, sj_harm, f0, note["su_gain"], note["sj_mix"], sr, exact)
    harm, bre = stage_fry(harm, bre, note["fry_a"], note["fry_b"], note["fry_fade"], sr, exact)
    bre = stage_sd(bre, mask, note["sd_strength"], sr, exact)
    harm, bre = stage_tension(harm, bre, f0, note["tension"], sr, exact)
    dyn = dyn_gain(bend, mask, note["pitch_dyn"], sr, exact) if note["pitch_dyn"] != 0 else None
    out = stage_mix(harm, uv, bre, mix, sa_uv, sa_bre, note["sa_mix"], dyn, exact)
    return harm, bre, out


def note_fields(**kw):
    d = dict(su_gain=0.0, sj_mix=0.0, sa_mix=0.0, sd_strength=0.0, tension=0.0, pitch_dyn=0.0, fry_a=0, fry_b=0, fry_fade=0)
    d.update(kw)
    return d


def mix_fields(**kw):
    d = dict(mix_harm=1.0, mix_breath=1.0, mix_unvoiced=1.0, volume=1.0)
    d.update(kw)
    return d


# ---------------------------------------------------------------------------------------------
# the judgement of tests/test_gpu_post_chain.py
# ---------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -23


def errors(got, ref32, truth, where=None):
    """(e_ref, e_got): the largest per-sample distance of the reference arithmetic and of ``got`` from the truth, over the
    peak of the note's truth.  ``where``: an index array restricting the maxima (the peak stays the whole note's)."""
    truth = np.asarray(truth, dtype=F64)
    if truth.size == 0:
        return 0.0, 0.0
    peak = max(float(np.max(np.abs(truth))), float(np.finfo(F32).tiny))
    d_ref = np.abs(np.asarray(ref32, dtype=F64) - truth)
    d_got = np.abs(np.asarray(got, dtype=F64) - truth)
    if where is not None:
        if len(where) == 0:
            return 0.0, 0.0
        d_ref, d_got = d_ref[where], d_got[where]
    return float(d_ref.max()) / peak, float(d_got.max()) / peak


def within(e_ref, e_got, factor=3.0):
    """The bound every stage is held to: three times the reference arithmetic's own error plus one fp32 rounding of the result."""
    return e_got <= factor * e_ref + EPS32


# ---------------------------------------------------------------------------------------------
# seeded inputs shared by tests/test_gpu_post_chain.py and the mutation checks of tests/test_post_ref.py
# ---------------------------------------------------------------------------------------------
def stems(seed, n, sr, amp=1.0):
    """(harm, uv, bre) fp32: a 0.3-amplitude sine plus a little noise, and two noise stems."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    harm = 0.3 * np.sin(2 * np.pi * (180.0 + 7.0 * (seed % 9)) * t + rng.uniform(0.0, 2 * np.pi)) + 0.02 * rng.standard_normal(n)
    uv, bre = 0.02 * rng.standard_normal(n), 0.05 * rng.standard_normal(n)
    return tuple((amp * v).astype(F32) for v in (harm, uv, bre))


def f0_track(seed, n):
    """fp32 f0 around 210 Hz with unvoiced (zero) stretches whose edges sit on the cascade's 512- and 2048-sample seams."""
    i = np.arange(n)
    f0 = 210.0 + 40.0 * np.sin(i / 97.0 + seed)
    for a, b in ((3, 5), (300, 512), (2048, 2100), (4090, 4096)):
        f0[a:b] = 0.0
    return f0.astype(F32)


def make_note(seed, n, sr, amp=1.0, voiced=False, layers=(), **fields):
    """One note's inputs as a dict: stems, f0 / mask / bend, the stems of the ``layers`` asked for ("su", "sj", "sa"), the
    goofer_post_note fields and the mix parameters (every scalar a Python float that fp32 holds exactly)."""
    harm, uv, bre = stems(seed, n, sr, amp)
    f0 = np.full(n, 220.0, dtype=F32) if voiced else f0_track(seed, n)
    rng = np.random.default_rng(seed + 77)
    d = dict(n=n, harm=harm, uv=uv, bre=bre, f0=f0, mask=(f0 > 0).astype(F32),
             bend=(np.linspace(-0.3, 0.6, n) + 0.2 * rng.standard_normal(n)).astype(F32),
             su_harm=None, sj_harm=None, sa_uv=None, sa_bre=None)
    if "su" in layers:
        d["su_harm"] = stems(seed + 1000, n, sr)[0]
    if "sj" in layers:
        d["sj_harm"] = stems(seed + 2000, n, sr)[0]
    if "sa" in layers:
        _, d["sa_uv"], d["sa_bre"] = stems(seed + 3000, n, sr)
    d.update(note_fields())
    d.update(mix_fields())
    d.update({k: (v if isinstance(v, (int, np.integer)) else float(F32(v))) for k, v in fields.items()})
    return d


def chain(note, sr, exact=False):
    """post_chain on a make_note dict."""
    return post_chain(note["harm"], note["uv"], note["bre"], note["f0"], note["mask"], note["bend"],
                      {k: note[k] for k in NOTE_FIELDS}, {k: note[k] for k in MIX_FIELDS}, sr,
                      su_harm=note["su_harm"], sj_harm=note["sj_harm"], sa_uv=note["sa_uv"], sa_bre=note["sa_bre"], exact=exact)


def flagged(note):
    """What goofer_post_batch looks at to decide that a note takes part in the chain."""
    return bool(note["n"] > 0 and (note["su_harm"] is not None or note["sj_harm"] is not None or note["sa_uv"] is not None or
                                   note["fry_a"] < note["fry_b"] or note["sd_strength"] > 0 or note["tension"] != 0 or
                                   note["pitch_dyn"] != 0))


CASCADE_LENGTHS = [1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 6145]
# (order, btype, f0_mode, cutoff factor): every order, both types and every f0 mode; with f0 around 210 Hz (1 Hz in mode 2) the
# factors reach the floor (20 Hz high-pass, 60 Hz low-pass), the 0.45 sr ceiling and the range between, and the unvoiced
# stretches (fc = the bare factor) switch between them inside a note.
CASCADE_SETTINGS = [
    (1, "highpass", 0, 0.05), (4, "highpass", 0, 1.0), (6, "highpass", 2, 200.0), (12, "highpass", 1, 1.0),
    (4, "highpass", 0, 400.0), (6, "highpass", 1, 0.01), (12, "highpass", 2, 30000.0),
    (1, "lowpass", 0, 0.1), (4, "lowpass", 0, 1.25), (6, "lowpass", 0, 3.0), (12, "lowpass", 1, 2.0),
    (6, "lowpass", 2, 1000.0), (4, "lowpass", 2, 1e6), (12, "lowpass", 0, 0.2),
]


def cascade_inputs():
    xs = [stems(40 + k, n, 44100)[0] for k, n in enumerate(CASCADE_LENGTHS)]
    return xs, [f0_track(k, n) for k, n in enumerate(CASCADE_LENGTHS)]


def seam_indices(n, period):
    """The 16 samples around every multiple of ``period`` inside a note of n samples."""
    i = np.arange(n)
    r = i % period
    return i[((r < 8) | (r >= period - 8)) & (i + 8 >= period)]


def fry_cases(sr):
    """Fry ranges whose two fades are one-point ramps, overlap, just touch and stay apart; ranges from 0 and up to n."""
    fade = int(0.01 * sr)
    out = []
    for k, d in enumerate((1, 2, fade - 1, fade, fade + 1, 2 * fade - 1, 2 * fade, 2 * fade + 1)):
        out.append(make_note(300 + k, d + 300, sr, fry_a=150, fry_b=150 + d, fry_fade=fade))
    out.append(make_note(310, 3 * fade, sr, fry_a=0, fry_b=2 * fade + 57, fry_fade=fade))
    out.append(make_note(311, 3 * fade, sr, fry_a=fade - 30, fry_b=3 * fade, fry_fade=fade))
    out.append(make_note(312, fade + 9, sr, fry_a=0, fry_b=fade + 9, fry_fade=fade))
    return out


def pd_cases(sr):
    """mask = 1 and pitch_dyn = +-1, so the mix is the pre-pd mix times the fp32 gain and shows the reference level.
    ``level_shift``: how far, relative to the level, the 95 % point lies above the order statistic below it: what dropping
    the interpolation would move the level by."""
    sigma = max(1, int(0.010 * sr))
    r = int(4.0 * sigma + 0.5)
    rng = np.random.default_rng(611)
    bends = []

    def noisy(n):
        return np.linspace(-0.3, 0.6, n) + 0.2 * rng.standard_normal(n)

    bends.append(("ramp_frac_0.05", noisy(5000)))             # 0.95 * 4999 = 4749.05
    bends.append(("ramp_frac_0.8", noisy(4005)))              # 0.95 * 4004 = 3803.8
    bends.append(("ramp_frac_0.3", noisy(3015)))              # 0.95 * 3014 = 2863.3
    n_tie = 22 * r + 2500                                     # a plateau wider than the filter: equal smoothed values around the
    tie = np.full(n_tie, 0.5)                                 # 95 % point, larger ones above them
    tie[:16 * r] = 0.1 + 0.05 * np.sin(np.arange(16 * r) / 50.0)
    tie[-100:] = 0.9
    bends.append(("plateau_tie", tie))
    bends.append(("n21", noisy(21)))                          # 0.95 * 20 = 19: no interpolation to do
    for n in (1, 2, 3, 255, 256, 257):
        bends.append(("n%d" % n, noisy(n)))
    bends.append(("all_zero", np.zeros(300)))
    bends.append(("all_negative", -(0.2 + np.abs(noisy(700)))))
    out = []
    for k, (name, bend) in enumerate(bends):
        c = make_note(600 + k, len(bend), sr, voiced=True, pitch_dyn=1.0 if k % 2 == 0 else -1.0)
        c["bend"] = bend.astype(F32)
        c["name"] = name
        s = np.sort(np.abs(gauss1d(c["bend"], sigma)))
        v = 0.95 * (len(s) - 1)
        k_lo = int(np.floor(v))
        c["level_shift"] = float((np.percentile(s, 95) - s[k_lo]) / max(s[k_lo], 1e-300))
        out.append(c)
    return out
