"""The synthesis core of one note (gf.synthesize behind the pulse train: csrc/binops.hip k_harm_shape / k_noise_spectra, csrc/fft.hip,
csrc/samples.hip, csrc/stems.hip) restated in plain numpy, stage by stage, in two arithmetics.  TEST INFRASTRUCTURE ONLY.

Written from this project's own oracle, ``oracle/goofer_ref.py`` (``synthesize`` and what it calls).

``synth_note(case, geo, exact=...)`` returns the named stages of one note:

``exact=False``  the REFERENCE ARITHMETIC: the oracle's own numpy expressions in the oracle's order, so fp32 / complex64 wherever
    numpy's promotion leaves the oracle fp32 / complex64.  ``rec, harm, uv, bre, pulse, mag, peak, mask_smooth, hp, env, env_noise``
    equal ``oracle.goofer_ref.synthesize(..., phi=..., return_parts=True)`` bit for bit (tests/test_synth_ref.py).
``exact=True``   the TRUTH: the same fp32 inputs and fp32 tables (window, bin frequencies, boost and brightness curves), every value
    operation after them in float64 / complex128 with no intermediate rounding.  What the reference defines as data or as a decision
    stays the reference's: the frame picks, ``voiced = pick > 0``, ``match_env_frames``, the ``> 1e-9`` test on the fp32 window
    sum, the fp32 ``linspace`` grids of ``smooth_mask``, the anchors and segments of the formant warp (``np.interp`` on the
    reference's abscissae), T, the padding mode, the zero tail.  ``f0`` is the single fp32 product in both.
``fft="plain"`` (with ``exact=False``): the transforms of the reference arithmetic replaced by a plain radix-2 decimation-in-time
    transform whose twiddles and butterflies are rounded to complex64 (chirp-z over it for sizes that are no power of two).
    numpy's fp32 pocketfft is about four times more accurate than an honest fp32 Cooley-Tukey, so a bound built on it alone would
    refuse a correct fp32 kernel: for the stages that hold a transform E_ref is the larger of the two.

The pulse train is an INPUT of both arithmetics (``pulse=``; the oracle's own when None): an ulp of f0 moves an onset by a sample,
and tests/test_gpu_kernels.py owns the pulse.  ``given`` = {stage: array} replaces a stage by what is handed in (the device's
output), so that the stages behind it are judged on their own error: ``env_harm``, ``S_harm`` (as k_harm_shape leaves it: the
high-passed, enveloped, boosted, brightened spectrum WITHOUT the 1 / mag, which the kernels apply behind the overlap-add),
``note_mag``, ``S_uv``, ``S_breath``, ``mask_short``; and, for tests that plant a fault into a stage, ``hp``, ``env_noise``,
``mask_smooth``, ``harm_pre`` (the harmonic stem in front of the peak gain).

Stages (device layout: one row per frame): f0, pulse, env_harm [T, bins] (the warped envelope row of every frame),
env_noise [T, bins], S_harm, note_mag, S_uv, S_breath, frames [T, n_fft] (windowed harmonic time frames, unnormalised),
mask_short (float64 knots), mask_smooth, harm / uv / bre, note_peak, rec, mix — and ``gain_uv`` / ``gain_bre``, the per-sample stem
gains (1 - ms) uv_strength and ms breath_strength before the peak gain.  In the oracle's layout, as it returns them: hp and env
[bins, T].  ``S_harm_unblurred`` / ``S_breath_unblurred``: the spectra in front of the sigma-0.5 bin blur.
"""
import numpy as np

from oracle import goofer_ref as R

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
EPS32 = 2.0 ** -23
MASK_DS = 4

ORACLE_PARTS = ("pulse", "mag", "peak", "mask_smooth", "hp", "env", "env_noise")


# ---------------------------------------------------------------------------------------------
# the plain fp32 transform
# ---------------------------------------------------------------------------------------------
def _bitrev(n):
    bits = n.bit_length() - 1
    idx = np.arange(n)
    out = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        out |= ((idx >> b) & 1) << (bits - 1 - b)
    return out


def fft_r2(x, inverse=False):
    """Radix-2 decimation-in-time transform along axis 0 (a power of two), unscaled: twiddles rounded to complex64, every
    butterfly a complex64 product and a complex64 sum."""
    x = np.asarray(x, dtype=C64)
    n = x.shape[0]
    assert n & (n - 1) == 0
    a = x[_bitrev(n)].reshape(n, -1)
    cols = a.shape[1]
    m = 2
    while m <= n:
        half = m // 2
        tw = np.exp((2j if inverse else -2j) * np.pi * np.arange(half) / m).astype(C64)
        a = a.reshape(n // m, m, cols)
        u, t = a[:, :half], a[:, half:] * tw[None, :, None]
        a = np.concatenate([u + t, u - t], axis=1)
        assert a.dtype == C64
        m *= 2
    return a.reshape(x.shape)


def fft_plain(x, inverse=False):
    """fft_r2, or for other sizes Bluestein's chirp-z over it (chirp rounded to complex64)."""
    x = np.asarray(x, dtype=C64)
    n = x.shape[0]
    if n & (n - 1) == 0:
        return fft_r2(x, inverse)
    L = 1 << (2 * n - 1).bit_length()
    k = np.arange(n, dtype=np.int64)
    w = np.exp((1j if inverse else -1j) * np.pi * ((k * k) % (2 * n)) / n).astype(C64)
    shp = (-1,) + (1,) * (x.ndim - 1)
    a = np.zeros((L,) + x.shape[1:], dtype=C64)
    a[:n] = x * w.reshape(shp)
    b = np.zeros(L, dtype=C64)
    b[:n] = np.conj(w)
    b[L - n + 1:] = np.conj(w[1:][::-1])
    conv = fft_r2(fft_r2(a) * fft_r2(b).reshape(shp), inverse=True) * F32(1.0 / L)
    return (conv[:n] * w.reshape(shp)).astype(C64)


def rfft_plain(frames):
    n = frames.shape[0]
    return fft_plain(np.asarray(frames, dtype=F32).astype(C64))[:n // 2 + 1]


def irfft_plain(S, n):
    S = np.asarray(S, dtype=C64).copy()
    S[0] = S[0].real
    S[n // 2] = S[n // 2].real
    full = np.concatenate([S, np.conj(S[1:n // 2][::-1])], axis=0)
    return (fft_plain(full, inverse=True).real * F32(1.0 / n)).astype(F32)


# ---------------------------------------------------------------------------------------------
# pieces, each in both arithmetics
# ---------------------------------------------------------------------------------------------
def _rfft(frames, exact, fft):
    if exact:
        return np.fft.rfft(np.asarray(frames, dtype=F64), axis=0)
    return rfft_plain(frames) if fft == "plain" else np.fft.rfft(frames, axis=0)


def _irfft(S, n_fft, exact, fft):
    if exact:
        return np.fft.irfft(np.asarray(S, dtype=C128), axis=0, n=n_fft)
    S = np.asarray(S, dtype=C64)
    return irfft_plain(S, n_fft) if fft == "plain" else np.fft.irfft(S, axis=0, n=n_fft).astype(F32)


def window_sum32(win, n_fft, hop, T):
    """The reference's fp32 summed squared window, frame-major (overlap_add): what its > 1e-9 test looks at."""
    ws = np.zeros(n_fft + hop * (T - 1), dtype=F32)
    w2 = win * win
    for i in range(T):
        ws[i * hop:i * hop + n_fft] += w2
    return ws


def overlap_add(frames, win, hop, exact):
    """[n_fft, T] frames -> the n_fft + hop (T - 1) samples of the normalised overlap-add."""
    n_fft, T = frames.shape
    full = n_fft + hop * (T - 1)
    if not exact:
        return R.overlap_add(frames, win, hop, full)
    w = win.astype(F64)
    y, ws = np.zeros(full), np.zeros(full)
    for i in range(T):
        y[i * hop:i * hop + n_fft] += frames[:, i] * w
        ws[i * hop:i * hop + n_fft] += w * w
    ok = window_sum32(win, n_fft, hop, T) > 1e-9
    y[ok] /= ws[ok]
    return y


def istft(S, win, hop, length, exact, fft):
    """R.istft: inverse transform, overlap-add, drop n_fft / 2 either side, zero tail up to ``length``."""
    n_fft = (S.shape[0] - 1) * 2
    frames = _irfft(S, n_fft, exact, fft)
    h = n_fft // 2
    full = n_fft + hop * (frames.shape[1] - 1)
    y = overlap_add(frames, win, hop, exact)[h:full - h]
    return np.pad(y, (0, length - y.shape[0])) if y.shape[0] < length else y[:length]


def warp_formants(env, orig, shifted, sr, exact):
    """R.warp_env_by_formants; the truth keeps the interpolated rows in float64."""
    if not exact:
        return R.warp_env_by_formants(env, orig, shifted, sr)
    nyq = sr / 2.0
    f = np.linspace(0.0, nyq, env.shape[0])
    out = np.zeros(env.shape, dtype=F64)
    for t in range(env.shape[1]):
        src, dst = [0.0], [0.0]
        for i in range(4):
            fo, fs = orig[i, t], shifted[i, t]
            if fo > 50.0 and fo < nyq and fs > 50.0:
                src.append(fo)
                dst.append(fs)
        src.append(nyq)
        dst.append(nyq)
        wf = R.LinInterp(np.array(dst), np.array(src))(f)
        out[:, t] = R.LinInterp(f, env[:, t])(wf)
    return out


def shift_formants(env, ratio, sr, exact):
    if not exact:
        return R.shift_formants(env, ratio, sr)
    f = np.linspace(0, sr / 2, env.shape[0])
    q = np.clip(f / ratio, 0, sr / 2)
    out = np.zeros(env.shape, dtype=F64)
    for t in range(env.shape[1]):
        out[:, t] = R.LinInterp(f, env[:, t])(q)
    return out


def highpass(freqs, f0_frames, exact):
    if not exact:
        return R.highpass_mask(freqs, f0_frames)
    return R.highpass_mask(freqs.astype(F64), f0_frames.astype(F64))


def brighten(S, voiced, curve, exact, blur=True):
    """R._voiced_brighten: * curve then the sigma-0.5 five-tap bin blur on the frames whose picked mask is > 0.
    ``blur=False`` (a copy): the curve alone, which is where a test that wants another blur starts from."""
    if not exact and blur:
        return R._voiced_brighten(S, voiced, curve)
    cols = np.nonzero(voiced > 0)[0]
    if not blur:
        S = S.copy()
    if cols.size:
        blk = S[:, cols] * (curve.astype(F64) if exact else curve)[:, None]
        S[:, cols] = R.gauss2d(blk, (0.5, 0)) if blur else blk
    return S


def mask_knots(mask, sigma, exact=False):
    """The smoothed decimated mask (float64 in both arithmetics); the truth accumulates the taps in long double."""
    short = np.asarray(mask)[::MASK_DS].astype(F32)
    s = max(1.0, sigma / MASK_DS)
    if not exact:
        return R.gauss1d(short, s)
    k, r = R.gauss_taps(s)
    pad = np.pad(short, (r, r), mode="reflect").astype(np.longdouble)
    kl = k.astype(np.longdouble)
    if short.size * k.size <= 1 << 22:
        win = np.lib.stride_tricks.sliding_window_view(pad, k.size)
        return (win * kl[None, :]).sum(axis=1).astype(F64)
    out = np.zeros(short.size, dtype=np.longdouble)
    for j in range(k.size):
        out += kl[j] * pad[j:j + short.size]
    return out.astype(F64)


def mask_upsample(knots, n, exact, at=None):
    """smooth_mask's linear upsample on the fp32 linspace grids; ``at``: other abscissae."""
    xo = np.linspace(0.0, 1.0, num=knots.size, dtype=F32)
    xn = np.linspace(0.0, 1.0, num=n, dtype=F32) if at is None else at
    out = R.LinInterp(xo, knots)(xn)
    return out if exact else out.astype(F32)


# ---------------------------------------------------------------------------------------------
# one note
# ---------------------------------------------------------------------------------------------
KW_DEFAULT = dict(pitch_shift=1.0, formant_shift=1.0, F1_shift=1.0, F2_shift=1.0, F3_shift=1.0, F4_shift=1.0, apply_brightness=True,
                  cut_subharm_below_f0=True, normalize=1.0, uv_strength=0.75, breath_strength=0.1)
MIX_DEFAULT = dict(mix_harm=1.0, mix_breath=1.0, mix_unvoiced=1.0, volume=1.0)


def formant_rows(case):
    """[4, rows] float64 tracks as gf.synthesize fits them to the envelope's rows."""
    fm = R.formants_int_keys(case.get("formants"))
    return np.stack([R.fit_length(fm[i], case["env"].shape[1]) for i in (1, 2, 3, 4)], axis=0)


def synth_note(case, geo, exact=False, fft="numpy", pulse=None, given=None, sigma=100.0):
    """The stages of one note.  ``case``: env fp32 [bins, rows], f0 / mask fp32 [n], phi fp32 [bins, T], formants {1..4: track} or
    None, kw (gf.synthesize's keywords), mix (the V / B / U weights and the volume)."""
    sr, n_fft, hop = geo
    given = given or {}
    kw = dict(KW_DEFAULT, **case.get("kw", {}))
    mixw = dict(MIX_DEFAULT, **case.get("mix", {}))
    dt, ct = (F64, C128) if exact else (F32, C64)
    win = R.sqrt_hann(n_fft)
    env = np.asarray(case["env"], dtype=F32)
    f0 = np.array(case["f0"], dtype=F32)
    vm = np.asarray(case["mask"], dtype=F32)
    n = len(f0)
    out = {}

    env_noise = R.gauss1d(env, 1.75, axis=0)
    f0 *= kw["pitch_shift"]
    out["f0"] = f0
    F = formant_rows(case)
    ratios = [kw["F1_shift"], kw["F2_shift"], kw["F3_shift"], kw["F4_shift"]]
    if exact:
        env = env.astype(F64)
    if any(r != 1.0 for r in ratios):
        env = warp_formants(env, F, F * np.asarray(ratios, dtype=F64)[:, None], sr, exact)
    if kw["formant_shift"] != 1.0:
        env = shift_formants(env, kw["formant_shift"], sr, exact)

    if pulse is None:
        pulse = R.pulse_train(f0.astype(F32), sr, Ra=0.02, Rg=1.7, Rk=0.8)
    pulse = np.asarray(pulse, dtype=F32)
    out["pulse"] = pulse
    xp = R.padded_signal(pulse, n_fft)
    T = max(1, 1 + (len(xp) - n_fft) // hop)
    idx = np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]
    frames = xp[idx].astype(dt)
    frames *= win[:, None]
    S = _rfft(frames, exact, fft)
    freqs = R.bin_freqs(sr, n_fft)
    hp = highpass(freqs, R.frame_picks(f0, hop, T), exact)
    if "hp" in given:
        hp = np.asarray(given["hp"], dtype=dt)
    out["hp"] = hp
    if kw["cut_subharm_below_f0"]:
        S *= hp
    env = R.match_env_frames(env, T)
    out["env"] = env
    if "env_harm" in given:
        env = np.asarray(given["env_harm"], dtype=dt).T
    out["env_harm"] = env.T
    mag = np.max(np.abs(S) + 1e-8)
    out["mag"] = float(mag)
    bright_h, bright_b = R.brightness_curves(sr, n_fft)
    boost = R.boost_curve(n_fft)
    voiced = R.frame_picks(vm, hop, T)
    # as k_harm_shape leaves the spectrum: the 1 / mag deferred
    Sd = S * env
    Sd *= (boost.astype(F64) if exact else boost)[:, None]
    if kw["apply_brightness"]:
        out["S_harm_unblurred"] = brighten(Sd, voiced, bright_h, exact, blur=False).T
        Sd = brighten(Sd, voiced, bright_h, exact)
    if "S_harm" in given:
        Sd = np.asarray(given["S_harm"], dtype=ct).T.copy()
    out["S_harm"] = Sd.T
    if "note_mag" in given:
        mag = dt(given["note_mag"])
    out["note_mag"] = float(mag)
    if "S_harm" in given:
        S = Sd / mag
    else:
        S = (S / mag) * env
        S *= (boost.astype(F64) if exact else boost)[:, None]
        if kw["apply_brightness"]:
            S = brighten(S, voiced, bright_h, exact)
    out["frames"] = (_irfft(Sd, n_fft, exact, fft) * (win.astype(dt))[:, None]).T
    harmonic = istft(S, win, hop, n, exact, fft)

    env_n = R.match_env_frames(env_noise, T)
    env_n = env_n if exact else env_n.astype(F32)                # [bins, T]
    if "env_noise" in given:
        env_n = np.asarray(given["env_noise"], dtype=dt).T
    out["env_noise"] = env_n.T
    phi = np.asarray(case["phi"], dtype=F32)
    if exact:
        phi = phi.astype(F64)
    U = np.cos(phi) + 1j * np.sin(phi)
    S_uv = U * env_n
    S_br = (U * env_n) * hp
    if kw["apply_brightness"]:
        out["S_breath_unblurred"] = brighten(S_br, voiced, bright_b, exact, blur=False).T
        S_br = brighten(S_br, voiced, bright_b, exact)
    if "S_uv" in given:
        S_uv = np.asarray(given["S_uv"], dtype=ct).T.copy()
    if "S_breath" in given:
        S_br = np.asarray(given["S_breath"], dtype=ct).T.copy()
    out["S_uv"], out["S_breath"] = S_uv.T, S_br.T
    knots = np.asarray(given["mask_short"], dtype=F64) if "mask_short" in given else mask_knots(vm, sigma, exact)
    out["mask_short"] = knots
    ms = mask_upsample(knots, n, exact)
    if "mask_smooth" in given:
        ms = np.asarray(given["mask_smooth"], dtype=dt)
    out["mask_smooth"] = ms
    aper_b = istft(S_br, win, hop, n, exact, fft)
    aper_u = istft(S_uv, win, hop, n, exact, fft)
    out["gain_bre"] = ms * kw["breath_strength"]
    out["gain_uv"] = (1.0 - ms) * kw["uv_strength"]
    bre = aper_b * ms * kw["breath_strength"]
    uv = aper_u * (1.0 - ms) * kw["uv_strength"]
    if "harm_pre" in given:
        harmonic = np.asarray(given["harm_pre"], dtype=dt).copy()
    out["harm_pre"] = harmonic.copy()
    out["voiced"] = voiced
    combined = harmonic + uv + bre
    peak = float(np.max(np.abs(combined)) + 1e-12)           # (an fp32 sum in the reference arithmetic: the oracle's)
    out["peak"] = peak
    out["note_peak"] = float(np.max(np.abs(combined)))       # what the kernels keep: the + 1e-12 is added where the gain is taken
    gain = (1.0 / peak) ** float(np.clip(kw["normalize"], 0.0, 1.0))
    harmonic = harmonic * gain if exact else _times(harmonic, gain)
    uv = uv * gain if exact else _times(uv, gain)
    bre = bre * gain if exact else _times(bre, gain)
    out["harm"], out["uv"], out["bre"] = harmonic, uv, bre
    out["rec"] = combined * gain
    w = {k: (F64(v) if exact else F32(v)) for k, v in mixw.items()}
    out["mix"] = ((harmonic * w["mix_harm"] + bre * w["mix_breath"]) + uv * w["mix_unvoiced"]) * w["volume"]
    out["T"] = T
    return out


def _times(x, g):
    x *= g                                                   # the oracle's in-place fp32 product
    return x


# ---------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------
STAGE_SCOPE = {"env_harm": "row", "env_noise": "row", "S_harm": "row", "S_uv": "row", "S_breath": "row", "frames": "row",
               "harm": "note", "uv": "note", "bre": "note", "rec": "note", "mix": "note"}


def unit_errors(x, truth, scope):
    """Per unit (row of a matrix, or the whole note): max |x - truth| / max |truth|.  A unit whose truth is all zero: 0.0 when x is
    all zero there, inf otherwise."""
    truth = np.asarray(truth)
    x = np.asarray(x)
    assert x.shape == truth.shape, (x.shape, truth.shape)
    if scope == "note":
        truth, x = truth.reshape(1, -1), x.reshape(1, -1)
    if truth.size == 0:
        return np.zeros(truth.shape[0])
    peak = np.max(np.abs(truth), axis=1).astype(F64)
    d = np.max(np.abs(x.astype(truth.dtype if np.iscomplexobj(truth) else F64) - truth), axis=1).astype(F64)
    zero = peak == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(zero, np.where(np.max(np.abs(x), axis=1) == 0, 0.0, np.inf), d / np.where(zero, 1.0, peak))
    return e


def e_ref(stage, truth, *refs):
    """The note's E_ref of a stage: the worst unit of the note, the larger over the yardsticks handed in."""
    scope = STAGE_SCOPE[stage]
    worst = 0.0
    for r in refs:
        e = unit_errors(r[stage], truth[stage], scope)
        worst = max(worst, float(np.max(e)) if e.size else 0.0)
    return worst


def within(e_got, E_ref, factor=3.0):
    """The project's rule, per unit: e <= factor * E_ref + 2^-23 (a zero-truth unit: e == 0)."""
    return bool(np.all(np.asarray(e_got) <= factor * E_ref + EPS32))


def judge(stage, got, truth, *refs, factor=3.0):
    """(ok, worst e_got, E_ref) of one stage of one note."""
    E = e_ref(stage, truth, *refs)
    e = unit_errors(got, truth[stage], STAGE_SCOPE[stage])
    return within(e, E, factor), (float(np.max(e)) if e.size else 0.0), E


# ---------------------------------------------------------------------------------------------
# the matrix of notes, shared by tests/test_synth_ref.py and tests/test_gpu_synth_stages.py
# ---------------------------------------------------------------------------------------------
GEOMETRIES = [(44100, 1024, 256), (22050, 512, 128), (44100, 2048, 512), (96000, 2048, 96), (44100, 768, 192), (44100, 1000, 250),
              (48000, 4096, 1024),
              # the transform forms the seven above leave out (csrc/fft.hip, with_transform): Bluestein at L = 256 / 512 / 2048 on a wave,
              # at L = 4096 on the workgroup, and the wave's native 768 points
              (16000, 130, 40), (22050, 320, 80), (44100, 2046, 512), (48000, 3000, 750), (44100, 1536, 384)]
CROSSING = ([1.3, 0.8, 1.1, 0.9], [1.5, 0.6, 0.7, 1.4], [0.7, 1.3, 1.3, 0.6])


def f32(v):
    return float(F32(v))


def _env(rng, sr, nb, rows):
    f = np.arange(nb) * (sr / 2.0 / (nb - 1))
    e = np.exp(-f / 3000.0)[:, None] * (1.0 + 0.3 * rng.random((1, rows)))
    e = e * (1.0 + 0.8 * np.exp(-0.5 * ((f[:, None] - 700.0 - 400.0 * rng.random((1, rows))) / 150.0) ** 2))
    e = e * (1.0 + 0.1 * rng.random((nb, rows))) + 1e-4
    return e.astype(F32)


def _formants(rng, rows, kind="plain"):
    t = np.arange(rows)
    F = np.stack([600.0 + 40 * np.sin(t / 3.0), 1500.0 + 90 * np.cos(t / 4.0), 2600.0 + 50 * np.sin(t / 5.0),
                  3500.0 + 70 * np.cos(t / 2.0)]).astype(F64)
    if kind == "crossing":
        F[0] = rng.uniform(600, 1100, rows)
        F[1] = rng.uniform(700, 1400, rows)
        F[2, ::5] = 0.0
        F[3, ::7] = rng.uniform(100, 21000, len(F[3, ::7]))
    if kind == "holes":                                     # zeros and NaNs, as a track can come out of a .goofy file
        F[0, ::3] = 0.0
        F[1, 1::4] = np.nan
        F[2, :] = 0.0
        F[3, -1] = np.nan
    return {i + 1: F[i] for i in range(4)}


def make_case(geo, seed, n, name, mask="random", f0="glide", rows="T", kw=None, mix=None, formants=None):
    sr, n_fft, hop = geo
    rng = np.random.default_rng(seed)
    nb = n_fft // 2 + 1
    T = 1 + n // hop
    n_rows = {"T": T, "T-1": max(1, T - 1), "T+2": T + 2, "1": 1}[rows]
    i = np.arange(n)
    if isinstance(mask, str):
        if mask == "random":
            m = (rng.random(n) > 0.4)
        elif mask == "blocks":
            m = np.repeat(rng.random(n // 37 + 1) > 0.4, 37)[:n]
        elif mask == "zero":
            m = np.zeros(n, bool)
        elif mask == "one":
            m = np.ones(n, bool)
        else:
            raise ValueError(mask)
    else:
        m = np.asarray(mask(i, n))
    m = m.astype(F32)
    if isinstance(f0, str):
        if f0 == "glide":
            f = 200.0 + 80.0 * i / max(1, n - 1)
        elif f0 == "straddle":                                # the frame picks fall on either side of 2656.25 Hz
            f = np.where((i // hop) % 2 == 0, 2656.0, 2656.5)
        else:
            raise ValueError(f0)
        f = f * m
    elif callable(f0):
        f = f0(i, n, m)
    else:
        f = np.full(n, float(f0)) * m
    c = dict(name=name, n=n, env=_env(rng, sr, nb, n_rows), f0=np.asarray(f, dtype=F32), mask=m,
             phi=rng.uniform(0.0, 2.0 * np.pi, size=(nb, T)).astype(F32), kw=dict(kw or {}), mix=dict(mix or {}),
             formants=_formants(rng, n_rows, formants) if formants else None)
    return c


def long_lengths(geo):
    hop = geo[2]
    base = 35 * hop
    return [base + ((k - base) % 4) for k in range(4)]       # n % 4 = 0, 1, 2, 3


def main_batch(geo):
    """About sixty notes of at most 36 frames: the lengths, envelope row counts, masks, f0 and parameters of the issue."""
    sr, n_fft, hop = geo
    L = long_lengths(geo)
    lens = [1, 2, 5, hop - 1, hop, hop + 1, n_fft - 1, n_fft, n_fft + 1, 4 * hop + 3] + L
    rows = ["T-1", "T", "T+2", "1"]
    notes = []
    s = 1000 * n_fft + hop

    def add(n, name, **k):
        notes.append(make_case(geo, s + len(notes), n, name, **k))

    for j, n in enumerate(lens):
        add(n, "len%d" % n, mask="blocks" if j % 2 else "random", rows=rows[j % 4])
    n0, n1 = 20 * hop + 2, 12 * hop + 1
    b = 9 * hop
    gap = min(int(0.050 * sr), 20 * hop)                     # 50 ms, or 20 hops where 50 ms would not fit a note of 36 frames (hop 96)
    add(L[1], "mask_zero", mask="zero")
    add(L[2], "mask_one", mask="one")
    for d in (-1, 0, 1):
        add(n0, "step_hop%+d" % d, mask=lambda i, n, d=d: i >= b + d)
    add(n0, "step_early", mask=lambda i, n: i >= hop + hop // 3)
    add(n0, "island", mask=lambda i, n: (i >= 7 * hop + 5) & (i < 8 * hop + hop // 2))
    add(max(n0, gap + 10 * hop), "gap50ms", mask=lambda i, n: ~((i >= n // 3) & (i < n // 3 + gap)))
    add(n0, "mask_random", mask="random")
    add(n0, "f0_under_mask0", mask=lambda i, n: i < n // 2, f0=lambda i, n, m: np.full(n, 233.0))
    add(n0, "mask1_over_f0_0", mask="one", f0=lambda i, n, m: np.where(i < n // 2, 0.0, 190.0))
    for hz in (2656.0, 2656.25, 2656.5, 2700.0):
        add(n1, "f0_%g" % hz, mask="one", f0=hz)
    add(n1, "f0_straddle", mask="one", f0="straddle")
    add(n1, "pitch_0.5", mask="blocks", kw=dict(pitch_shift=0.5))
    add(n1, "pitch_2", mask="blocks", kw=dict(pitch_shift=2.0))
    one = [dict(apply_brightness=False), dict(cut_subharm_below_f0=False), dict(normalize=0.0), dict(normalize=0.5),
           dict(normalize=1.0), dict(uv_strength=0.0), dict(breath_strength=0.0)]
    for k in one:
        add(n1, "kw_" + "_".join("%s=%s" % kv for kv in k.items()), mask="blocks", kw=k)
    add(n1, "mix_negative", mask="blocks", mix=dict(mix_harm=-1.0, mix_breath=0.5, mix_unvoiced=-0.25, volume=f32(0.7)))
    for r in (0.8, 1.25):
        add(n1, "formant_shift_%g" % r, mask="blocks", kw=dict(formant_shift=f32(r)))
    for q in range(4):
        for r in (0.7, 1.4):
            add(n1, "F%d_%g" % (q + 1, r), mask="blocks", kw={"F%d_shift" % (q + 1): r}, formants="plain", rows=rows[(q + 1) % 3])
    for r in CROSSING:
        add(n1, "crossing_%s" % r, mask="blocks", kw={"F%d_shift" % (q + 1): r[q] for q in range(4)}, formants="crossing")
    add(n1, "formant_holes", mask="blocks", kw=dict(F1_shift=1.3, F2_shift=0.8, F3_shift=1.2, F4_shift=0.9, formant_shift=f32(1.1)),
        formants="holes")
    rng = np.random.default_rng(s)
    for q in range(6):
        k = dict(pitch_shift=f32(rng.uniform(0.6, 1.7)), formant_shift=f32(rng.uniform(0.7, 1.4)), normalize=f32(rng.uniform(0, 1)),
                 uv_strength=f32(rng.uniform(0, 1.5)), breath_strength=f32(rng.uniform(0, 0.5)), apply_brightness=bool(q % 2),
                 cut_subharm_below_f0=bool(q % 3), F2_shift=float(np.round(rng.uniform(0.7, 1.4), 2)),
                 F3_shift=float(np.round(rng.uniform(0.7, 1.4), 2)))
        add(n1 + q, "combo%d" % q, mask="random" if q % 2 else "blocks", kw=k, formants="plain", rows=rows[q % 4],
            mix=dict(mix_harm=f32(rng.uniform(-1, 1)), mix_breath=f32(rng.uniform(0, 2)), volume=f32(rng.uniform(0.2, 1.5))))
    return notes


def sigma_batch(geo, tag):
    """The masks whose smoothing matters, for the transition sigmas that are not the default (the sigma is per batch)."""
    sr, n_fft, hop = geo
    notes = []
    s = 2000 * n_fft + hop + tag
    n0 = 20 * hop + 1
    b = 9 * hop

    def add(n, name, **k):
        notes.append(make_case(geo, s + len(notes), n, name, **k))

    for n in (1, 5, hop + 1, n_fft + 1) + tuple(long_lengths(geo)[1:3]):
        add(n, "len%d" % n, mask="blocks")
    add(n0, "mask_zero", mask="zero")
    add(n0, "mask_one", mask="one")
    add(n0, "step_hop", mask=lambda i, n: i >= b)
    add(n0, "island", mask=lambda i, n: (i >= 7 * hop + 5) & (i < 8 * hop + hop // 2))
    add(n0 + 2, "mask_random", mask="random")
    return notes


def tiny_batch(geo):
    """Seventy notes of one to nine samples (one k_mask_short tile holds many notes), then one note of 35 hops + 40 samples that
    spans tiles at the short rate."""
    s = 3000 * geo[1] + geo[2]
    notes = [make_case(geo, s + j, 1 + j % 9, "tiny%d" % j, mask=("one", "zero", "random")[j % 3]) for j in range(70)]
    notes.append(make_case(geo, s + 70, 35 * geo[2] + 40, "after_tiny", mask="blocks"))
    return notes


# ---------------------------------------------------------------------------------------------
# long runs: a batch for tests/test_gpu_walker_runs.py (option "walk_run") and what a partition into runs must cover on it
# ---------------------------------------------------------------------------------------------
# Frames per note, in batch order: notes of 1..5 frames, forty one-frame notes in a row, notes of 61 / 64 / 65 / 67, 127 .. 130,
# 257 and 307 frames around the 64-frame record block and the runs 61, 62, 64, 65, 95, 128 and 256, and five fillers.  The ORDER
# is the result of a search for run_coverage() to hold at every one of those runs (halo 3; run 256 also at halo 21) and is
# asserted by tests/test_synth_ref.py: a change here that loses a condition fails there, without a GPU.
LONG_FRAMES = (64, 25, 5, 25, 4, 130, 257, 3, 29) + (1,) * 40 + (27, 9, 127, 23, 65, 61, 129, 12, 67, 1, 2, 128, 3, 307, 4, 30, 35, 17, 25)
# (halo 3 for hop == n_fft / 4; 21 at n_fft 2048 with hop 96, whose floor is 168 frames)
LONG_RUNS = ((61, 3), (62, 3), (64, 3), (65, 3), (95, 3), (128, 3), (256, 3), (256, 21))


def run_coverage(frame_off, run, halo, blocks):
    """What the partition of a batch's frame axis into runs of ``run`` frames reaches.  A wave owns the frames [f0, f1) of a run,
    starts ``min(t0, halo)`` frames earlier (t0: f0's index in its note) at fs, and — ``blocks``: the two stem walkers of
    csrc/stems.hip — holds the frame records of [fs + 64 j, fs + 64 j + 64).  {condition: holds}:
      t0=0 / 1 / 2 / 3 / >halo   a run behind the first starts at that frame of a note
      ends_last, ends_last-1     a run in front of the last ends on a note's last frame (whose owner flushes the trailing hops) /
                                 on its last but one
      3_notes, 3_runs            a run holds three whole notes; a note spans three runs
      refill_inside, refill_first   (blocks, run + halo > 64) frame fs + 64 of a run, inside the run, is a later frame of its note /
                                 in another run the first frame of a note
      final_block                (blocks) the last run's last record block reaches past the batch's last frame"""
    f_off = np.asarray(frame_off, dtype=np.int64)
    total = int(f_off[-1])
    note_of = np.repeat(np.arange(f_off.size - 1), np.diff(f_off))
    t_of = np.arange(total) - f_off[note_of]
    T_of = np.diff(f_off)[note_of]
    c = {k: False for k in ("t0=0", "t0=1", "t0=2", "t0=3", "t0>halo", "ends_last", "ends_last-1", "3_notes", "3_runs")}
    if blocks:
        c["final_block"] = False
        if run + halo > 64:
            c["refill_inside"] = c["refill_first"] = False
    starts = list(range(0, total, run))
    for f0 in starts:
        f1 = min(f0 + run, total)
        t0 = int(t_of[f0])
        fs = f0 - min(t0, halo)
        if f0 > 0:
            for k in (0, 1, 2, 3):
                c["t0=%d" % k] |= t0 == k
            c["t0>halo"] |= t0 > halo
        if f1 < total:
            c["ends_last"] |= bool(t_of[f1 - 1] == T_of[f1 - 1] - 1)
            c["ends_last-1"] |= bool(t_of[f1 - 1] == T_of[f1 - 1] - 2)
        whole = np.count_nonzero((f_off[:-1] >= f0) & (f_off[1:] <= f1) & (np.diff(f_off) > 0))
        c["3_notes"] |= whole >= 3
        if blocks and run + halo > 64 and fs + 64 < f1:
            c["refill_inside"] |= bool(t_of[fs + 64] > 0)
            c["refill_first"] |= bool(t_of[fs + 64] == 0)
        if blocks and f1 == total:
            last = fs + 64 * ((total - 1 - fs) // 64)
            c["final_block"] = last + 64 > total
    first_run, last_run = f_off[:-1] // run, (f_off[1:] - 1) // run
    c["3_runs"] = bool(np.any(last_run - first_run >= 2))
    return c


def long_batch(geo):
    """The notes of LONG_FRAMES (transition sigma 100, like main_batch): sample counts that leave 0, 1, hop / 2 and hop - 1
    samples behind a note's last hop; the long notes cycle through the masks one / step / zero / blocks — flat hops and skipped
    transforms inside long runs — and alternate between formant shifts (warped envelope rows) and none (the source rows)."""
    sr, n_fft, hop = geo
    s = 4000 * n_fft + hop
    rows = ["T", "T-1", "T+2", "1"]
    notes, longs = [], 0
    for k, T in enumerate(LONG_FRAMES):
        rest = (0, 1, hop // 2, hop - 1)[k % 4]
        n = max(1, (T - 1) * hop + rest)
        kw, formants = {}, None
        if T < 40:
            mask = ("random", "one", "zero", "blocks")[k % 4]
        else:
            mask = ("one", lambda i, n, k=k: i >= (n // 3 if k % 2 else 2 * n // 3) + 5, "zero", "blocks")[longs % 4]
            if longs % 2 == 0:
                kw, formants = {"F%d_shift" % (1 + longs % 4): (0.8, 1.3)[(longs // 2) % 2], "F2_shift": 1.2}, "plain"
            if longs % 5 == 3:
                kw = dict(kw, formant_shift=f32(1.1))
            if longs == 4:
                kw = dict(kw, apply_brightness=False)
            longs += 1
        notes.append(make_case(geo, s + k, n, "long%d_T%d" % (k, T), mask=mask, rows=rows[k % 4], kw=kw, formants=formants))
    return notes


def batches(geo):
    """{batch name: (transition sigma, notes)}"""
    return {"main": (100.0, main_batch(geo)), "sigma4": (4.0, sigma_batch(geo, 4)), "sigma2000": (2000.0, sigma_batch(geo, 2000)),
            "tiny": (100.0, tiny_batch(geo))}


def oracle_note(case, geo, sigma=100.0):
    """oracle.goofer_ref.synthesize on a case: (rec, harm, uv, bre, parts)."""
    sr, n_fft, hop = geo
    return R.synthesize(case["env"], case["f0"], case["mask"], np.empty(case["n"], bool), sr, n_fft=n_fft, hop_length=hop,
                        formants=case["formants"], phi=case["phi"], noise_transition_smoothness=sigma, return_parts=True,
                        **case["kw"])
