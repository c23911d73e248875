"""The GOOFER.py analyse/synth call surface, served by the MI355X backend.

Drop-in for the functions ``SillySampler.py`` / ``test.py`` call on the reference module
(``import goofer_amd.core as gf``): same names, positional order, array layouts (``[bins, frames]``
numpy arrays in, numpy arrays out) and error behaviour, but every array operation on the hot path
runs in libgoofer_hip.so on the GPU.  Host code here only marshals: it never computes audio.

Reference: GOOFER.py:355-413 (stft/istft), :473-554 (pulse train), :149-168 (knot decode),
:971-1220 (synthesize).  Per-call overheads (H2D/D2H of one note) make the single-note surface a
convenience; throughput comes from :func:`synthesize_batch`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .device import Context, check_noise_seed, check_phi_seed, default_context, default_params, row_stride

DSTORAGE = np.float16
DCOMPUTE = np.float32

def _ctx(sr, n_fft, hop, ctx=None) -> Context:
    return (ctx or default_context()).plan(sr, n_fft, hop)


MASK_DS = 4          # smooth_mask_ds decimation (GOOFER.py:556)


# -- feature files (host-side format code, byte-compatible with GOOFER.py:287-339) -----------------
def _formant_slot(key):
    """1..4 for a formant-track key (an int, or a string 'F<n>' / 'f<n>'), else None."""
    if isinstance(key, str):
        if not key[:1] in ("F", "f"):
            return None
        try:
            key = int(key[1:])
        except Exception:
            return None
    if isinstance(key, (int, np.integer)) and 1 <= int(key) <= 4:
        return int(key)
    return None


def formants_to_int_keys(d):
    """{1..4: ndarray} from a formant dict with int or 'F<n>' keys; absent tracks become one zero (GOOFER.py:48-62).
    The tracks keep the order the input listed them in (the dict is pickled into the .goofy file)."""
    slots = ((_formant_slot(k), v) for k, v in d.items()) if isinstance(d, dict) else ()
    tracks = {slot: np.asarray(v) for slot, v in slots if slot is not None}
    tracks.update({i: np.zeros(1, dtype=np.float64) for i in (1, 2, 3, 4) if i not in tracks})
    return tracks


def save_features(path, features, f0_interp, voicing_mask, formants, sr, y_len):
    fields = {}
    if isinstance(features, dict) and features.get("mode") == "knots":
        fields.update(mode=np.array(["knots"]), knot_vals_log=features["knot_vals_log"], hz_knots=features["hz_knots"],
                      n_bins=np.array([features["n_bins"]], dtype=np.int32),
                      n_fft=np.array([features["n_fft"]], dtype=np.int32),
                      env_sr=np.array([features["sr"]], dtype=np.int32))
    else:
        dense = np.asarray(features, dtype=DSTORAGE)
        fields.update(mode=np.array(["full"]), env_spec=dense, n_fft=np.array([dense.shape[0] * 2 - 2], dtype=np.int32))
    fields.update(f0_interp=np.asarray(f0_interp).astype(DSTORAGE), voicing_mask=np.asarray(voicing_mask).astype(DSTORAGE),
                  formants=formants_to_int_keys(formants), sr=np.array([sr], dtype=np.int32),
                  y_len=np.array([y_len], dtype=np.int64))
    with open(path, "wb") as fh:
        np.savez_compressed(fh, **fields)


def load_features(path):
    z = np.load(path, allow_pickle=True)
    if str(z["mode"][0]) == "knots":
        env = {"mode": "knots", "knot_vals_log": z["knot_vals_log"], "hz_knots": z["hz_knots"],
               "n_bins": int(z["n_bins"][0]), "n_fft": int(z["n_fft"][0]), "sr": int(z["env_sr"][0])}
    else:
        env = np.asarray(z["env_spec"], dtype=DCOMPUTE)
    return (env, np.asarray(z["f0_interp"], dtype=DCOMPUTE), np.asarray(z["voicing_mask"], dtype=DCOMPUTE),
            formants_to_int_keys(z["formants"].item()), int(z["sr"][0]), int(z["y_len"][0]))


# -- single-array entry points ---------------------------------------------------------------------
def _check_window(window, n_fft):
    """The kernels window with the plan's sqrt-Hann (GOOFER.py:12-18: ``np.sqrt(np.hanning(n_fft))`` in fp32, the only window the
    reference ever passes to stft / istft, :1099, :1146).  A caller's ``window`` must BE that window (to fp32 rounding): any other
    one used to be silently ignored, which is a wrong answer — it raises instead."""
    if window is None:
        return
    w = np.asarray(window)
    ref = np.sqrt(np.hanning(n_fft)).astype(np.float32)
    if w.shape != ref.shape or not np.allclose(w.astype(np.float64), ref.astype(np.float64), rtol=0.0, atol=3e-7):
        raise ValueError("goofer_amd.stft / istft support the reference's cached window only: sqrt(hanning(n_fft)) in fp32 "
                         "(GOOFER.py:12-18); got a different window of shape %s" % (w.shape,))


def stft(x, n_fft=2048, hop_length=512, window=None, sr=44100, ctx=None):
    """complex64 ``[bins, T]``.  ``window``: None or the reference's cached sqrt-Hann (anything else raises: `_check_window`)."""
    _check_window(window, n_fft)
    c = _ctx(sr, n_fft, hop_length, ctx)
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    T = 1 + n // hop_length
    S = c.rfft_frames(c.tensor(x), c.tensor(np.array([0, n], dtype=np.int64)), c.tensor(np.array([0, T], dtype=np.int64)), T)
    return np.ascontiguousarray(S.cpu().numpy().T)


def istft(S, hop_length=512, window=None, length=None, sr=44100, ctx=None):
    S = np.asarray(S, dtype=np.complex64)
    n_fft = (S.shape[0] - 1) * 2
    _check_window(window, n_fft)
    c = _ctx(sr, n_fft, hop_length, ctx)
    T = S.shape[1]
    n = hop_length * (T - 1) if length is None else int(length)
    # the backend derives T from the note length (T = 1 + n//hop); feed it a length in that class
    n_dev = hop_length * (T - 1)
    St = c.tensor(np.ascontiguousarray(S.T))
    y = c.irfft_ola(St, c.tensor(np.array([0, n_dev], dtype=np.int64)), c.tensor(np.array([0, T], dtype=np.int64)), n_dev)
    y = y.cpu().numpy()
    if n > n_dev:
        y = np.pad(y, (0, n - n_dev))
    return y[:n]


def pulse_train_numba(f0_interp, sr, Ra=0.02, Rg=1.7, Rk=0.8, ctx=None):
    """gf.pulse_train_numba (GOOFER.py:473-554).  Ra, Rg, Rk other than gf.synthesize's constants rebuild the handle's pulse
    tables for this call (Context.pulse_model) and put the constants back behind it."""
    c = ctx or default_context()
    if c.geom is None:
        c.plan(int(sr), 1024, 256)
    elif c.geom[0] != int(sr):
        c.plan(int(sr), c.geom[1], c.geom[2])
    f0 = np.asarray(f0_interp, dtype=np.float32)
    if f0.size == 0:
        return np.zeros(0, dtype=np.float32)
    before = getattr(c, "lf", (0.02, 1.7, 0.8))
    c.pulse_model(Ra, Rg, Rk)
    try:
        return c.pulse_train(c.tensor(f0), c.tensor(np.array([0, f0.size], dtype=np.int64))).cpu().numpy()
    finally:
        c.pulse_model(*before)


def decode_env_from_knots(env_pack, ctx=None):
    """fp32 ``[bins, T]`` from a knots dict (GOOFER.py:149-168)."""
    assert env_pack["mode"] == "knots"
    c = _ctx(int(env_pack["sr"]), int(env_pack["n_fft"]), int(env_pack["n_fft"]) // 4, ctx)
    knots = np.ascontiguousarray(np.asarray(env_pack["knot_vals_log"]).astype(np.float16).T)
    env = c.knot_decode(c.tensor(knots.view(np.uint16)).view(torch.float16), np.asarray(env_pack["hz_knots"], dtype=np.float32))
    out = env.cpu().numpy().T
    return np.ascontiguousarray(out[: int(env_pack["n_bins"])])


def gaussian_taps(sigma, truncate=4.0):
    """Normalised fp64 taps, radius int(truncate*sigma + 0.5) (GOOFER.py:247-252)."""
    r = int(truncate * sigma + 0.5)
    t = np.arange(-r, r + 1)
    k = np.exp(-0.5 * (t / sigma) ** 2)
    return k / k.sum()


# -- analysis: the half of extract_features that is not Praat (GOOFER.py:940-969, 97-147) ------------------
# -- small numeric helpers the reference exposes at module level (SillySampler.py / SillyEditor.py call them) ---------
def to_compute(x):
    return np.asarray(x, dtype=np.float32)                      # GOOFER.py:72


def hz_to_mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)                  # GOOFER.py:74


def mel_to_hz(m):
    return 700.0 * (10 ** (m / 2595.0) - 1.0)                   # GOOFER.py:75


def rms(x):
    return float(np.sqrt(np.mean(np.square(x)) + 1e-12))        # GOOFER.py:170-171 (a scalar reduction: host)


def gaussian_filter1d(input_array, sigma, axis=-1, truncate=4.0, ctx=None):
    """gf.gaussian_filter1d (GOOFER.py:241-261) on the device: numpy-'reflect' padding, fp64 accumulate in tap order,
    every 1-D line along ``axis`` filtered independently.  Returns float64 (complex128 for complex input)."""
    arr = np.asarray(input_array)
    radius = int(truncate * sigma + 0.5) if sigma > 0.0 else 0
    if radius <= 0 or arr.size == 0:                            # nothing to blur: a copy, dtype untouched
        return arr.copy()
    if np.iscomplexobj(arr):
        return (gaussian_filter1d(arr.real, sigma, axis, truncate, ctx) +
                1j * gaussian_filter1d(arr.imag, sigma, axis, truncate, ctx))
    c = ctx or default_context()
    moved = np.moveaxis(arr, axis, -1)
    lines = np.ascontiguousarray(moved, dtype=np.float64).reshape(-1, moved.shape[-1])
    out = c.gauss_rows_f64(c.tensor(lines), gaussian_taps(sigma, truncate)).cpu().numpy()
    return np.moveaxis(out.reshape(moved.shape), -1, axis)


def smooth_mask_ds(mask, sigma=100, ds=4, sr=44100, n_fft=1024, hop_length=256, ctx=None):
    """gf.smooth_mask_ds (GOOFER.py:556-569) on the device: mask[::4] -> Gaussian max(1, sigma / 4) -> linear upsample."""
    if ds != MASK_DS:
        raise ValueError("the device path decimates by %d (GOOFER.py:556 default)" % MASK_DS)
    c = _ctx(sr, n_fft, hop_length, ctx)
    m = np.ascontiguousarray(mask, dtype=np.float32)
    if m.size == 0:
        return m.copy()
    return c.smooth_mask_ds(c.tensor(m), sigma=float(sigma)).cpu().numpy()


def _axis_sigmas(sigma):
    """(sigma of axis 0, sigma of axis 1), negatives clamped to 0, from a number or a pair."""
    pair = tuple(sigma) if isinstance(sigma, (list, tuple)) else (sigma, sigma)
    if len(pair) != 2:
        raise ValueError("sigma must be a float or a 2-tuple for 2D arrays.")
    return tuple(max(float(v), 0.0) for v in pair)


def gaussian_filter(input_array, sigma, ctx=None):
    """gf.gaussian_filter (GOOFER.py:263-285): the separable blur of a matrix, one gaussian_filter1d pass (on the device)
    per axis whose sigma is positive."""
    arr = np.asarray(input_array)
    if arr.ndim != 2:
        raise ValueError("gaussian_filter expects a 2D array.")
    if 0 in arr.shape:
        return arr.copy()
    for axis, s in enumerate(_axis_sigmas(sigma)):
        if s > 0.0:
            arr = gaussian_filter1d(arr, s, axis=axis, ctx=ctx)
    return arr


class _LinearInterp:
    """The callable gf.interp1d returns (GOOFER.py:173-239).  Inside [x[0], x[-1]] it is np.interp; outside either the two
    end segments continued (their slopes carry the reference's +1e-10 in the denominator) or a constant.  A single point
    is a constant function (with a fill value: the fill everywhere but at that point)."""

    def __init__(self, x, y, fill_value):
        self.x, self.y = x, y
        self.extrapolate = fill_value == "extrapolate"
        self.fill_value = fill_value
        if len(x) > 1:
            self.edge_slopes = ((y[1] - y[0]) / (x[1] - x[0] + 1e-10), (y[-1] - y[-2]) / (x[-1] - x[-2] + 1e-10))

    def _fill(self):
        try:
            return float(self.fill_value)
        except (TypeError, ValueError):
            raise ValueError("fill_value must be 'extrapolate' or a number")

    def __call__(self, q):
        q = np.asarray(q)
        x, y = self.x, self.y
        if len(x) == 1:
            if self.extrapolate:
                return np.full_like(q, y[0], dtype=y.dtype)
            out = np.full_like(q, self._fill())
            out[np.isclose(q, x[0])] = y[0]
            return out
        below, above = q < x[0], q > x[-1]
        if self.extrapolate:
            out = np.interp(q, x, y)
            for side, x_end, y_end, slope in ((below, x[0], y[0], self.edge_slopes[0]), (above, x[-1], y[-1], self.edge_slopes[1])):
                if np.any(side):
                    out[side] = y_end + slope * (q[side] - x_end)
            return out
        fill = self._fill()
        inside = ~(below | above)
        out = np.empty_like(q)
        if np.any(inside):
            out[inside] = np.interp(q[inside], x, y)
        out[~inside] = fill
        return out


def interp1d(x, y, kind="linear", fill_value="extrapolate"):
    """gf.interp1d: a host-side convenience like the reference's (the hot path interpolates in its kernels)."""
    if kind != "linear":
        raise ValueError("Only 'linear' interpolation is supported.")
    x, y = np.asarray(x), np.asarray(y)
    if len(x) == 0:
        raise ValueError("x cannot be empty")
    return _LinearInterp(x, y, fill_value)


def stretch_feature(feature, stretch, kind="linear", ctx=None):
    """gf.stretch_feature (GOOFER.py:597-616) on the device (fp32 rows in, fp64 math, fp32 out like the synth uses it)."""
    feature = np.asarray(feature)
    if stretch == 1.0:
        return feature.copy()
    if kind != "linear":
        raise ValueError("Only 'linear' interpolation is supported.")
    c = ctx or default_context()
    n_new = int(feature.shape[-1] * stretch)
    if feature.ndim == 1:
        if len(feature) == 0:
            raise ValueError("x cannot be empty")
        return c.stretch_rows(c.tensor(feature.astype(np.float32)), n_new).cpu().numpy().astype(np.float64)
    if feature.ndim == 2:
        if feature.shape[1] == 0:
            raise ValueError("x cannot be empty")
        rows = torch.empty((feature.shape[1], feature.shape[0]), dtype=torch.float32, device=c.device)
        rows.copy_(torch.as_tensor(np.ascontiguousarray(feature.T, dtype=np.float32)))
        return c.stretch_rows(rows, n_new).cpu().numpy().T.astype(np.float64)
    raise ValueError("Only 1D or 2D features are supported.")


def _vibrato_wave(length, sr, speed, seeded):
    """sin(2 pi speed t + phase) with a 0.1 s linear fade-in; the phase is drawn (legacy RNG) only for a seeded call."""
    phase = np.random.uniform(0, 2 * np.pi) if seeded else 0
    wave = np.sin(2 * np.pi * speed * (np.arange(length) / sr) + phase)
    n_fade = int(0.1 * sr)
    if n_fade < length:
        wave[:n_fade] *= np.linspace(0, 1, n_fade)
    return wave


def _smoothed_noise(length, sr, speed, ctx):
    """legacy-RNG normal draws, Gaussian-smoothed (sigma = sr / (6 speed) samples, on the device), peak-normalised."""
    noise = gaussian_filter1d(np.random.randn(length), sigma=sr / (speed * 6), ctx=ctx)
    noise /= np.max(np.abs(noise) + 1e-6)
    return noise


def create_volume_jitter(length, sr, speed=6.0, strength=0.1, seed=None, vibrato=False, ctx=None):
    """gf.create_volume_jitter (GOOFER.py:638-660): the multiplicative volume curve 1 + strength * x of the 'sr' / 'sd' flags —
    x a faded sinusoid (clipped to [0.5, 1.5]) or smoothed noise.  Draws come from the legacy global generator in the
    reference's order (seed, then phase or noise)."""
    if seed is not None:
        np.random.seed(seed)
    if vibrato:
        return np.clip(1.0 + _vibrato_wave(length, sr, speed, seed is not None) * strength, 0.5, 1.5)
    return 1.0 + _smoothed_noise(len(np.arange(length)), sr, speed, ctx) * strength     # (np.arange: the reference's length rule)


def make_mel_knots(sr, n_fft, K):
    """(bin freqs fp32, mel-spaced knot Hz fp32) — the codec's knot grid (GOOFER.py:77-82)."""
    from .synthetic import mel_knots_hz
    return np.fft.rfftfreq(n_fft, 1.0 / sr).astype(np.float32), mel_knots_hz(sr, K)


def _knot_bins(hz, sr, n_fft, nb):
    """int32 nearest bin of every knot frequency (GOOFER.py:114)."""
    res = sr / n_fft
    return np.clip(np.round(hz / res).astype(int), 0, nb - 1).astype(np.int32)


KNOT_CANDIDATES = tuple(range(32, 193, 16))     # compress_env_to_knots' K_start, K_step, K_max defaults


def knot_candidate_tables(sr, n_fft):
    """(hz fp32, bins int32) of every candidate of KNOT_CANDIDATES back to back, exactly as compress_env_to_knots makes them:
    the tables goofer_envelope_knots_batch scores."""
    nb = n_fft // 2 + 1
    hz = [make_mel_knots(sr, n_fft, K)[1] for K in KNOT_CANDIDATES]
    return (np.ascontiguousarray(np.concatenate(hz), dtype=np.float32),
            np.ascontiguousarray(np.concatenate([_knot_bins(h, sr, n_fft, nb) for h in hz]), dtype=np.int32))


def compress_env_to_knots(env_spec, sr, n_fft, eps=1e-2, K_start=32, K_step=16, K_max=192, smooth_sigma_bins=0.5, ctx=None):
    """Smallest mel-knot count whose 2-tap lerp reproduces the (sigma 0.5 blurred) envelope to < eps max relative
    error on <= 256 probe frames; knots sampled at the nearest bin, log, fp16.  Blur, error metric and knot
    gather run on the device; the loop over the 9 candidate K is host logic."""
    c = _ctx(sr, n_fft, n_fft // 4, ctx)
    rows = c.rows_from(np.asarray(env_spec, dtype=np.float32).T)
    T, nb = rows.shape
    taps = gaussian_taps(smooth_sigma_bins) if smooth_sigma_bins > 0 and int(4.0 * smooth_sigma_bins + 0.5) > 0 else np.ones(1)
    env2 = c.gauss_bins_f64(rows, taps)
    probe = c.tensor(np.linspace(0, T - 1, min(256, T), dtype=int).astype(np.int64))
    chosen = None
    for K in list(range(K_start, K_max + 1, K_step)) + [None]:
        last = K is None
        _, hz = make_mel_knots(sr, n_fft, K_max if last else K)
        d_at = c.tensor(_knot_bins(hz, sr, n_fft, nb))
        if not last and not (c.knot_fit_error(env2, probe, d_at, hz) < eps):
            continue
        vals = c.knot_gather(env2, d_at).cpu().numpy().T
        chosen = {"mode": "knots", "knot_vals_log": np.ascontiguousarray(vals), "hz_knots": hz.astype(np.float32),
                  "n_bins": int(nb), "n_fft": int(n_fft), "sr": int(sr)}
        break
    return chosen


def envelope_features(y, sr, n_fft=1024, hop_length=256, ctx=None):
    """(env_spec fp64 [bins, T], env_knots) = |stft| + 1e-8 -> sigma-2 bin blur -> knot encode (GOOFER.py:942-946, 968):
    one ``Context.envelope_knots`` call for this signal.  Raises ValueError for a signal that is not 1-D or is empty."""
    from . import trackers
    y = np.asarray(y, dtype=np.float32)
    if y.ndim != 1 or y.size == 0:
        raise ValueError(f"envelope_features expects a non-empty mono signal, got shape {y.shape}")
    c = _ctx(sr, n_fft, hop_length, ctx)
    knots, K, f_off, env = c.envelope_knots(c.tensor(y), [y.size], want_env=True)
    env_knots = trackers.knots_pack(knots.cpu().numpy(), K.cpu().numpy(), f_off, 0, sr, n_fft, c.n_bins)
    return np.ascontiguousarray(env.cpu().numpy().T), env_knots


def extract_features(y, sr, n_fft=1024, hop_length=256, f0_min=75, f0_max=600, f0_merge_range=2, pitch_tracker=None, ctx=None):
    """gf.extract_features (GOOFER.py:940-969) -> (env_spec fp64 [bins, T], f0 per sample, voicing mask, formants {1..5}, knots).
    The envelope half runs on the GPU.  The f0 and formant tracks come from a tracker
    ``pitch_tracker(y, sr, hop_length, n_frames) -> (f0_track [frames'], {1..5: [n_frames]})`` — the reference computes them
    with Praat (third-party, unpinned: SURVEY §8 c, parity unpinned): ``goofer_amd.trackers`` makes the reference's own
    parselmouth calls when that package is installed, ``GOOFER_TRACKER`` names another one, and without any this raises
    ``trackers.TrackerUnavailable`` (a NotImplementedError).  ``f0_max`` is accepted and unused, as in the reference.
    ``extract_features_batch`` of this one signal; raises the exception it reports for it (ValueError for a signal that is
    not 1-D or is empty)."""
    from . import trackers
    out = trackers.analyse_batch([y], sr, n_fft, hop_length, f0_min, f0_merge_range, tracker=pitch_tracker, ctx=ctx)[0]
    if isinstance(out, BaseException):
        raise out
    return out


def extract_features_batch(signals, sr, n_fft=1024, hop_length=256, f0_min=75, f0_merge_range=2, pitch_tracker=None, ctx=None):
    """``extract_features`` for a list of signals at one sample rate, in batched device passes: one 5-tuple per signal, or
    the exception that signal raised (trackers.analyse_batch).  A signal's result does not depend on the others."""
    from . import trackers
    return trackers.analyse_batch(signals, sr, n_fft, hop_length, f0_min, f0_merge_range, tracker=pitch_tracker, ctx=ctx)


# -- synthesize --------------------------------------------------------------------------------------
def _fit(x, T):
    x = np.asarray(x, dtype=np.float64)
    if x.size >= T:
        return x[:T]
    return np.zeros(T) if x.size == 0 else np.pad(x, (0, T - x.size), mode="edge")


def note_params_from_kwargs(n=1, **kw):
    p = default_params(n)
    p["pitch_shift"] = kw.get("pitch_shift", 1.0)
    p["formant_shift"] = kw.get("formant_shift", 1.0)
    p["f_shift"] = [kw.get("F1_shift", 1.0), kw.get("F2_shift", 1.0), kw.get("F3_shift", 1.0), kw.get("F4_shift", 1.0)]
    p["uv_strength"] = kw.get("uv_strength", 0.75)
    p["breath_strength"] = kw.get("breath_strength", 0.1)
    p["normalize"] = kw.get("normalize", 1.0)
    p["apply_brightness"] = int(bool(kw.get("apply_brightness", True)))
    p["cut_below_f0"] = int(bool(kw.get("cut_subharm_below_f0", True)))
    if kw.get("f0_jitter"):
        p["f0_jitter"] = kw.get("f0_jitter_strength", 1.5)
    if kw.get("volume_jitter"):
        p["vol_jitter_harm"] = kw.get("volume_jitter_strength_harm", 50)
        p["vol_jitter_breath"] = kw.get("volume_jitter_strength_breath", 100)
    if kw.get("add_subharm"):
        if kw.get("subharm_f0_jitter", 0) > 0.0:
            p["subharm_f0_jitter"] = kw["subharm_f0_jitter"]
        if np.size(kw.get("subharm_semitones", -12)) > 16:
            raise NotImplementedError("at most sixteen sub-harmonic ratios per call on the device path")
        p["subharm_weight"] = kw.get("subharm_weight", 0.5)
    return p


def subharm_from_kwargs(kw):
    """The call-level half of gf.synthesize's add_subharm arguments (GOOFER.py:979-980) for Context.synth_batch."""
    if not kw.get("add_subharm"):
        return None
    return {"semitones": kw.get("subharm_semitones", -12), "vibrato": kw.get("subharm_vibrato", False),
            "rate": kw.get("subharm_vibrato_rate", 6.0), "depth": kw.get("subharm_vibrato_depth", 0.1),
            "delay": kw.get("subharm_vibrato_delay", 0.1)}


def _stretch64(x, a, b, factor):
    """concat(x[:a], stretch_feature(x[a:b], factor), x[b:]) of a 1-D float32 array in the type the reference holds it in
    afterwards: FLOAT64 — its interp1d is np.interp on float64 abscissae (GOOFER.py:173-239, 597-606, 1019-1053).  None where
    the result is not float64 (a one-sample region comes back in y's own type) or the reference raises (an empty one)."""
    x = np.asarray(x)
    n = x.shape[0]
    a, b, _ = slice(a, b).indices(n)
    b = max(a, b)
    seg = x[a:b]
    if seg.size < 2:
        return None
    mid = np.interp(np.linspace(0, 1, int(seg.size * factor)), np.linspace(0, 1, seg.size), seg)
    return np.concatenate([x[:a].astype(np.float64), mid, x[b:].astype(np.float64)])


def _roughness_params(params, kw):
    """roughness_on needs the stems BEFORE the peak gain (the gain is taken from the roughened sum, GOOFER.py:1195-1217): the
    batch runs with normalize = 0 (gain 1) and `_finish` applies the reference's gain."""
    if kw.get("roughness_on"):
        params = params.copy()
        params["normalize"] = 0.0
    return params


_SYNTH_CALL_ARGS = ("env_spec", "f0_interp", "voicing_mask", "y", "sr", "n_fft", "hop_length", "phi", "phi_seed", "noise_seed", "seed",
                    "ctx")
_NOTE_ARRAYS = ("env_spec", "f0_interp", "voicing_mask", "y")
SYNTH_FRAME_BUDGET = 1 << 18      # STFT frames per synthesis pass (about 25 minutes of audio at 44.1 kHz, hop 256)


def _synth_defaults():
    """gf.synthesize's keyword arguments and their defaults (the notes' settings start from these)."""
    global _SYNTH_DEFAULTS
    if _SYNTH_DEFAULTS is None:
        import inspect
        _SYNTH_DEFAULTS = {k: v.default for k, v in inspect.signature(synthesize).parameters.items() if k not in _SYNTH_CALL_ARGS}
    return _SYNTH_DEFAULTS


_SYNTH_DEFAULTS = None


def synth_pass_key(kw, has_phi=False, f64_missing=False):
    """(strict, loose) pass key of a note with the merged keywords ``kw``: notes share a ``goofer_synth_batch`` pass when their
    strict parts are equal and their loose parts compatible.  Strict: the route (time-stretched or not), injected phases,
    noise_transition_smoothness, the sub-harmonic call settings and the volume jitter's form and speed — the last two only
    for notes that use them, so they also keep the spectra route (sub-harmonic layer, volume jitter) apart from the walkers.
    ``f64_missing``: a stretched note with f0 jitter or the sub-harmonic layer whose f0 stays float32 (a one-sample region).
    Loose: f0_jitter_speed of a note with f0 jitter, None (fits any pass) otherwise."""
    sub = None
    if kw.get("add_subharm"):
        st = np.atleast_1d(np.asarray(kw.get("subharm_semitones", -12), dtype=np.float64))
        sub = (tuple(st.tolist()), bool(kw.get("subharm_vibrato", False)), float(kw.get("subharm_vibrato_rate", 6.0)),
               float(kw.get("subharm_vibrato_depth", 0.1)), float(kw.get("subharm_vibrato_delay", 0.1)),
               bool(kw.get("subharm_f0_jitter", 0) > 0.0))
    vol = (bool(kw.get("volume_vibrato")), float(kw.get("volume_jitter_speed", 150))) if kw.get("volume_jitter") else None
    strict = (bool(kw.get("stretch_factor", 1.0) != 1.0), bool(has_phi), float(kw.get("noise_transition_smoothness", 100)), sub, vol,
              bool(f64_missing))
    loose = float(kw.get("f0_jitter_speed", 100)) if kw.get("f0_jitter") else None
    return strict, loose


def plan_synth_passes(keys, frames, frame_budget=SYNTH_FRAME_BUDGET):
    """Device passes of synthesize_batch: ``keys`` the notes' synth_pass_key (None: the note renders nothing), ``frames``
    their STFT frame counts.  Inside a strict key, a note without f0 jitter joins the first f0 jitter speed of its group;
    passes are then cut by ``frame_budget`` in note order (trackers.plan_keyed_passes).  Returns [[note index, ...], ...]."""
    from .trackers import plan_keyed_passes
    speeds = {}
    for k in keys:
        if k is not None and k[1] is not None:
            speeds.setdefault(k[0], k[1])
    entries = [(i, (k[0], k[1] if k[1] is not None else speeds.get(k[0])), int(f)) for i, (k, f) in enumerate(zip(keys, frames))
               if k is not None]
    return [idxs for _, idxs in plan_keyed_passes(entries, frame_budget)]


def _empty4():
    z = np.zeros(0, dtype=np.float32)
    return z, z.copy(), z.copy(), z.copy()


def _cut(length, a, b, factor):
    """(a, b, stretched length) of concat(x[:a], stretch_feature(x[a:b], factor), x[b:]) on an axis of ``length``."""
    a, b, _ = slice(a, b).indices(length)
    b = max(a, b)
    if b - a == 0:
        raise ValueError("x cannot be empty")                   # what gf.interp1d raises for an empty stretch region
    return a, b, int((b - a) * factor)


def _rough_settings(kw, sr):
    """The roughness layer's settings (GOOFER.py:901-940, 1195-1217): k and h lists as zip() pairs them, alpha, the two smoothing
    sigmas, noise amplitude and high-pass corner."""
    k_list = list(kw.get("rough_k_list", (2, 3, 4)))
    h_list = kw.get("rough_h_list")
    if h_list is None:                                        # default partial weights: 0.45, 0.28, 0.18, then x 0.6 per further partial
        base = (0.45, 0.28, 0.18)
        h_list = [base[i] if i < 3 else base[2] * 0.6 ** (i - 2) for i in range(len(k_list))]
    k_list, h_list = k_list[:len(h_list)], list(h_list)[:len(k_list)]          # zip() of the reference
    sig_n = max(1.0, (float(kw.get("rough_noise_smooth_ms", 120.0)) * 0.001 * sr) / 6.0)
    sig_a = max(1.0, (float(kw.get("rough_alpha_slew_ms", 120.0)) * 0.001 * sr) / 6.0)
    return (tuple(float(v) for v in k_list), tuple(float(v) for v in h_list), float(kw.get("rough_alpha", 0.6)), sig_n, sig_a,
            float(kw.get("rough_noise_amp", 0.6)), float(kw.get("rough_hp_fc", 320.0)))


def _prepare_note(c, note, kw, seed, phi, sr, n_fft, hop, phi_seed=None, noise_seed=None):
    """Everything gf.synthesize does for one note before the device renders it, in its order: the checks that make it raise,
    the fresh Philox key, then the legacy-RNG draws (f0, sub-harmonic, harmonic volume, breath volume jitter, then the
    roughness noises re-seeded 1337 + idx).  With a ``noise_seed`` none of them is drawn here and the global generator is
    left alone: the job records which streams the note draws (``want``) and the pass makes them on the device
    (``_pass_noise``, ``_roughness``).  Returns the note's job, or the four empty stems of a note with no samples."""
    env_spec = note["env_spec"]
    if isinstance(env_spec, dict) and env_spec.get("mode") == "knots":
        env_spec = decode_env_from_knots(env_spec, ctx=c)
        c.plan(sr, n_fft, hop)
    if isinstance(env_spec, torch.Tensor):                    # device-resident: [bins, T] on this context's device
        env = env_spec if env_spec.dtype in (torch.float32, torch.float64) else env_spec.float()
    else:
        env = np.asarray(env_spec)
        if env.dtype not in (np.float32, np.float64):
            env = env.astype(np.float32)                      # to_compute (fp64 is rounded on the device, the same bits)
    n = len(note["y"])
    f0 = _f32(note["f0_interp"])
    mask = _f32(note["voicing_mask"])
    if n == 0:
        return _empty4()
    if f0.ndim != 1 or mask.ndim != 1:
        raise ValueError("f0_interp and voicing_mask must be 1-D arrays")
    T_env = env.shape[1]
    if env.ndim != 2 or env.shape[0] != c.n_bins:
        raise ValueError(f"env_spec must be [{c.n_bins}, frames] for n_fft {n_fft}, got {list(env.shape)}")
    fm = formants_to_int_keys(kw.get("formants"))
    F = np.stack([_fit(fm[i], T_env) for i in (1, 2, 3, 4)], axis=1)           # [T_env, 4] fp64
    params = _roughness_params(note_params_from_kwargs(1, **kw), kw)
    job = {"kw": kw, "env": env, "T_env": T_env, "F": F, "f64_missing": False}
    if kw.get("stretch_factor", 1.0) != 1.0:
        # gf.synthesize with stretch_factor != 1 (GOOFER.py:1019-1067): the envelope is warped and its blurred noise copy made
        # first, then both, f0 (already scaled by pitch_shift) and the mask are resampled along time; the synth runs on the
        # stretched features with its in-kernel warps and blur switched off
        factor = float(kw["stretch_factor"])
        f_shift = [kw.get("F%d_shift" % i, 1.0) for i in (1, 2, 3, 4)]
        ps = kw.get("pitch_shift", 1.0)
        if ps != 1.0:
            f0 = f0 * _f32(np.float32(ps), like=f0) if isinstance(f0, torch.Tensor) else (f0 * np.float32(ps)).astype(np.float32)
        s0, s1 = kw.get("start_sec"), kw.get("end_sec")
        if s0 is not None and s1 is not None:
            a, b = int(s0 * sr), int(s1 * sr)
            fa, fb = int((s0 * sr) / hop), int((s1 * sr) / hop)
        else:
            a, b, fa, fb = 0, None, 0, None
        # f0_interp is a float64 array from here on in the reference: the jitter's product and the sub-harmonic phase trackers work on
        # it (their float32 versions land one event in ~10^5 a sample off, which a soak run of random keyword sets found)
        # (_stretch64 is host arithmetic: a device-resident f0 comes to the host here, and only here)
        needs64 = bool(kw.get("f0_jitter") or kw.get("add_subharm"))
        f0_64 = _stretch64(f0.cpu().numpy() if isinstance(f0, torch.Tensor) else f0, a, b, factor) if needs64 else None
        s_cut, _, e_cut = _cut(len(f0), a, b, factor), _cut(len(mask), a, b, factor), _cut(T_env, fa, fb, factor)
        n = s_cut[0] + s_cut[2] + len(f0) - s_cut[1]
        if n == 0:
            return _empty4()
        if len(mask) != len(f0):                              # (the ragged stretch cuts both on one sample axis)
            raise ValueError("f0_interp and voicing_mask must have the same length")
        f0_64 = f0_64 if f0_64 is not None and f0_64.size == n else None
        params = params.copy()
        params["pitch_shift"], params["formant_shift"], params["f_shift"] = 1.0, 1.0, [1.0, 1.0, 1.0, 1.0]
        job.update(stretched=True, f0=f0, mask=mask, s_cut=s_cut[:2], e_cut=e_cut[:2], rows_out=e_cut[0] + e_cut[2] + T_env - e_cut[1],
                   f_shift=f_shift, ratio=float(kw.get("formant_shift", 1.0)), anchor=any(v != 1.0 for v in f_shift),
                   f0_64=f0_64, f64_missing=needs64 and f0_64 is None)
    else:
        if len(f0) < n or len(mask) < n:
            raise ValueError(f"f0_interp and voicing_mask need len(y) = {n} samples")
        job.update(stretched=False, f0=f0[:n], mask=mask[:n], rows_out=T_env)
    job["n"] = n
    frames = 1 + n // hop
    if phi is not None:
        phi = np.asarray(phi)
        if phi.dtype not in (np.float32, np.float64):
            phi = phi.astype(np.float32)
        if phi.shape != (c.n_bins, frames):
            raise ValueError(f"phi must be [{c.n_bins}, {frames}] for this note, got {list(phi.shape)}")
    job.update(phi=phi, phi_seed=phi_seed, frames=frames, params=params)
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
    job["seed"] = int(seed) & 0xFFFFFFFFFFFFFFFF
    # jitter flags draw from the legacy global np.random stream in the reference's order: f0, sub-harmonic, harm volume, breath volume
    vib = bool(kw.get("volume_jitter") and kw.get("volume_vibrato"))          # the sinusoid variant draws nothing
    want = (bool(kw.get("f0_jitter")), bool(kw.get("add_subharm") and kw.get("subharm_f0_jitter", 0) > 0.0),
            bool(kw.get("volume_jitter") and not vib))
    host = noise_seed is None                                 # a seeded note: the same draws of its own seed, made by the pass
    job.update(want=want, legacy_seed=noise_seed)
    job["noise_f0"] = np.random.randn(n) if want[0] and host else None
    job["noise_sub"] = np.random.randn(n) if want[1] and host else None
    job["noise_vol"] = (np.random.randn(n), np.random.randn(n)) if want[2] and host else None
    job["rough"] = None
    if kw.get("roughness_on"):
        rs = _rough_settings(kw, sr)
        noises = None                                         # (a seeded note: _rough_noise makes them on the device)
        if host:
            noises = []
            for idx in range(len(rs[0])):                     # make_smooth_noise re-seeds the LEGACY global generator
                np.random.seed(1337 + idx)
                noises.append(np.random.randn(n).astype(np.float32).astype(np.float64))
        job["rough"] = (rs, noises)
    return job


def _f32(x, like=None):
    """np.asarray(x, dtype=np.float32), or for a device tensor (``like``: a scalar onto like's device) the same rounding there."""
    if isinstance(x, torch.Tensor):
        return x if x.dtype == torch.float32 else x.to(torch.float32)
    if like is not None:
        return torch.tensor(np.float32(x), device=like.device)
    return np.asarray(x, dtype=np.float32)


def _concat(arrs, dtype):
    return np.concatenate([np.ascontiguousarray(a, dtype=dtype).ravel() for a in arrs]) if arrs else np.zeros(0, dtype=dtype)


def _device_concat(c, arrs, dtype):
    """_concat on the device: one upload when every array is on the host, else one torch.cat of device tensors and uploads."""
    if not any(isinstance(a, torch.Tensor) for a in arrs):
        return c.tensor(_concat(arrs, dtype))
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    return torch.cat([a.reshape(-1).to(c.device, tdt) if isinstance(a, torch.Tensor)
                      else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).ravel()).to(c.device) for a in arrs])


def _noise(c, js, key, part=None):
    """One fp64 device array of a jitter's host draws for the pass (zeros for the notes without them), or None."""
    if not any(j[key] is not None for j in js):
        return None
    return c.tensor(np.concatenate([(j[key] if part is None else j[key][part]) if j[key] is not None else np.zeros(j["n"])
                                    for j in js]))


def _noise_seeds(seeds, n, who):
    """The per-note legacy seeds of a batch call as a checked list (None entries: that note draws on the host): the length and
    anything that is not an integer in [0, 2**32) raise ValueError — before a context exists."""
    seeds = [None] * n if seeds is None else [check_noise_seed(s, "noise_seeds[%d]" % i) for i, s in enumerate(seeds)]
    if len(seeds) != n:
        raise ValueError(f"{who}: {n} notes and {len(seeds)} noise seeds")
    return seeds


def _pass_noise(c, js):
    """The pass's four fp64 jitter arrays (f0, sub-harmonic f0, harmonic volume, breath volume; None: no note of the pass
    draws it).  The unseeded notes' host draws are uploaded (``_noise``: zeros elsewhere; an array only seeded notes draw is
    zeroed on the device, nothing uploaded); then one goofer_legacy_normal_jobs fills the seeded notes' slices: a note's
    draws are one job, its streams in the reference's order."""
    streams = (("noise_f0", None, 0), ("noise_sub", None, 1), ("noise_vol", 0, 2), ("noise_vol", 1, 2))
    total = sum(j["n"] for j in js)
    out = []
    for key, part, w in streams:
        t = _noise(c, js, key, part)
        if t is None and any(j["want"][w] and j["legacy_seed"] is not None for j in js):
            t = torch.zeros(total, dtype=torch.float64, device=c.device)
        out.append(t)
    off = c.offsets([j["n"] for j in js])
    table = [(j["legacy_seed"], j["n"], [(out[k], int(off[i])) for k, (_, _, w) in enumerate(streams) if j["want"][w]], False)
             for i, j in enumerate(js) if j["legacy_seed"] is not None and any(j["want"])]
    if table:
        c.legacy_normal_jobs(table)
    return out


def _ingest(c, arrays, lengths):
    """ld-strided fp32 rows of [bins, T] host arrays, one upload and one goofer_ingest_rows launch.  Envelopes already on the
    device ([bins, T] views of frame-major rows, analyse_device's) are rounded to fp32 into the row stride there instead, with
    the same round-to-nearest-even; host arrays in such a pass are uploaded frame-major beside them."""
    if not any(isinstance(a, torch.Tensor) for a in arrays):
        dt = np.float64 if any(a.dtype == np.float64 for a in arrays) else np.float32
        return c.ingest_rows(c.tensor(_concat(arrays, dt)), lengths, c.n_bins)
    f64 = any(a.dtype == (torch.float64 if isinstance(a, torch.Tensor) else np.float64) for a in arrays)
    tdt = torch.float64 if f64 else torch.float32
    parts = [a.T.to(tdt) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a.T)).to(c.device, tdt) for a in arrays]
    rows = c.rows(sum(int(v) for v in lengths), c.n_bins)
    rows.copy_(torch.cat(parts) if len(parts) > 1 else parts[0])
    return rows


def _phase_seeds(seeds, phis, n, who):
    """The per-note numpy phase seeds of a batch call as a checked list (None entries: not seeded): the length, a negative or
    non-integer seed and a note with both a seed and a phase array raise ValueError — before a context exists."""
    seeds = [None] * n if seeds is None else [check_phi_seed(s, "phi_seeds[%d]" % i) for i, s in enumerate(seeds)]
    if len(seeds) != n:
        raise ValueError(f"{who}: {n} notes and {len(seeds)} phase seeds")
    both = [i for i, (s, p) in enumerate(zip(seeds, phis)) if s is not None and p is not None]
    if both:
        raise ValueError(f"{who}: note {both[0]} has a phase array and a phase seed; give one of them")
    return seeds


def _phases(c, js):
    """The injected phase rows of a pass (its notes all have them, or none: synth_pass_key): the notes' arrays through
    goofer_ingest_rows, the seeded notes' numpy streams drawn on the device (goofer_phase_fill), one matrix."""
    seeds = [j["phi_seed"] for j in js]
    arrays = [k for k, j in enumerate(js) if j["phi"] is not None]
    frames = [j["frames"] for j in js]
    if not arrays and seeds[0] is None:
        return None
    if len(arrays) == len(js):
        return _ingest(c, [j["phi"] for j in js], frames)
    d_phi = c.phase_fill(seeds, frames)
    if arrays:                                                # the arrays' rows, ingested back to back, to their notes' places
        rows = _ingest(c, [js[k]["phi"] for k in arrays], [frames[k] for k in arrays])
        f_off, a_off = c.offsets(frames), c.offsets([frames[k] for k in arrays])
        for q, k in enumerate(arrays):
            d_phi[int(f_off[k]):int(f_off[k + 1])].copy_(rows[int(a_off[q]):int(a_off[q + 1])])
    return d_phi


def _run_pass(c, js, sr):
    """One goofer_synth_batch for the jobs of a pass (and, for the time-stretched route, the ragged warp, blur and stretch in
    front of it).  Returns (host stems {rec, harm, uv, bre}, sample offsets)."""
    env_lens = [j["T_env"] for j in js]
    lens = [j["n"] for j in js]
    kw = js[0]["kw"]
    d_env = _ingest(c, [j["env"] for j in js], env_lens)
    d_phi = _phases(c, js)
    params = c._c_params(np.concatenate([j["params"] for j in js]))
    seeds = np.array([j["seed"] for j in js], dtype=np.uint64)
    params["seed"][:, 0] = (seeds & np.uint64(0xFFFFFFFF)).astype(np.uint32)    # the kernels XOR it with the batch seed 0: each
    params["seed"][:, 1] = (seeds >> np.uint64(32)).astype(np.uint32)            # note's key is the key of its single call
    F = c.tensor(np.concatenate([j["F"] for j in js]))
    fm = _device_concat(c, [j["f0"] for j in js] + [j["mask"] for j in js], np.float32)
    n_in = fm.numel() // 2
    d_f0, d_mask = fm[:n_in], fm[n_in:]
    jit = next((j["kw"] for j in js if j["kw"].get("f0_jitter")), kw)
    sub = next((j["kw"] for j in js if j["kw"].get("add_subharm")), None)
    vol = next((j["kw"] for j in js if j["kw"].get("volume_jitter")), kw)
    vib = bool(vol.get("volume_jitter") and vol.get("volume_vibrato"))
    extra = {}
    if js[0]["stretched"]:
        env_n = c.gauss_bins(d_env, gaussian_taps(1.75))
        env_h = d_env
        if any(j["anchor"] or j["ratio"] != 1.0 for j in js):
            env_h = c.warp_bins_ragged(d_env, env_lens, F, [j["f_shift"] for j in js], [j["ratio"] for j in js], [j["anchor"] for j in js])
        env_h, env_n, d_f0, d_mask = c.stretch_ragged(env_h, env_n, env_lens, [j["e_cut"] for j in js], [j["rows_out"] for j in js],
                                                      d_f0, d_mask, [len(j["f0"]) for j in js], [j["s_cut"] for j in js], lens)
        d_env, F, env_lens = env_h, None, [j["rows_out"] for j in js]
        extra["env_noise"] = env_n
        if any(j["f0_64"] is not None for j in js):
            # the fp64 f0 of the notes with jitter or the sub-harmonic layer; the others hold their (exact) fp32 values widened
            f64 = d_f0.double()
            off = c.offsets(lens)
            idx = np.concatenate([np.arange(off[i], off[i + 1]) for i, j in enumerate(js) if j["f0_64"] is not None])
            f64[c.tensor(idx)] = c.tensor(np.concatenate([j["f0_64"] for j in js if j["f0_64"] is not None]))
            extra["f0_64"] = f64
    n_f0, n_sub, n_vh, n_vb = _pass_noise(c, js)
    out = c.synth_batch(d_env, env_lens, d_f0, d_mask, lens, params, formants=F, phi=d_phi, seed=0,
                        transition_sigma=float(kw.get("noise_transition_smoothness", 100)), want_mix=False,
                        noise_f0=n_f0, noise_vol=(n_vh, n_vb) if n_vh is not None else None,
                        f0_jitter_speed=float(jit.get("f0_jitter_speed", 100)), vol_jitter_speed=float(vol.get("volume_jitter_speed", 150)),
                        subharm=subharm_from_kwargs(sub) if sub is not None else None, volume_vibrato=vib,
                        noise_subharm=n_sub, **extra)
    s_off = out["sample_off"]
    rough = _roughness(c, js, out, d_mask, s_off, sr) if any(j["rough"] is not None for j in js) else {}
    host = {k: out[k].cpu().numpy() for k in ("rec", "harm", "uv", "bre")}
    return host, s_off, rough


def _rough_noise(c, host, lens, n_k):
    """The roughness layer's unfiltered noises of one setting group, fp64 [n_k x sum(lens)] flat: noise k of every note back to
    back.  ``host``: per note its host draws (an unseeded note: uploaded, zeros for the others) or None — a seeded note, whose
    rows are made in place by one float32-rounded job per partial (the generator re-seeded 1337 + k: nothing of the note's own
    seed reaches them).  A group of seeded notes uploads nothing."""
    N = sum(lens)
    if all(h is None for h in host):
        d_flat = torch.empty(n_k * N, dtype=torch.float64, device=c.device)
    else:
        d_flat = c.tensor(np.concatenate([h[k] if h is not None else np.zeros(ln) for k in range(n_k) for h, ln in zip(host, lens)]))
    o = c.offsets(lens)
    table = [(1337 + k, lens[q], [(d_flat, k * N + int(o[q]))], True) for k in range(n_k) for q, h in enumerate(host) if h is None]
    if table:
        c.legacy_normal_jobs(table)
    return d_flat


def _roughness(c, js, out, d_mask, s_off, sr):
    """gf.synthesize's roughness_on layer for the pass's notes that have it (only `reconstruct` hears it, GOOFER.py:1195-1217):
    one goofer_gauss_rows_f64 pair and one goofer_vocal_roughness per distinct setting, f0 as the synthesis left it from one
    fetch.  Returns {note position in the pass: roughened harmonic stem (host)}."""
    f0_all = c.debug_fetch("f0")                               # f0_interp as the synthesis left it (scaled, stretched, jittered)
    groups = {}
    for i, j in enumerate(js):
        if j["rough"] is not None:
            groups.setdefault(j["rough"][0], []).append(i)
    res = {}
    for (k_list, h_list, alpha, sig_n, sig_a, amp, fc), idxs in groups.items():
        sl = [slice(int(s_off[i]), int(s_off[i + 1])) for i in idxs]
        lens = [js[i]["n"] for i in idxs]
        cat = lambda t: torch.cat([t[s] for s in sl]) if len(sl) > 1 else t[sl[0]].contiguous()    # noqa: E731
        harm, mask = cat(out["harm"]), cat(d_mask)
        d_f0 = c.tensor(np.concatenate([f0_all[s] for s in sl]))
        nz = None
        if k_list:                                            # [n_k, N]: noise k of every note back to back, one ragged row each
            d_flat = _rough_noise(c, [js[i]["rough"][1] for i in idxs], lens, len(k_list))
            nz = c.gauss_rows_f64(d_flat, gaussian_taps(sig_n), lengths=lens * len(k_list)).reshape(len(k_list), -1)
        a_track = (mask.float() * np.float32(alpha)).double().contiguous()      # alpha * vmask in fp32, filtered in fp64
        a_slew = c.gauss_rows_f64(a_track, gaussian_taps(sig_a), lengths=lens).float()
        rough = c.vocal_roughness(harm, d_f0, mask, nz, list(k_list), list(h_list), amp, fc, a_slew, lengths=lens).cpu().numpy()
        o = np.concatenate([[0], np.cumsum(lens)])
        for q, i in enumerate(idxs):
            res[i] = rough[o[q]:o[q + 1]]
    return res


def synthesize_batch(notes, sr, n_fft=1024, hop_length=256, *, seeds=None, phis=None, phi_seeds=None, noise_seeds=None, ctx=None, **kw):
    """gf.synthesize for many notes in batched device passes -> one (reconstruct, harmonic, aper_uv, aper_bre) fp32 tuple per
    note, or the exception that note's ``synthesize`` call raises (an empty stretch region, more than sixteen sub-harmonic
    ratios, a non-1-D f0 or mask, ...).

    ``notes``: mappings with ``env_spec`` ([bins, T] fp32 / fp64 array or a knots dict), ``f0_interp``, ``voicing_mask`` and
    ``y`` (only its length is used), plus any ``synthesize`` keyword, which overrides ``**kw`` for that note.  One geometry
    (``sr``, ``n_fft``, ``hop_length``) per call.  ``seeds``: one Philox key per note (None entries or ``seeds=None``: a
    fresh key each, like ``synthesize(seed=None)``); ``phis``: one injected [bins, T] phase array (or None) per note;
    ``phi_seeds``: one numpy seed (or None) per note, ``synthesize(phi_seed=)`` — a note takes an array or a seed, not both.
    Seeded notes share their passes with array-injected ones; their phases are drawn on the device (goofer_phase_fill).
    ``noise_seeds``: one int in [0, 2**32) (or None) per note, ``synthesize(noise_seed=)``: note i renders what a reference
    process produces that calls ``np.random.seed(noise_seeds[i])`` immediately before ``gf.synthesize`` — its f0, sub-harmonic
    and volume jitter normals and its roughness noises are drawn on the device (goofer_legacy_normal_jobs), and numpy's global
    generator is neither read nor advanced for that note.  Seeded and unseeded notes share passes; the unseeded ones keep
    their host draws in note order, so the global state after the call is what those notes alone leave.

    Result i equals ``synthesize(**notes[i] merged over kw, sr=sr, ..., seed=seeds[i], phi=phis[i], phi_seed=phi_seeds[i],
    noise_seed=noise_seeds[i])`` bit for bit, and the legacy ``np.random`` state afterwards equals its state after those calls
    in list order: every host draw is made in note order before any device work.  Notes are cut into passes by ``synth_pass_key`` / ``plan_synth_passes``.  The
    returned arrays may be views into one host block per stem and pass: copy before writing in place.  An unknown keyword
    or ``seeds`` / ``phis`` of the wrong length raise before anything is drawn or launched, a bad legacy seed or ``noise_seeds``
    of the wrong length ValueError likewise; a note with ``len(y) == 0`` gives four empty arrays."""
    notes = list(notes)
    defaults = _synth_defaults()
    for name in list(kw) + [k for note in notes for k in note if k not in _NOTE_ARRAYS]:
        if name not in defaults:
            raise TypeError(f"synthesize() got an unexpected keyword argument '{name}'")
    for note in notes:
        missing = [k for k in _NOTE_ARRAYS if k not in note]
        if missing:
            raise TypeError(f"synthesize() missing required argument '{missing[0]}'")
    n = len(notes)
    seeds = [None] * n if seeds is None else list(seeds)
    phis = [None] * n if phis is None else list(phis)
    if len(seeds) != n or len(phis) != n:
        raise ValueError(f"synthesize_batch: {n} notes, {len(seeds)} seeds and {len(phis)} phase arrays")
    phi_seeds = _phase_seeds(phi_seeds, phis, n, "synthesize_batch")
    noise_seeds = _noise_seeds(noise_seeds, n, "synthesize_batch")
    c = _ctx(sr, n_fft, hop_length, ctx)
    base = {**defaults, **kw}
    results, jobs = [None] * n, [None] * n
    for i, note in enumerate(notes):
        merged = {**base, **{k: v for k, v in note.items() if k not in _NOTE_ARRAYS}}
        try:
            r = _prepare_note(c, note, merged, seeds[i], phis[i], sr, n_fft, hop_length, phi_seeds[i], noise_seeds[i])
        except Exception as e:                                  # the note's own refusal: its slot, the others render
            results[i] = e
            continue
        if isinstance(r, tuple):
            results[i] = r
        else:
            jobs[i] = r
    _render(c, jobs, results, sr)
    return results


def _render(c, jobs, results, sr):
    """The device half of synthesize_batch: the prepared ``jobs`` (None: nothing to render) cut into passes and rendered, each
    result into its slot of ``results``."""
    keys = [synth_pass_key(j["kw"], j["phi"] is not None or j["phi_seed"] is not None, j["f64_missing"]) if j is not None else None
            for j in jobs]
    for idxs in plan_synth_passes(keys, [j["frames"] if j is not None else 0 for j in jobs]):
        js = [jobs[i] for i in idxs]
        host, s_off, rough = _run_pass(c, js, sr)
        for q, i in enumerate(idxs):
            s = slice(int(s_off[q]), int(s_off[q + 1]))
            rec, harm, uv, bre = (host[k][s] for k in ("rec", "harm", "uv", "bre"))
            if q in rough:                                    # the peak gain of the roughened sum, like the reference
                combined = rough[q] + uv + bre
                peak = float(np.max(np.abs(combined)) + 1e-12)
                gain = (1.0 / peak) ** float(np.clip(js[q]["kw"].get("normalize", 1.0), 0.0, 1.0))
                rec, harm, uv, bre = combined * np.float32(gain), harm * np.float32(gain), uv * np.float32(gain), bre * np.float32(gain)
            results[i] = (rec, harm, uv, bre)


def resynthesize_batch(signals, sr, n_fft=1024, hop_length=256, *, f0_min=75, f0_merge_range=2, pitch_tracker=None, variants=None,
                       seeds=None, phis=None, phi_seeds=None, noise_seeds=None, ctx=None, **synth_kw):
    """The reference's wav-to-wav flow (GOOFER.py:1222-1330, test.py) for many signals: per signal ``extract_features``, then
    one ``synthesize`` per variant on those features.  Returns per signal a (reconstruct, harmonic, aper_uv, aper_bre) tuple
    (``variants=None``) or a list of them, one per variant (any ``variants`` list, one entry too); a signal whose analysis raised gets that exception in its slot,
    and a variant whose synthesis raised gets its exception in the list.  The other signals still render.

    ``signals``: mono arrays at one ``sr``.  ``variants``: keyword dicts, each layered over ``synth_kw``; ``formants`` defaults
    to the signal's own extracted formants, as both reference scripts pass them.  ``seeds`` / ``phis``: one Philox key / one
    injected phase array (or None) per (signal, variant), signal-major: entry ``i * len(variants) + v``; ``phi_seeds``: one numpy
    phase seed (or None) per (signal, variant) in the same order, ``synthesize(phi_seed=)`` — an array or a seed, not both.
    ``noise_seeds``: one legacy seed (an int in [0, 2**32), or None) per SIGNAL, given to each of its variants as
    ``synthesize(noise_seed=)``: every variant renders as if ``np.random.seed(noise_seeds[i])`` ran just before its
    ``synthesize``.  Its draws are made on the device and numpy's global generator is neither read nor advanced for it.

    Result (i, v) equals, bit for bit, ``env, f0, mask, forms, _ = extract_features(y_i, sr, n_fft, hop_length, f0_min=...,
    f0_merge_range=..., pitch_tracker=...)`` then ``synthesize(env, f0, mask, y_i, sr, n_fft, hop_length, formants=forms,
    **{**synth_kw, **variants[v]}, seed=..., phi=..., phi_seed=..., noise_seed=noise_seeds[i])`` run signal by signal and
    variant by variant, and the legacy ``np.random`` state afterwards is the state after those calls: every host draw is made in that order before the device
    work of its pass.  (A host tracker is called for the signals of an analysis pass before that pass's draws.)

    Signals are analysed in device passes of at most ``trackers.FRAME_BUDGET`` STFT frames (``trackers.plan_passes``); each
    analysis pass is synthesised (``plan_synth_passes``) before the next one starts, so device memory is bounded by a pass.
    The envelope, per-sample f0 and voicing mask stay on the device from analysis to synthesis (``trackers.analyse_device``);
    the one case that brings a signal's f0 to the host is a time-stretched variant with ``f0_jitter`` or ``add_subharm``,
    whose fp64 stretch is host arithmetic (``_stretch64``).  A one-frame f0 track is post-processed on the host.  An unknown
    keyword, ``seeds`` / ``phis`` of the wrong length, a bad legacy seed or ``noise_seeds`` of the wrong length raise before
    anything is analysed or drawn."""
    from . import trackers
    signals = list(signals)
    one = variants is None
    variants = [{}] if one else [dict(v) for v in variants]
    defaults = _synth_defaults()
    for name in list(synth_kw) + [k for v in variants for k in v]:
        if name not in defaults:
            raise TypeError(f"synthesize() got an unexpected keyword argument '{name}'")
    n, V = len(signals), len(variants)
    seeds = [None] * (n * V) if seeds is None else list(seeds)
    phis = [None] * (n * V) if phis is None else list(phis)
    if len(seeds) != n * V or len(phis) != n * V:
        raise ValueError(f"resynthesize_batch: {n} signals x {V} variants, {len(seeds)} seeds and {len(phis)} phase arrays")
    phi_seeds = _phase_seeds(phi_seeds, phis, n * V, "resynthesize_batch")
    noise_seeds = _noise_seeds(noise_seeds, n, "resynthesize_batch")
    c = _ctx(sr, n_fft, hop_length, ctx)
    track_fn = trackers.get(pitch_tracker)
    results = [None] * n
    entries = []
    for i, y in enumerate(signals):
        y = np.asarray(y)
        entries.append((i, int(sr), 1 + (y.shape[0] if y.ndim else 0) // int(hop_length)))
    for _, idxs in trackers.plan_passes(entries):
        feats = trackers.analyse_device([signals[i] for i in idxs], sr, n_fft, hop_length, f0_min, f0_merge_range, tracker=track_fn,
                                        ctx=c, want_env=True)
        c.plan(sr, n_fft, hop_length)
        jobs, slots = [], []
        for i, f in zip(idxs, feats):
            if isinstance(f, BaseException):
                results[i] = f
                continue
            note = {"env_spec": f["env"].T, "f0_interp": f["f0"], "voicing_mask": f["mask"], "y": signals[i]}
            out = [None] * V
            for v, var in enumerate(variants):
                merged = {**defaults, "formants": f["formants"], **synth_kw, **var}
                try:
                    r = _prepare_note(c, note, merged, seeds[i * V + v], phis[i * V + v], sr, n_fft, hop_length,
                                      phi_seeds[i * V + v], noise_seeds[i])
                except Exception as e:                          # the variant's own refusal: its slot, the others render
                    out[v] = e
                    continue
                if isinstance(r, tuple):
                    out[v] = r
                else:
                    jobs.append(r)
                    slots.append((out, v))
            results[i] = out
        rendered = [None] * len(jobs)
        _render(c, jobs, rendered, sr)
        for (out, v), r in zip(slots, rendered):
            out[v] = r
        del feats, jobs                                          # the pass's device buffers go before the next pass
    if one:
        results = [r if isinstance(r, BaseException) else r[0] for r in results]
    return results


def resynthesize(y, sr, n_fft=1024, hop_length=256, *, noise_seed=None, **kw):
    """``resynthesize_batch`` for one signal: its (reconstruct, harmonic, aper_uv, aper_bre), or a list of them with
    ``variants``.  ``noise_seed``: the signal's legacy seed (``resynthesize_batch(noise_seeds=[noise_seed])``).  Raises what the
    analysis or a synthesis raised."""
    res = resynthesize_batch([y], sr, n_fft, hop_length, noise_seeds=[noise_seed], **kw)[0]
    if isinstance(res, BaseException):
        raise res
    for r in res if isinstance(res, list) else ():
        if isinstance(r, BaseException):
            raise r
    return res


def _signal_arrays(signals):
    """``signals`` as contiguous fp32 1-D arrays: what the batch functions over finished audio plan for"""
    return [np.ascontiguousarray(s, dtype=np.float32).reshape(-1) for s in signals]


def _signal_tensor(c, xs):
    """the arrays back to back on ``c``'s device, one pad sample behind them (never an empty tensor)"""
    return c.tensor(np.concatenate(xs + [np.zeros(1, dtype=np.float32)]))


def _by_csr(flat, off):
    """a flat device result on the host, sliced by the CSR ``off``: one array per signal"""
    flat = flat.cpu().numpy()
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def resample_batch(signals, sr_in, sr_out, ctx=None):
    """Audio-rate conversion of many signals in one device pass (goofer_amd.rate; goofer_rate_convert): ``signals``, 1-D arrays
    at ``sr_in``, come back as a list of fp32 arrays at ``sr_out``, signal i with ceil(len_i * sr_out / sr_in) samples.  The
    converter is a polyphase Kaiser-windowed sinc, this project's own definition (include/goofer_hip.h); not GOOFER.py's
    stretch_feature, which interpolates feature rows.  ``sr_in == sr_out`` is refused: there is nothing to convert."""
    from . import rate as RT
    c = ctx or default_context()
    xs = _signal_arrays(signals)
    plan = RT.plan(sr_in, sr_out, [len(s) for s in xs])
    if not plan.total_out:
        return [np.zeros(0, dtype=np.float32) for _ in xs]
    y = c.rate_convert(_signal_tensor(c, xs), None, plan)
    c.check()
    return _by_csr(y, plan.out_off)


def limit_batch(signals, sr, ceiling=32767.0 / 32768.0, lookahead_ms=5.0, ctx=None, true_peak=False):
    """The look-ahead peak limiter over many signals in one device pass (goofer_amd.limit; goofer_limit): ``signals``, 1-D
    arrays at ``sr``, come back as a list of fp32 arrays of the same lengths whose samples stay within ``ceiling`` (0 < ceiling
    <= 1), with two fp32 arrays: per signal its greatest ``|x|`` and the smallest gain it was given (0 and 1 for an empty one).
    ``lookahead_ms``: how far ahead of a peak the gain starts to fall, and how long after it it recovers.  This project's own
    definition (include/goofer_hip.h); a signal that never exceeds the ceiling comes back bit for bit.  ``true_peak``: the
    ceiling holds for the signal reconstructed between the samples too (goofer_limit_tp; ``sr`` of 8000 to 192000 Hz), and the
    first statistic is the true peak."""
    from . import limit as LM
    xs = _signal_arrays(signals)
    plan = LM.plan(sr, [len(s) for s in xs], ceiling, lookahead_ms, bool(true_peak))
    if not plan.n:
        return [], np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32)
    c = ctx or default_context()
    y, peak, gain = c.limit(_signal_tensor(c, xs), None, plan)
    c.check()
    return _by_csr(y, plan.in_off), peak.cpu().numpy(), gain.cpu().numpy()


def true_peak_batch(signals, sr, ctx=None):
    """The true peak of many signals in one device pass (goofer_amd.limit; goofer_true_peak): ``signals``, 1-D arrays at ``sr``
    (8000 to 192000 Hz); returns fp32 ``[n]``, per signal the greatest magnitude, linear, of the signal reconstructed at 4 times
    its rate (2 times from 96 kHz on), 0 for an empty one — after ITU-R BS.1770-4 Annex 2, this project's own definition
    (include/goofer_hip.h).  ``limit.dbtp`` makes dBTP of one."""
    from . import limit as LM
    xs = _signal_arrays(signals)
    plan = LM.true_peak_plan(sr, [len(s) for s in xs])
    if not plan.n:
        return np.zeros(0, dtype=np.float32)
    c = ctx or default_context()
    peak = c.true_peak(_signal_tensor(c, xs), None, plan)
    c.check()
    return peak.cpu().numpy()


def loudness_batch(signals, sr, target=None, max_gain_db=20.0, ctx=None):
    """Integrated loudness of many signals in one device pass (goofer_amd.loudness; goofer_loudness_measure): ``signals``, 1-D
    arrays at ``sr`` (8000 to 192000 Hz), are measured after ITU-R BS.1770-4 for one channel and, with a ``target`` in LUFS,
    each scaled to it, the gain capped at ``max_gain_db``.  Returns ``(ys, loud, gain, seg_energy)``: the scaled signals as a
    list of fp32 arrays (None when ``target`` is None: measure only), ``loud`` float64 ``[n, 2]`` (integrated loudness and the
    greatest momentary loudness, LUFS; -inf for a signal without a block above the gates), ``gain`` fp32 ``[n]`` (1 where
    nothing was measured) and a list of float64 arrays, each signal's K-weighted energy per whole 100 ms segment
    (``loudness.momentary`` makes the momentary-loudness curve of one).  This project's own definition (include/goofer_hip.h)."""
    from . import loudness as LD
    xs = _signal_arrays(signals)
    plan = LD.plan(sr, [len(s) for s in xs])
    if target is not None:
        target, max_gain_db = LD.parse((target, max_gain_db))
    if not plan.n:
        return (None if target is None else []), np.zeros((0, 2)), np.zeros(0, dtype=np.float32), []
    c = ctx or default_context()
    y, loud, gain, seg = c.loudness(_signal_tensor(c, xs), None, plan, target, max_gain_db)
    c.check()
    return (None if y is None else _by_csr(y, plan.in_off)), loud.cpu().numpy(), gain.cpu().numpy(), _by_csr(seg, plan.seg_off)


def bus_mix(xs, sr, tracks, loudness=None, limit=None, ctx=None):
    """Finished tracks panned and mixed onto a stereo bus in one device pass (goofer_amd.bus; goofer_bus_mix): ``xs``, 1-D
    arrays at ``sr``, one ``bus.Track`` (or its ``(gain_db, pan, start_ms, mute)`` prefix) each.  ``loudness``: None, a target
    in LUFS or a ``(target, max_gain_db)`` pair: the stereo programme measured on the sum of the two channels' energies and
    both channels scaled by one gain (goofer_loudness_link).  ``limit``: None or what ``limit_batch``'s ``Renderer`` form
    takes (``limit.parse``; the true-peak triple included): the channel-linked limiter (goofer_limit_linked).  Returns the
    fp32 frames ``[N, 2]``, N the largest start + length of a track that sounds, and a dict of the stages' statistics
    (``lufs_in``, ``momentary_max``, ``gain``; ``peak_in``, ``min_gain``).  This project's own definition
    (include/goofer_hip.h)."""
    from . import bus as B
    from . import limit as LM
    from . import loudness as LD
    xs = _signal_arrays(xs)
    tracks = [t if isinstance(t, B.Track) else B.Track(*t) for t in tracks]
    loudness, limit = None if loudness is None else LD.parse(loudness), None if limit is None else LM.parse(limit)
    c = ctx or default_context()
    ds = [c.tensor(np.concatenate([x, np.zeros(1, dtype=np.float32)])) for x in xs]      # (never an empty tensor)
    plan = B.plan(ds, [len(x) for x in xs], tracks, sr)
    N, stats = plan.total_out, {}
    bus = c.bus_mix(ds, plan)
    if loudness is not None:
        bus, loud, gain, _ = c.loudness(bus, None, LD.plan(sr, [N, N]), *loudness, channels=2)
    if limit is not None:
        bus, peak, gmin = c.limit(bus, None, LM.plan(sr, [N, N], *limit, channels=2))
    c.check()
    if loudness is not None:
        stats.update({"lufs_in": float(loud.cpu()[0, 0]), "momentary_max": float(loud.cpu()[0, 1]), "gain": float(gain.cpu()[0])})
    if limit is not None:
        stats.update({"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0])})
    return np.ascontiguousarray(bus.cpu().numpy().reshape(2, N).T), stats


def compress_batch(signals, sr, threshold_db, ratio, knee_db=6.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0, curve=False, ctx=None):
    """Many signals through the dynamic range compressor in one device pass (goofer_amd.compress; goofer_compress): ``signals``,
    1-D arrays at ``sr`` (8000 to 192000 Hz), each compressed above ``threshold_db`` (dB re full scale) at ``ratio`` with a soft
    knee of ``knee_db``, a decoupled smooth peak detector with the time constants ``attack_ms`` and ``release_ms``, and
    ``makeup_db`` of gain.  Returns ``(ys, max_reduction)``: the compressed signals as a list of fp32 arrays and float64
    ``[n]``, every signal's greatest gain reduction in dB; with ``curve`` also a list of float64 arrays, the gain reduction in
    dB per sample.  This project's own definition (include/goofer_hip.h)."""
    from . import compress as CP
    xs = _signal_arrays(signals)
    plan = CP.plan(sr, [len(s) for s in xs], CP.Compressor(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db))
    if not plan.n:
        return ([], np.zeros(0), []) if curve else ([], np.zeros(0))
    c = ctx or default_context()
    y, red, yl = c.compress(_signal_tensor(c, xs), None, plan, curve=curve)
    c.check()
    return (_by_csr(y, plan.in_off), red.cpu().numpy(), _by_csr(yl, plan.in_off)) if curve else (_by_csr(y, plan.in_off), red.cpu().numpy())


def eq_batch(signals, sr, bands, ctx=None):
    """Many signals through the parametric equaliser in one device pass (goofer_amd.eq; goofer_eq): ``signals``, 1-D arrays at
    ``sr`` (8000 to 192000 Hz), each through the cascade of ``bands`` — ``eq.Band`` objects, ``(kind, f0_hz[, gain_db[, q]])``
    tuples or the string ``kind:f0[:gain_db[:q]],...``, at most eight, kinds ``highpass lowpass lowshelf highshelf peak notch``
    — run in float64 and rounded once.  Returns the filtered signals as a list of fp32 arrays of the same lengths; bands that
    are all the identity (0 dB shelves and peaks, or none) give the input's bits.  This project's own definition
    (include/goofer_hip.h)."""
    from . import eq as EQ
    xs = _signal_arrays(signals)
    plan = EQ.plan(sr, [len(s) for s in xs], bands)
    if not plan.total:
        return [np.zeros(0, dtype=np.float32) for _ in xs]
    c = ctx or default_context()
    y = c.eq(_signal_tensor(c, xs), None, plan)
    c.check()
    return _by_csr(y, plan.in_off)


def reverb_batch(signals, sr, reverb, ctx=None):
    """Many signals through the convolution reverb in one device pass (goofer_amd.reverb; goofer_reverb): ``signals``, 1-D arrays
    at ``sr`` (8000 to 192000 Hz), each convolved with the impulse response of ``reverb`` — a ``reverb.Reverb``, a tuple
    ``(ir[, wet_db[, dry_db[, predelay_ms[, tail]]]])`` with ``ir`` an array of up to 2^18 taps or a ``reverb.Room``, or the
    string ``room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]]`` / ``ir:PATH[:WET_DB[:PREDELAY_MS]]`` — and mixed with itself,
    ``dry x + wet (h * x)``.  Returns the signals as a list of fp32 arrays, each pre-delay + taps - 1 samples longer with the tail
    (the default; a signal without a sample stays empty).  This project's own definition (include/goofer_hip.h)."""
    from . import reverb as RV
    xs = _signal_arrays(signals)
    plan = RV.plan(sr, [len(s) for s in xs], reverb)
    if not plan.total_out:
        return [np.zeros(0, dtype=np.float32) for _ in xs]
    c = ctx or default_context()
    y = c.reverb(_signal_tensor(c, xs), None, plan, plan.reverb.spectra(c, plan.sr))
    c.check()
    return _by_csr(y, plan.out_off)


def synthesize(env_spec, f0_interp, voicing_mask, y, sr, n_fft=1024, hop_length=256, glottal_smoothing=False,
               stretch_factor=1.0, start_sec=None, end_sec=None, apply_brightness=True, normalize=1.0, uv_strength=0.75,
               breath_strength=0.1, noise_transition_smoothness=100, pitch_shift=1.0, formant_shift=1.0, f0_jitter=False,
               f0_jitter_speed=100, f0_jitter_strength=1.5, volume_jitter=False, volume_vibrato=False, volume_jitter_speed=150,
               volume_jitter_strength_harm=50, volume_jitter_strength_breath=100, add_subharm=False, subharm_semitones=-12,
               subharm_weight=0.5, subharm_vibrato=False, cut_subharm_below_f0=True, subharm_vibrato_rate=6.0,
               subharm_vibrato_depth=0.1, subharm_f0_jitter=0, subharm_vibrato_delay=0.1, F1_shift=1.0, F2_shift=1.0,
               F3_shift=1.0, F4_shift=1.0, formants=None, roughness_on=False, rough_k_list=(2, 3, 4), rough_h_list=None,
               rough_alpha=0.6, rough_hp_fc=320.0, rough_noise_amp=0.6, rough_noise_smooth_ms=120.0, rough_alpha_slew_ms=120.0,
               *, phi=None, phi_seed=None, noise_seed=None, seed=None, ctx=None):
    """gf.synthesize for one note on the GPU -> (reconstruct, harmonic, aper_uv, aper_bre), fp32: synthesize_batch of this
    one note.

    The positional order and keyword set are the reference's (GOOFER.py:971-983; ``glottal_smoothing`` is accepted and
    unused there too); an unknown keyword raises TypeError like it does there.  Five keyword-ONLY additions:
    ``phi`` ``[bins, T]`` injects the aperiodic branch's random phases (parity runs); ``phi_seed``, a non-negative integer
    of any size, injects the phases the reference draws with that seed — ``np.random.default_rng(phi_seed).uniform(0, 2 pi,
    (bins, T)).astype(float32)`` for the note's own frame count T (behind a time stretch: the stretched note's), made on the
    device, the same bits as passing that array as ``phi``; both together, or a negative seed, raise ValueError.  Otherwise
    the device draws the phases from Philox keyed by ``seed`` (a fresh key per call when None, like the reference's unseeded
    generator); ``ctx`` picks the device context.  ``noise_seed``, an integer in [0, 2**32) (anything else: ValueError), renders
    what a reference process produces that calls ``np.random.seed(noise_seed)`` immediately before ``gf.synthesize``: the
    f0, sub-harmonic f0, harmonic and breath volume jitter normals are one run of that seed's legacy stream and each
    roughness partial's noise is the stream of 1337 + idx, all drawn on the device (goofer_legacy_normal_jobs; equal to the
    host's draws up to the last place of ``log``).  numpy's global generator is then neither read nor advanced — not seeded
    with ``noise_seed``, and not left re-seeded by the roughness layer as the reference leaves it.  None (default): the draws
    come from the global generator on the host, as they always have."""
    note = {k: v for k, v in locals().items() if k not in ("sr", "n_fft", "hop_length", "phi", "phi_seed", "noise_seed", "seed", "ctx")}
    if phi is not None and phi_seed is not None:
        raise ValueError("synthesize: phi and phi_seed are exclusive; give one of them")
    phi_seed = check_phi_seed(phi_seed)
    res = synthesize_batch([note], sr, n_fft, hop_length, seeds=[seed], phis=[phi], phi_seeds=[phi_seed], noise_seeds=[noise_seed],
                           ctx=ctx)[0]
    if isinstance(res, BaseException):
        raise res
    return res
