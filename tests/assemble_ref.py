"""The note assembly (csrc/assemble.hip: k_env_edit, k_row_recs + k_env_rows, k_env_fry, k_sample_assemble) restated in plain
numpy, stage by stage, in two arithmetics.  TEST INFRASTRUCTURE ONLY.

Written from this project's own oracle, ``oracle/sampler_ref.py:assemble`` (346-571), which tests/test_oracle_sampler.py pins to
the reference's golden vectors; the oracle's small helpers (``segment_indices``, ``_loop_env_concat``, ``stretch_prefix_*``,
``sanitize_formant``, ``_canon_formants``; ``goofer_ref.gauss1d``, ``LinInterp``, ``stretch_feature``, ``lerp_plan``) are called,
the body of ``assemble`` is restated so that every stage a kernel writes can be looked at on its own:

``edited``   the note's source rows [start_frame, end_frame) after knot decode, br, es, fw (sampler_ref.py:351-409): the rows
             k_env_edit writes, in the note's logical order (``reverse`` applied), ``[rows, bins]``
``env``      after slicing / the L0, L1, L2 loops / the velocity prefix stretch / the formant-strength bells (:417-491)
``env_fry``  after the vf bin squeeze (:554-568); equal to ``env`` without vf
``mask``, ``f0``, ``bend`` (midi_curve - base, the pd side output, :505-506), ``f0_growl`` (f0 times the multiplier array handed in)
``decisions``  every index decision: cut points, the loop mode taken, the fractional source row of every output frame, fw lo /
             hi, the es clamp-at-zero sites, which bells are on in which frame, the fry rows with their lo / hi.

All matrices are returned frames-major (``[rows, bins]``: the device's layout); the oracle's are ``[bins, frames]``.

``exact=False``  the REFERENCE ARITHMETIC: the oracle's dtypes and order of operations; ``env_fry`` / ``f0`` / ``mask`` /
    ``formants`` equal ``sampler_ref.assemble`` bit for bit (tests/test_assemble_ref.py).  The bell loop is vectorised over
    frames (element-wise: the same bits).
``exact=True``   the TRUTH: the same steps in float64 from the fp16 knots (the fp32 lerp weights, bin-frequency tables and
    sanitised formant tracks are inputs), no intermediate rounding.  Every index decision, the es clamp sites among them, is
    taken from the ``exact=False`` run, so the two differ in rounding only.  The sample-domain outputs are float64 in the
    oracle already: the two runs agree on them.

THE JUDGEMENT (``errors`` / ``within``), per row so that quiet frames cannot hide behind loud ones: for a stage of one note,
``peak_t = max_b |truth[t, b]|``, ``e_x(t) = max_b |x[t, b] - truth[t, b]| / peak_t`` for x = the exact=False result cast to
fp32 and x = the device's, ``E_ref = max_t e_ref(t)``; every row must satisfy ``e_gpu(t) <= factor * E_ref + 2^-23`` (factor 3
unless a stage documents another), a row whose truth is all zero must be exactly zero.  The note-level E_ref is used because
rows that are plain copies have e_ref = 0 by construction.
"""
import numpy as np

from goofer_amd import synthetic as syn
from oracle import goofer_ref as G
from oracle import sampler_ref as SR

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -23
CHUNK = 64


# ---------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------
def _decode(pack, exact):
    """goofer_ref.decode_env_from_knots (:219-227); the truth takes the fp16 knots and the fp32 lerp weights to float64."""
    if not exact:
        return G.decode_env_from_knots(pack)
    vals = np.asarray(pack["knot_vals_log"]).astype(F64)
    hz = np.asarray(pack["hz_knots"]).astype(F32)
    n_fft, sr, n_bins = int(pack["n_fft"]), int(pack["sr"]), int(pack["n_bins"])
    idx, w0, w1 = G.lerp_plan(np.fft.rfftfreq(n_fft, 1.0 / sr).astype(F32), hz)
    return np.exp(w0.astype(F64)[:, None] * vals[idx] + w1.astype(F64)[:, None] * vals[idx + 1])[:n_bins]


def _frames(env_pre, env_tail, p, sr, hop):
    """Slicing, the three loop modes and the velocity prefix stretch of the frame axis (:417-430, :457, :465-468)."""
    want_f = int(np.ceil(p.length * sr / hop))
    n_tail = env_tail.shape[1]
    if n_tail >= want_f:
        mode, tail_env = "slice", env_tail[:, :want_f]
    else:
        reps, rem = want_f // n_tail, want_f % n_tail                 # ZeroDivisionError on an empty tail, like the oracle
        if p.loop_mode == "stretch":
            mode, tail_env = "stretch", G.stretch_feature(env_tail, want_f / n_tail)
        elif p.loop_mode == "avg":
            tile = (env_tail + env_tail[:, ::-1]) / 2.0
            mode, tail_env = "avg", np.concatenate([tile] * reps + ([tile[:, :rem]] if rem else []), axis=1)
        else:
            mode, tail_env = "concat", SR._loop_env_concat(env_tail, want_f)
    return mode, want_f, np.concatenate([env_pre, tail_env], axis=1)


def _stages(features, p, hop, exact, dec, f0_mul, mutate):
    env_spec, f0_src, vmask, forms, sr, ylen = features
    f0_src, vmask = np.array(f0_src), np.array(vmask)                 # (the oracle edits its inputs in place: copies here)
    forms = {k: np.array(v) for k, v in forms.items()}
    mutate = mutate or {}
    if isinstance(env_spec, dict) and env_spec.get("mode") == "knots":
        env_spec = _decode(env_spec, exact)
    else:
        env_spec = np.array(env_spec, dtype=F64) if exact else np.array(env_spec)
    out_dec = {}
    if p.reverse:                                                     # :353-357
        env_spec = env_spec[:, ::-1]
        f0_src = f0_src[::-1]
        vmask = vmask[::-1]
        forms = {k: list(forms[k])[::-1] for k in forms}
    seg = SR.segment_indices(p, sr, ylen, hop)
    s0, s1, s2 = seg["start_sample"], seg["consonant_sample"], seg["end_sample"]
    f_0, f_1, f_2 = seg["start_frame"], seg["consonant_frame"], seg["end_frame"]
    out_dec["seg"] = seg

    env_pre, env_tail = env_spec[:, f_0:f_1], env_spec[:, f_1:f_2]
    f0_pre, f0_tail = f0_src[s0:s1], f0_src[s1:s2]
    mask_pre, mask_tail = vmask[s0:s1], vmask[s1:s2]

    if p.brightness_env != 1.0 and (env_pre.size or env_tail.size):   # br, :366-375
        nb = env_spec.shape[0]
        fr = np.linspace(1e-6, sr * 0.5, nb, dtype=F32)
        nf = np.clip(fr / (sr * 0.5), 0.02, 1.0)
        if exact:
            nf = nf.astype(F64)
        tilt = nf ** np.clip(p.brightness_env - 1.0, -0.9, 1.0)
        tilt /= (tilt.mean() + 1e-12)
        if env_pre.size:
            env_pre *= tilt[:, None].astype(env_pre.dtype)
        if env_tail.size:
            env_tail *= tilt[:, None].astype(env_tail.dtype)

    if p.env_shape != 0.0 and (env_pre.size or env_tail.size):        # es, :377-393
        s = abs(p.env_shape)

        def rematch(orig, mod):
            m0 = np.mean(orig, axis=0, keepdims=True)
            m1 = np.mean(mod, axis=0, keepdims=True)
            return (mod * (m0 / (m1 + 1e-12))).astype(orig.dtype)

        def clamp0(x, key):
            """np.maximum(0.0, x); the truth clamps where the reference arithmetic did."""
            if not exact:
                out_dec[key] = x < 0
                return np.maximum(0.0, x)
            return np.where(dec[key], 0.0, x).astype(x.dtype)

        def shape_block(b, key):
            if not b.size:
                return b
            blur = G.gauss1d(b, (1.0 + 6.0 * s) if p.env_shape < 0.0 else (0.8 + 4.0 * s), axis=0)
            if key == "es_clamp_tail" and "es_shift_frame" in mutate:   # (test_assemble_ref: the window one bin off on one row)
                t = mutate["es_shift_frame"]
                blur[:, t] = np.roll(blur[:, t], 1)
            if p.env_shape < 0.0:
                return clamp0(rematch(b, blur), key)
            out = b + (5 * s) * (b - blur)
            return rematch(b, clamp0(out, key))

        env_pre, env_tail = shape_block(env_pre, "es_clamp_pre"), shape_block(env_tail, "es_clamp_tail")

    if p.formant_width != 0.0 and env_spec.size:                      # fw, :395-409
        def widen(e):
            nb = e.shape[0]
            c = nb / 2.0
            w = np.clip((np.arange(nb, dtype=np.float64) - c) * (1.0 + p.formant_width) + c, 0, nb - 1)
            lo = np.floor(w).astype(int)
            hi = np.minimum(lo + 1, nb - 1)
            out_dec["fw_lo"], out_dec["fw_hi"] = lo, hi
            fr = (w - lo)[:, None]
            out = np.empty_like(e)
            out[:] = (1 - fr) * e[lo, :] + fr * e[hi, :]
            return out
        if env_pre.size:
            env_pre = widen(env_pre)
        if env_tail.size:
            env_tail = widen(env_tail)

    edited = np.concatenate([env_pre, env_tail], axis=1).T.copy()     # what k_env_edit leaves: rows f_0 .. f_2

    if p.force_voiced:                                                # FV, :411-415
        if mask_pre.size:
            mask_pre[:] = 1.0
        if mask_tail.size:
            mask_tail[:] = 1.0

    want_s = int(p.length * sr)                                       # :417-438
    mode, want_f, env_new = _frames(env_pre, env_tail, p, sr, hop)
    rows = np.arange(env_spec.shape[1], dtype=F64)[None, :]           # the same walk over the row numbers: which rows land where
    _, _, tap_rows = _frames(rows[:, f_0:f_1], rows[:, f_1:f_2], p, sr, hop)
    out_dec["loop"] = mode

    n_ts = len(f0_tail)
    if n_ts >= want_s:
        f0_loop, mask_loop = f0_tail[:want_s], mask_tail[:want_s]
    else:
        reps, rem = want_s // n_ts, want_s % n_ts
        f0_loop = np.concatenate([f0_tail] * reps + ([f0_tail[:rem]] if rem else []))
        mask_loop = np.concatenate([mask_tail] * reps + ([mask_tail[:rem]] if rem else []))

    fm_new = {}
    for k in forms:                                                   # :440-455
        pre = forms[k][f_0:f_1]
        tr = np.asarray(forms[k][f_1:f_2], dtype=F32)
        if tr.size == 0:
            lp = np.zeros(want_f, dtype=F32)
        elif p.loop_mode == "stretch":
            lp = G.stretch_feature(tr, want_f / float(tr.size)).astype(F32)
        else:
            reps, rem = want_f // tr.size, want_f % tr.size
            tile = (tr + tr[::-1]) * 0.5 if p.loop_mode == "avg" else tr
            lp = np.tile(tile, reps)
            if rem > 0:
                lp = np.concatenate([lp, tile[:rem]])
            lp = lp.astype(F32)
        fm_new[k] = np.concatenate([pre, lp])

    f0_new = np.concatenate([f0_pre, f0_loop])                        # :457-463
    mask_new = np.concatenate([mask_pre, mask_loop])
    T_target = env_new.shape[1]
    for k in fm_new:
        f = fm_new[k]
        fm_new[k] = np.pad(f, (0, T_target - len(f)), mode="edge") if len(f) < T_target else f[:T_target]

    vel = float(2.0 ** (1.0 - (p.velocity / 100.0)))                  # :465-474
    n_pre_f, n_pre_s = env_pre.shape[1], len(f0_pre)
    out_dec["vel_active"] = bool(abs(vel - 1.0) > 1e-6 and n_pre_f > 1 and n_pre_s > 1)
    if out_dec["vel_active"]:
        env_new = SR.stretch_prefix_2d(env_new, n_pre_f, vel)
        tap_rows = SR.stretch_prefix_2d(tap_rows, n_pre_f, vel)
        Tn = env_new.shape[1]
        for k in list(fm_new):
            f = SR.stretch_prefix_1d(np.asarray(fm_new[k], dtype=np.float64), n_pre_f, vel)
            fm_new[k] = np.pad(f, (0, Tn - len(f)), mode="edge") if len(f) < Tn else f[:Tn]
        f0_new = SR.stretch_prefix_1d(f0_new, n_pre_s, vel)
        mask_new = SR.stretch_prefix_1d(mask_new, n_pre_s, vel)
    out_dec["tap_rows"] = tap_rows[0]

    fm_new = SR._canon_formants(fm_new, T_target)                     # :476-491, the loop over frames vectorised
    T = env_new.shape[1]
    tracks = [SR.sanitize_formant(fm_new.get(nm, np.zeros(T)), T, sr, min_hz=lo, sigma_frames=4)
              for nm, lo in (("F1", 120.0), ("F2", 300.0), ("F3", 1500.0), ("F4", 2000.0))]
    fr = np.linspace(0.0, sr / 2.0, env_new.shape[0], dtype=F32)
    frx = fr.astype(F64) if exact else fr
    gain = np.ones_like(env_new, dtype=F64 if exact else F32)
    bell_on = np.zeros((4, T), dtype=bool)
    for k, (tr, sv, sg) in enumerate(zip(tracks, p.formant_strength, (100.0, 200.0, 350.0, 500.0))):
        if abs(sv) < 1e-6:
            continue
        fc64 = tr.astype(F64)                                         # float(tr[t])
        on = np.isfinite(fc64) & ~(fc64 <= 50.0) & ~(fc64 >= (sr * 0.5))
        bell_on[k] = on
        if not on.any():
            continue
        fc = fc64[on] if exact else tr[on]                            # (fp32 array - python float: fp32, the value is an fp32 already)
        w = np.exp(-0.5 * ((frx[:, None] - fc[None, :]) / sg) ** 2)
        if not exact:
            w = w.astype(F32)
        if mutate.get("bell_skip", (None,))[0] == k:                   # (test_assemble_ref: a bell left out of one 64-bin chunk)
            _, t, c = mutate["bell_skip"]
            w[c * CHUNK:(c + 1) * CHUNK, int(np.count_nonzero(on[:t]))] = 0.0
        gain[:, on] *= 1.0 + ((1.0 + sv) - 1.0) * w
    out_dec["bell_on"] = bell_on
    env_new = env_new * gain                                          # (env_new *= gain: the product keeps env_new's dtype either way)
    env = env_new.T.copy()

    n_tot = len(f0_new)                                               # pitch curve, :493-501
    t_s = np.arange(n_tot) / sr
    semis = p.bend.astype(np.float64) / 100.0 + p.pitch_m
    tc = p.flags.get("t", 0)
    if tc:
        semis = semis + (tc / 100.0)
    t_p = np.arange(len(semis)) * (60.0 / (p.tempo * 96.0))
    midi_curve = G.LinInterp(t_p, semis)(np.clip(t_s, t_p[0], t_p[-1]))
    f0_new = mask_new * SR.midi_to_hz(midi_curve)

    bend = None                                                       # pd, :503-506 (what the device hands the post chain)
    if p.pitch_dyn != 0.0:
        bend = midi_curve - (p.pitch_m + ((p.flags.get("t", 0) or 0) / 100.0))

    vf = float(p.flags.get("vf", 0))                                  # fry, :513-568
    vh = max(1.0, float(p.flags.get("vh", 50)))
    vl = np.clip(float(p.flags.get("vl", 15)), 0.0, 100.0)
    fry_mask = None
    if vf != 0:
        vf = float(np.clip(vf, -100.0, 100.0))
        n = len(f0_new)
        L = int(round(n * (abs(vf) / 100.0)))
        if L > 0:
            gl = int(np.clip(int(round(L * (vl / 100.0))), 0, L))
            cl = L - gl
            if vf > 0:
                if cl > 0:
                    f0_new[:cl] = vh * (mask_new[:cl] > 0)
                if gl > 0:
                    w = np.linspace(0.0, 1.0, gl, endpoint=True)
                    f0_new[cl:L] = (1.0 - w) * (vh * (mask_new[cl:L] > 0)) + w * f0_new[cl:L]
            else:
                st = n - L
                if gl > 0:
                    w = np.linspace(1.0, 0.0, gl, endpoint=True)
                    sl = slice(st, st + gl)
                    f0_new[sl] = (1.0 - w) * (vh * (mask_new[sl] > 0)) + w * f0_new[sl]
                if cl > 0:
                    f0_new[st + gl:n] = vh * (mask_new[st + gl:n] > 0)
        mid = n // 2
        if vf > 0:
            a, b = 0, max(0, min(n, int(round(mid * (vf / 100.0)))))
        else:
            a, b = max(0, n - int(round((n - mid) * (abs(vf) / 100.0)))), n
        if b > a:
            fry_mask = np.zeros(n, dtype=F32)
            fry_mask[a:b] = 1.0
            fade = int(0.01 * sr)
            if fade > 0:
                a1 = min(b, a + fade)
                if a1 > a:
                    fry_mask[a:a1] *= np.linspace(0.0, 1.0, a1 - a, endpoint=True)
                b0 = max(a, b - fade)
                if b > b0:
                    fry_mask[b0:b] *= np.linspace(1.0, 0.0, b - b0, endpoint=True)
    fry_rows = []
    if fry_mask is not None and env_new.size:
        nb, nf = env_new.shape
        centers = np.minimum(len(fry_mask) - 1, (np.arange(nf) * hop + hop // 2)).astype(int)
        fm_fr = fry_mask[centers]
        bins = np.arange(nb, dtype=np.float64)
        for j in np.nonzero(fm_fr > 1e-6)[0]:
            s = 1.0 - float(fm_fr[j]) * (1.0 - 0.92)
            if abs(s - 1.0) < 1e-6:
                continue
            src = np.clip(bins / s, 0.0, nb - 1.0)
            lo = np.floor(src).astype(np.int32)
            hi = np.minimum(lo + 1, nb - 1)
            fr_ = src - lo
            col = env_new[:, j]
            env_new[:, j] = (1.0 - fr_) * col[lo] + fr_ * col[hi]
            fry_rows.append(int(j))
    out_dec["fry_rows"] = fry_rows

    return {"edited": edited, "edit_lo": f_0, "env": env, "env_fry": env_new.T.copy(), "mask": mask_new, "f0": f0_new, "bend": bend,
            "f0_growl": None if f0_mul is None else f0_new * np.asarray(f0_mul, dtype=F64), "formants": fm_new, "fry_mask": fry_mask,
            "decisions": out_dec}


def stages(features, params, hop, exact=False, f0_mul=None, decisions=None, _mutate=None):
    """The stages of one note (module docstring).  ``exact=True`` runs the reference arithmetic first for its decisions unless
    they are handed in (``decisions`` of an ``exact=False`` result)."""
    if exact and decisions is None:
        decisions = _stages(features, params, hop, False, None, f0_mul, _mutate)["decisions"]
    return _stages(features, params, hop, exact, decisions, f0_mul, _mutate)


def both(features, params, hop, f0_mul=None):
    """(reference arithmetic, truth) of one note."""
    ref = stages(features, params, hop, f0_mul=f0_mul)
    return ref, stages(features, params, hop, exact=True, f0_mul=f0_mul, decisions=ref["decisions"])


# ---------------------------------------------------------------------------------------------
# the judgement
# ---------------------------------------------------------------------------------------------
def row_errors(x, truth):
    """e_x(t) of every row of ``x`` [rows, bins] against ``truth``; a row whose truth is all zero has error 0 if x is exactly
    zero there and inf otherwise.  A value that is not finite makes the row's error nan, which no bound admits."""
    x, truth = np.asarray(x, dtype=F64), np.asarray(truth, dtype=F64)
    assert x.shape == truth.shape, (x.shape, truth.shape)
    if x.size == 0:
        return np.zeros(x.shape[0])
    peak = np.max(np.abs(truth), axis=1)
    d = np.max(np.abs(x - truth), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(peak > 0.0, d / peak, np.where(d == 0.0, 0.0, np.inf))


def errors(gpu, ref, truth):
    """(E_ref of the note, e_gpu per row) for one stage of one note; ``ref`` is cast to fp32 first (what a device can store)."""
    e_ref = row_errors(np.asarray(ref).astype(F32), truth)
    return (float(e_ref.max()) if e_ref.size else 0.0), row_errors(gpu, truth)


def within(E_ref, e_gpu, factor=3.0):
    """Every row inside factor * E_ref + 2^-23."""
    return bool(np.all(np.asarray(e_gpu) <= factor * E_ref + EPS32))


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two fp32 arrays (sign-magnitude order; +0 and -0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------
# the cases: one matrix per geometry, shared by tests/test_assemble_ref.py (CPU) and tests/test_gpu_assemble_oracle.py
# ---------------------------------------------------------------------------------------------
GEOMETRIES = [(44100, 1024, 256), (48000, 2048, 512), (22050, 512, 128), (44100, 1100, 275), (44100, 1150, 250), (44100, 768, 192),
              (44100, 600, 150), (16000, 64, 16), (44100, 2046, 512)]
GEO_IDS = ["%d_%d_%d" % g for g in GEOMETRIES]

# (family, flags, keyword changes of the request); the families are the rows of the E_ref table
_FLAG_CASES = [
    ("plain", "", {}), ("br", "br40", {}), ("br", "br-60", {}),
    ("es", "es-80", {}), ("es", "es-10", {}), ("es", "es10", {}), ("es", "es80", {}),
    ("fw", "fw80", {}), ("fw", "fw-80", {}),
    ("bells", "fsta40", {}), ("bells", "fsta-40", {}), ("bells", "fstb40", {}), ("bells", "fstb-40", {}), ("bells", "fstc40", {}),
    ("bells", "fstc-40", {}), ("bells", "fstd40", {}), ("bells", "fstd-40", {}), ("bells", "fsta40fstb-40fstc40fstd-40", {}),
    ("vf", "vf40vl0", {}), ("vf", "vf-40vl100", {}), ("vf", "vf60vl100", {}), ("vf", "vf-60vl0", {}),
    ("plain", "FV1", {}), ("plain", "R1", {}),
    ("loops", "L0", {"short_tail": True, "length_ms": 300.0}), ("loops", "L0", {"length_ms": 500.0}),
    ("loops", "L1", {"length_ms": 450.0}), ("loops", "L2", {"length_ms": 500.0}),
    ("velocity", "", {"velocity": 0.0}), ("velocity", "", {"velocity": 60.0}), ("velocity", "", {"velocity": 140.0}),
    ("velocity", "", {"velocity": 200.0}),
    ("plain", "pd50", {}), ("plain", "pd-50", {}), ("plain", "sj30", {}),
]
SAMPLE_COUNTS = (1023, 1024, 1025, 4097)


def edge_formant_source(seed, sr, n_fft, hop, seconds):
    """make_source with F1 a few Hz above the sanitiser's 120 Hz floor (1.3 of the F1 bell's 100 Hz sigma from 0 Hz: as close as a
    sanitised track gets) and F4 just below its 0.48 sr ceiling (0.02 sr from Nyquist: inside the F4 bell's 500 Hz sigma at 16
    and 22.05 kHz), with stretches beyond both limits that the sanitiser has to bridge."""
    src = syn.make_source(seed, sr, n_fft, hop, seconds)
    T = 1 + src["y_len"] // hop
    t = np.arange(T, dtype=F64)
    f = {k: v.copy() for k, v in src["formants"].items()}
    f[1] = 127.0 + 5.0 * np.sin(t / 5.0)
    f[4] = 0.4795 * sr - 0.002 * sr * (1.0 + np.sin(t / 3.0))
    f[1][T // 3:T // 3 + 3] = 60.0
    f[4][T // 2:T // 2 + 2] = 0.49 * sr
    return dict(src, formants=f)


def _request(seed, flags, sr, length_ms=160.0, offset_ms=20.0, consonant_ms=40.0, cutoff_ms=20.0, velocity=100.0, hop=256,
             short_tail=False, samples=None):
    if short_tail:                                                    # a tail of five frames: shorter than the L0 cross-fade's 2 x 8
        cutoff_ms = -(consonant_ms + 5.5 * hop * 1000.0 / sr)
    req = syn.make_request(seed, flags, length_ms=length_ms, offset_ms=offset_ms, consonant_ms=consonant_ms, cutoff_ms=cutoff_ms,
                           velocity=velocity)
    if samples is not None:                                           # int(length * sr) == samples, no consonant
        req["consonant"] = "0"
        req["length"] = repr((samples + 0.5) * 1000.0 / sr)
    return req


def matrix(sr, n_fft, hop):
    """The notes of one geometry: dicts with ``name``, ``family``, ``src`` (a synthetic source dict), ``req`` (the request dict)
    and ``hard`` (made by make_hard_source).  Plain and hard sources alternate; seeds are fixed, and every request is one the
    oracle accepts."""
    cases = []

    def add(family, name, src, req):
        cases.append({"name": name, "family": family, "src": src, "req": req, "hard": bool(src.get("hard"))})

    def source(i, hard=None):
        secs = 0.25 + 0.05 * (i % 4)
        hard = bool(i % 2 if hard is None else hard)
        return dict((syn.make_hard_source if hard else syn.make_source)(7000 + i, sr, n_fft, hop, seconds=secs), hard=hard)

    for i, (family, flags, kw) in enumerate(_FLAG_CASES):
        kw = dict(kw)
        kw.setdefault("length_ms", 120.0 + 20.0 * (i % 8))
        add(family, "%s_%d" % (flags or "plain", i) + "".join("_%s%g" % (k[:3], v) for k, v in kw.items() if k == "velocity"),
            source(i), _request(7100 + i, flags, sr, hop=hop, **kw))
    i = len(_FLAG_CASES)
    add("bells", "edge_formants", edge_formant_source(7000 + i, sr, n_fft, hop, 0.3),
        _request(7100 + i, "fsta40fstd40", sr, hop=hop, length_ms=200.0))
    add("bells", "edge_formants_neg", edge_formant_source(7001 + i, sr, n_fft, hop, 0.3),
        _request(7101 + i, "fsta-40fstd-40L1", sr, hop=hop, length_ms=420.0))
    for k in range(6):                                                # every flag at once
        rng = np.random.default_rng(7300 + k)
        add("random", "random_%d" % k, source(i + 2 + k), _request(7200 + k, syn.random_flags(rng), sr, hop=hop,
                                                                   length_ms=float(rng.integers(120, 501)),
                                                                   velocity=float(rng.choice([60, 100, 100, 140]))))
    for k, n in enumerate(SAMPLE_COUNTS):                             # the tile of k_sample_assemble<4> and its neighbours
        add("plain", "samples_%d" % n, source(i + 8 + k, hard=k % 2), _request(7400 + k, "", sr, hop=hop, samples=n))
    add("plain", "under_one_hop", source(i + 12, hard=1), _request(7410, "", sr, hop=hop, samples=max(1, hop // 2)))
    add("plain", "no_consonant", source(i + 13, hard=0), _request(7411, "fstb40", sr, hop=hop, consonant_ms=0.0, length_ms=140.0))
    return cases


CROSSING_SHIFTS = ("fa30fb-20fc10fd-10", "fa50fb-40fc-30fd40", "fa-30fb30fc30fd-40")   # test_warp_bins_crossing_anchors_follow_numpy_interp


def has_flag(case, name):
    return bool(SR.parse_flags(case["req"]["flags"]).get(name) or 0)


def fused_matrix(sr, n_fft, hop):
    """The hard-source notes of ``matrix`` with formant shifts whose anchors cross (the three ratio sets in turn, every other
    note with 'g' for the uniform stage as well), as (index in the matrix, case) in two groups: the notes whose batch may take
    the fused warp (no 'vf': launch_assemble keeps the warp apart for a batch with a fry edit; no 'sg' / 'sr': Renderer.run
    assembles on its own for a batch that mixes them with others), and the rest."""
    fused, rest = [], []
    for i, c in enumerate(matrix(sr, n_fft, hop)):
        if not c["hard"]:
            continue
        req = dict(c["req"], flags=c["req"]["flags"] + CROSSING_SHIFTS[(i // 2) % 3] + ("g50" if (i // 2) % 2 else ""))
        (rest if any(has_flag(c, k) for k in ("vf", "sg", "sr")) else fused).append((i, dict(c, req=req)))
    return fused, rest


def features_of(src):
    """The oracle's ``features`` tuple of a synthetic source (copies: the oracle edits its inputs in place)."""
    return (src["env_pack"], src["f0"].copy(), src["mask"].copy(), {k: v.copy() for k, v in src["formants"].items()}, src["sr"],
            src["y_len"])


def growl_factor(case_index, n):
    """The sj layer's multiplier array the tests supply themselves: 0.5 * 2^N(0, 0.09), seeded by the case."""
    return 0.5 * 2.0 ** np.random.default_rng(7500 + case_index).normal(0.0, 0.09, n)
