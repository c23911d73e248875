"""The sample-domain stages in front of the spectra that the sh / sr / sg flags drive (csrc/jitter.hip, the sub-harmonic layer of
csrc/pulse.hip, their glue in csrc/synth.hip) restated per note in plain numpy.  TEST INFRASTRUCTURE ONLY.

Every function performs the reference's operations in the reference's precisions, as the kernels' comments cite them
(GOOFER.py:638-766, 1069-1097, 1185-1193): float64 wherever numpy makes float64 of it, fp32 where the reference holds an fp32
array (the f0 it multiplies in place, the sub-harmonic pulse's time grid and its stored samples, the stems).

  smooth_fir / smooth_noise   gaussian_filter1d along the samples ('reflect' padding, repeated for a note shorter than the
                              radius; one sample degenerates to 'edge'), summed in ascending tap order, / max(|x| + 1e-6)
  f0_after_jitter             f0 * (1 + ((1 + noise_s / max * strength) - 1) * mask)
  volume_gains                1 + (j - 1) * vjm for the harmonic and the breath stem, noise or vibrato form
  sub_layer                   vibrato, increments, the wrapped tracker, the two-decimal pulse cache, the LF pulses, the sum
  cases                       the ragged batch of tests/test_gpu_presynth_stages.py

The keyword arguments after ``variant`` names build WRONG variants (half-up rounding, no key cache, end_max without its carry, a
covering set of the latest event only, 'symmetric' padding, a maximum without + 1e-6): tests/test_presynth_ref.py shows that each
of them breaks the bound the GPU test asserts, i.e. that the GPU test would notice the kernel doing the same.
"""
import functools
import math

import numpy as np

from oracle import goofer_ref as R

F32, F64 = np.float32, np.float64

GEO = (44100, 1024, 256)
LENGTHS = (6000, 3, 100, 255, 1, 257, 1023, 256, 2048, 1025)
C_PULSE = 7.0        # the c of the layer's bound: derived in tests/test_gpu_presynth_stages.py


# ---------------------------------------------------------------------------------------------
# smoothing                                                                 GOOFER.py:654-655, 667-668, 1189
# ---------------------------------------------------------------------------------------------
def smooth_fir(x, sigma, pad="reflect"):
    """The normalised Gaussian FIR of radius int(4 sigma + .5) over x (any float type, taken to float64 sample by sample) with
    numpy's padding; ascending tap order, one product and one addition per tap."""
    x = np.asarray(x).astype(F64)
    k, r = R.gauss_taps(float(sigma))
    if k is None:
        return x.copy()
    p = np.pad(x, (r, r), mode=pad)
    out = np.zeros(x.size, dtype=F64)
    for j in range(k.size):
        out += k[j] * p[j:j + x.size]
    return out


def smooth_noise(z, sigma, pad="reflect", eps=1e-6):
    """(smoothed z / max, max) with max = np.max(|smoothed| + 1e-6)."""
    s = smooth_fir(z, sigma, pad)
    mx = float(np.max(np.abs(s) + eps))
    return s / mx, mx


# ---------------------------------------------------------------------------------------------
# 'sh': f0 jitter                                                            GOOFER.py:662-670, 1069-1071
# ---------------------------------------------------------------------------------------------
def f0_after_jitter(f0_scaled, mask, noise, strength, sigma, f0_64=None, pad="reflect", eps=1e-6):
    """(float64 product, its fp32 cast).  ``f0_scaled``: fp32 f0 * pitch_shift; ``f0_64``: the float64 array that takes the
    product instead (the reference's f0 behind its time stretch).  strength <= 0: the arrays as they came."""
    f32 = np.asarray(f0_scaled, dtype=F32)
    base = f32.astype(F64) if f0_64 is None else np.asarray(f0_64, dtype=F64)
    if not strength > 0.0:
        return base.copy(), (f32.copy() if f0_64 is None else base.astype(F32))
    s, _ = smooth_noise(noise, sigma, pad, eps)
    jit = 1.0 + s * float(strength)
    fac = 1.0 + (jit - 1.0) * np.asarray(mask, dtype=F32).astype(F64)
    v = base * fac
    return v, v.astype(F32)


# ---------------------------------------------------------------------------------------------
# 'sr': volume jitter                                                        GOOFER.py:638-660, 1185-1191
# ---------------------------------------------------------------------------------------------
def vibrato_env(n, sr, speed):
    """gf.create_volume_jitter(vibrato=True) before its strength and clip: zero-phase sine, 0.1 s fade-in when shorter than n."""
    z = np.sin(2 * np.pi * float(speed) * (np.arange(n) / float(sr)) + 0)
    fade = int(0.1 * sr)
    if fade < n:
        z[:fade] *= np.linspace(0, 1, fade)
    return z


def volume_gains(n, sr, mask, noise_h, noise_b, sh, sb, speed, vibrato, pad="reflect", eps=1e-6):
    """The factors (harm, breath) as float64 arrays.  sh / sb: the strengths as the fp32 parameters hold them."""
    sh, sb = float(F32(sh)), float(F32(sb))
    vjm = smooth_fir(np.asarray(mask, dtype=F32), 20.0, pad)
    if vibrato:
        z = vibrato_env(n, sr, speed)
        jh = np.clip(1.0 + z * sh, 0.5, 1.5)
        jb = np.clip(1.0 + z * sb, 0.5, 1.5)
    else:
        sigma = sr / (float(speed) * 6)
        jh = 1.0 + smooth_noise(noise_h, sigma, pad, eps)[0] * sh
        jb = 1.0 + smooth_noise(noise_b, sigma, pad, eps)[0] * sb
    return 1.0 + (jh - 1.0) * vjm, 1.0 + (jb - 1.0) * vjm


# ---------------------------------------------------------------------------------------------
# 'sg': the sub-harmonic layer                                               GOOFER.py:437-471, 672-766, 1076-1097
# ---------------------------------------------------------------------------------------------
def sub_vibrato(f0, sr, vib, keep64):
    """apply_subharm_vibrato on an fp32 (keep64: float64) array: voiced samples times 1 + depth sin(2 pi rate t), the sine faded
    in over int(delay sr) samples when that is shorter than the note; the result in the array's own type."""
    f = np.asarray(f0, dtype=F64)
    n = f.size
    v = np.sin(2 * np.pi * float(vib["rate"]) * (np.arange(n) / float(sr)) + 0)
    k = int(float(vib["delay"]) * sr)
    if k < n:
        v[:k] *= np.linspace(0, 1, k)
    out = f.copy()
    on = f > 0
    out[on] = f[on] * (1 + v[on] * float(vib["depth"]))
    return out if keep64 else out.astype(F32).astype(F64)


def lf_pulse_sub(T, n):
    """(raw fp32 samples, fp32 peak) of gf.lf_model_pulse(T, Ra .02, Rg 1.7, Rk 1, smoothing=False) at n samples: the time grid is
    np.linspace(0, T, n, endpoint=False, dtype=float32), np.pi * t stays fp32, everything behind it is float64 until the store."""
    T = float(T)
    t = (np.arange(n, dtype=F64) * (T / n)).astype(F32)
    Tp = 0.02 * T
    Tc = Tp + 1.0 * (T - Tp)
    p = np.zeros(n, dtype=F32)
    t64 = t.astype(F64)
    rise = t64 < Tp
    p[rise] = (np.sin((F32(np.pi) * t[rise]).astype(F64) / (2 * Tp)) ** 2).astype(F32)
    fall = (~rise) & (t64 < Tc)
    tau = (t64[fall] - Tp) / (Tc - Tp)
    p[fall] = (np.exp(-1.7 * tau) * np.cos(np.pi * tau / 2)).astype(F32)
    return p, F32(np.max(np.abs(p)))


def _round_n(x, rounding):
    return int(round(x)) if rounding == "even" else int(math.floor(x + 0.5))


def _track(inc):
    """The wrapped tracker in sample order: (event samples, phase in front of each sample, phase behind it before the wrap)."""
    ev, ph = [], 0.0
    before, after = np.empty(len(inc)), np.empty(len(inc))
    for i, a in enumerate(inc.tolist()):
        before[i] = ph
        ph += a
        after[i] = ph
        if ph >= 1.0:
            ev.append(i)
            ph -= 1.0
    return np.array(ev, dtype=np.int64), before, after


def _gather_search(ev_i, ev_n, ev_end_max, pulses, n, latest_only):
    """The placement as a search of the event list (k_subharm_place's shape): per sample the last event starting at or before
    it, back while the end_max of the event in front passes the sample.  For the wrong variants; the restatement adds slices."""
    out, cover = np.zeros(n), np.zeros(n, dtype=np.int64)
    if not len(ev_i):
        return out, cover
    last_of = np.searchsorted(ev_i, np.arange(n), side="right") - 1
    for j in range(n):
        last = int(last_of[j])
        if last < 0:
            continue
        first = last
        if not latest_only:
            while first > 0 and ev_end_max[first - 1] > j:
                first -= 1
        for k in range(first, last + 1):
            d = j - int(ev_i[k])
            if d < ev_n[k]:
                out[j] += float(pulses[k][d])
                cover[j] += 1
    return out, cover


def sub_layer(f0, mask, sr, ratios, weight, vib=None, f0_64=None, rounding="even", cache=True, carry=True, covering="all"):
    """The layer of one note.  ``f0``: the fp32 f0 the layer tracks (scaled, jittered); ``f0_64``: the float64 array in its place.
    ``weight``: the fp32 parameter.  Returns a dict:
      fm        the modulated f0 (float64 values; fp32-rounded unless f0_64) — the same array for every ratio
      inc       per ratio, the tracker's increments (0 where mask <= 0, f <= 0 or sub < 1e-2)
      events    per ratio, a dict of arrays over the events in sample order: i, sub (the event's own), sub_used (the lender's),
                T, n, n_own, end_max, and the flags lent (n differs from n_own), clamped (n came from the max(3, .)), tie (sr T is
                exactly x.5), fragile (the phase at the event or in front of it within 1e-9 of 1), key_edge (rint(100 sub) is not the printed key, or 100 sub is
                within 1e-6 of x.5 without being it: printf's exact decimal and a rounded product could part)
      raw       the float64 sum over ratios times the mask, before the division
      max       the note's maximum of |raw|
      layer     raw / max (if max > 1e-6) * weight
      C, A      per sample: covering events, and the sum of their |normalised pulse value| (times the mask)
    """
    sr = float(sr)
    m32 = np.asarray(mask, dtype=F32)
    m = m32.astype(F64)
    f = np.asarray(f0, dtype=F32).astype(F64) if f0_64 is None else np.asarray(f0_64, dtype=F64).copy()
    n_s = f.size
    fm = sub_vibrato(f, sr, vib, f0_64 is not None) if vib else f
    total = np.zeros(n_s)
    C, A = np.zeros(n_s, dtype=np.int64), np.zeros(n_s)
    incs, events = [], []
    shapes = {}
    for ratio in ratios:
        ratio = float(ratio)
        sub = fm * ratio
        inc = np.where((m32 > 0) & (fm > 0) & ~(sub < 1e-2), sub / sr, 0.0)
        incs.append(inc)
        ev_i, before, after = _track(inc)
        ne = len(ev_i)
        e = {k: np.zeros(ne, dtype=t) for k, t in (("sub", F64), ("sub_used", F64), ("T", F64), ("n", np.int64), ("n_own", np.int64),
                                                    ("end_max", np.int64), ("lent", bool), ("clamped", bool), ("tie", bool),
                                                    ("fragile", bool), ("key_edge", bool))}
        e["i"] = ev_i
        lender = {}
        pulses = []
        buf = np.zeros(n_s)
        for k, i in enumerate(ev_i.tolist()):
            own = float(sub[i])
            key = f"{own:.2f}"
            used = lender.setdefault(key, own) if cache else own
            T = 1.0 / used
            n = max(3, _round_n(sr * T, rounding))
            n_own = max(3, _round_n(sr * (1.0 / own), rounding))
            x = sr * T
            h = own * 100.0
            e["sub"][k], e["sub_used"][k], e["T"][k], e["n"][k], e["n_own"][k] = own, used, T, n, n_own
            e["lent"][k] = n != n_own
            e["clamped"][k] = round(x) < 3
            e["tie"][k] = (x - math.floor(x)) == 0.5
            e["fragile"][k] = abs(after[i] - 1.0) < 1e-9 or abs(before[i] - 1.0) < 1e-9
            frac = h - math.floor(h)
            e["key_edge"][k] = int(key.replace(".", "")) != int(np.rint(h)) or (abs(frac - 0.5) < 1e-6 and frac != 0.5)
            if (n, T) not in shapes:
                raw, pk = lf_pulse_sub(T, n)
                shapes[(n, T)] = (raw / pk) if pk > 0 else raw                  # fp32 / fp32: the reference's `pulse /= max`
            p = shapes[(n, T)]
            pulses.append(p)
        ends = ev_i + e["n"]
        if carry:
            e["end_max"] = np.maximum.accumulate(ends) if ne else ends
        else:                                                                   # WRONG: every strip of 64 events starts afresh
            e["end_max"] = np.concatenate([np.maximum.accumulate(ends[a:a + 64]) for a in range(0, ne, 64)]) if ne else ends
        if carry and covering == "all":
            for k, i in enumerate(ev_i.tolist()):
                p = pulses[k]
                end = min(n_s, i + p.size)
                buf[i:end] += p[:end - i].astype(F64)                           # ascending events: the order of the reference
                C[i:end] += 1
                A[i:end] += np.abs(p[:end - i].astype(F64))
        else:
            buf, cov = _gather_search(ev_i, e["n"], e["end_max"], pulses, n_s, covering == "latest")
            C += cov
            A += np.abs(buf)
        total = buf + total
        events.append(e)
    raw = total * m
    A = A * np.abs(m)
    mx = float(np.max(np.abs(raw))) if n_s else 0.0
    w = float(F32(weight))
    layer = (raw / mx if mx > 1e-6 else raw) * w
    return {"fm": fm, "inc": incs, "events": events, "raw": raw, "max": mx, "layer": layer, "C": C, "A": A, "weight": w}


def layer_bound(truth, sub, c=C_PULSE):
    """The GPU test's bound on |pulse - truth| per sample: the fp32 store, and c fp32 roundings on the layer's terms."""
    scale = (sub["weight"] / sub["max"]) if sub["max"] > 1e-6 else sub["weight"]
    return 2.0 ** -24 * np.abs(truth) + c * 2.0 ** -23 * scale * sub["A"] + 2.0 ** -149


def ulp32(x):
    """The spacing of fp32 at |x| (of the smallest subnormal at 0)."""
    x = np.abs(np.asarray(x, dtype=F32))
    return (np.nextafter(x, F32(np.inf)) - x).astype(F64)


# ---------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------
SH = dict(strength=0.5, speed=100.0)                          # f0 jitter: sigma = sr / 600 = 73.5, radius 294
SR_NOISE = dict(speed=150.0, harm=0.8, breath=1.6)            # volume jitter, noise form: sigma 49, radius 196
SR_VIB = dict(speed=40.0, harm=1.6, breath=0.7)               # vibrato form: 1.6 reaches both clip limits
HARM_ONLY = (8, 9)                                            # the notes whose vol_jitter_breath is 0
SG_WEIGHT = 0.5
SG_CASES = {                                                  # name: (subharm dict, subharm_f0_jitter, with f0_64)
    "one": (dict(semitones=-12), 0.0, False),
    "three": (dict(semitones=[-12, -7, 12]), 0.0, False),
    "vibrato": (dict(semitones=-12, vibrato=True, rate=6.0, depth=0.1, delay=0.05), 0.0, False),
    "jitter": (dict(semitones=-12), 0.3, False),
    "f0_64": (dict(semitones=[-12, 12], vibrato=True, rate=5.0, depth=0.05, delay=0.01), 0.0, True),
}


def ratios_of(subharm):
    return [float(2.0 ** (v / 12.0)) for v in np.atleast_1d(np.asarray(subharm["semitones"], dtype=F64))]


def flagged(k, parity=0):
    return k % 2 == parity


def _masks(rng):
    m = [np.ones(n, dtype=F32) for n in LENGTHS]
    m[0][3000:3300] = 0
    m[0][5200:5300] = 0
    m[2] = rng.uniform(0.1, 1.0, LENGTHS[2]).astype(F32)                        # fractional, a few exact zeros
    m[2][[7, 8, 60]] = 0
    m[3][:] = 0                                                                 # all unvoiced (flagged at parity 1)
    m[5][:40] = 0
    m[5][200:] = 0
    m[6][:] = 0                                                                 # all unvoiced (flagged at parity 0)
    m[7] = rng.uniform(0.0, 1.0, LENGTHS[7]).astype(F32)
    m[7][100:120] = 0
    m[8][300:340] = 0
    m[9][:130] = 0
    m[9][700:900] = 0
    return m


@functools.lru_cache(maxsize=None)
def cases(sr=GEO[0]):
    """The ragged batch, built once: ten notes (LENGTHS), every third with a pitch shift, env / phi for the synthesis behind the
    stages, the masks, one f0 set for the jitter groups and a designed one for the sub-harmonic group, the injected draws."""
    assert sr == GEO[0]
    n_fft, hop = GEO[1], GEO[2]
    nb = n_fft // 2 + 1
    rng = np.random.default_rng(20240611)
    masks = _masks(rng)
    ps = [F32(1.0) if k % 3 != 1 else F32((1.1225, 0.8909, 1.05)[k // 3]) for k in range(len(LENGTHS))]
    notes = []
    for k, n in enumerate(LENGTHS):
        T = 1 + n // hop
        i = np.arange(n)
        f0 = (150.0 + 90.0 * rng.random() + 40.0 * np.sin(i / 300.0 + k) + 3.0 * rng.random(n)).astype(F32)
        if k in (0, 5, 9):
            f0 = f0 * masks[k]                                                  # unvoiced f0 is zero in these, kept in the others
        notes.append({"name": "n%d_%d" % (k, n), "n": n, "T": T, "ps": ps[k], "mask": masks[k], "f0": f0,
                      "env": (1.0 + rng.random((T, nb))).astype(F32),
                      "phi": rng.uniform(-np.pi, np.pi, (T, nb)).astype(F32)})
    # the sub-harmonic group's f0 (notes 0, 2, 4, 6, 8 carry the layer; their pitch_shift is 1 except note 4's)
    sg = [c["f0"].copy() for c in notes]
    a = np.empty(6000, dtype=F32)
    a[:400] = 431.3
    a[400:700] = 16.0                                                           # -12 semitones: sub 8 Hz, sr T = 5512.5
    a[700:1300] = 201.7
    a[1300:] = (1830.0 + 20.0 * rng.random(4700)).astype(F32)
    a[3100:3200] = 0.0                                                          # (inside the unvoiced block 3000 .. 3300)
    a[3300:3310] = 0.015                                                        # voiced, 0 < sub < 1e-2
    a[3310:3330] = 0.0                                                          # voiced by the mask, no f0
    sg[0] = a
    sg[2] = np.full(100, 9001.0, dtype=F32)                                     # +12 semitones: sub 18 kHz, n clamped to 3
    sg[4] = np.full(1, 300.0, dtype=F32)
    sg[6] = np.full(1023, 220.0, dtype=F32)                                     # (all unvoiced)
    b = np.empty(2048, dtype=F32)
    b[:1000] = 100.052                                                          # sub 50.026 -> key 50.03, n 882
    b[1000:] = 100.066                                                          # sub 50.033 -> key 50.03, own n 881: lent 882
    sg[8] = b
    N = sum(LENGTHS)
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    noise = {name: rng.standard_normal(N) for name in ("f0", "vol_h", "vol_b", "sub")}
    f0_64 = {}
    for group, f0s in (("plain", [c["f0"] for c in notes]), ("sg", sg)):
        scaled = np.concatenate([f * c["ps"] for f, c in zip(f0s, notes)]).astype(F32)
        # a float64 f0 that is no fp32 number and whose cast is the scaled fp32 f0 (under a quarter of an ulp away)
        f0_64[group] = scaled.astype(F64) * (1.0 + 2.0 ** -26 * rng.uniform(-1, 1, N))
        assert np.array_equal(f0_64[group].astype(F32), scaled)
    return {"notes": notes, "sg_f0": sg, "off": off, "N": N, "noise": noise, "f0_64": f0_64}


def scaled_f0(c, f0=None):
    return (np.asarray(c["f0"] if f0 is None else f0, dtype=F32) * c["ps"]).astype(F32)


def nan_outside(x, off, parity):
    """The injected draws with the slices of the notes WITHOUT the flag filled with NaN."""
    x = x.copy()
    for k in range(len(off) - 1):
        if not flagged(k, parity):
            x[off[k]:off[k + 1]] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def sg_truth(case, variant=()):
    """sub_layer of every flagged note of the sub-harmonic group under SG_CASES[case] (the jitter case: from the restatement's own
    jittered f0), cached.  ``variant``: sorted (keyword, value) pairs of a wrong variant."""
    return {k: sg_note(case, k, **dict(variant)) for k in range(len(LENGTHS)) if flagged(k)}


def sg_jittered_f0(case, k):
    """The fp32 f0 the layer of note k tracks: scaled, and under subharm_f0_jitter jittered a second time."""
    d = cases()
    c = d["notes"][k]
    a, b = int(d["off"][k]), int(d["off"][k + 1])
    f0s = scaled_f0(c, d["sg_f0"][k])
    sjit = SG_CASES[case][1]
    return f0_after_jitter(f0s, c["mask"], d["noise"]["sub"][a:b], sjit, GEO[0] / (SH["speed"] * 6))[1] if sjit > 0 else f0s


def sg_note(case, k, f0s=None, **variant):
    """sub_layer of note k under SG_CASES[case]; ``f0s``: the fp32 f0 to track in place of the restatement's own."""
    d = cases()
    subharm, _, with64 = SG_CASES[case]
    a, b = int(d["off"][k]), int(d["off"][k + 1])
    return sub_layer(sg_jittered_f0(case, k) if f0s is None else f0s, d["notes"][k]["mask"], GEO[0], ratios_of(subharm), SG_WEIGHT,
                     vib=subharm if subharm.get("vibrato") else None, f0_64=d["f0_64"]["sg"][a:b] if with64 else None, **variant)
