"""The signal matrix of the tracker's oracle tests (tests/test_gpu_tracker_oracle.py): rates, hops and signals from fixed
seeds, and the restatement's answers for each, stage by stage, with its fragility flags.  Numpy only, so the restatement can
run in worker processes."""
import numpy as np

import tracker_ref as R
import tracker_truth as T

RATES = (8000, 11000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000)
# every hop at two rates or more, 8000 and 96000 among them; 2048 is longer than the 22.05 kHz pitch window (882)
HOPS = {8000: (64, 100, 441), 11000: (96, 512), 11025: (256, 1024), 16000: (64, 441), 22050: (100, 256, 2048),
        32000: (96, 1024), 44100: (441, 512), 48000: (64, 256), 88200: (100, 1024), 96000: (96, 512, 256)}
LONG = (22050, 64, 20.0)          # one long signal through the single-wave Viterbi (pitch stages only)
# and hop 1 on one short signal at 8 kHz


def harmonic(sr, f0, seed, n_harm=12):
    """A harmonic source along the f0 contour (per sample), harmonics below 0.45 sr, random phases from seed."""
    rng = np.random.default_rng(seed)
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    y = np.zeros(len(f0))
    for h in range(1, n_harm + 1):
        on = h * f0 < 0.45 * sr
        y[on] += np.cos(h * ph[on] + rng.uniform(0, 2 * np.pi)) / h
    return 0.5 * y / np.abs(y).max()


def voice(sr, dur=0.5, seed=0):
    """The ground-truth synth's vibrato and steady segments, dur seconds."""
    y, _, _ = T.synth(sr, segments=(("vibrato", dur / 2), ("steady", dur - dur / 2)), seed=seed)
    return y


def signals(sr, hop, full):
    """{name: signal} at (sr, hop); full: every kind, else the core set."""
    rng = np.random.default_rng(sr + 7 * hop)
    t = lambda d: np.arange(int(d * sr)) / sr                                  # noqa: E731
    out = {"synth": T.synth(sr)[0][int(0.2 * sr):int(1.1 * sr)],
           "glide": harmonic(sr, 76.0 * (940.0 / 76.0) ** (t(0.6) / 0.6), 1),
           "segments": np.concatenate([voice(sr, 0.2, 1), np.zeros(int(0.1 * sr)), 0.05 * rng.standard_normal(int(0.1 * sr)),
                                       voice(sr, 0.2, 2)])}
    if not full:
        return out
    v = voice(sr, 0.4, 3)
    n = R.min_length(sr)
    n550 = -(-R.FORMANT_WIN * sr // R.FORMANT_SR)                           # the fewest samples with 550 at 11 kHz
    click = np.zeros(int(0.3 * sr))
    click[len(click) // 2] = 0.8
    f = np.concatenate([np.full(int(0.2 * sr), 200.0), np.full(int(0.2 * sr), 400.0), np.full(int(0.2 * sr), 200.0)])
    out.update({
        "octave": harmonic(sr, f, 2),
        "sine2k": 0.5 * np.sin(2 * np.pi * 2000.0 * t(0.3)),
        "pair": 0.3 * np.sin(2 * np.pi * 1800.0 * t(0.3)) + 0.3 * np.sin(2 * np.pi * 2300.0 * t(0.3) + 1.0),
        "noise": 0.3 * rng.standard_normal(int(0.3 * sr)),
        "square": np.clip(4.0 * np.sign(np.sin(2 * np.pi * 150 * t(0.3))), -1, 1),
        "dc_voice": 0.5 + 0.3 * v,
        "click": click,
        "peak1e-9": v * (1e-9 / np.abs(v).max()),
        "peak1e-11": v * (1e-11 / np.abs(v).max()),
        "peak1e4": v * (1e4 / np.abs(v).max()),
        "len_min": v[:n],
        "len_min_hop-1": v[:n + hop - 1],
        "len_min_hop": v[:n + hop],
        "len_550": v[:n550],
        "len_550-1": v[:n550 - 1],
    })
    return out


def matrix():
    """[(sr, hop, name, signal)]: every kind at each rate's first hop, the core set at its others, and the long signal."""
    cases = []
    for sr in RATES:
        for k, hop in enumerate(HOPS[sr]):
            cases += [(sr, hop, name, y) for name, y in signals(sr, hop, k == 0).items()]
    cases.append((8000, 1, "hop1", voice(8000, 0.12, 9)))
    sr, hop, dur = LONG
    cases.append((sr, hop, "long", np.tile(voice(sr, 1.0, 4), int(dur))))
    return cases


def restate(case):
    """The restatement's answers for one case (see the oracle tests)."""
    sr, hop, name, y = case
    cands, frag, peaks = R.pitch_candidates(y, sr, hop)
    f0, _, vfrag = R.viterbi_diag(cands, 0.01 * sr / hop)
    out = {"cands": cands, "cand_fragile": frag, "peaks": peaks, "f0": f0, "path_fragile": vfrag}
    if name != "long":
        x11 = R.resample(y, sr)
        forms, ffrag = R.formants_of_11k(x11, sr, hop)
        out.update(x11=x11, formants=forms, formant_fragile=ffrag)
    return out
