"""Ground-truth signals for the tracker tests: harmonic sources of a known f0 contour shaped by five resonators.

Each harmonic h of the source carries the magnitude response of the five resonators' cascade at h * f0(t), so the
spectrum is exactly that of a band-limited pulse train through the filters, sample by sample along the contour.  The
harmonics stop below 5.4 kHz, inside the formant analysis' band.  Segments: a 100 -> 300 Hz glide, silence, 220 Hz with
5.5 Hz +-50 cent vibrato, white noise at -40 dB, and 140 Hz steady.
"""
import numpy as np

FORMANTS = (700.0, 1220.0, 2600.0, 3500.0, 4500.0)
BANDWIDTHS = (80.0, 90.0, 120.0, 150.0, 200.0)
TOP_HZ = 5400.0

# (kind, seconds)
SEGMENTS = (("glide", 0.6), ("silence", 0.2), ("vibrato", 0.5), ("noise", 0.2), ("steady", 0.3))


def resonance_gain(f, sr):
    """|H(f)| of the cascade of the five two-pole resonators, 1 at DC."""
    g = np.ones_like(f)
    z1 = np.exp(-2j * np.pi * f / sr)
    for F, B in zip(FORMANTS, BANDWIDTHS):
        r = np.exp(-np.pi * B / sr)
        a1, a2 = -2.0 * r * np.cos(2.0 * np.pi * F / sr), r * r
        g *= np.abs(1.0 + a1 + a2) / np.abs(1.0 + a1 * z1 + a2 * z1 * z1)
    return g


def contour(sr, segments=SEGMENTS):
    """(f0 per sample, 0 where unvoiced; kind label per sample)."""
    f0, kind = [], []
    for k, dur in segments:
        n = int(round(dur * sr))
        t = np.arange(n) / sr
        if k == "glide":
            f = 100.0 * 3.0 ** (t / dur)
        elif k == "vibrato":
            f = 220.0 * 2.0 ** (50.0 / 1200.0 * np.sin(2.0 * np.pi * 5.5 * t))
        elif k == "steady":
            f = np.full(n, 140.0)
        else:
            f = np.zeros(n)
        f0.append(f)
        kind += [k] * n
    return np.concatenate(f0), np.array(kind)


def synth(sr, segments=SEGMENTS, seed=0):
    """(signal, f0 per sample, kind per sample)."""
    f0, kind = contour(sr, segments)
    phase = 2.0 * np.pi * np.cumsum(f0) / sr
    y = np.zeros(len(f0))
    voiced = f0 > 0
    for h in range(1, int(TOP_HZ // 100.0) + 1):
        fh = h * f0
        on = voiced & (fh < TOP_HZ)
        if not on.any():
            break
        y[on] += resonance_gain(fh[on], sr) * np.cos(h * phase[on])
    y *= 0.5 / np.abs(y).max()
    rng = np.random.default_rng(seed)
    noise = kind == "noise"
    y[noise] = 0.01 * rng.standard_normal(noise.sum())
    return y, f0, kind


def frame_truth(f0, kind, centres, half, sr):
    """Truth at frame centres (sample indices): f0 (0 unvoiced), kind, and whether the frame is clear of every segment edge:
    its window (centre +- half) and two frames' spacing on either side lie inside one segment."""
    c = np.clip(np.round(centres).astype(np.int64), 0, len(f0) - 1)
    edges = np.flatnonzero(kind[1:] != kind[:-1]) + 1
    spacing = np.diff(centres).mean() if len(centres) > 1 else 0.0
    reach = half + 2.0 * spacing
    clear = np.ones(len(c), bool)
    for e in edges:
        clear &= np.abs(centres - e) > reach
    clear &= (centres - reach >= 0) & (centres + reach < len(f0))
    return f0[c], kind[c], clear


def score(y_f0, y_forms, f0, kind, sr, hop):
    """The ground-truth figures of one tracked signal (f0 track and [frames, 5] formants in the restatement's layouts)."""
    import tracker_ref as R
    n = len(f0)
    W = R.pitch_window(sr)
    centres = R.pitch_starts(n, sr, hop) + 0.5 * W
    tf0, tk, clear = frame_truth(f0, kind, centres, 0.5 * W, sr)
    tv, ev = tf0 > 0, np.asarray(y_f0) > 0
    both = clear & tv & ev
    ratio = np.asarray(y_f0)[both] / tf0[both]
    quiet = clear & ((tk == "silence") | (tk == "noise"))
    fc = (R.formant_starts(n, sr, hop) + 0.5 * R.FORMANT_WIN) * sr / R.FORMANT_SR
    ff0, _, fclear = frame_truth(f0, kind, fc, 0.5 * R.FORMANT_WIN * sr / R.FORMANT_SR, sr)
    sel = fclear & (ff0 > 0) & (ff0 <= 250.0)
    ferr = [np.abs(np.asarray(y_forms)[sel, k] / FORMANTS[k] - 1.0) for k in range(3)]
    return {
        "f0_within_1pct": float(np.mean(np.abs(ratio - 1.0) <= 0.01)) if both.any() else 0.0,
        "octave_errors": int(np.sum(np.abs(np.log2(ratio)) > 0.5)),
        "voicing_agree": float(np.mean((tv == ev)[clear])),
        "quiet_unvoiced": float(np.mean(~ev[quiet])),
        "formant_median": [float(np.median(e)) for e in ferr],
        "formant_p90": [float(np.percentile(e, 90)) for e in ferr],
        "n_voiced": int(both.sum()), "n_quiet": int(quiet.sum()), "n_formant": int(sel.sum()),
    }


def assert_meets_bars(s):
    """The accuracy bars of the tracker (set on the CPU restatement)."""
    assert s["n_voiced"] > 50 and s["n_quiet"] >= 10 and s["n_formant"] > 30, s
    assert s["f0_within_1pct"] >= 0.98, s
    assert s["octave_errors"] == 0, s
    assert s["voicing_agree"] >= 0.97, s
    assert s["quiet_unvoiced"] >= 0.99, s
    assert max(s["formant_median"]) <= 0.05, s
    assert max(s["formant_p90"]) <= 0.10, s
