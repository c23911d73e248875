"""CPU restatement of the native f0 / formant tracker (goofer_amd/csrc/tracker.hip), numpy in fp64, written plainly.

Only the tests import this.  It states the algorithm the kernels implement, so that the GPU can be checked frame by frame
and the algorithm itself against ground truth without a device.

Pitch: Boersma (1993) autocorrelation method — Hann window of three periods of the floor, autocorrelation divided by the
window's own, parabolic peak refinement, octave cost, an unvoiced candidate from the frame's peak against the signal's,
and a Viterbi path with octave-jump and voiced/unvoiced costs.
Formants: windowed-sinc resampling to 2 x 5500 Hz, pre-emphasis from 50 Hz, a 50 ms Gaussian window, Burg LPC of order 10,
the roots of the predictor polynomial by Aberth's method with Newton polishing, roots with 50 < f < 5450 Hz sorted.
"""
import numpy as np

FLOOR, CEILING = 75, 950.0
PERIODS = 3
MAX_CAND = 15
SILENCE, VOICING = 0.03, 0.45
OCTAVE_COST, OCTAVE_JUMP, VUV_COST = 0.01, 0.35, 0.14
SILENT_PEAK = 1e-10                   # a signal whose peak deviation from its mean is below this (-200 dB) is silence

FORMANT_SR = 11000
N_FORMANTS, ORDER = 5, 10
FORMANT_WIN = 550                     # 50 ms at 11 kHz
PRE_EMPH_HZ = 50.0
SINC_ZEROS = 20                       # half-width of the resampling kernel in output-rate zero crossings


# -- geometry ------------------------------------------------------------------------------------------------------
def min_length(sr):
    """Samples in one pitch window (3 / 75 Hz = 40 ms)."""
    return -(-PERIODS * sr // FLOOR)


def pitch_frames(n, sr, hop):
    """floor((dur - win) / dt) + 1 in integers; 0 when the signal is shorter than a window."""
    d = FLOOR * n - PERIODS * sr
    return 0 if d < 0 else d // (FLOOR * hop) + 1


def pitch_window(sr):
    return PERIODS * sr // FLOOR


def pitch_starts(n, sr, hop):
    nf, W = pitch_frames(n, sr, hop), pitch_window(sr)
    first = (n - (nf - 1) * hop - W) // 2
    return first + hop * np.arange(nf, dtype=np.int64)


def resampled_length(n, sr):
    return n * FORMANT_SR // sr


def formant_frames(n, sr, hop):
    m = resampled_length(n, sr)
    return 0 if m < FORMANT_WIN else (m - FORMANT_WIN) * sr // (FORMANT_SR * hop) + 1


def formant_starts(n, sr, hop):
    """Frame starts at 11 kHz: centres m/2 + (i - (nf-1)/2) * dt, rounded exactly in integers, clamped into the signal."""
    m, nf = resampled_length(n, sr), formant_frames(n, sr, hop)
    i = np.arange(nf, dtype=np.int64)
    num = (m - FORMANT_WIN) * sr + (2 * i - nf + 1) * hop * FORMANT_SR
    return np.clip((num + sr) // (2 * sr), 0, m - FORMANT_WIN)


# -- pitch ---------------------------------------------------------------------------------------------------------
def hann(W):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 1.0) / (W + 1.0))


def lag_range(sr):
    ceiling = min(CEILING, 0.5 * sr)
    return int(np.floor(sr / ceiling)), -(-sr // FLOOR)


def frame_candidates(x, w, rw, sr, global_peak):
    """(freqs, strengths) of one frame; slot 0 is the unvoiced candidate, the voiced ones follow in lag order."""
    W = len(x)
    min_lag, max_lag = lag_range(sr)
    ceiling = min(CEILING, 0.5 * sr)
    xc = x - x.mean()
    local_peak = np.abs(xc).max()
    ratio = 0.0 if global_peak <= SILENT_PEAK else local_peak / global_peak
    uv = VOICING + max(0.0, 2.0 - ratio / (SILENCE / (1.0 + VOICING)))
    xw = xc * w
    r0 = float(np.dot(xw, xw))
    freqs, strengths = [0.0], [uv]
    if r0 <= 0.0:
        return np.array(freqs), np.array(strengths)
    lo, hi = max(1, min_lag - 1), min(max_lag + 1, W - 1)
    r = np.correlate(xw, xw, mode="full")[W - 1:W + hi] / (r0 * rw[:hi + 1])
    peaks = []
    for t in range(max(lo + 1, min_lag), min(max_lag, hi - 1) + 1):
        if r[t] > 0.5 * VOICING and r[t] > r[t - 1] and r[t] >= r[t + 1]:
            dr = 0.5 * (r[t + 1] - r[t - 1])
            d2r = 2.0 * r[t] - r[t - 1] - r[t + 1]
            delta = dr / d2r if d2r > 0.0 else 0.0
            rm = r[t] + 0.5 * dr * delta
            if rm > 1.0:
                rm = 1.0 / rm
            f = sr / (t + delta)
            if f < FLOOR or f > ceiling:
                continue
            peaks.append((f, rm - OCTAVE_COST * np.log2(FLOOR / f)))
    if len(peaks) > MAX_CAND - 1:                        # the strongest, earlier lag first among equals, kept in lag order
        keep = np.sort(np.argsort([-s for _, s in peaks], kind="stable")[:MAX_CAND - 1])
        peaks = [peaks[k] for k in keep]
    for f, s in peaks:
        freqs.append(f)
        strengths.append(s)
    return np.array(freqs), np.array(strengths)


def transition(fp, fc, tsc):
    if fp == 0.0 and fc == 0.0:
        return 0.0
    if fp == 0.0 or fc == 0.0:
        return VUV_COST * tsc
    return OCTAVE_JUMP * tsc * abs(np.log2(fp / fc))


def viterbi(cands, tsc):
    """Maximum total strength minus transition costs; the first best on ties; unvoiced frames report 0."""
    nf = len(cands)
    if nf == 0:
        return np.zeros(0)
    delta = cands[0][1].copy()
    back = []
    for i in range(1, nf):
        fp, fc = cands[i - 1][0], cands[i][0]
        nd = np.empty(len(fc))
        bp = np.empty(len(fc), dtype=np.int64)
        for c in range(len(fc)):
            best, arg = -np.inf, 0
            for p in range(len(fp)):
                v = delta[p] - transition(fp[p], fc[c], tsc)
                if v > best:
                    best, arg = v, p
            nd[c] = best + cands[i][1][c]
            bp[c] = arg
        delta = nd
        back.append(bp)
    c = int(np.argmax(delta))
    f0 = np.zeros(nf)
    for i in range(nf - 1, -1, -1):
        f0[i] = cands[i][0][c]
        if i > 0:
            c = int(back[i - 1][c])
    return f0


def track_pitch(y, sr, hop):
    y = np.asarray(y, dtype=np.float64)
    if len(y) < min_length(sr):
        raise ValueError(f"signal of {len(y)} samples is shorter than one pitch window ({min_length(sr)} samples)")
    W = pitch_window(sr)
    w = hann(W)
    rw = np.correlate(w, w, mode="full")[W - 1:] / np.dot(w, w)
    gp = np.abs(y - y.mean()).max()
    cands = [frame_candidates(y[s:s + W], w, rw, sr, gp) for s in pitch_starts(len(y), sr, hop)]
    return viterbi(cands, 0.01 * sr / hop)


# -- formants ------------------------------------------------------------------------------------------------------
def resample(y, sr):
    """Windowed-sinc low-pass interpolation to 11 kHz: output m at input position m * sr / 11000, cut-off at the lower
    Nyquist, Hann-windowed over +-SINC_ZEROS zero crossings of the output rate."""
    n = len(y)
    m = resampled_length(n, sr)
    fc = 0.5 * min(sr, FORMANT_SR) / sr                   # cycles per input sample
    half = SINC_ZEROS * max(1.0, sr / FORMANT_SR)
    out = np.zeros(m)
    for j in range(m):
        p = j * float(sr) / FORMANT_SR
        k = np.arange(max(0, int(np.ceil(p - half))), min(n - 1, int(np.floor(p + half))) + 1)
        d = k - p
        h = 2.0 * fc * np.sinc(2.0 * fc * d) * (0.5 + 0.5 * np.cos(np.pi * d / half))
        out[j] = np.dot(h, y[k])
    return out


def gauss_window(W):
    """Praat's Gaussian-like window for Burg analysis: exp(-48 (i - mid)^2 / (W + 1)^2), lifted to zero at the ends."""
    i = np.arange(1, W + 1, dtype=np.float64)
    e12 = np.exp(-12.0)
    return (np.exp(-48.0 * (i - 0.5 * (W + 1)) ** 2 / (W + 1.0) ** 2) - e12) / (1.0 - e12)


def burg(x, order):
    """Burg's method: predictor a[0..m] (a[0] = 1) of the order reached (lower when the residual vanishes)."""
    f = x.astype(np.float64).copy()
    b = f.copy()
    a = np.array([1.0])
    for m in range(1, order + 1):
        ff, bb = f[m:], b[m - 1:-1]
        den = np.dot(ff, ff) + np.dot(bb, bb)
        if den <= 0.0:
            break
        k = -2.0 * np.dot(ff, bb) / den
        a = np.concatenate([a, [0.0]])
        a = a + k * a[::-1]
        f[m:], b[m:] = ff + k * bb, bb + k * ff
    return a


def poly_roots(a, iters=100):
    """Roots of z^m + a1 z^(m-1) + ... + am by Aberth-Ehrlich iteration (all roots updated together), then two Newton steps."""
    m = len(a) - 1
    if m == 0:
        return np.zeros(0, complex)
    z = 0.9 * np.exp(1j * (2.0 * np.pi * np.arange(m) / m + 0.25))

    def pd(zz):
        p = np.ones_like(zz)
        d = np.zeros_like(zz)
        for c in a[1:]:
            d = d * zz + p
            p = p * zz + c
        return p, d

    for _ in range(iters):
        p, d = pd(z)
        ratio = np.where(d != 0, p / np.where(d != 0, d, 1), 0)
        diff = z[:, None] - z[None, :]
        np.fill_diagonal(diff, 1.0)
        s = (1.0 / diff).sum(axis=1) - 1.0
        w = ratio / (1.0 - ratio * s)
        z = z - w
        if np.all(np.abs(w) <= 1e-14 * np.maximum(np.abs(z), 1e-300)):
            break
    for _ in range(2):
        p, d = pd(z)
        z = z - np.where(d != 0, p / np.where(d != 0, d, 1), 0)
    return z


def frame_formants(x):
    if not np.any(x):
        return np.zeros(N_FORMANTS)
    a = burg(x, ORDER)
    z = poly_roots(a)
    f = np.arctan2(z.imag, z.real) * FORMANT_SR / (2.0 * np.pi)
    f = np.sort(f[(z.imag > 0) & (f > 50.0) & (f < 0.5 * FORMANT_SR - 50.0)])[:N_FORMANTS]
    return np.concatenate([f, np.zeros(N_FORMANTS - len(f))])


def track_formants(y, sr, hop):
    """[frames, 5] formant frequencies in Hz (0: not found)."""
    x = resample(np.asarray(y, dtype=np.float64), sr)
    alpha = np.exp(-2.0 * np.pi * PRE_EMPH_HZ / FORMANT_SR)
    xe = x.copy()
    xe[1:] = x[1:] - alpha * x[:-1]
    w = gauss_window(FORMANT_WIN)
    starts = formant_starts(len(y), sr, hop)
    return np.array([frame_formants(xe[s:s + FORMANT_WIN] * w) for s in starts]).reshape(len(starts), N_FORMANTS)


def track(y, sr, hop):
    return track_pitch(y, sr, hop), track_formants(y, sr, hop)
