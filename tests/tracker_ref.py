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
EPS = 1e-9                            # a decision this close to flipping marks its frame fragile (the *_diag helpers)
ROOT_EPS = 1e-6                       # the same for a root against a formant cut-off (relative): the formant bound
ABERTH_ITERS = 100
CLOSE_ROOTS = 1e-3                    # roots closer than this in the z plane are ill-conditioned

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
    freqs, strengths, _, _ = frame_candidates_diag(x, w, rw, sr, global_peak)
    return freqs, strengths


def frame_candidates_diag(x, w, rw, sr, global_peak, eps=EPS):
    """frame_candidates plus (fragile, peaks): fragile when a decision is within ``eps`` of flipping — a peak test
    (r > 0.5 voicing, r > r[t-1], r >= r[t+1]) at any lag of the scan, a frequency against the floor or the ceiling
    (relative), the 14th against the 15th strength when more than 14 peaks are pruned, the signal's peak against the
    silence level (relative) — or when the frame's mean-removed peak is rounding residue (<= 1e-12 |mean|).  peaks: the
    voiced peaks found before pruning."""
    W = len(x)
    min_lag, max_lag = lag_range(sr)
    ceiling = min(CEILING, 0.5 * sr)
    mean = x.mean()
    xc = x - mean
    local_peak = np.abs(xc).max()
    fragile = bool(abs(mean) > 0.0 and local_peak <= 1e-12 * abs(mean))
    fragile |= bool(abs(global_peak - SILENT_PEAK) <= eps * SILENT_PEAK)
    ratio = 0.0 if global_peak <= SILENT_PEAK else local_peak / global_peak
    uv = VOICING + max(0.0, 2.0 - ratio / (SILENCE / (1.0 + VOICING)))
    xw = xc * w
    r0 = float(np.dot(xw, xw))
    freqs, strengths = [0.0], [uv]
    if r0 <= 0.0:
        return np.array(freqs), np.array(strengths), fragile, 0
    lo, hi = max(1, min_lag - 1), min(max_lag + 1, W - 1)
    r = np.correlate(xw, xw, mode="full")[W - 1:W + hi] / (r0 * rw[:hi + 1])
    peaks = []
    for t in range(max(lo + 1, min_lag), min(max_lag, hi - 1) + 1):
        m = (r[t] - 0.5 * VOICING, r[t] - r[t - 1], r[t] - r[t + 1])
        if min(m) > -eps and min(abs(v) for v in m) <= eps:
            fragile = True
        if r[t] > 0.5 * VOICING and r[t] > r[t - 1] and r[t] >= r[t + 1]:
            dr = 0.5 * (r[t + 1] - r[t - 1])
            d2r = 2.0 * r[t] - r[t - 1] - r[t + 1]
            delta = dr / d2r if d2r > 0.0 else 0.0
            rm = r[t] + 0.5 * dr * delta
            if rm > 1.0:
                rm = 1.0 / rm
            f = sr / (t + delta)
            if abs(f - FLOOR) <= eps * FLOOR or abs(f - ceiling) <= eps * ceiling:
                fragile = True
            if f < FLOOR or f > ceiling:
                continue
            peaks.append((f, rm - OCTAVE_COST * np.log2(FLOOR / f)))
    n_peaks = len(peaks)
    if len(peaks) > MAX_CAND - 1:                        # the strongest, earlier lag first among equals, kept in lag order
        order = np.argsort([-s for _, s in peaks], kind="stable")
        fragile |= bool(peaks[order[MAX_CAND - 2]][1] - peaks[order[MAX_CAND - 1]][1] <= eps)
        keep = np.sort(order[:MAX_CAND - 1])
        peaks = [peaks[k] for k in keep]
    for f, s in peaks:
        freqs.append(f)
        strengths.append(s)
    return np.array(freqs), np.array(strengths), fragile, n_peaks


def transition(fp, fc, tsc):
    if fp == 0.0 and fc == 0.0:
        return 0.0
    if fp == 0.0 or fc == 0.0:
        return VUV_COST * tsc
    return OCTAVE_JUMP * tsc * abs(np.log2(fp / fc))


def viterbi(cands, tsc):
    """Maximum total strength minus transition costs; the first best on ties; unvoiced frames report 0."""
    return viterbi_diag(cands, tsc)[0]


def viterbi_diag(cands, tsc, eps=EPS):
    """viterbi plus, per frame, how close the path came to another: gap[i] for i >= 1 is the best minus the second-best
    predecessor score of the candidate chosen at frame i (inf with one predecessor), gap[0] the best minus the second-best
    final score, and fragile[i] when a gap at frame i or at any later frame (or the final gap) is within eps of a tie,
    relative to the size of the scores (a flip there changes frame i's choice)."""
    nf = len(cands)
    if nf == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, bool)
    delta = np.asarray(cands[0][1], dtype=np.float64).copy()
    back, gaps, tols = [], [], []
    for i in range(1, nf):
        fp, fc = np.asarray(cands[i - 1][0], np.float64)[:, None], np.asarray(cands[i][0], np.float64)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            oct_ = OCTAVE_JUMP * tsc * np.abs(np.log2(fp / fc))     # transition(), one predecessor per row
        tr = np.where((fp == 0.0) & (fc == 0.0), 0.0, np.where((fp == 0.0) | (fc == 0.0), VUV_COST * tsc, oct_))
        v = delta[:, None] - tr
        bp = np.argmax(v, axis=0)                                   # the first best predecessor
        cols = np.arange(v.shape[1])
        best = v[bp, cols]
        v[bp, cols] = -np.inf
        second = v.max(axis=0)
        delta = best + np.asarray(cands[i][1], np.float64)
        back.append(bp)
        gaps.append(best - second)
        tols.append(eps * np.maximum(1.0, np.abs(best)))
    c = int(np.argmax(delta))
    srt = np.sort(delta)[::-1]
    gap = np.full(nf, np.inf)
    near = np.zeros(nf, bool)
    gap[0] = srt[0] - srt[1] if len(srt) > 1 else np.inf
    final_near = gap[0] <= eps * max(1.0, abs(srt[0]))
    f0 = np.zeros(nf)
    for i in range(nf - 1, -1, -1):
        f0[i] = cands[i][0][c]
        if i > 0:
            gap[i] = gaps[i - 1][c]
            near[i] = gap[i] <= tols[i - 1][c]
            c = int(back[i - 1][c])
    # a near-tie at frame i (between predecessors at i - 1) can change frames 0 .. i - 1; the final one, every frame
    fragile = np.zeros(nf, bool)
    later = final_near
    for i in range(nf - 1, -1, -1):
        fragile[i] = later
        later = later or near[i]
    return f0, gap, fragile


def track_pitch(y, sr, hop):
    return viterbi(pitch_candidates(y, sr, hop)[0], 0.01 * sr / hop)


def pitch_candidates(y, sr, hop, eps=EPS):
    """Every frame's (freqs, strengths), with frame_candidates_diag's fragile flags and peak counts."""
    y = np.asarray(y, dtype=np.float64)
    if len(y) < min_length(sr):
        raise ValueError(f"signal of {len(y)} samples is shorter than one pitch window ({min_length(sr)} samples)")
    W = pitch_window(sr)
    w = hann(W)
    rw = np.correlate(w, w, mode="full")[W - 1:] / np.dot(w, w)
    gp = np.abs(y - y.mean()).max()
    out = [frame_candidates_diag(y[s:s + W], w, rw, sr, gp, eps) for s in pitch_starts(len(y), sr, hop)]
    return [o[:2] for o in out], np.array([o[2] for o in out], bool), np.array([o[3] for o in out], np.int64)


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


def poly_roots(a, iters=ABERTH_ITERS):
    """Roots of z^m + a1 z^(m-1) + ... + am by Aberth-Ehrlich iteration (all roots updated together), then two Newton steps."""
    return poly_roots_diag(a, iters)[0]


def poly_roots_diag(a, iters=ABERTH_ITERS):
    """poly_roots plus the number of Aberth iterations run (iters when it did not converge) and the largest step of the
    last one relative to its root."""
    m = len(a) - 1
    if m == 0:
        return np.zeros(0, complex), 0, 0.0
    z = 0.9 * np.exp(1j * (2.0 * np.pi * np.arange(m) / m + 0.25))

    def pd(zz):
        p = np.ones_like(zz)
        d = np.zeros_like(zz)
        for c in a[1:]:
            d = d * zz + p
            p = p * zz + c
        return p, d

    used = iters
    for it in range(iters):
        p, d = pd(z)
        ratio = np.where(d != 0, p / np.where(d != 0, d, 1), 0)
        diff = z[:, None] - z[None, :]
        np.fill_diagonal(diff, 1.0)
        s = (1.0 / diff).sum(axis=1) - 1.0
        w = ratio / (1.0 - ratio * s)
        z = z - w
        step = float(np.max(np.abs(w) / np.maximum(np.abs(z), 1e-300)))
        if np.all(np.abs(w) <= 1e-14 * np.maximum(np.abs(z), 1e-300)):
            used = it + 1
            break
    for _ in range(2):
        p, d = pd(z)
        z = z - np.where(d != 0, p / np.where(d != 0, d, 1), 0)
    return z, used, step


def frame_formants(x):
    return frame_formants_diag(x)[0]


def frame_formants_diag(x, root_eps=ROOT_EPS, close=CLOSE_ROOTS):
    """frame_formants plus a fragile flag: a root within root_eps (relative) of the 50 Hz or 5450 Hz cut-off, or within
    root_eps |z| of the real axis while its |frequency| is inside the band (the z.imag > 0 test), Burg stopped below order
    10, Aberth used all its iterations with its last step still above EPS (a stall at rounding level is converged), or
    two roots closer than ``close``."""
    if not np.any(x):
        return np.zeros(N_FORMANTS), False
    a = burg(x, ORDER)
    z, used, step = poly_roots_diag(a)
    fragile = len(a) - 1 < ORDER or (used >= ABERTH_ITERS and not step <= EPS)
    f = np.arctan2(z.imag, z.real) * FORMANT_SR / (2.0 * np.pi)
    lo, hi = 50.0, 0.5 * FORMANT_SR - 50.0
    fa = np.abs(f)
    fragile |= bool(np.any((np.abs(fa - lo) <= root_eps * lo) | (np.abs(fa - hi) <= root_eps * hi)))
    fragile |= bool(np.any((np.abs(z.imag) <= root_eps * np.abs(z)) & (fa > lo * (1 - root_eps)) & (fa < hi * (1 + root_eps))))
    if len(z) > 1:
        d = np.abs(z[:, None] - z[None, :])
        np.fill_diagonal(d, np.inf)
        fragile |= bool(d.min() < close)
    f = np.sort(f[(z.imag > 0) & (f > 50.0) & (f < 0.5 * FORMANT_SR - 50.0)])[:N_FORMANTS]
    return np.concatenate([f, np.zeros(N_FORMANTS - len(f))]), bool(fragile)


def formants_of_11k(x, sr, hop):
    """track_formants' frame stage on an 11 kHz signal x, its frames placed as for a signal at sr with hop: ([frames, 5]
    formants, [frames] fragile flags)."""
    x = np.asarray(x, dtype=np.float64)
    m = len(x)
    nf = 0 if m < FORMANT_WIN else (m - FORMANT_WIN) * sr // (FORMANT_SR * hop) + 1
    i = np.arange(nf, dtype=np.int64)
    starts = np.clip(((m - FORMANT_WIN) * sr + (2 * i - nf + 1) * hop * FORMANT_SR + sr) // (2 * sr), 0, m - FORMANT_WIN)
    alpha = np.exp(-2.0 * np.pi * PRE_EMPH_HZ / FORMANT_SR)
    xe = x.copy()
    xe[1:] = x[1:] - alpha * x[:-1]
    w = gauss_window(FORMANT_WIN)
    out = [frame_formants_diag(xe[s:s + FORMANT_WIN] * w) for s in starts]
    return (np.array([o[0] for o in out]).reshape(nf, N_FORMANTS), np.array([o[1] for o in out], bool))


def track_formants(y, sr, hop):
    """[frames, 5] formant frequencies in Hz (0: not found)."""
    return formants_of_11k(resample(np.asarray(y, dtype=np.float64), sr), sr, hop)[0]


def track(y, sr, hop):
    return track_pitch(y, sr, hop), track_formants(y, sr, hop)
