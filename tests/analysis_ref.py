"""CPU restatement of the envelope and knot-search analysis (GOOFER.py:97-147, 942-946), used only by the tests.

Built from the oracle (``oracle/goofer_ref.py``: ``stft``, ``gauss1d``, ``mel_knots``, ``lerp_matrix``) so that the GPU's
cold-sample analysis can be checked stage by stage:

* ``candidate_errors``: the max relative error of every candidate knot count K = 32, 48, ..., 192 with exactly the
  arithmetic of ``compress_env_to_knots`` (which returns only the chosen pack), and ``decide`` / ``margin`` on top of it;
* ``probe_rows``: the probe frames of the K search, numpy's ``linspace(0, T - 1, min(256, T), dtype=int)``;
* ``truth_envelope``: the same envelope in fp64 throughout, the yardstick for the oracle and the GPU alike;
* the signals the tests analyse, including the ones built to sit on the eps = 1e-2 decision boundary and on the frames the
  probe set skips.
"""
import functools

import numpy as np

from oracle import goofer_ref as R

EPS = 1e-2
CANDIDATES = tuple(range(32, 193, 16))          # compress_env_to_knots' K_start, K_step, K_max
F32 = np.float32


# -- the K search ---------------------------------------------------------------------------------------------------
def probe_rows(T):
    return np.linspace(0, T - 1, min(256, T), dtype=int)


def candidate_bins(sr, n_fft, K):
    """(knot Hz fp32, nearest bin of each) as compress_env_to_knots makes them."""
    n_bins = n_fft // 2 + 1
    _, hz = R.mel_knots(sr, n_fft, K)
    return hz, np.clip(np.round(hz / (sr / n_fft)).astype(int), 0, n_bins - 1)


def candidate_errors(env_spec, sr, n_fft):
    """fp64 [11]: max relative error of the lerp from each candidate's knots over the probe frames, as compress_env_to_knots
    computes it (fp32 envelope, sigma 0.5 blur in fp64, fp32 log knots, fp32 lerp, error in fp64).  NaN propagates like
    numpy's max does."""
    env = R.gauss1d(np.asarray(env_spec, dtype=F32), 0.5, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        log_env = np.log(np.maximum(env, 1e-8)).astype(F32)
        freqs = np.fft.rfftfreq(n_fft, 1.0 / sr).astype(F32)
        probe = probe_rows(log_env.shape[1])
        env_probe = env[:, probe]
        out = np.empty(len(CANDIDATES))
        for c, K in enumerate(CANDIDATES):
            hz, at = candidate_bins(sr, n_fft, K)
            rec = R.lerp_matrix(freqs, hz) @ log_env[at, :][:, probe]
            out[c] = np.max(np.abs(np.exp(rec) - env_probe) / (env_probe + 1e-8))
    return out


def decide(errors, eps=EPS):
    """(K, candidate index) compress_env_to_knots picks from ``errors``: the first under eps, else the last (K = 192)."""
    for c, e in enumerate(errors):
        if e < eps:
            return CANDIDATES[c], c
    return CANDIDATES[-1], len(CANDIDATES) - 1


def deciding(errors, eps=EPS):
    """The candidates whose errors decide K: every one up to and including the chosen (all of them for the fallback)."""
    return np.asarray(errors[:decide(errors, eps)[1] + 1], dtype=np.float64)


def margin(errors, eps=EPS):
    """Smallest |err / eps - 1| over the deciding candidates (inf when they are all non-finite: no rounding can move K)."""
    d = deciding(errors, eps)
    d = d[np.isfinite(d)]
    return float(np.min(np.abs(d / eps - 1.0))) if d.size else np.inf


# -- envelopes ------------------------------------------------------------------------------------------------------
def truth_envelope(y, sr, n_fft, hop):
    """fp64 [bins, T]: |STFT| + 1e-8 -> sigma-2 bin blur of the fp32 signal, with fp64 padded frames and window, complex128
    rfft and fp64 blur."""
    x = np.asarray(y, dtype=F32).astype(np.float64)
    h = n_fft // 2
    xp = np.pad(x, h, mode="reflect" if len(x) >= 2 else "edge")
    if len(xp) < n_fft:
        xp = np.pad(xp, (0, n_fft - len(xp)), mode="edge")
    T = max(1, 1 + (len(xp) - n_fft) // hop)
    frames = xp[np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]] * (np.hanning(n_fft) ** 0.5)[:, None]
    S = np.fft.rfft(frames, axis=0)
    return R.gauss1d(np.abs(S) + 1e-8, 2.0, axis=0)


def frame_error(a, ref):
    """Per frame max_b |a - ref| / max_b ref  ([T] fp64): the envelope error of a frame relative to its own level."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.max(np.abs(a - ref), axis=0) / np.max(np.abs(ref), axis=0)


# -- signals --------------------------------------------------------------------------------------------------------
GEOMETRIES = ((44100, 1024, 256), (22050, 512, 128), (48000, 2048, 512), (96000, 2048, 96),
              (44100, 768, 192), (44100, 1000, 250), (16000, 64, 16), (44100, 512, 512))
KINDS = ("zeros", "dither", "voiced", "bursts", "square", "clicks")
DIP_KINDS = frozenset(("voiced", "bursts", "square", "clicks"))    # deep spectral dips: see test_dip_kinds_defeat_the_element_bound


def lengths_for(sr, n_fft, hop):
    """Edge lengths (reflect padding wider than the signal), lengths of 255, 256, 257 and 513 frames, and about 0.7 s."""
    edge = [1, 2, 3, hop - 1, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n_fft + 1]
    frames = [(T - 1) * hop for T in (255, 256, 257, 513)]
    return sorted(set(v for v in edge + frames if v >= 1)) + [int(0.7 * sr)]


def resonator(n, at, amp, r, f, sr):
    """A click at sample ``at`` through a two-pole resonator (radius r, centre f Hz), like the clicks of
    test_gpu_analyse_batch: the impulse response amp r^m sin((m + 1) th) / sin th in closed form."""
    th = 2 * np.pi * f / sr
    m = np.arange(n - at, dtype=np.float64)
    y = np.zeros(n)
    y[at:] = amp * r ** m * np.sin((m + 1) * th) / np.sin(th)
    return y


def harmonic(n, sr, f0, rng, partials=12):
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.02 * np.sin(2 * np.pi * 5 * t))) / sr
    y = sum(np.sin(k * ph) / k for k in range(1, partials + 1) if k * f0 < 0.45 * sr)
    return 0.3 * y / max(np.max(np.abs(y)), 1e-30) + 0.003 * rng.standard_normal(n)


def make_signal(kind, n, sr, seed):
    """fp32 samples of one content kind."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        y = np.zeros(n)
    elif kind == "dither":                                        # int16 dither, +-1 LSB
        y = rng.integers(-1, 2, size=n) / 32768.0
    elif kind == "voiced":
        y = harmonic(n, sr, float(rng.uniform(110, 330)), rng)
    elif kind == "bursts":                                        # white noise whose level jumps by 40 dB
        block = max(sr // 20, 1)
        y = np.repeat(rng.choice([0.005, 0.5], size=n // block + 1), block)[:n] * rng.standard_normal(n)
    elif kind == "square":                                        # a clipped square
        y = np.clip(1.6 * np.sign(np.sin(2 * np.pi * 220.0 * np.arange(n) / sr + 0.3)), -1, 1)
    elif kind == "clicks":
        y = np.zeros(n)
        for k, (r, f) in enumerate(((0.7, 0.2 * sr), (0.8, 0.2 * sr), (0.9, 0.05 * sr))):
            y += resonator(n, (k * n) // 3, 0.5, r, f, sr)
    else:
        raise ValueError(kind)
    return np.asarray(y, dtype=F32)


def signal_set(sr, n_fft, hop):
    """[(kind, fp32 samples)]: every length of lengths_for with the kinds in rotation, and every kind at about 0.7 s."""
    lens = lengths_for(sr, n_fft, hop)
    out = []
    for i, n in enumerate(lens[:-1]):
        kind = KINDS[(i + n_fft) % len(KINDS)]
        out.append((kind, make_signal(kind, n, sr, seed=1000 * i + n_fft)))
    for j, kind in enumerate(KINDS):
        out.append((kind, make_signal(kind, lens[-1], sr, seed=77 + j)))
    return out


# -- the eps decision boundary --------------------------------------------------------------------------------------
BOUNDARY_GEOM = (44100, 1024, 256)
BOUNDARY_N = 4096


def _click_errors(amp):
    sr, n_fft, hop = BOUNDARY_GEOM
    y = resonator(BOUNDARY_N, BOUNDARY_N // 2, amp, 0.8, 9000.0, sr).astype(F32)
    env, _ = R.envelope_of(y, sr, n_fft, hop)
    return y, candidate_errors(env, sr, n_fft)


@functools.lru_cache(maxsize=None)
def boundary_amplitude(c, target):
    """Click amplitude near the 1e-8 floor at which candidate c's oracle error equals ``target`` (bisection in log
    amplitude; relative error rises continuously with amplitude there)."""
    lo, hi = -12.0, -2.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if _click_errors(10.0 ** mid)[1][c] < target:
            lo = mid
        else:
            hi = mid
    return 10.0 ** (0.5 * (lo + hi))


def boundary_signals(cands=(0, 1, 2), rel=1e-2):
    """[(candidate index, side -1 / +1, fp32 samples, oracle errors)]: the deciding candidate's error at eps (1 + side rel)."""
    out = []
    for c in cands:
        for side in (-1, 1):
            y, errs = _click_errors(boundary_amplitude(c, EPS * (1 + side * rel)))
            out.append((c, side, y, errs))
    return out


# -- frames the probe set skips -------------------------------------------------------------------------------------
def skipped_probes(T):
    """Frames an exact integer linspace (j (T - 1) // (num - 1)) probes and numpy's floor of j * step does not."""
    num = min(256, T)
    if num < 2:
        return []
    exact = {j * (T - 1) // (num - 1) for j in range(num)}
    return sorted(exact - set(probe_rows(T).tolist()))


def with_burst(n, start, m, sr, amp=0.3, seed=0):
    """Silence with a short Hann-shaped harmonic burst over samples [start, start + m)."""
    y = np.zeros(n)
    y[start:start + m] = amp * harmonic(m, sr, 250.0, np.random.default_rng(seed), partials=8) * np.hanning(m)
    return y.astype(F32)


def own_samples(frame, n_fft, hop):
    """(start, length) of samples that frame ``frame`` sees and no earlier frame does: the window's second half past the
    previous frame's reach (all of the frame's own samples when hop = n_fft)."""
    lo = frame * hop - n_fft // 2                                # first sample of the frame in signal coordinates
    start = max(lo, (frame - 1) * hop + n_fft // 2)              # past frame - 1's last sample
    return start, lo + n_fft - start
