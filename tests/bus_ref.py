"""The stereo bus restated in numpy (the definition: include/goofer_hip.h, "stereo bus"): the pan law in float64, the mix in the
fp32 order of the definition, the cover table by brute force, the channel-linked limiter and loudness gate on top of limit_ref,
true_peak_ref and loudness_ref (which stay as they are), and the interleaving int16 conversion."""
import math

import numpy as np

import limit_ref as LR
import loudness_ref as LR2
import true_peak_ref as TR

TILE = 2048
MIN_GAIN_DB, MAX_GAIN_DB = -144.0, 24.0


def gains(gain_db, pan):
    """(gl, gr), fp32: g = 10^(gain_db / 20), theta = (pan + 1) pi / 4 in float64; exact at pan -1, 0 and 1"""
    gain_db, pan = float(gain_db), float(pan)
    if not math.isfinite(gain_db) or not MIN_GAIN_DB <= gain_db <= MAX_GAIN_DB or not -1.0 <= pan <= 1.0:
        raise ValueError("gain_db in [-144, 24], pan in [-1, 1]")
    g = 10.0 ** (gain_db / 20.0)
    if pan == -1.0:
        return np.float32(g), np.float32(0.0)
    if pan == 1.0:
        return np.float32(0.0), np.float32(g)
    if pan == 0.0:
        return np.float32(g * math.sqrt(0.5)), np.float32(g * math.sqrt(0.5))
    th = (pan + 1.0) * math.pi / 4.0
    return np.float32(g * math.cos(th)), np.float32(g * math.sin(th))


def mix(xs, tracks, total_out):
    """The planar bus, fp32 [2 total_out]: ``tracks`` = [(start, gl, gr)] for the signals ``xs``; the sum in ascending track index
    from +0.0f, one rounded multiply and one rounded add per term, a track only where it sounds."""
    N = int(total_out)
    out = np.zeros(2 * N, dtype=np.float32)
    for x, (start, gl, gr) in zip(xs, tracks):
        x = np.asarray(x, dtype=np.float32)
        lo, hi = int(start), min(int(start) + len(x), N)
        if hi <= lo:
            continue
        seg = x[:hi - lo]
        out[lo:hi] = out[lo:hi] + np.float32(gl) * seg
        out[N + lo:N + hi] = out[N + lo:N + hi] + np.float32(gr) * seg
    return out


def cover(starts, lens, total_out):
    """(tile_off, tile_tracks) by brute force: every tile against every track"""
    tiles = (int(total_out) + TILE - 1) // TILE
    off, lst = [0], []
    for t in range(tiles):
        a, b = t * TILE, min((t + 1) * TILE, int(total_out))
        for i, (s, n) in enumerate(zip(starts, lens)):
            if n > 0 and max(a, int(s)) < min(b, int(s) + int(n)):
                lst.append(i)
        off.append(len(lst))
    return np.array(off, dtype=np.int64), np.array(lst, dtype=np.int32)


def limit_linked(chans, taps, W, c, tp_taps=None):
    """([y_c], g, peak_in, min_gain) of one group: the limiter's definition on a[i] = max_c |x_c[i]| (with ``tp_taps``: max_c
    e_c[i], the true-peak envelope), fp32; y_c = x_c g.  limit_ref makes a and r from the signal it is given, so it is given a.
    The maximum ignores a NaN operand (the kernel's fmaxf); for every other input np.fmax is np.maximum."""
    xs = [np.asarray(x, dtype=np.float32) for x in chans]
    if tp_taps is None:
        a = np.fmax.reduce([np.abs(x) for x in xs])
    else:
        a = np.fmax.reduce([TR.envelope(x, tp_taps, np.float32) for x in xs])
    _, g, peak, gmin = LR.limit(a, taps, W, c)
    return [x * g for x in xs], g, np.float32(peak), gmin


def loud_linked(E0, E1, S, target=None, cap=LR2.MAX_GAIN_DB):
    """(L, momentary_max, g) of a stereo programme from its channels' segment energies: the gate on E0 + E1"""
    return LR2.stats(np.asarray(E0, dtype=np.float64) + np.asarray(E1, dtype=np.float64), S, target, cap)


def pcm16_planar(x, ch=2):
    """int16 [n, ch]: out[i, c] = pcm16(x[c n + i])"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x) // ch
    return np.ascontiguousarray(LR.pcm16(x).reshape(ch, n).T)


def burst_pair(n=9000, lo=4090, hi=4100, seed=3):
    """A quiet pair (|x| <= 0.3) of ``n`` samples with a burst of 1.5 at [lo, hi] in L only: the burst straddles the tile
    boundary at 4096, R is quiet throughout."""
    rng = np.random.default_rng(seed)
    L = (0.3 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    R = (0.3 * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    a, b = min(lo, n), min(hi + 1, n)
    L[a:b] = np.float32(1.5) * np.where(np.arange(a, b) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return L, R


LOOKS = (1, 7, 240)
CEILINGS = (np.float32(0.891), np.float32(0.5), np.float32(32767.0 / 32768.0))
