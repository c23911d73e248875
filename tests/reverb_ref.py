"""The convolution reverb restated in numpy (include/goofer_hip.h, "convolution reverb"), for tests/test_reverb_ref.py,
tests/test_reverb_plan.py and tests/test_gpu_reverb.py.

Three things: ``reference``, the definition in float64 (one zero-padded np.fft convolution per signal; ``direct`` is the same by
np.convolve, for short cases); ``tables``, the host planner's tables; and ``tiled``, a model of the kernels' scheme in np.float32
/ np.complex64 — the same blocks of 1024 samples counted from the signal's start, the same partitions, the same order over p —
from which the tolerance is measured (tests/test_reverb_ref.py).  The model's transform is numpy's, not the kernels', and it
multiplies and adds where they fuse: the factor 4 in the tolerance covers both.

The inputs come from an integer hash, not from a numpy generator: the same numbers on every numpy."""
import math

import numpy as np

B = 1024                            # GOOFER_REVERB_BLOCK
RUN = 32                            # GOOFER_REVERB_RUN
MAX_TAPS = 1 << 18
MAX_PREDELAY = 1 << 16
TOL = 2.0 ** -19                    # GOOFER_REVERB_TOL

LENGTHS = [0, 1, B - 1, B, B + 1, 3 * B + 17, 700]
IR_LENGTHS = [1, B, B + 1, 2 * B + 5]
PREDELAYS = [0, 1, B - 1, B + 3]
WET, DRY = 0.5, 0.75                # the gains of the batch cases (linear)


def noise(n, seed) -> np.ndarray:
    """n numbers in [-1, 1) from a 32-bit integer hash of (seed, index): fp32, the same on every platform"""
    v = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)
    v &= np.uint64(0xFFFFFFFF)
    for s, m in ((16, 0x45D9F3B), (16, 0x45D9F3B), (16, 1)):
        v = ((v ^ (v >> np.uint64(s))) * np.uint64(m)) & np.uint64(0xFFFFFFFF)
    return (v.astype(np.float64) / 2147483648.0 - 1.0).astype(np.float32)


def signals(seed=0):
    """the batch of the GPU tests: LENGTHS, noise of 0.3 peak with a step of DC in the longest"""
    xs = [0.3 * noise(n, 100 * seed + i) for i, n in enumerate(LENGTHS)]
    xs[5][B + 100:] += np.float32(0.2)
    return [x.astype(np.float32) for x in xs]


def ir(L, seed=0) -> np.ndarray:
    """an impulse response of L taps: decaying noise, unit peak at tap 0"""
    h = noise(L, 7000 + seed).astype(np.float64) * np.exp(-3.0 * np.arange(L) / max(L, 1))
    h[0] = 1.0
    return h.astype(np.float32)


def n_out(n, L, pre, tail) -> int:
    return 0 if n == 0 else n + (pre + L - 1 if tail else 0)


def reference(x, h, pre=0, tail=True, dry=1.0, wet=1.0) -> np.ndarray:
    """The definition in float64: y[i] = dry x[i] + wet sum_k h[k] x[i - pre - k] for 0 <= i < n_out; one zero-padded FFT
    convolution.  ``dry`` / ``wet`` are taken as the fp32 numbers the library is given."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n, L = len(x), len(h)
    m = n_out(n, L, pre, tail)
    if m == 0:
        return np.zeros(0)
    size = 1 << int(math.ceil(math.log2(n + L)))
    c = np.fft.irfft(np.fft.rfft(x, size) * np.fft.rfft(h, size), size)[:n + L - 1]
    y = np.zeros(max(m, pre + n + L - 1))
    y[pre:pre + n + L - 1] = float(np.float32(wet)) * c
    y[:n] += float(np.float32(dry)) * x
    return y[:m]


def direct(x, h, pre=0, tail=True, dry=1.0, wet=1.0) -> np.ndarray:
    """``reference`` by np.convolve: for short cases"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    m = n_out(len(x), len(h), pre, tail)
    if m == 0:
        return np.zeros(0)
    y = np.zeros(max(m, pre + len(x) + len(h) - 1))
    y[pre:pre + len(x) + len(h) - 1] = float(np.float32(wet)) * np.convolve(x, h)
    y[:len(x)] += float(np.float32(dry)) * x
    return y[:m]


def tables(lengths, L, pre, tail):
    """goofer_host_reverb_plan's tables: (out_off, blk_off, runs): int64 [n + 1] twice, int32 [n_runs, 3]"""
    outs = [n_out(int(n), L, pre, tail) for n in lengths]
    blks = [(m + B - 1) // B for m in outs]
    runs = [(i, first, min(RUN, nb - first)) for i, nb in enumerate(blks) for first in range(0, nb, RUN)]
    return (np.concatenate([[0], np.cumsum(outs)]).astype(np.int64), np.concatenate([[0], np.cumsum(blks)]).astype(np.int64),
            np.array(runs, dtype=np.int32).reshape(-1, 3))


def ir_spectra(h):
    """H[p] (complex64 [P, B + 1]) and the live flags of goofer_reverb_ir: partition p and B zeros, transformed in float32; a
    partition whose taps are all zero is exact zeros"""
    h = np.asarray(h, dtype=np.float32)
    P = (len(h) + B - 1) // B
    parts = np.zeros((P, 2 * B), dtype=np.float32)
    for p in range(P):
        seg = h[p * B:(p + 1) * B]
        parts[p, :len(seg)] = seg
    live = np.any(parts != 0.0, axis=1)
    H = np.fft.rfft(parts, axis=1).astype(np.complex64)
    H[~live] = 0
    return H, live


def _mac(X, H):
    """complex64 X H, bins 0 and B (both real) element by element, as the packed slot 0 of the kernels' rows does"""
    y = X * H
    y[0] = np.float32(X[0].real * H[0].real)
    y[-1] = np.float32(X[-1].real * H[-1].real)
    return y


def tiled(x, h, pre=0, tail=True, dry=1.0, wet=1.0, skip=True) -> np.ndarray:
    """The kernels' scheme in float32 / complex64: block j of the signal is the transform of x[(j - 1) B - pre .. (j + 1) B - pre),
    Y[b] = sum of X[q] H[b - q] over q = max(0, b - P + 1) .. b ascending (p descending), live partitions only with ``skip``; the
    last B samples of the inverse transform of Y[b] are c[b B .. (b + 1) B); y = dry x + wet c in fp32."""
    x = np.asarray(x, dtype=np.float32)
    n, L = len(x), len(h)
    m = n_out(n, L, pre, tail)
    if m == 0:
        return np.zeros(0, dtype=np.float32)
    dry, wet = np.float32(dry), np.float32(wet)
    xp = np.zeros(max(m, n), dtype=np.float32)
    xp[:n] = x
    if wet == 0.0:
        y = xp[:m].copy()
        return y if dry == 1.0 else (dry * y).astype(np.float32)
    H, live = ir_spectra(h)
    P, nb = len(H), (m + B - 1) // B
    pad = np.zeros(B + pre + nb * B + B, dtype=np.float32)          # pad[B + pre + i] = x[i]
    pad[B + pre:B + pre + n] = x
    X = np.fft.rfft(np.stack([pad[j * B:(j + 2) * B] for j in range(nb)]), axis=1).astype(np.complex64)
    c = np.zeros(nb * B, dtype=np.float32)
    for b in range(nb):
        acc = np.zeros(B + 1, dtype=np.complex64)
        for q in range(max(0, b - P + 1), b + 1):
            if live[b - q] or not skip:
                acc = acc + _mac(X[q], H[b - q])
        c[b * B:(b + 1) * B] = np.fft.irfft(acc, 2 * B)[B:].astype(np.float32)
    return (dry * xp[:m] + wet * c[:m]).astype(np.float32)


def error(y, ref) -> float:
    """max |y - ref| / max |ref| of one signal (0 for an empty one; an all-zero reference must be met exactly)"""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert y.shape == ref.shape
    if not len(ref):
        return 0.0
    peak = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(y - ref)))
    return err / peak if peak > 0.0 else (0.0 if err == 0.0 else math.inf)


def batch_cases():
    """(L, pre, tail) of the GPU test of the batch: every IR length with every pre-delay, tail on and off"""
    return [(L, pre, tail) for L in IR_LENGTHS for pre in PREDELAYS for tail in (True, False)]


def long_cases():
    """(x, h) with more partitions than a run has blocks, and with the most there are: L = 40 B + 3 over 8 B samples, L = 2^18
    over 2000 samples (258 output blocks)"""
    return [(0.3 * noise(8 * B, 31), ir(40 * B + 3, 1)), (0.3 * noise(2000, 32), ir(MAX_TAPS, 2))]


def dead_case():
    """(xs, h): 70 partitions, number 33 all zero, over signals of 40 B + 5, 100 B - 1 and 700 samples; pre-delay 2, DRY, WET"""
    h = ir(69 * B + 11, 3)
    h[33 * B:34 * B] = 0.0
    return [0.3 * noise(n, 50 + i) for i, n in enumerate((40 * B + 5, 100 * B - 1, 700))], h


IMPULSE_AT = [0, 1, B - 1, B, B + 1, 2 * B - 1]
IMPULSE_LEN = 2 * B + 5             # samples of the signal that holds the unit sample
IMPULSE_PRE = [0, B + 3]


def impulse(q) -> np.ndarray:
    x = np.zeros(IMPULSE_LEN, dtype=np.float32)
    x[q] = 1.0
    return x


def tolerance_rule(worst) -> float:
    """4 times the model's worst error, rounded up to a power of two"""
    return 2.0 ** math.ceil(math.log2(4.0 * worst))


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
