"""The look-ahead peak limiter restated in numpy (the definition: include/goofer_hip.h, "look-ahead peak limiter"): the
look-ahead, the raised-cosine table in float64, and the eight steps in two flavours — fp32, every operation rounded as the
definition says, which the kernel must give bit for bit; and float64, which takes the fp32 r and the fp32 table, so that every
min / compare decision up to step 3 is the same, and does steps 4 to 8 in float64."""
import math

import numpy as np

MAX_LOOK, CEILING, LOOK_MS = 1024, np.float32(32767.0 / 32768.0), 5.0


def look(sr, look_ms=LOOK_MS):
    """W = floor(look_ms * sr / 1000 + 0.5), float64"""
    return int(math.floor(float(look_ms) * float(sr) / 1000.0 + 0.5))


def table64(W):
    """w[j], j = -W .. W, divided by its float64 sum (before the rounding to fp32)"""
    j = np.arange(-W, W + 1, dtype=np.float64)
    w = 1.0 + np.cos(np.pi * j / float(W + 1))
    return w / w.sum()


def table32(W):
    return table64(W).astype(np.float32)


def ratio(x, c):
    """steps 1 and 2: (a, r), fp32; the division is numpy's fp32 one, correctly rounded"""
    a = np.abs(np.asarray(x, dtype=np.float32))
    c = np.float32(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a > c, c / a, np.float32(1.0)).astype(np.float32)
    return a, r


def window_min(r, W):
    """step 3: m[i] = min r[k], k in [i - W, i + W] within the signal"""
    n = len(r)
    if n == 0:
        return r.copy()
    pad = np.concatenate([np.full(W, np.inf, r.dtype), r, np.full(W, np.inf, r.dtype)])
    return np.lib.stride_tricks.sliding_window_view(pad, 2 * W + 1).min(axis=1)


def limit_batch(signals, taps, W, c, dtype=np.float32):
    """[(y, g, peak_in, min_gain)] of the signals on the table ``taps`` (fp32 [2W + 1]).  dtype float32: the definition's own
    arithmetic; float64: steps 4 to 8 without rounding worth speaking of.  Every signal is taken by itself up to step 4; the tap
    loop of step 5 then runs once, over the signals' padded d arrays laid end to end (the same operations per sample, fewer
    numpy calls), and each signal reads its own stretch of the result."""
    one = dtype(1.0)
    xs = [np.asarray(x, dtype=np.float32) for x in signals]
    ar = [ratio(x, c) for x in xs]
    pads, starts, at = [], [], 0
    for _, r in ar:
        d = one - window_min(r, W).astype(dtype)               # steps 3 and 4
        if len(d):                                             # d[clamp(i + j, 0, n - 1)] = pad[i + j + W]
            pads.append(np.concatenate([np.full(W, d[0], dtype), d, np.full(W, d[-1], dtype)]))
        starts.append(at)
        at += len(d) + 2 * W if len(d) else 0
    dp = np.concatenate(pads + [np.zeros(0, dtype)])
    w = np.asarray(taps, dtype=np.float32).astype(dtype)
    span = max(len(dp) - 2 * W, 0)
    acc = np.zeros(span, dtype=dtype)
    for k in range(2 * W + 1):                                 # j = k - W, ascending
        acc = acc + w[k] * dp[k:k + span]                      # one rounded multiply, one rounded add
    out = []
    for x, (a, r), s0 in zip(xs, ar, starts):
        s = np.maximum(one - acc[s0:s0 + len(x)], dtype(0.0))
        g = np.minimum(s, r.astype(dtype))
        y = x.astype(dtype) * g
        out.append((y, g, (a.max() if len(a) else np.float32(0.0)), (g.min() if len(g) else dtype(1.0))))
    return out


def limit(x, taps, W, c, dtype=np.float32):
    """(y, g, peak_in, min_gain) of one signal"""
    return limit_batch([x], taps, W, c, dtype)[0]


def bound(x, W):
    """|fp32 y - float64 y| per sample: one rounding per product and one per add of the 2W + 1 taps, and the four of d, s, and
    the product y (with slack for g's own): (2 (2W + 1) + 4) 2^-24 |x[i]|."""
    return (2 * (2 * W + 1) + 4) * 2.0 ** -24 * np.abs(np.asarray(x, dtype=np.float64))


def pcm16(y):
    """goofer_pcm16 on the host: clip to [-1, 1 - 2^-15], * 32768, round half to even"""
    return np.round(np.clip(np.asarray(y, dtype=np.float64), -1.0, 1.0 - 1.0 / 32768) * 32768.0).astype("<i2")


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
