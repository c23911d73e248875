"""numpy / Python-int restatement of the seeded phase stream (goofer_phase_fill, goofer_amd/csrc/noise.hip), word for word.

The reference draws the aperiodic branch's phases as ``np.random.default_rng(seed).uniform(0, 2 pi, (bins, T)).astype(float32)``
(GOOFER.py:1151-1152).  That is numpy's PCG64 (XSL-RR 128/64):

  seed     np.random.PCG64(seed).state["state"] -> the 128-bit ``state`` and ``inc`` (the SeedSequence hashing stays numpy's)
  step     state <- state * MULT + inc (mod 2^128)
  output   of the NEW state: x = hi ^ lo, v = rotr64(x, hi >> 58), d = (v >> 11) * 2^-53 (float64)
  value    float32(0.0 + 2 pi * d), the float64 product rounded to nearest even
  order    element (b, t) is draw k = b * T + t (C order over (bins, T))
  jump     k steps: state <- A_k state + G_k inc, A_k = MULT^k, G_k = 1 + MULT + .. + MULT^(k-1); (A, G) of 2^j steps from a
           64-entry table, composed over the set bits of k: (A1, G1) o (A2, G2) = (A1 A2, G1 A2 + G2)
"""
import numpy as np

MULT = 47026247687942121848144207491837523525
M128 = (1 << 128) - 1
M64 = (1 << 64) - 1
TWO_PI = 2.0 * np.pi


def seed_words(seed):
    """(state, inc) of np.random.PCG64(seed) as Python ints."""
    st = np.random.PCG64(seed).state["state"]
    return int(st["state"]), int(st["inc"])


def step(state, inc):
    return (state * MULT + inc) & M128


def output(state):
    hi, lo = state >> 64, state & M64
    x = hi ^ lo
    r = hi >> 58
    return ((x >> r) | (x << ((64 - r) & 63))) & M64


def jump_table():
    """[(A, G)] of 2^j steps, j = 0 .. 63."""
    tab, A, G = [], MULT, 1
    for _ in range(64):
        tab.append((A, G))
        A, G = (A * A) & M128, (G * A + G) & M128
    return tab


_TABLE = jump_table()


def jump(state, inc, k):
    """The state ``k`` steps on (k < 2^64 by the table; larger k by repeating its top entry's square)."""
    j = 0
    A, G = None, None
    while k >> j:
        if j < 64:
            A, G = _TABLE[j]
        else:
            A, G = (A * A) & M128, (G * A + G) & M128
        if (k >> j) & 1:
            state = (A * state + G * inc) & M128
        j += 1
    return state


def values(words):
    """float32 phases of generator outputs (a uint64 array)."""
    d = (np.asarray(words, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)
    return (np.float64(0.0) + np.float64(TWO_PI) * d).astype(np.float32)


def phases(seed, n_bins, T):
    """uniform(0, 2 pi, (n_bins, T)).astype(float32) of default_rng(seed), stepped draw by draw."""
    state, inc = seed_words(seed)
    words = np.empty(n_bins * T, dtype=np.uint64)
    for k in range(n_bins * T):
        state = step(state, inc)
        words[k] = output(state)
    return values(words).reshape(n_bins, T)


def phases_by_jump(seed, n_bins, T, frames=None):
    """The same matrix the way the kernel makes it: per bin one jump to draw b * T + t0, then steps along the frames.
    ``frames``: (t0, t1) to make only those columns."""
    state0, inc = seed_words(seed)
    t0, t1 = (0, T) if frames is None else frames
    words = np.empty((n_bins, t1 - t0), dtype=np.uint64)
    for b in range(n_bins):
        s = jump(state0, inc, b * T + t0)
        for t in range(t1 - t0):
            s = step(s, inc)
            words[b, t] = output(s)
    return values(words)


def numpy_phases(seed, n_bins, T):
    return np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=(n_bins, T)).astype(np.float32)
