"""The dynamic range compressor restated in numpy (the definition: include/goofer_hip.h, "dynamic range compressor"), and the
inputs of tests/test_compress_plan.py and tests/test_gpu_compress.py.

``sequential`` is the definition as a plain loop, in float64 or in long double; ``blocked`` is the same recurrences vectorised
across blocks of 4096 samples — a sweep over the columns from the neutral state, a walk over the blocks' carries, a second
sweep from the true states — which keeps a reference of 16 M samples at a second or so.  The wrong variants that
tests/test_compress_plan.py holds against the bounds are arguments of ``sequential``.

Tolerances (derived, not measured): a detector error of d dB moves the gain by a relative ln(10) / 20 d = 0.1151 d, so
|yl - yl_ref| <= 2^-22 dB keeps g within 2^-25; with the one fp32 rounding (2^-24), |y - y_ref| <= 2^-23 |y_ref| + 2^-149,
y_ref the unrounded product."""
import functools
import math

import numpy as np

TILE = 4096
RUN_TILES = 16
ROUND_TILES = 4096
FLOOR = 1e-6
TOL_DB = 2.0 ** -22                 # |yl - yl_ref|, dB
TOL_REL, TOL_ABS = 2.0 ** -23, 2.0 ** -149      # |y - y_ref| <= TOL_REL |y_ref| + TOL_ABS
RATES = (8000, 44100, 48000, 96000)
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5, 16 * 4096 + 301)      # the last: over 16 tiles
THRESHOLD = -20.0
# (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db)
SETS = {"defaults": (THRESHOLD, 4.0, 6.0, 5.0, 100.0, 0.0),
        "hard": (THRESHOLD, math.inf, 0.0, 0.0, 100.0, 0.0),
        "norelease": (THRESHOLD, 4.0, 6.0, 5.0, 0.0, 0.0),
        "slow": (THRESHOLD, 3.0, 40.0, 50.0, 1000.0, 6.0)}


def words(a):
    """the bit patterns of an fp32 or float64 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def coefficient(ms, sr, dtype=np.float64):
    """aA / aR: 0 for 0 ms, else exp(-1 / (ms * 1e-3 * sr)) — in float64 whatever ``dtype`` is, as the definition has it (the
    coefficients are the host's float64 numbers; a long-double exp would be another filter: 1 - a has 12 bits fewer than a)"""
    return dtype(0.0 if ms == 0 else math.exp(-1.0 / (float(ms) * 1e-3 * float(sr))))


def levels(x, settings, dtype=np.float64, hard_knee=False, floor_after_log=False):
    """xl of the definition for every sample of x (vectorised: it has no state).  Wrong variants: ``hard_knee`` ignores W;
    ``floor_after_log`` applies the constant 1e-6 to the level in dB instead of to |x|."""
    T, R, W, _, _, _ = settings
    T, W = dtype(T), dtype(0.0 if hard_knee else W)
    s = dtype(1.0) / dtype(R) - dtype(1.0)
    a = np.abs(np.asarray(x).astype(dtype))
    with np.errstate(divide="ignore"):
        if floor_after_log:
            xg = np.maximum(dtype(20.0) * np.log10(a), dtype(FLOOR))
        else:
            xg = dtype(20.0) * np.log10(np.maximum(a, dtype(FLOOR)))
    d = xg - T
    xl = -s * d
    if W > 0:
        knee = np.abs(dtype(2.0) * d) <= W
        xl = np.where(knee, -s * ((d + W / dtype(2.0)) * (d + W / dtype(2.0))) / (dtype(2.0) * W), xl)
    return np.where(dtype(2.0) * d < -W, dtype(0.0), xl)


def sequential(x, sr, settings, dtype=np.float64, state_dtype=None, zero_every=0, history=(0.0, 0.0), swap=False, **wrong):
    """The definition as a plain loop: (y1, yl), arrays of ``dtype`` (float64 or longdouble).  Wrong variants: ``state_dtype``
    rounds both states to it after every sample; ``zero_every`` loses both states every so many samples; ``history`` is the
    state (y1, yl) in front of the signal; ``swap`` exchanges attack and release; ``hard_knee`` / ``floor_after_log``: see
    ``levels``."""
    _, _, _, att, rel, _ = settings
    if swap:
        att, rel = rel, att
    aA, aR = coefficient(att, sr, dtype), coefficient(rel, sr, dtype)
    xl = levels(x, settings, dtype, **wrong)
    n = len(xl)
    y1, yl = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    plain = dtype is np.float64 and state_dtype is None
    if plain:                                                   # Python floats are float64: the same arithmetic, faster
        aA, aR, xl = float(aA), float(aR), xl.tolist()
    bA, bR = 1.0 - aA, 1.0 - aR
    p, q = (float(history[0]), float(history[1])) if plain else (dtype(history[0]), dtype(history[1]))
    o1, ol = [0.0] * n, [0.0] * n
    for i in range(n):
        if zero_every and i and i % zero_every == 0:
            p, q = p * 0, q * 0
        v = xl[i]
        r = aR * p + bR * v
        p = v if v >= r else r
        q = aA * q + bA * p
        if state_dtype is not None:
            p, q = dtype(state_dtype(p)), dtype(state_dtype(q))
        o1[i], ol[i] = p, q
    y1[:], yl[:] = o1, ol
    return y1, yl


def blocked(x, sr, settings, block=TILE):
    """(y1, yl) in float64 like ``sequential``, vectorised across blocks of ``block`` samples.  Samples past the end count as
    xl = 0; a block's release summary is the pair (C, B) of the map y -> max(C, aR^block y + B), from the neutral (0, 0)."""
    _, _, _, att, rel, _ = settings
    aA, aR = float(coefficient(att, sr)), float(coefficient(rel, sr))
    bA, bR = 1.0 - aA, 1.0 - aR
    n = len(x)
    nb = -(-n // block)
    if nb == 0:
        return np.zeros(0), np.zeros(0)
    xl = np.zeros(nb * block)
    xl[:n] = levels(x, settings)
    xl = np.ascontiguousarray(xl.reshape(nb, block).T)          # [block, nb]: a column sweep reads a row
    C, B = np.zeros(nb), np.zeros(nb)
    for j in range(block):
        b = bR * xl[j]
        C = np.maximum(xl[j], aR * C + b)
        B = aR * B + b
    AR, st, s = aR ** block, np.zeros(nb), 0.0
    for k in range(nb):
        st[k] = s
        s = max(C[k], AR * s + B[k])
    y1 = np.empty_like(xl)
    e = np.zeros(nb)
    for j in range(block):
        st = np.maximum(xl[j], aR * st + bR * xl[j])
        y1[j] = st
        e = aA * e + bA * st
    AA, at, s = aA ** block, np.zeros(nb), 0.0
    for k in range(nb):
        at[k] = s
        s = AA * s + e[k]
    yl = np.empty_like(xl)
    for j in range(block):
        at = aA * at + bA * y1[j]
        yl[j] = at
    return y1.T.reshape(-1)[:n], yl.T.reshape(-1)[:n]


def gain(yl, makeup_db, dtype=np.float64):
    """g of the definition: 10^((M - yl) / 20), exactly 1 where M - yl == 0"""
    ex = (dtype(makeup_db) - np.asarray(yl).astype(dtype)) / dtype(20.0)
    return np.where(ex == 0, dtype(1.0), np.power(dtype(10.0), ex))


def product(x, yl, makeup_db, dtype=np.float64):
    """double(x) * g, not rounded to fp32: what the output bound is taken against"""
    return np.asarray(x).astype(dtype) * gain(yl, makeup_db, dtype)


def output(x, yl, makeup_db):
    """y of the definition: the float64 product rounded once to fp32"""
    return product(x, yl, makeup_db).astype(np.float32)


def max_reduction(yl):
    return float(np.max(yl)) if len(yl) else 0.0


def within_output_bound(y, want, scale=1.0, slack=0.0):
    """|y - want| <= scale (TOL_REL |want| + TOL_ABS) + slack |want| per sample; the worst ratio to the full bound"""
    want = np.asarray(want).astype(np.longdouble)
    err = np.abs(np.asarray(y).astype(np.longdouble) - want)
    bound = TOL_REL * np.abs(want) + TOL_ABS
    ok = bool(np.all(err <= scale * bound + slack * np.abs(want)))
    return ok, float(np.max(err / bound)) if len(want) else 0.0


# ---- fixtures --------------------------------------------------------------------------------------------------------------

def signal(sr, n, seed, first_db=15.0, last_db=None):
    """An amplitude-modulated sine plus noise whose level steps every 20 ms between about 20 dB under and 15 dB over THRESHOLD
    (attack, release and knee all at work); the first step is ``first_db`` over, so that the shortest signal is compressed
    too.  A few exact zeros and samples of 2^-90 sit in it (the detector's floor): no non-zero sample lies below 2^-100."""
    rng = np.random.default_rng([sr, n, seed])
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    step = max(8, sr // 50)
    k = -(-n // step)
    lev = rng.choice(np.array([-20.0, -12.0, -4.0, -1.0, 2.0, 7.0, 15.0]), size=k)
    lev[0] = first_db
    if last_db is not None:
        lev[-1] = last_db
    amp = np.repeat(10.0 ** ((THRESHOLD + lev) / 20.0), step)[:n]
    t = np.arange(n) / float(sr)
    x = amp * (np.sin(2.0 * np.pi * 220.0 * t) * (1.0 + 0.3 * np.sin(2.0 * np.pi * 5.0 * t)) / 1.3 + 0.05 * rng.standard_normal(n))
    x = x.astype(np.float32)
    if n >= 15:
        at = rng.choice(n, size=min(6, n // 5), replace=False)
        x[at[::2]] = 0.0
        x[at[1::2]] = np.float32(2.0 ** -90)
    x[(x != 0) & (np.abs(x) < np.float32(2.0 ** -100))] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def batch(sr):
    """the signals of LENGTHS at ``sr``, back to back in one batch (86 k samples); each ends loud, so that a detector state
    handed to the next signal would be far from the zero it has to start with"""
    return tuple(signal(sr, n, i, last_db=15.0) for i, n in enumerate(LENGTHS))


LONG = len(LENGTHS) - 1             # the signal over 16 tiles


@functools.lru_cache(maxsize=None)
def reference(sr, name, i, flavour="f64"):
    """(y1, yl) of signal i of batch(sr) under SETS[name] by ``sequential``: 'f64' or 'ld'"""
    return sequential(batch(sr)[i], sr, SETS[name], np.float64 if flavour == "f64" else np.longdouble)


@functools.lru_cache(maxsize=None)
def quiet_signal(sr=48000, n=3 * TILE + 77, knee_db=6.0):
    """every sample at or under THRESHOLD - knee / 2: the identity property's input"""
    rng = np.random.default_rng([sr, n, 99])
    top = 10.0 ** ((THRESHOLD - knee_db / 2.0) / 20.0) * (1.0 - 2.0 ** -20)
    x = (top * rng.uniform(-1.0, 1.0, n)).astype(np.float32)
    x[5], x[6] = 0.0, np.float32(top)
    assert float(np.abs(x).max()) <= top
    return x


@functools.lru_cache(maxsize=None)
def long_signal(sr=48000, tiles=ROUND_TILES + RUN_TILES + 3, tail=1234):
    """One signal longer than a round of the carry kernels (ROUND_TILES tiles), loud over the 20 ms in front of the round
    boundary and quiet behind it, so that the state which crosses it is large and what follows depends on it."""
    n = tiles * TILE + tail
    rng = np.random.default_rng([sr, n, 7])
    step = sr // 50
    k = -(-n // step)
    lev = rng.choice(np.array([-20.0, -4.0, 2.0, 15.0]), size=k)
    kb = ROUND_TILES * TILE // step
    lev[kb - 1:kb + 1], lev[kb + 1:kb + 4] = 15.0, -20.0
    amp = np.repeat((10.0 ** ((THRESHOLD + lev) / 20.0)).astype(np.float32), step)[:n]
    x = amp * rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return sr, x
