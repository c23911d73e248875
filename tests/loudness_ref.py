"""The loudness definition of include/goofer_hip.h (after ITU-R BS.1770-4, one channel) restated sample by sample in numpy only:
coefficients, recurrences, segments, gating and gain.  Two flavours of the arithmetic, float64 and ``np.longdouble``; both use
the float64 coefficients, which are part of the definition.  The keyword switches produce deliberately WRONG variants, which
the host tests use to show that the GPU tests' bounds would catch them.  Also here: the inputs the GPU tests and the host tests
share (``batch``, ``gating_fixture``), cached per process."""
import functools
import math

import numpy as np

MIN_SR, MAX_SR = 8000, 192000
MAX_GAIN_DB = 20.0
TILE = 4096
RUN_TILES = 16                      # tiles a thread of the tile-to-tile kernel walks
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
TOL = 2.0 ** -26                    # |E - E_longdouble| <= TOL * max E, per signal
RATES = (8000, 44100, 48000, 96000)

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def seg_len(sr):
    return int(math.floor(sr / 10.0 + 0.5))


def coefficients(sr):
    """float64 [10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2"""
    K, Q = math.tan(math.pi * 1681.974450955533 / sr), 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
         (1.0 - K / Q + K * K) / a0]
    K, Q = math.tan(math.pi * 38.13547087602444 / sr), 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return np.array(c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def transition(sr):
    """the 4x4 matrix A of the state (u1, u2, v1, v2) for x = 0"""
    c = coefficients(sr)
    return np.array([[-c[3], -c[4], 0.0, 0.0], [1.0, 0.0, 0.0, 0.0],
                     [c[6] - c[5] * c[3], c[7] - c[5] * c[4], -c[8], -c[9]], [0.0, 0.0, 1.0, 0.0]], dtype=np.float64)


def weighted_squares(x, sr, dtype=np.float64, state_dtype=None, zero_every=0, history=None):
    """v[i]^2 of the signal x, ``dtype`` [n], and the final (x1, x2, u1, u2, v1, v2).  WRONG on purpose: ``state_dtype`` rounds
    the state to that type after every sample; ``zero_every`` N zeroes the state at every multiple of N; ``history`` starts
    from another signal's final state."""
    conv = float if dtype is np.float64 else dtype            # (Python floats are IEEE doubles, and the loop is faster on them)
    c = [conv(v) for v in coefficients(sr)]
    xs = [conv(v) for v in np.asarray(x, dtype=np.float32).astype(np.float64)]
    zero = conv(0.0)
    x1, x2, u1, u2, v1, v2 = history if history is not None else (zero,) * 6
    out = [zero] * len(xs)
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = c
    for i, xv in enumerate(xs):
        if zero_every and i and i % zero_every == 0:
            u1 = u2 = v1 = v2 = zero
        u = b0 * xv + b1 * x1 + b2 * x2 - a1 * u1 - a2 * u2
        v = d0 * u + d1 * u1 + d2 * u2 - e1 * v1 - e2 * v2
        out[i] = v * v
        if state_dtype is not None:
            u, v = conv(state_dtype(u)), conv(state_dtype(v))
        x2, x1, u2, u1, v2, v1 = x1, xv, u1, u, v1, v
    return np.array(out, dtype=dtype), (x1, x2, u1, u2, v1, v2)


def seg_energy(sq, S, partial=False):
    """E[k], the sums of sq over whole segments of S.  WRONG on purpose: ``partial`` counts a trailing partial segment."""
    kn = len(sq) // S
    E = sq[:kn * S].reshape(kn, S).sum(axis=1)
    if partial and len(sq) > kn * S:
        E = np.concatenate([E, [sq[kn * S:].sum()]])
    return E


def blocks(E, S):
    E = np.asarray(E)
    kb = max(0, len(E) - 3)
    return (E[0:kb] + E[1:kb + 1] + E[2:kb + 2] + E[3:kb + 3]) / (4 * S) if kb else np.zeros(0, dtype=E.dtype)


def gate_classes(z):
    """(under the absolute gate, between the gates, above both) as boolean arrays, and the two thresholds"""
    ab = z > ABS_GATE
    rel = 0.1 * z[ab].mean() if ab.any() else np.inf
    return (~ab, ab & ~(z > rel), ab & (z > rel)), (ABS_GATE, rel)


def stats(E, S, target=None, max_gain_db=MAX_GAIN_DB, rel_factor=0.1, abs_gate=True):
    """(L, momentary_max, g) of a signal's segment energies; g is an fp32.  WRONG on purpose: ``rel_factor`` 10^-0.8 puts the
    relative gate at -8 LU, ``abs_gate`` False drops the absolute gate."""
    z = blocks(E, S)
    one = np.float32(1.0)
    if not len(z):
        return -np.inf, -np.inf, one
    if np.isnan(z).any():
        return np.nan, np.nan, (np.float32(np.nan) if target is not None else one)
    with np.errstate(divide="ignore"):
        mm = -0.691 + 10.0 * np.log10(z.max())
    ab = z > ABS_GATE if abs_gate else np.ones(len(z), bool)
    if not ab.any():
        return -np.inf, mm, one
    keep = ab & (z > rel_factor * z[ab].mean())
    if not keep.any():
        return -np.inf, mm, one
    L = -0.691 + 10.0 * np.log10(z[keep].mean())
    if target is None:
        return L, mm, one
    g = min(10.0 ** ((float(target) - float(L)) / 20.0), 10.0 ** (float(max_gain_db) / 20.0))
    return L, mm, np.float32(g)


def measure(x, sr, target=None, max_gain_db=MAX_GAIN_DB, dtype=np.float64):
    """(E, L, momentary_max, g) of one signal"""
    S = seg_len(sr)
    E = seg_energy(weighted_squares(x, sr, dtype)[0], S)
    return (E,) + stats(E, S, target, max_gain_db)


def ungated(E, S):
    """-0.691 + 10 log10 of the mean over all blocks (what the gates are there to improve on)"""
    return -0.691 + 10.0 * np.log10(blocks(E, S).mean())


# ---- shared inputs ---------------------------------------------------------------------------------------------------------

def _noisy(rng, n, sr, amp):
    """noise + a 20 Hz sine of amplitude 0.5 + a DC step in the middle: the high-pass state is large at tile boundaries"""
    t = np.arange(n, dtype=np.float64)
    x = amp * (0.1 * rng.standard_normal(n) + 0.5 * np.sin(2.0 * np.pi * 20.0 * t / sr) + 0.3 * (t >= n // 2))
    return x.astype(np.float32)


def _groups(sr):
    """the signals of one rate in groups that stay together: tile-sized ones; a signal over four tiles and five segments, the
    loudest signal (a +-1 square) and, directly behind it, an all-zero one; then the signals around one block, each alone"""
    S = seg_len(sr)
    rng = np.random.default_rng(20261020 + sr)
    a = [_noisy(rng, n, sr, 0.5) for n in (0, 1, S - 1, S)]
    a += [_noisy(rng, 4095, sr, 0.4), _noisy(rng, 4096, sr, 0.3), _noisy(rng, 4097, sr, 0.35), _noisy(rng, 8192, sr, 0.2)]
    sq = np.where((np.arange(2 * S + 9) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    c = [_noisy(rng, max(4 * TILE, 5 * S) + S // 2 + 7, sr, 1.0), sq, np.zeros(2 * S + 5, np.float32)]
    groups = [a, c, [_noisy(rng, 4 * S - 1, sr, 0.6)], [_noisy(rng, 4 * S, sr, 0.05)], [_noisy(rng, 4 * S + 1, sr, 0.7)]]
    if sr == 8000:
        # Over RUN_TILES tiles: the kernel that carries the state from tile to tile gives a thread RUN_TILES consecutive tiles and
        # scans the threads, so only such a signal has a state that crosses from one thread to the next.  The DC step sits 300
        # samples in front of that boundary: the high-pass state is large there.
        n = RUN_TILES * TILE + 4464
        t = np.arange(n, dtype=np.float64)
        x = 0.1 * rng.standard_normal(n) + 0.5 * np.sin(2.0 * np.pi * 20.0 * t / sr) + 0.3 * (t >= RUN_TILES * TILE - 300)
        groups.append([_noisy(rng, 1234, sr, 0.5), x.astype(np.float32)])
    return groups


@functools.lru_cache(maxsize=None)
def batch(sr):
    """The ragged batches of one rate, a tuple of lists of fp32 signals, none above 100 000 samples: the groups in order, a new
    batch where the next group does not fit (the lengths the GPU tests ask for do not fit one batch from 44.1 kHz on)."""
    out = [[]]
    for g in _groups(sr):
        if out[-1] and sum(len(x) for x in out[-1] + g) > 100000:
            out.append([])
        out[-1] += g
    return tuple(out)


@functools.lru_cache(maxsize=None)
def trio(sr):
    """(b, i): batch(sr)[b][i] is the signal over four tiles, [i + 1] the loudest one and [i + 2] the all-zero one"""
    for b, xs in enumerate(batch(sr)):
        for i in range(len(xs) - 2):
            if len(xs[i + 2]) and not np.any(xs[i + 2]):
                return b, i
    raise AssertionError


@functools.lru_cache(maxsize=None)
def runs_signal():
    """(sr, b, i): batch(sr)[b][i] is the signal over RUN_TILES tiles"""
    sr = 8000
    for b, xs in enumerate(batch(sr)):
        for i, x in enumerate(xs):
            if len(x) > RUN_TILES * TILE:
                return sr, b, i
    raise AssertionError


def long_signal():
    """(sr, x): 4096 + 20 tiles and a bit at 8 kHz, 16.9 M samples — the tile-to-tile kernel takes 4096 tiles a round, so the state
    crosses from one round to the next; a DC step 300 samples in front of that boundary.  Too long for the restatement as a
    whole: ``window_energy`` restates a few segments of it."""
    sr = 8000
    n = (4096 + 20) * TILE + 1234
    rng = np.random.default_rng(9)
    x = 0.1 * rng.standard_normal(n, dtype=np.float32)
    x += np.resize((0.5 * np.sin(2.0 * np.pi * np.arange(400) / 400.0)).astype(np.float32), n)     # 20 Hz
    x[4096 * TILE - 300:] += np.float32(0.3)
    return sr, x


def window_energy(x, sr, k0, k1, warm=10, dtype=np.longdouble):
    """E[k0 .. k1) of a long signal, by the restatement started from zero ``warm`` segments ahead of k0.  The slowest pole has
    radius 0.970 at 8 kHz and 0.995 at 48 kHz: ten segments on, less than 1e-100 of the state in front of them is left."""
    S = seg_len(sr)
    a = max(0, k0 - warm)
    return seg_energy(weighted_squares(x[a * S:k1 * S], sr, dtype)[0], S)[k0 - a:]


@functools.lru_cache(maxsize=None)
def nan_signal(sr):
    """5 segments and a bit, a NaN in the middle"""
    S = seg_len(sr)
    x = _noisy(np.random.default_rng(77 + sr), 5 * S + 3, sr, 0.5)
    x[len(x) // 2] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def gating_fixtures():
    """At 8 kHz: 2 s loud, 2 s at -30 dB relative to it, 2 s at -80 dBFS, in three orders.  The loud and the quiet part are 0.25
    and 0.75 of a segment longer, so that in every order one segment is loud for a quarter of its length: the block that holds
    only that much of the loud part lies about 12 LU under the mean of the blocks above both gates, between the relative gate
    (10 LU under the mean of the absolutely gated blocks, half of which are the -30 dB ones) and one 2 LU higher."""
    sr = 8000
    rng = np.random.default_rng(5)
    n = 2 * sr + 200
    t = np.arange(n) / sr
    loud = 0.5 * np.sin(2 * np.pi * 997.0 * t) + 0.02 * rng.standard_normal(n)
    parts = [loud, loud[:2 * sr] * 10.0 ** (-30.0 / 20.0), 1e-4 * np.sin(2 * np.pi * 997.0 * np.arange(2 * sr + 600) / sr)]
    orders = ((0, 1, 2), (2, 0, 1), (1, 2, 0))
    return sr, tuple(np.concatenate([parts[k] for k in o]).astype(np.float32) for o in orders)


@functools.lru_cache(maxsize=None)
def under_gate_signal():
    """1 s at 8 kHz, -80 dBFS: every block is under the absolute gate"""
    return 8000, (1e-4 * np.sin(2 * np.pi * 997.0 * np.arange(8000) / 8000.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def quiet_tone():
    """1 s of a 997 Hz sine at 8 kHz that measures about -60 LUFS"""
    return 8000, (10.0 ** ((-60.0 + 3.01) / 20.0) * np.sin(2 * np.pi * 997.0 * np.arange(8000) / 8000.0)).astype(np.float32)


def all_inputs():
    """every (key, rate, signal) the GPU tests measure"""
    out = []
    for sr in RATES:
        out += [((sr, b, i), sr, x) for b, xs in enumerate(batch(sr)) for i, x in enumerate(xs)]
        out.append((("nan", sr), sr, nan_signal(sr)))
    out += [(("gate", k), 8000, x) for k, x in enumerate(gating_fixtures()[1])]
    out += [(("under",), 8000, under_gate_signal()[1]), (("tone",), 8000, quiet_tone()[1])]
    return out


@functools.lru_cache(maxsize=None)
def reference(key, flavour="ld"):
    """(E as float64, L, momentary_max) of an input by the restatement, cached: key = (rate, batch, signal), ("nan", rate) or
    ("gate", k); the long-double flavour ("ld") or the float64 one ("f64").  E is rounded to float64 at the end only."""
    dtype = np.longdouble if flavour == "ld" else np.float64
    if key[0] == "nan":
        sr, x = key[1], nan_signal(key[1])
    elif key[0] == "gate":
        sr, xs = gating_fixtures()
        x = xs[key[1]]
    elif key[0] == "under":
        sr, x = under_gate_signal()
    elif key[0] == "tone":
        sr, x = quiet_tone()
    else:
        sr, x = key[0], batch(key[0])[key[1]][key[2]]
    S = seg_len(sr)
    E = seg_energy(weighted_squares(x, sr, dtype)[0], S)
    L, mm, _ = stats(E, S)
    return E, float(L), float(mm)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
