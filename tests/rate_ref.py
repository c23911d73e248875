"""Output-rate conversion restated in numpy (the definition: include/goofer_hip.h, "output-rate conversion"): geometry, the
Kaiser-windowed sinc table in float64, the output index arithmetic (m, q, p), and the sum in two flavours — fp32, one rounded
multiply and one rounded add per tap in ascending j as the kernel must do it (bit for bit), and float64 on the same table."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA, MAX_PHASES = 32, 0.945, 14.0, 1024
PAIRS = [(44100, 48000), (48000, 44100), (44100, 22050), (22050, 44100), (44100, 96000), (44100, 8000), (32000, 48000)]


def geometry(sr_in, sr_out):
    """(L, M, H)"""
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    return L, M, (ZEROS * max(L, M) + L - 1) // L


def i0(x):
    """sum_k ((x/2)^k / k!)^2 in float64 (all terms positive)"""
    x = np.asarray(x, dtype=np.float64)
    t, term, total = 0.25 * x * x, np.ones_like(x), np.ones_like(x)
    for k in range(1, 120):
        term = term * (t / float(k * k))
        total = total + term
    return total


def taps64(sr_in, sr_out):
    """The table before rounding: float64 [L, 2H], each row divided by its sum."""
    L, M, H = geometry(sr_in, sr_out)
    fc = ROLLOFF * min(1.0, L / M)
    j = np.arange(-H + 1, H + 1, dtype=np.float64)[None, :]
    t = j - np.arange(L, dtype=np.float64)[:, None] / float(L)
    inside = np.abs(t) < H
    w = np.where(inside, i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / H) ** 2))) / i0(BETA), 0.0)
    z = fc * t
    zs = np.where(z == 0.0, 1.0, z)
    sinc = np.where(z == 0.0, 1.0, np.sin(np.pi * zs) / (np.pi * zs))
    h = fc * sinc * w
    return h / h.sum(axis=1, keepdims=True)


def taps32(sr_in, sr_out):
    return taps64(sr_in, sr_out).astype(np.float32)


def out_len(n, L, M):
    return (int(n) * L + M - 1) // M


def out_offsets(lengths, L, M):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    for i, n in enumerate(lengths):
        off[i + 1] = off[i] + out_len(n, L, M)
    return off


def index(n, L, M):
    """(m, q int64 [m], p int64 [m])"""
    m = out_len(n, L, M)
    km = np.arange(m, dtype=np.int64) * M
    return m, km // L, km % L


def convert(x, taps, L, M, H, dtype=np.float32, ks=None):
    """y of one signal on the table ``taps`` (fp32 [L, 2H]).  dtype float32: the definition's own arithmetic; float64: the
    same sum without rounding worth speaking of.  With float64 also returns A = sum_j |h_p[j] x[q + j]| per sample.  ``ks``:
    the output indices wanted (default: all m of them)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    if ks is None:
        m, q, p = index(n, L, M)
    else:
        km = np.asarray(ks, dtype=np.int64) * M
        m, q, p = len(km), km // L, km % L
    y = np.zeros(m, dtype=dtype)
    A = np.zeros(m, dtype=np.float64)
    xt, tt = x.astype(dtype), np.asarray(taps, dtype=np.float32).astype(dtype)
    for c in range(2 * H):                                    # j = c - H + 1, ascending
        at = q + (c - H + 1)
        ok = (at >= 0) & (at < n)
        term = tt[p[ok], c] * xt[at[ok]]                       # one rounded multiply ...
        y[ok] = y[ok] + term                                   # ... one rounded add
        if dtype == np.float64:
            A[ok] += np.abs(term)
    return (y, A) if dtype == np.float64 else y


def convert_batch(signals, taps, L, M, H, dtype=np.float32):
    return [convert(x, taps, L, M, H, dtype) for x in signals]


def bound(A, H):
    """|fp32 sum - float64 sum| per sample: one rounding per product and one per add, (2H + 1) 2^-24 sum_j |h x|."""
    return (2 * H + 1) * 2.0 ** -24 * np.asarray(A, dtype=np.float64)


def margin(L, M, H):
    """outputs to leave out at each end so that a window lies inside the signal"""
    return -(-2 * H * L // M) + 2
