"""numpy restatement of the library's normal stream (goofer_normal_fill, goofer_amd/csrc/noise.hip), word for word.

block    Philox-4x32 with 10 rounds and the standard constants (Random123's philox4x32-10)
key      batch seed ^ note id
counter  (index of the sample pair inside the note, stream tag, 0, 0x6A09E667)
normals  Box-Muller in float64: u1 = ((w0 | (w1 & 0x1FFFFF) << 32) + 1) * 2^-53, u2 = (w2 | (w3 & 0x1FFFFF) << 32) * 2^-53,
         r = sqrt(-2 ln u1); sample 2q = r cos(2 pi u2), sample 2q + 1 = r sin(2 pi u2)
"""
import math

import numpy as np

TAGS = {"f0": 0, "vol_harm": 1, "vol_breath": 2, "subharm_f0": 3, "growl": 4}
C3 = 0x6A09E667
_M0, _M1, _W0, _W1, _LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """The raw block function: ``counter`` four and ``key`` two arrays (or scalars) of 32-bit words -> four uint64 arrays of
    32-bit words.  The 32 x 32 -> 64-bit products are exact in uint64."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _LO for k in key)
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def normals(seed, note_id, tag, n):
    """The ``n`` float64 normals of stream ``tag`` of the note ``note_id`` in a batch rendered with ``seed``."""
    key = (int(seed) ^ int(note_id)) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 1) // 2, dtype=np.uint64)
    w0, w1, w2, w3 = philox4x32((q, tag, 0, C3), (key & 0xFFFFFFFF, key >> 32))
    m21 = np.uint64(0x1FFFFF)
    u1 = ((w0 | ((w1 & m21) << _S32)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (w2 | ((w3 & m21) << _S32)).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(2 * q.size, dtype=np.float64)
    z[0::2], z[1::2] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return z[:n]


def growl(seed, note_id, n, mix):
    """The 'sj' layer's f0 factor 0.5 * 2^N(0, mix^2)."""
    return 0.5 * 2.0 ** (float(mix) ** 2 * normals(seed, note_id, TAGS["growl"], n))


# ---- the statistics both the restatement and the device output are held to, each in units of its standard error ----
def stats(z):
    """{mean, var, m4, acf (largest of lags 1..16), ks (sqrt(n) * D against the normal CDF)} of draws claimed to be N(0, 1)."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    out = {"mean": abs(z.mean()) * math.sqrt(n), "var": abs((z * z).mean() - 1.0) / math.sqrt(2.0 / n),
           "m4": abs((z ** 4).mean() - 3.0) / math.sqrt(96.0 / n),
           "acf": max(abs(float(np.dot(z[:-k], z[k:])) / (n - k)) * math.sqrt(n) for k in range(1, 17))}
    s = np.sort(z)
    cdf = 0.5 * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(s / math.sqrt(2.0)))
    i = np.arange(1, n + 1, dtype=np.float64)
    out["ks"] = math.sqrt(n) * max(float(np.max(i / n - cdf)), float(np.max(cdf - (i - 1) / n)))
    return out


def correlation(a, b):
    """sample correlation of two streams in standard errors (1 / sqrt(n))"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return abs(float(np.dot(a, b)) / a.size) * math.sqrt(a.size)


# the fixed (batch seed, note id) keys the CPU and GPU statistics tests share, 2^20 draws per stream
STAT_N = 1 << 20
STAT_KEYS = [(0, 0), (0, 1), (1, 0), (2026, 7), (0xDEADBEEF, 1023), (1 << 63, 5), (12345, (1 << 32) + 3), (0xFFFFFFFFFFFFFFFF, 0),
             (987654321, (7 << 40) + 11), (42, 42), (0x5A5A5A5A, 999), (31337, (1 << 33) - 1)]
SE_MAX = 5.0           # every moment and correlation: five standard errors
KS_MAX = 2.0            # sqrt(n) * D


def assert_normal(z, what=""):
    st = stats(z)
    print(what, {k: round(v, 3) for k, v in st.items()})
    for k in ("mean", "var", "m4", "acf"):
        assert st[k] < SE_MAX, (what, k, st[k])
    assert st["ks"] < KS_MAX, (what, "ks", st["ks"])
    return st
