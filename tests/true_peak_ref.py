"""True-peak detection restated in numpy (the definition: include/goofer_hip.h, "true-peak detection"): the oversampling
factor, the R - 1 rows of the Kaiser-windowed sinc in float64, the interval maxima u, the envelope e, the meter, and the limiter
with a[i] = e[i], whose steps 2 to 8 are limit_ref's own.  Two flavours, as in limit_ref: fp32, every operation rounded as the
definition says (24 taps in ascending order, vectors over samples), which the kernels must give bit for bit; and float64, which
makes e in float64 on the fp32 table, rounds it to fp32 once and goes on as limit_ref's float64 flavour does."""
import numpy as np

import limit_ref as L
import rate_ref

ZEROS, BETA, MIN_SR, MAX_SR = 12, 8.0, 8000, 192000


def factor(sr):
    """R: 4 below 96 kHz, else 2"""
    return 4 if int(sr) < 96000 else 2


def table64(R):
    """float64 [R - 1, 2Z]: row p - 1 holds h_p[j], j = -Z+1 .. Z, divided by its sum (taken in ascending j)"""
    Z = ZEROS
    j = np.arange(-Z + 1, Z + 1, dtype=np.float64)
    i0b = rate_ref.i0(np.float64(BETA))
    rows = []
    for p in range(1, R):
        t = j - float(p) / float(R)
        u = t / float(Z)
        w = rate_ref.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / i0b
        h = np.sin(np.pi * t) / (np.pi * t) * w
        s = 0.0
        for v in h:
            s += float(v)
        rows.append(h / s)
    return np.array(rows)


def table32(R):
    return table64(R).astype(np.float32)


def _rows(taps, dtype):
    return np.asarray(taps, dtype=np.float32).reshape(-1, 2 * ZEROS).astype(dtype)


def inter(x, taps, dtype=np.float32):
    """u[i], 0 <= i < n: the greatest |reconstruction| at the R - 1 grid points between samples i and i + 1, x outside the signal
    taken as 0.  A NaN among the operands of a max is ignored (np.fmax, the kernel's fmaxf).  The float64 flavour takes x as it
    comes (a float64 signal is not rounded: property (c) is measured on the float64 output of the limiter)."""
    x = np.asarray(x, dtype=dtype)
    n, Z = len(x), ZEROS
    pad = np.concatenate([np.zeros(Z - 1, dtype), x, np.zeros(Z, dtype)])      # x[i + j] = pad[i + j + Z - 1]: column c at pad[i + c]
    u = np.zeros(n, dtype)
    for row in _rows(taps, dtype):
        acc = np.zeros(n, dtype)
        for c in range(2 * Z):                                                # j = c - Z + 1, ascending
            acc = acc + row[c] * pad[c:c + n]                                  # one rounded multiply, one rounded add
        u = np.fmax(u, np.abs(acc))
    return u


def envelope(x, taps, dtype=np.float32):
    """e[i] = max(|x[i]|, u[i], u[i - 1]), u[-1] = 0"""
    a = np.abs(np.asarray(x, dtype=dtype))
    u = inter(x, taps, dtype)
    e = np.fmax(a, u)
    e[1:] = np.fmax(e[1:], u[:-1])
    return e


def true_peak(x, taps, dtype=np.float32):
    """max_i e[i]; 0 for an empty signal"""
    e = envelope(x, taps, dtype)
    return np.fmax.reduce(e) if len(e) else dtype(0.0)


def dbtp(v):
    return 20.0 * np.log10(np.maximum(np.asarray(v, dtype=np.float64), 1e-300))


def limit_batch(signals, taps, W, c, tp_taps, dtype=np.float32):
    """[(y, g, peak_in, min_gain)] of the limiter with true-peak detection: limit_ref's steps 2 to 8 on a[i] = e[i].  limit_ref
    makes a and r from the signal it is given and rounds that signal to fp32 first, so it is given e: its g, peak_in and
    min_gain are the definition's, and y = x g is step 8 on the samples themselves."""
    xs = [np.asarray(x, dtype=np.float32) for x in signals]
    es = [envelope(x, tp_taps, dtype).astype(np.float32) for x in xs]
    out = []
    for x, (_, g, peak, gmin) in zip(xs, L.limit_batch(es, taps, W, c, dtype)):
        out.append((x.astype(dtype) * g, g, np.float32(peak), gmin))
    return out


def limit(x, taps, W, c, tp_taps, dtype=np.float32):
    return limit_batch([x], taps, W, c, tp_taps, dtype)[0]


def abs_sum(x, taps):
    """float64 per sample: the greatest sum_j |h_p[j] x[i + j]| over the phases and the two intervals sample i answers for"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    n, Z = len(x), ZEROS
    pad = np.concatenate([np.zeros(Z - 1), x, np.zeros(Z)])
    A = np.zeros(n)
    for row in np.abs(_rows(taps, np.float64)):
        acc = np.zeros(n)
        for c in range(2 * Z):
            acc += row[c] * pad[c:c + n]
        A = np.maximum(A, acc)
    B = A.copy()
    B[1:] = np.maximum(B[1:], A[:-1])
    return B


def bound(x, W, c, tp_taps):
    """|fp32 y - float64 y| per sample, derived.  limit_ref.bound covers steps 4 to 8.  In front of them the fp32 e differs
    from the float64 one by the roundings of a 24-tap sum, one per product and one per add: at most 25 * 2^-24 * sum_j |h x|
    (the max over phases and intervals does not widen it).  r = min(1, c / e) has slope at most 1 / c in e, the float64 flavour
    rounds e to fp32 once and each division rounds once: |dr| <= 25 * 2^-24 * A / c + 3 * 2^-24.  The taps w are positive with
    sum 1, so s moves by at most the greatest dr among the r it is made from, those of [i - 2W, i + 2W], and g = min(s, r) by no
    more; y = x g."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.zeros(0)
    dr = 25.0 * 2.0 ** -24 * abs_sum(x, tp_taps) / float(c) + 3.0 * 2.0 ** -24
    pad = np.concatenate([np.zeros(2 * W), dr, np.zeros(2 * W)])
    D = np.lib.stride_tricks.sliding_window_view(pad, 4 * W + 1).max(axis=1)
    return L.bound(x, W) + np.abs(x) * D


def burst(c, length=3 * ZEROS, amp=1.3):
    """A quarter-rate sine of amplitude ``amp`` c sampled at 45 degrees, ``length`` samples: every sample is +-amp c / sqrt(2)
    (0.92 c), the reconstruction between them reaches about amp c."""
    k = np.arange(length, dtype=np.float64)
    return (amp * float(c) * np.sin(0.5 * np.pi * k + 0.25 * np.pi)).astype(np.float32)


def property_inputs(n=12000, seed=20261020):
    """The five inputs of property (c): white noise low-passed at 0.9, 0.5 and 1.0 of the Nyquist rate (rFFT bins zeroed) and
    scaled to peak 3, 1.5 and 8; a 0.95 square wave at 0.0371 of the rate; a chirp of amplitude 1.4 from 0.001 to 0.49."""
    rng = np.random.default_rng(seed)
    out = []
    for cut, peak in ((0.9, 3.0), (0.5, 1.5), (1.0, 8.0)):
        X = np.fft.rfft(rng.standard_normal(n))
        X[int(np.floor(cut * (len(X) - 1))) + 1:] = 0.0
        v = np.fft.irfft(X, n)
        out.append((v * (peak / np.abs(v).max())).astype(np.float32))
    k = np.arange(n, dtype=np.float64)
    out.append((0.95 * np.where(np.sin(2.0 * np.pi * 0.0371 * k) >= 0.0, 1.0, -1.0)).astype(np.float32))
    f = 0.001 + (0.49 - 0.001) * k / float(n - 1)
    out.append((1.4 * np.sin(2.0 * np.pi * np.cumsum(f))).astype(np.float32))
    return out


PROPERTY_LOOKS = (7, 48, 240)
PROPERTY_CEILINGS = (np.float32(0.891), np.float32(0.5), np.float32(32767.0 / 32768.0))
PROPERTY_FREQS = (0.25, 0.3, 0.4, 0.45)


def sine_readings(R, n=2048):
    """Property (a): {f: (least, greatest)} of the meter's reading in dB on unit sines at f of the sample rate over the 13 start
    phases pi / 4 + 2 pi k / 13 (k = 0 at a quarter of the rate is the sine whose sample peak is -3.01 dBFS), away from the
    signal's ends, float64 sums on the fp32 table."""
    t32, k, out = table32(R), np.arange(n, dtype=np.float64), {}
    for f in PROPERTY_FREQS:
        db = []
        for ph in range(13):
            x = np.sin(2.0 * np.pi * f * k + 0.25 * np.pi + 2.0 * np.pi * ph / 13.0)
            db.append(float(dbtp(envelope(x, t32, np.float64)[4 * ZEROS:-4 * ZEROS].max())))
        out[f] = (min(db), max(db))
    return out
