"""The equaliser's definition of include/goofer_hip.h restated in numpy only: the cookbook coefficients and the cascade, sample by
sample.  Three flavours of the arithmetic, all on the float64 coefficients, which are part of the definition: ``np.longdouble``
(the truth), plain sequential float64, and ``tiled``, a float64 model of the kernels' own scheme — zero-state runs of 16 carried
by each section's 2 x 2 powers inside a tile of 4096, zero-state tiles carried by the coupled matrices, all from the planner's
tables, the state travelling as (u[i-1], u[i-1] - u[i-2]) per section as it does there.  ``tiled`` is what the accepted ranges
were measured with (``corners``; tests/test_eq_ref.py runs them).  Also here: the inputs the GPU tests and the host tests share, cached per process."""
import functools
import math

import numpy as np

MIN_SR, MAX_SR = 8000, 192000
MAX_BANDS = 8
F_MIN_DIV, F_MAX_REL = 600.0, 0.45
Q_MIN, Q_MAX = 0.1, 8.0
SHELF_Q_MAX = 2.0                   # lowshelf, highshelf: q up to this
MAX_GAIN_DB = 9.0
TILE, SPT, LEVELS = 4096, 16, 8
RUN_TILES = 16                      # tiles a thread of the tile-to-tile kernel walks
ROUND_TILES = 4096                  # tiles a round of that kernel takes
TOL = 2.0 ** -26                    # |y - truth| <= 2^-24 |truth| + TOL max |truth|, per signal
CORNER_RATES = (8000, 44100, 48000, 96000, 192000)
RATES = (8000, 48000)               # the GPU tests' batches
Q_DEFAULT = math.sqrt(0.5)
KINDS = ("highpass", "lowpass", "lowshelf", "highshelf", "peak", "notch")
GAINED = ("lowshelf", "highshelf", "peak")
SHELVES = ("lowshelf", "highshelf")


def coefficients(kind, f0, gain_db, q, sr):
    """float64 [5]: b0 b1 b2 a1 a2 of one band, the header's formulas in the header's order of operations"""
    w0 = 2.0 * math.pi * f0 / float(sr)
    cs, sn = math.cos(w0), math.sin(w0)
    alpha = sn / (2.0 * q)
    A = math.pow(10.0, gain_db / 40.0)
    r = 2.0 * math.sqrt(A) * alpha
    if kind == "highpass":
        b0, b1, b2, a0, a1, a2 = (1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha
    elif kind == "lowpass":
        b0, b1, b2, a0, a1, a2 = (1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha
    elif kind == "notch":
        b0, b1, b2, a0, a1, a2 = 1.0, -2.0 * cs, 1.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha
    elif kind == "peak":
        b0, b1, b2, a0, a1, a2 = 1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A, 1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A
    elif kind == "lowshelf":
        b0, b1, b2 = A * ((A + 1.0) - (A - 1.0) * cs + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - r)
        a0, a1, a2 = (A + 1.0) + (A - 1.0) * cs + r, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - r
    elif kind == "highshelf":
        b0, b1, b2 = A * ((A + 1.0) + (A - 1.0) * cs + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - r)
        a0, a1, a2 = (A + 1.0) - (A - 1.0) * cs + r, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - r
    else:
        raise ValueError(kind)
    return np.array([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0], dtype=np.float64)


def kept(bands):
    """the bands the planner keeps: a shelf or a peak with 0 dB is the identity and is dropped"""
    return [b for b in bands if not (b[0] in GAINED and b[2] == 0.0)]


def cascade_coefficients(bands, sr):
    """float64 [K, 5] of the kept bands, ``bands`` as (kind, f0, gain_db, q) tuples"""
    return np.array([coefficients(*b, sr) for b in kept(bands)], dtype=np.float64).reshape(-1, 5)


def transition(coef, conv=float):
    """T, the 2K x 2K transition matrix of the state (u_1[i-1], u_1[i-2], .., u_K[i-1], u_K[i-2]) for x = 0, as a list of
    rows of ``conv`` numbers (float; mpmath.mpf for exact powers)"""
    K = len(coef)
    D = 2 * K
    zero = conv(0.0)
    T = [[zero] * D for _ in range(D)]
    for s in range(K):
        b0, b1, b2, a1, a2 = (conv(float(v)) for v in coef[s])
        if s:
            for j in range(2 * s):
                T[2 * s][j] = b0 * T[2 * s - 2][j]
            T[2 * s][2 * s - 2] = T[2 * s][2 * s - 2] + b1
            T[2 * s][2 * s - 1] = T[2 * s][2 * s - 1] + b2
        T[2 * s][2 * s], T[2 * s][2 * s + 1] = -a1, -a2
        T[2 * s + 1][2 * s] = conv(1.0)
    return T


def to_diff(M):
    """C M C for a 2K x 2K matrix (nested lists of any number type), C block diagonal with the blocks [[1, 0], [1, -1]]: M in the
    coordinates (u[i-1], u[i-1] - u[i-2]) per section, in which the planner stores its powers and the kernels carry the state"""
    D = len(M)
    r = [[(M[i - 1][j] - M[i][j]) if i & 1 else M[i][j] for j in range(D)] for i in range(D)]
    return [[(-r[i][j]) if j & 1 else (r[i][j] + r[i][j + 1]) for j in range(D)] for i in range(D)]


def pole_radius(coef):
    """the largest pole radius of the cascade"""
    return max((float(np.abs(np.roots([1.0, c[3], c[4]])).max()) for c in coef), default=0.0)


def cascade(x, coef, dtype=np.longdouble, taps=None):
    """u_K of one signal, ``dtype`` [n]: the recurrence as written, sequentially from zero history.  With ``taps``, a sequence
    of section counts: {k: u_k} instead (a cascade's first k sections are the cascade of those k bands)."""
    conv = float if dtype is np.float64 else dtype            # (Python floats are IEEE doubles, and the loop is faster on them)
    u = [conv(v) for v in np.asarray(x, dtype=np.float32).astype(np.float64)]
    zero = conv(0.0)
    out = {0: np.array(u, dtype=dtype)} if taps and 0 in taps else {}
    for k, c in enumerate(coef):
        b0, b1, b2, a1, a2 = (conv(v) for v in c)
        h1 = h2 = s1 = s2 = zero
        for i, xv in enumerate(u):
            y = b0 * xv + b1 * h1 + b2 * h2 - a1 * s1 - a2 * s2
            h2, h1, s2, s1 = h1, xv, s1, y
            u[i] = y
        if taps and k + 1 in taps:
            out[k + 1] = np.array(u, dtype=dtype)
    return out if taps else np.array(u, dtype=dtype)


def cascade_many(x, coefs, dtype=np.longdouble):
    """u_K of ONE signal through MANY cascades at once, ``dtype`` [C, n]: ``coefs`` [C, K, 5] (pad a shorter cascade with the
    exact identity 1 0 0 0 0).  The same recurrence as ``cascade``, vectorised over the cascades, for the corner run."""
    coefs = np.asarray(coefs, dtype=np.float64).astype(dtype)
    C, K, _ = coefs.shape
    xs = np.asarray(x, dtype=np.float32).astype(dtype)
    out = np.zeros((len(xs), C), dtype=dtype)
    h = np.zeros((K, 2, C), dtype=dtype)                      # per section: its input's two last samples
    s = np.zeros((K, 2, C), dtype=dtype)                      # ... and its output's
    b0, b1, b2, a1, a2 = (np.ascontiguousarray(coefs[:, :, j].T) for j in range(5))     # [K, C]
    for i in range(len(xs)):
        v = np.full(C, xs[i], dtype=dtype)
        for k in range(K):
            y = b0[k] * v + b1[k] * h[k, 0] + b2[k] * h[k, 1] - a1[k] * s[k, 0] - a2[k] * s[k, 1]
            h[k, 1], h[k, 0], s[k, 1], s[k, 0] = h[k, 0], v, s[k, 0], y
            v = y
        out[i] = v
    return out.T


def _tile_pass(X, flat, coef, sec, starts):
    """The kernels' pass over every tile at once, float64: X [nt, 256, 16], the signal's samples cut as the kernel cuts them;
    every section a zero-state run per thread, the scan with the section's powers ``sec`` [K, 8, 2, 2], the run again from its
    true state.  ``starts`` [nt, 2K] or None for zero.  Returns (u_K as [nt, 256, 16], the tiles' end states [nt, 2K])."""
    nt, R, _ = X.shape
    K = len(coef)
    u = X.copy()
    at = np.arange(nt * R).reshape(nt, R) * SPT
    h1 = np.where(at >= 1, flat[np.maximum(at - 1, 0)], 0.0)
    h2 = np.where(at >= 2, flat[np.maximum(at - 2, 0)], 0.0)
    ends = np.zeros((nt, 2 * K))

    def run(st1, st2, keep):
        a, b, s1, s2 = h1, h2, st1, st2
        for e in range(SPT):
            xv = u[:, :, e].copy()
            y = (((b0 * xv + b1 * a) + b2 * b) - a1 * s1) - a2 * s2
            b, a, s2, s1 = a, xv, s1, y
            if keep:
                u[:, :, e] = y
        return s1, s2
    for k in range(K):
        b0, b1, b2, a1, a2 = (float(v) for v in coef[k])
        P = sec[k]
        zero = np.zeros((nt, R))
        v1, v2 = run(zero, zero, False)
        v1, v2 = v1.copy(), v1 - v2                             # carried as (u[i-1], u[i-1] - u[i-2]), like starts and ends
        if starts is not None:
            t1, t2 = starts[:, 2 * k], starts[:, 2 * k + 1]
            v1[:, 0], v2[:, 0] = (P[0, 0, 0] * t1 + P[0, 0, 1] * t2) + v1[:, 0], (P[0, 1, 0] * t1 + P[0, 1, 1] * t2) + v2[:, 0]
        for l in range(LEVELS):
            off = 1 << l
            o1, o2 = v1[:, :-off].copy(), v2[:, :-off].copy()
            v1[:, off:] = (P[l, 0, 0] * o1 + P[l, 0, 1] * o2) + v1[:, off:]
            v2[:, off:] = (P[l, 1, 0] * o1 + P[l, 1, 1] * o2) + v2[:, off:]
        st1, st2 = np.zeros((nt, R)), np.zeros((nt, R))
        st1[:, 1:], st2[:, 1:] = v1[:, :-1], v2[:, :-1]
        if starts is not None:
            st1[:, 0], st2[:, 0] = starts[:, 2 * k], starts[:, 2 * k + 1]
        ends[:, 2 * k], ends[:, 2 * k + 1] = v1[:, -1], v2[:, -1]
        st2 = st1 - st2                                         # back to u[i-2]
        run(st1, st2, True)
        h1, h2 = st1, st2
    return u, ends


def tiled(x, coef, sec, car):
    """u_K of one signal, float64 [n], by the kernels' scheme with the planner's tables: ``coef`` [K, 5], ``sec`` [K, 8, 2, 2]
    (EqPlan.section_mats), ``car`` [9, 2K, 2K] (EqPlan.carry_mats; the tiles are carried one by one with car[0], each row
    summed in ascending column, as the kernel walks up to 16 of them; beyond that the kernel scans runs of 16, in another order)."""
    n, K = len(x), len(coef)
    if n == 0 or K == 0:
        return np.asarray(x, dtype=np.float32).astype(np.float64)
    nt = -(-n // TILE)
    flat = np.zeros(nt * TILE)
    flat[:n] = np.asarray(x, dtype=np.float32)
    X = flat.reshape(nt, TILE // SPT, SPT)
    _, ends = _tile_pass(X, flat, coef, sec, None)
    starts = np.zeros((nt, 2 * K))
    M = car[0]
    for t in range(nt - 1):
        for i in range(2 * K):
            a = M[i, 0] * starts[t, 0]
            for j in range(1, (i | 1) + 1):
                a = a + M[i, j] * starts[t, j]
            starts[t + 1, i] = a + ends[t, i]
    u, _ = _tile_pass(X, flat, coef, sec, starts)
    return u.reshape(-1)[:n]


def error(got, truth):
    """max_i (|got - truth| - 2^-24 |truth|) / max |truth|, what TOL bounds (<= 0: within the fp32 rounding alone); inf where
    got is not finite and truth is"""
    truth = np.asarray(truth, dtype=np.longdouble)
    top = float(np.abs(truth).max()) if len(truth) else 0.0
    if top == 0.0:
        return 0.0 if not np.any(np.asarray(got) != 0) else math.inf
    d = np.abs(np.asarray(got).astype(np.longdouble) - truth) - np.longdouble(2.0 ** -24) * np.abs(truth)
    d = np.where(np.isfinite(np.asarray(got, dtype=np.float64)), d, np.inf)
    return float(d.max()) / top


def carry_error(got, truth):
    """max_i |got - truth| / max |truth| of a float64 flavour: what the corner run measures"""
    truth = np.asarray(truth, dtype=np.longdouble)
    return float(np.abs(np.asarray(got).astype(np.longdouble) - truth).max() / np.abs(truth).max())


# ---- shared inputs ---------------------------------------------------------------------------------------------------------

def noisy(rng, n, sr, step_at=None, amp=1.0):
    """noise of 0.3 rms + a 40 Hz sine of amplitude 0.5 + a DC step of 0.3 at ``step_at`` (default: the middle): wide-band content
    and a large low-frequency state at tile boundaries"""
    t = np.arange(n, dtype=np.float64)
    at = n // 2 if step_at is None else step_at
    x = amp * (0.3 * rng.standard_normal(n) + 0.5 * np.sin(2.0 * np.pi * 40.0 * t / sr) + 0.3 * (t >= at))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def hazard_input(sr):
    """16 tiles of the input above, the step 300 samples in front of the eighth tile boundary: the corner run's signal"""
    return noisy(np.random.default_rng(20261021 + sr), 16 * TILE, sr, 8 * TILE - 300)


def corners(sr, f_min_div=F_MIN_DIV, q_max=Q_MAX, shelf_q_max=SHELF_Q_MAX, gain=MAX_GAIN_DB):
    """The corners of the accepted range at one rate, a list of band lists, every band at the highest q of its kind and the
    greatest gain.  At the lowest f0: one band and eight equal bands, every kind, boost and cut; chains of eight that cut and
    then boost, the boost by peaks and by either shelf (a later boost amplifies the earlier sections' carry noise); chains
    that boost and then cut; inverse pairs, which are the identity in exact arithmetic (four shelves or peaks one way, then
    four the other); unequal splits, 2 + 6, 6 + 2, 1 + 7 and 3 + 5.  Then six seeded random chains of eight with f0 between the lowest and
    1.5 times it."""
    f_min = sr / f_min_div
    if f_min * f_min_div < sr:                                # the smallest float64 the planner accepts
        f_min = math.nextafter(f_min, math.inf)

    def band(kind, sign=0, f0=f_min):
        return (kind, f0, sign * gain if kind in GAINED else 0.0, min(q_max, shelf_q_max) if kind in SHELVES else q_max)
    out = []
    for kind in KINDS:
        for sign in ((1, -1) if kind in GAINED else (0,)):
            out += [[band(kind, sign)], [band(kind, sign)] * MAX_BANDS]
    cuts = [("notch", 0), ("peak", -1), ("lowshelf", -1), ("highshelf", -1), ("highpass", 0), ("lowpass", 0)]
    for boost in ("peak", "lowshelf", "highshelf"):
        for kind, sign in cuts + [("lowshelf", 1)]:
            out.append([band(kind, sign)] * 4 + [band(boost, 1)] * 4)           # cut (or a low shelf's boost), then boost
    for kind in GAINED:
        out.append([band(kind, 1)] * 4 + [band(kind, -1)] * 4)                  # boost, then the inverse cut
    out.append([band("peak", 1)] * 4 + [band("notch")] * 4)
    out.append([band("lowshelf", 1)] * 4 + [band("highpass")] * 4)
    for a, b in ((2, 6), (6, 2), (1, 7), (3, 5)):
        out += [[band("notch")] * a + [band("peak", 1)] * b, [band("lowshelf", -1)] * a + [band("peak", 1)] * b,
                [band("highpass")] * a + [band("lowshelf", 1)] * b]
    out.append([band("notch")] * 2 + [band("peak", 1)] * 2)
    rng = np.random.default_rng(600)
    for _ in range(6):
        kinds = [KINDS[k] for k in rng.integers(len(KINDS), size=MAX_BANDS)]
        out.append([band(k, 1 if rng.random() < 0.5 else -1, f_min * (1.0 + 0.5 * rng.random())) for k in kinds])
    return out


def lengths():
    """the GPU batches' lengths: around a run of 16, around a tile, two tiles and one, more tiles than a thread of the carry walks"""
    return (0, 1, 2, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 16 * TILE + 100, 0)


@functools.lru_cache(maxsize=None)
def batch(sr):
    """the ragged batch of one rate, a tuple of fp32 signals; the DC step of a signal over a tile sits 300 samples in front of its
    last tile boundary"""
    rng = np.random.default_rng(77 + sr)
    out = []
    for n in lengths():
        last = (n - 1) // TILE * TILE if n > TILE else 0
        out.append(noisy(rng, n, sr, last - 300 if last else None, amp=0.8))
    return tuple(out)


def chain(sr, K):
    """the band lists of the GPU tests: one band, a real chain of three, a vocal chain of eight, written for 48 kHz (high-pass at
    96 Hz, a presence bell, an air shelf; a low shelf, two cuts, a low-pass, a resonant high-pass at 120 Hz); the frequencies move
    with the rate, so that every rate holds them"""
    r = sr / 48000.0
    full = [("highpass", 96.0 * r, 0.0, Q_DEFAULT), ("peak", 3000.0 * r, 3.0, 1.0), ("highshelf", 10000.0 * r, 4.0, Q_DEFAULT),
            ("lowshelf", 200.0 * r, 3.0, Q_DEFAULT), ("peak", 600.0 * r, -4.0, 1.5), ("peak", 7000.0 * r, -6.0, 4.0),
            ("lowpass", 18000.0 * r, 0.0, Q_DEFAULT), ("highpass", 120.0 * r, 0.0, 2.0)]
    return full[:K]


CHAINS = (1, 3, 8)


@functools.lru_cache(maxsize=None)
def _references(sr):
    coef = cascade_coefficients(chain(sr, MAX_BANDS), sr)
    return tuple(cascade(x, coef, taps=range(1, MAX_BANDS + 1)) for x in batch(sr))


def reference(sr, K):
    """the long-double restatement of every signal of batch(sr) through chain(sr, K), 1 <= K <= MAX_BANDS: a tuple of longdouble
    arrays; one walk through the eight bands per signal, cached, gives every prefix"""
    return tuple(r[K] for r in _references(sr))


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
