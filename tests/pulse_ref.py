"""The main pulse train of csrc/pulse.hip (k_pulse_onsets_par / k_pulse_onsets_scan, k_onset_finish, k_pulse_tiles,
k_pulse_place over the plan's k_pulse_peak / k_pulse_shape_table) restated in numpy with its stages exposed, a float64 truth
beside it, the per-sample bound that holds the device to the truth, and the notes that reach each path of the chain.  Host only;
tests/test_pulse_ref.py pins it, tests/test_gpu_pulse_train.py judges the device with it.

train(f0, sr, Ra, Rg, Rk, exact)
    exact=False is oracle.goofer_ref.pulse_train (GOOFER.py:473-554), stage by stage:
      phase    p_i = fl64(p_{i-1} + f0[i] / sr), strictly in order (np.cumsum adds in order), p_{-1} = 0
      onsets   after sample i the reference has recorded R_i = max(R_{i-1}, floor(p_i)) onsets (its `while phase >= next_k`,
               next_k = R + 1): R_i - R_{i-1} onsets at sample i
      last     last_valid_f0 = the most recent f0 > 1e-6 at or before the onset sample, 160 Hz before any
      T, T0    T = 1 / max(last, 1e-6), T0 = clip(round_half_even(sr T), 3, 8192)
      cache    five slots keyed by T0, slot 0 overwritten when full: an onset uses the shape computed for the period of that T0's
               first (or re-cached) use, Tshape
      shape    raw_j = LF(j; T0, Tshape) in float64, stored as fp32; m = the fp32 maximum of |raw|; v_j = fp32(raw_j / m), the
               division in float64
      sum      pulse[i : min(i + T0, n)] += v, fp32, onsets in ascending order
    exact=True keeps every decision and data item (onsets, T0, Tshape, the cache's choices, the cut at the note's end) and does
    every value operation in float64: v_j = raw_j / max |raw|, summed in float64.
    Both return, per sample, C = the number of pulses covering it and A = sum |v_k| over them (float64 values), and TAB (below).

table_row(T0, sr, Ra, Rg, Rk)   the device's documented arithmetic (k_pulse_peak, k_pulse_shape_table): the shape at the NOMINAL
    period T0 / sr, fp32 raw, divided in float64 by the fp32 peak, rounded to fp32.

THE BOUND, per sample:   |x - truth| <= c 2^-24 A + 2^-149,   c = (C + 2) (1 + 2^-20) + t

  A device sample is the fp32 sum, in ascending onset order, of table values w_k = fp32(fp32(raw'_k) / fp32(m')), raw' and m'
  taken at the nominal period.  Against the truth's v_k = raw_k / m, to first order and relative to |v_k|:
    1  the fp32 rounding of the raw sample: 2^-24 (the device's sin / exp / cos differ from numpy's by ulps of float64, which
       can only decide an fp32 tie: the half ulp holds either way);
    1  the fp32 rounding of the peak: the maximum of the rounded samples is the rounded maximum, 2^-24;
    1  the division: exact in float64 up to 2^-53, then one fp32 rounding, 2^-24;
    C - 1  fp32 additions: each rounds a partial sum that is at most sum |w_k| in size, so (C - 1) 2^-24 sum |w_k|;
    (C + 2) 2^-20 for every second-order term: they are under (C + 2)^2 2^-48, i.e. within this slack while C <= 14 (asserted).
  The 2^-149 covers a result below the normal range.  A sample no pulse covers has A = 0: the device must write an exact 0.

  t, the tabulation term (TAB = t 2^-24 A, returned per sample).  The LF shape depends on the period only through ratios,
  ti / Tp = j / (Ra T0) and tau = (j / T0 - Ra) / (Rk (1 - Ra)), except for the two 1e-12 guards of lf_raw:
      rise   sin^2(x),  x = pi ti / (2 Tp + 1e-12) = x0 / (1 + 1e-12 / (2 Ra T))
      fall   exp(-Rg tau) cos(pi tau / 2),  tau = tau0 / (1 + 1e-12 / (Rk (1 - Ra) T))
  Between the period of the shape the truth uses (f = 1 / Tshape) and the nominal one (f' = sr / T0) the argument moves by the
  relative amount eta_r = 1e-12 |f - f'| / (2 Ra) on the rise and eta_f = 1e-12 |f - f'| / (Rk (1 - Ra)) on the fall.  So
      rise   |d ln sin^2 x| = 2 x cot(x) eta_r <= 2 eta_r                               (x cot x <= 1 on [0, pi / 2])
      fall   |d ln v| = tau eta_f (Rg + (pi / 2) tan(pi tau / 2))
  (times 1.01 for the curvature; where eta_f tau / (1 - tau) > 1e-3 the first order says nothing and the term is infinite: a
  sample whose tau is within 1e-5 of 1, none in the cases).  The peak moves by at most max_j (rel_j |raw_j|) / m relative.  A
  sample's t is (rel_j + rel_peak) summed over its covering pulses, weighted by |v_k|.  The fall's term grows like 1 / (1 - tau)
  towards the shape's zero, where v itself vanishes: in units of the PEAK it stays under eta_f (Rg + pi / 2).  Largest in the
  cases (tests/test_pulse_ref.py prints them per batch): t = 3.41 in (f), T0 = 5 at 8 020 Hz (|f - f'| = 800 Hz, eta_f = 1.0e-9)
  on the pulse's last live sample, tau = 0.995; t = 2.92 at 47 kHz and 96 kHz (T0 clamped to 3, f' = 32 kHz, eta_f = 1.9e-8);
  0.97 at 21 kHz and 44.1 kHz; 0.77 in (e); under 0.25 elsewhere, 0 wherever f0 = fp32(sr / T0).
  The branch tests (ti < Tp, ti < Tc) are ratio comparisons as well; a rounding decides them only where j / T0 equals Ra or
  Ra + Rk (1 - Ra) exactly.  At Tp both branches give 1.  At Tc the fall's last value is e^-Rg cos(pi / 2) = 6e-17 e^-Rg against
  the 0 behind it, which this bound does not cover: no T0 of the cases is such a multiple (250 for the default model).

  c is not tuned on the device: tests/test_pulse_ref.py asserts that the reference arithmetic (exact=False) and table_row
  placed by the reference's onsets stay inside the bound on every case.

THE TILE RULE of k_pulse_tiles / k_pulse_place, restated (tile_lists): tiles of 2048 samples from the first sample of the batch;
a tile inside one note has the covering list first .. last, first = the first onset whose running end_max = max(i + T0) exceeds
the tile's first sample, last = the last onset starting at or before the tile's last sample.  Up to 512 onsets are staged in LDS;
a longer list, or a tile across a note boundary, takes the per-sample search.

cases(sr): the batches, each the smallest that reaches its path (see the table in cases' docstring).
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
PI = 3.141592653589793
DEFAULT = (0.02, 1.7, 0.8)
T0_MIN, T0_MAX = 3, 8192
TILE, MAXON = 2048, 512
A_T0 = (3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2410, 4095, 4096, 4097, 8191, 8192)
G_T0 = (3, 2049, 8192)
F_LENGTHS = (1, 2, 7, 8, 9, 15, 2047, 2048, 2049)
F_HEAD = 16
D_F0 = (11000.0, 11025.0, 13230.0, 21000.0)


# ---------------------------------------------------------------------------------------------
# the shape
# ---------------------------------------------------------------------------------------------
def _lf(T0, T, Ra, Rg, Rk):
    """raw float64 samples of a T0-sample pulse of period T (GOOFER.py:508-519), the rise / fall masks"""
    j = np.arange(T0, dtype=F64)
    ti = (j * T) / T0
    Tp = Ra * T
    Tc = Tp + Rk * (T - Tp)
    v = np.zeros(T0)
    a = ti < Tp
    b = (~a) & (ti < Tc)
    s = np.sin(PI * ti[a] / (2.0 * Tp + 1e-12))
    v[a] = s * s
    tau = (ti[b] - Tp) / (Tc - Tp + 1e-12)
    v[b] = np.exp(-Rg * tau) * np.cos(PI * tau / 2.0)
    return v, a, b


def shape32(T0, T, Ra, Rg, Rk):
    """the reference's cached shape: fp32 raw, divided in float64 by its fp32 peak, rounded to fp32; and the peak"""
    buf = _lf(T0, T, Ra, Rg, Rk)[0].astype(F32)
    m = F32(np.max(np.abs(buf))) if T0 else F32(0)
    if m > 0:
        buf = (buf.astype(F64) / F64(m)).astype(F32)
    return buf, m


def shape64(T0, T, Ra, Rg, Rk):
    v = _lf(T0, T, Ra, Rg, Rk)[0]
    m = np.max(np.abs(v)) if T0 else 0.0
    return v / m if m > 0 else v


def table_peak(T0, sr, Ra=DEFAULT[0], Rg=DEFAULT[1], Rk=DEFAULT[2]):
    return shape32(T0, F64(T0) / F64(sr), Ra, Rg, Rk)[1]


def table_row(T0, sr, Ra=DEFAULT[0], Rg=DEFAULT[1], Rk=DEFAULT[2]):
    return shape32(T0, F64(T0) / F64(sr), Ra, Rg, Rk)[0]


def tab_rel(T0, T, sr, Ra, Rg, Rk):
    """per sample of the shape: the first-order bound of |v'_j / v_j - 1| between the period T and the nominal T0 / sr (the
    module docstring's t, the sample's own part plus the peak's)"""
    v, a, b = _lf(T0, T, Ra, Rg, Rk)
    df = abs(1.0 / T - F64(sr) / T0)
    eta_r = 1e-12 * df / (2.0 * Ra)
    eta_f = 1e-12 * df / (Rk * (1.0 - Ra))
    rel = np.zeros(T0)
    rel[a] = 2.0 * eta_r
    tau = (np.arange(T0, dtype=F64)[b] / T0 - Ra) / (Rk * (1.0 - Ra))
    tau = np.clip(tau, 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = tau * eta_f * (Rg + (PI / 2.0) * np.tan(PI * tau / 2.0))
        r = np.where(eta_f * tau > 1e-3 * (1.0 - tau), np.inf, r)
    rel[b] = np.where(eta_f > 0, r, 0.0)
    rel *= 1.01
    m = np.max(np.abs(v))
    nz = v != 0
    pk = float(np.max(rel[nz] * np.abs(v[nz]))) / m if nz.any() and m > 0 else 0.0
    return np.where(nz, rel + pk, 0.0)


# ---------------------------------------------------------------------------------------------
# onsets
# ---------------------------------------------------------------------------------------------
def onsets(f0, sr, rounding="even", clamp=(T0_MIN, T0_MAX)):
    """onset samples, their periods T, lengths T0 and sr * T (the value that was rounded); rounding / clamp other than the
    defaults are the planted faults of tests/test_pulse_ref.py"""
    f0 = np.ascontiguousarray(f0, dtype=F32)
    n = f0.size
    sr = F64(sr)
    phase = np.cumsum(f0.astype(F64) / sr)
    assert np.all(np.isfinite(phase))
    R = np.maximum.accumulate(np.maximum(np.floor(phase), 0.0)).astype(np.int64)
    oi = np.repeat(np.arange(n, dtype=np.int64), np.diff(R, prepend=0))
    valid = f0 > F32(1e-6)
    at = np.maximum.accumulate(np.where(valid, np.arange(n), -1))
    last = np.where(at >= 0, f0[np.maximum(at, 0)].astype(F64), 160.0)[oi]
    T = 1.0 / np.maximum(last, 1e-6)
    x = sr * T
    r = {"even": np.rint, "up": lambda y: np.floor(y + 0.5), "trunc": np.trunc}[rounding](x)
    T0 = np.clip(r, clamp[0], clamp[1]).astype(np.int64)
    return oi, T, T0, x


def _both(f0, sr, Ra, Rg, Rk):
    f0 = np.ascontiguousarray(f0, dtype=F32)
    n = f0.size
    oi, T, T0, x = onsets(f0, sr)
    p32, p64 = np.zeros(n, dtype=F32), np.zeros(n, dtype=F64)
    C, A, TAB = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    keys, bank = [], []
    Tshape = np.zeros(oi.size)
    for k in range(oi.size):
        t0, i = int(T0[k]), int(oi[k])
        if t0 in keys:
            c = keys.index(t0)
        else:
            s64 = shape64(t0, T[k], Ra, Rg, Rk)
            entry = (shape32(t0, T[k], Ra, Rg, Rk)[0], s64, np.abs(s64) * tab_rel(t0, T[k], sr, Ra, Rg, Rk), T[k])
            if len(keys) < 5:
                keys.append(t0)
                bank.append(entry)
                c = len(keys) - 1
            else:
                keys[0], bank[0], c = t0, entry, 0
        s32, s64, tab, Tshape[k] = bank[c]
        end = min(i + t0, n)
        p32[i:end] += s32[:end - i]
        p64[i:end] += s64[:end - i]
        C[i:end] += 1
        A[i:end] += np.abs(s64[:end - i])
        TAB[i:end] += tab[:end - i]
    end_max = np.maximum.accumulate(oi + T0) if oi.size else np.zeros(0, dtype=np.int64)
    return {"n": n, "oi": oi, "ot": T0, "T": T, "Tshape": Tshape, "x": x, "end_max": end_max, "pulse32": p32, "pulse64": p64,
            "C": C, "A": A, "TAB": TAB}


def train(f0, sr, Ra=DEFAULT[0], Rg=DEFAULT[1], Rk=DEFAULT[2], exact=False):
    r = dict(_both(f0, sr, Ra, Rg, Rk))
    r["pulse"] = r["pulse64"] if exact else r["pulse32"]
    return r


def c_of(t):
    """the bound's c per sample (module docstring)"""
    assert t["C"].max(initial=0) <= 14
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(t["A"] > 0, t["TAB"] / (2.0 ** -24 * np.where(t["A"] > 0, t["A"], 1.0)), 0.0)
    return (t["C"] + 2.0) * (1.0 + 2.0 ** -20) + tt


def bound(t):
    return c_of(t) * 2.0 ** -24 * t["A"] + 2.0 ** -149


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def judge(x, truths):
    """The rule of the GPU test for one batch: x = its fp32 pulse, truths = train(exact=True) of its notes.  Returns the worst
    error / bound, the first sample outside the bound (note, sample) or None, whether every uncovered sample is an exact +0.0,
    whether everything is finite."""
    worst, first, zeros, finite, o = 0.0, None, True, True, 0
    for k, t in enumerate(truths):
        n = t["n"]
        seg = np.asarray(x[o:o + n])
        o += n
        finite = finite and bool(np.all(np.isfinite(seg)))
        with np.errstate(invalid="ignore"):
            ratio = np.abs(seg.astype(F64) - t["pulse64"]) / bound(t)
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        if n and ratio.max() > 1.0 and first is None:
            first = (k, int(np.argmax(ratio > 1.0)))
        worst = max(worst, float(ratio.max(initial=0.0)))
        zeros = zeros and not bits(seg[t["C"] == 0]).any()
    return {"worst": worst, "first": first, "zeros": zeros, "finite": finite, "ok": first is None and zeros and finite}


# ---------------------------------------------------------------------------------------------
# the tile rule, and the device as documented (with the planted faults)
# ---------------------------------------------------------------------------------------------
def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def tile_lists(lens, trains):
    """per tile of the batch: None where it crosses a note boundary, else (note, first, last) of its covering list (last <
    first: empty)"""
    off = offsets(lens)
    N = int(off[-1])
    res = []
    for g0 in range(0, N, TILE):
        gl = min(g0 + TILE, N) - 1
        a, b = int(np.searchsorted(off, g0, "right")) - 1, int(np.searchsorted(off, gl, "right")) - 1
        if a != b:
            res.append(None)
            continue
        t = trains[a]
        j_lo, j_hi = g0 - int(off[a]), gl - int(off[a])
        res.append((a, int(np.searchsorted(t["end_max"], j_lo, "right")), int(np.searchsorted(t["oi"], j_hi, "right")) - 1))
    return res


def list_sizes(lens, trains):
    return [None if t is None else t[2] - t[1] + 1 for t in tile_lists(lens, trains)]


FAULTS = ("half_up", "trunc", "clamp_2048", "clamp_2", "row_offset", "row_short", "latest_three", "first_512", "own_end",
          "no_cut")


def device_model(f0s, sr, model=DEFAULT, fault=None):
    """The device as its comments document it, for one batch: table_row(T0) placed at the restatement's onsets, cut at the note's
    end, summed in fp32 in ascending order.  fault: one of FAULTS."""
    lens = [len(f) for f in f0s]
    off = offsets(lens)
    N = int(off[-1])
    out = np.zeros(N + T0_MAX + 1, dtype=F32)
    rounding = {"half_up": "up", "trunc": "trunc"}.get(fault, "even")
    clamp = {"clamp_2048": (T0_MIN, 2048), "clamp_2": (2, T0_MAX)}.get(fault, (T0_MIN, T0_MAX))
    rows = {}

    def row(t0):
        if t0 not in rows:
            r = table_row(t0, sr, *model)
            if fault == "row_offset":                         # row T0 read at T0 (T0 - 1) / 2 - 2: a sample late
                r = np.concatenate([r[1:], table_row(t0 + 1, sr, *model)[:1] if t0 < T0_MAX else np.zeros(1, dtype=F32)])
            if fault == "row_short":
                r = r.copy()
                r[-1] = 0
            rows[t0] = r
        return rows[t0]

    for q, f0 in enumerate(f0s):
        n, base = lens[q], int(off[q])
        oi, _, T0, _ = onsets(f0, sr, rounding, clamp)
        kmin, kmax = None, None
        if fault in ("latest_three", "own_end", "first_512") and oi.size:
            j = np.arange(n)
            last = np.searchsorted(oi, j, "right") - 1
            if fault == "latest_three":
                kmin = last - 2
            if fault == "own_end":                            # back from `last` while the onset in front ends behind the sample
                kmin = last.copy()
                own = oi + T0
                for s in range(n):
                    m = kmin[s]
                    while m > 0 and own[m - 1] > s:
                        m -= 1
                    kmin[s] = m
            if fault == "first_512":                          # the LDS list holds the first 512 of a longer covering list
                end_max = np.maximum.accumulate(oi + T0)
                g = base + j
                t_lo = g // TILE * TILE
                inside = (t_lo >= base) & (np.minimum(t_lo + TILE, N) <= base + n)
                k0 = np.searchsorted(end_max, t_lo - base, "right")
                kmax = np.where(inside, k0 + MAXON, oi.size)
        for k in range(oi.size):
            i, t0 = int(oi[k]), int(T0[k])
            end = i + t0 if fault == "no_cut" else min(i + t0, n)
            r = row(t0)[:end - i]
            if kmin is not None:
                r = np.where(kmin[i:end] <= k, r, F32(0))
            if kmax is not None:
                r = np.where(k < kmax[i:end], r, F32(0))
            out[base + i:base + end] += r
    return out[:N]


# ---------------------------------------------------------------------------------------------
# which notes the parallel phase scan must hand to the walk (k_pulse_onsets_par)
# ---------------------------------------------------------------------------------------------
def scan_verdict(f0, sr):
    """'walk': a sample's sequential phase is an exact positive integer, so the scan's sum lies inside its band (the scan
    differs from the walk by less than the band's half width: csrc/pulse.hip); 'scan': every sample's phase is more than twice
    the band away from an integer; 'either' otherwise."""
    f0 = np.ascontiguousarray(f0, dtype=F32)
    p = np.cumsum(f0.astype(F64) / F64(sr))
    i = np.arange(f0.size)
    tol = 2.3e-16 * (i // TILE * TILE + TILE) * p
    d = np.abs(p - np.rint(p))
    if np.any((d == 0) & (p > 0)):
        return "walk"
    return "scan" if np.all((d > 2.0 * tol) | (p == 0)) else "either"


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _first_onset(f, sr, which=0):
    probe = np.full(int((which + 1.5) * float(sr) / float(f)) + 32, f, dtype=F32)
    oi, _, T0, _ = onsets(probe, sr)
    return int(oi[which]), int(T0[which])


def one_onset_note(T0, sr):
    """(a): f0 = fp32(sr / T0) up to and including the first onset, zero behind it, onset + T0 + 8 samples"""
    f = F32(F64(sr) / T0)
    i, t0 = _first_onset(f, sr)
    assert t0 == T0
    n = i + T0 + 8
    f0 = np.zeros(n, dtype=F32)
    f0[:i + 1] = f
    return f0


def two_onset_note(f, sr):
    """(c): constant f0, two onsets and the whole second pulse (+ 8 samples)"""
    i, t0 = _first_onset(F32(f), sr, 1)
    return np.full(i + t0 + 8, f, dtype=F32)


def ragged_note(n, head, sr):
    """(f): n voiced samples whose last onset falls on sample n - 2 (n >= 7), T0 = 5 or 6, behind `head` zero-f0 samples"""
    m = max(1, int(round((n - 1.5) / 5.5)))
    f = F32(F64(sr) * m / (n - 1.5)) if n >= 7 else F32(8000.0)
    return np.concatenate([np.zeros(head, dtype=F32), np.full(n, f, dtype=F32)])


def const(f, n):
    return np.full(n, f, dtype=F32)


LF_MODELS = ((0.01, 1.47, 0.34), (0.05, 3.0, 1.0), (0.2, 0.5, 0.6))      # golden("pulse_train_lf")'s non-default models


@functools.lru_cache(maxsize=None)
def cases(sr=44100):
    """{batch name: {"group", "names", "f0s", "model"}} at the rate sr.  Groups:

    a  one-onset notes, one table row each (A_T0), whole, plus the eight exact zeros behind it              44100
    b  the clamps: 4 Hz (T0 8192), three notes above sr / 3.5 (T0 3; the highest overlaps), a tie that rounds up (12 600 Hz at
       44100: 3.5 -> 4; 12 800 Hz at 96000: 7.5 -> 8)                                                      44100, 96000
    c  ties sr * (1 / f0) = k + 0.5 exactly: 8 Hz (5512.5 -> 5512) and 1800 Hz (24.5 -> 24) at 44100, 4 Hz at 22050, 256 Hz at
       48000 and 512 Hz at 96000 (187.5 -> 188)
    d  dense notes of 3 * 2048 + 100 samples, each a batch of its own (D_F0)                               44100
    e  7 400 samples of 6 Hz, then 9 850 of 9 000 Hz: the look-back held open by one long pulse            44100
    f  the ragged batch (F_LENGTHS voiced samples each, every second note behind F_HEAD zero-f0 samples)   44100
    g  rows 3, 2049, 8192 of (a) under LF_MODELS, then at the default again (g3)                           44100
    """
    sr = int(sr)
    out = {}

    def put(name, group, notes, model=DEFAULT):
        out[name] = {"group": group, "names": [k for k, _ in notes], "f0s": [f for _, f in notes], "model": model}
    if sr == 44100:
        put("a", "a", [("T0_%d" % t, one_onset_note(t, sr)) for t in A_T0])
        put("b", "b", [("4Hz", const(4.0, 30000)), ("21000Hz", const(21000.0, 400)), ("20000Hz", const(20000.0, 400)),
                       ("14700Hz", const(14700.0, 400)), ("12600Hz", const(12600.0, 400))])
        put("c", "c", [("8Hz", two_onset_note(8.0, sr)), ("1800Hz", two_onset_note(1800.0, sr))])
        for f in D_F0:
            put("d%d" % f, "d", [("%dHz" % f, const(f, 3 * TILE + 100))])
        put("e", "e", [("6Hz_9000Hz", np.concatenate([const(6.0, 7400), const(9000.0, 9850)]))])
        put("f", "f", [("n%d" % n, ragged_note(n, F_HEAD if k % 2 else 0, sr)) for k, n in enumerate(F_LENGTHS)])
        for m, model in enumerate(LF_MODELS + (DEFAULT,)):
            put("g%d" % m, "g", [("T0_%d" % t, one_onset_note(t, sr)) for t in G_T0], model)
    elif sr == 96000:
        put("b", "b", [("4Hz", const(4.0, 60000)), ("47000Hz", const(47000.0, 400)), ("40000Hz", const(40000.0, 400)),
                       ("32000Hz", const(32000.0, 400)), ("12800Hz", const(12800.0, 400))])
        put("c", "c", [("512Hz", two_onset_note(512.0, sr))])
    elif sr == 48000:
        put("c", "c", [("256Hz", two_onset_note(256.0, sr))])
    elif sr == 22050:
        put("c", "c", [("4Hz", two_onset_note(4.0, sr))])
    return out


RATES = (44100, 22050, 48000, 96000)


@functools.lru_cache(maxsize=None)
def truth(sr, name):
    """train(exact=True) of every note of a batch (pulse32 = the reference arithmetic beside it); built once, left unchanged"""
    b = cases(sr)[name]
    return tuple(train(f, sr, *b["model"], exact=True) for f in b["f0s"])
