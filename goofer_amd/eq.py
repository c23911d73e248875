"""The parametric equaliser: a signal's spectrum shaped on the device, behind the rate conversion and in front of the compressor.

Every other link of the finishing chain acts on level or peaks.  This one is a cascade of up to eight Audio-EQ-Cookbook biquads
(high-pass, low-pass, the two shelves, peak, notch) run in float64 over every signal of a ragged batch, the definition this
project's own (``include/goofer_hip.h``): the coefficients, the tile table and the powers of the cascade's
state-transition matrix come from the library's host planner (``goofer_host_eq_plan``), the kernels are ``goofer_eq``
(``Context.eq``).  ``core.eq_batch`` is the numpy-in, numpy-out form; ``Renderer.render`` / ``render_phrase`` take ``eq``, and
``python -m goofer_amd.phrase`` takes ``--eq hp:80,peak:3000:3:1,hs:10000:4``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

MAX_BANDS = 8                       # GOOFER_EQ_MAX_BANDS
MIN_SR = 8000                       # GOOFER_EQ_MIN_SR
MAX_SR = 192000                     # GOOFER_EQ_MAX_SR
F_MIN_DIV = 600.0                   # GOOFER_EQ_F_MIN_DIV: f0_hz * 600 >= sr
F_MAX_REL = 0.45                    # GOOFER_EQ_F_MAX_REL
Q_MIN = 0.1                         # GOOFER_EQ_Q_MIN
Q_MAX = 8.0                         # GOOFER_EQ_Q_MAX
SHELF_Q_MAX = 2.0                   # GOOFER_EQ_SHELF_Q_MAX
MAX_GAIN_DB = 9.0                   # GOOFER_EQ_MAX_GAIN_DB
TOL = 2.0 ** -26                    # GOOFER_EQ_TOL
TILE = 4096                         # GOOFER_EQ_TILE
SPT = 16                            # GOOFER_EQ_SPT
LEVELS = 8                          # GOOFER_EQ_LEVELS
RUN_TILES = 16                      # GOOFER_EQ_RUN_TILES
Q_DEFAULT = math.sqrt(0.5)

KINDS = ("highpass", "lowpass", "lowshelf", "highshelf", "peak", "notch")      # GOOFER_EQ_HIGHPASS .. GOOFER_EQ_NOTCH, in order
SHORT = {"hp": "highpass", "lp": "lowpass", "ls": "lowshelf", "hs": "highshelf", "peak": "peak", "notch": "notch"}
GAINED = ("lowshelf", "highshelf", "peak")
SHELVES = ("lowshelf", "highshelf")


def n_mats(K) -> int:
    """GOOFER_EQ_MATS(K)"""
    return 4 * LEVELS * K + 4 * (1 + LEVELS) * K * K


@dataclass(frozen=True)
class Band:
    """One band of the definition: ``kind`` (one of ``KINDS``, or the command line's ``hp lp ls hs peak notch``), centre or
    corner frequency ``f0_hz``, ``gain_db`` ([-9, 9] for the shelves and the peak; 0 for the others, which ignore it) and
    ``q`` ([0.1, 8], for the two shelves [0.1, 2]; default sqrt(1/2)).  ``f0_hz`` is checked against the sample rate by ``plan``."""
    kind: str
    f0_hz: float
    gain_db: float = 0.0
    q: float = Q_DEFAULT

    def __post_init__(self):
        kind = SHORT.get(self.kind, self.kind)
        if kind not in KINDS:
            raise ValueError("eq: a band's kind is one of %s (or %s); got %r" % (", ".join(KINDS), " ".join(SHORT), self.kind))
        object.__setattr__(self, "kind", kind)
        for name in ("f0_hz", "gain_db", "q"):
            object.__setattr__(self, name, float(getattr(self, name)))
        ok = (self.f0_hz > 0.0 and math.isfinite(self.f0_hz) and Q_MIN <= self.q <= (SHELF_Q_MAX if kind in SHELVES else Q_MAX) and
              (abs(self.gain_db) <= MAX_GAIN_DB if kind in GAINED else self.gain_db == 0.0))
        if not ok:                  # (a NaN fails every comparison)
            raise ValueError("eq: f0_hz > 0, q in [%g, %g] (lowshelf and highshelf: up to %g), gain_db in [-%g, %g] for lowshelf, highshelf and peak "
                             "and 0 for the others; got %r" % (Q_MIN, Q_MAX, SHELF_Q_MAX, MAX_GAIN_DB, MAX_GAIN_DB, self.astuple()))

    def astuple(self):
        return (self.kind, self.f0_hz, self.gain_db, self.q)

    @property
    def identity(self) -> bool:
        """a shelf or a peak with 0 dB: the identity in exact arithmetic, dropped by the planner"""
        return self.kind in GAINED and self.gain_db == 0.0


def parse(eq) -> tuple:
    """``eq`` as Renderer.render takes it — a sequence of ``Band`` objects or ``(kind, f0_hz[, gain_db[, q]])`` tuples, or the
    command line's string, bands joined by commas, each ``kind:f0[:gain_db[:q]]`` — as a tuple of ``Band``.  Raises ValueError
    for anything else, for more than eight bands and for settings outside the definition's ranges."""
    if isinstance(eq, Band):
        eq = (eq,)
    if isinstance(eq, str):
        bands = []
        for part in eq.split(","):
            toks = part.strip().split(":")
            if not 2 <= len(toks) <= 4:
                raise ValueError("eq: bands joined by commas, each kind:f0[:gain_db[:q]]; got %r" % part)
            try:
                bands.append((toks[0].strip(), *[float(v) for v in toks[1:]]))
            except ValueError:
                raise ValueError("eq: kind:f0[:gain_db[:q]], numbers behind the kind; got %r" % part) from None
        eq = bands
    if not isinstance(eq, (tuple, list)):
        raise ValueError("eq is a sequence of Band objects or (kind, f0_hz[, gain_db[, q]]) tuples, or 'kind:f0[:gain_db[:q]],...'")
    out = []
    for b in eq:
        if not isinstance(b, Band):
            if not isinstance(b, (tuple, list)) or not 2 <= len(b) <= 4 or not isinstance(b[0], str):
                raise ValueError("eq: a band is a Band or (kind, f0_hz[, gain_db[, q]]); got %r" % (b,))
            b = Band(*b)
        out.append(b)
    if len(out) > MAX_BANDS:
        raise ValueError("eq: at most %d bands, got %d" % (MAX_BANDS, len(out)))
    return tuple(out)


@dataclass
class EqPlan(SP.SignalPlan):
    """What goofer_eq takes for one ragged batch: ``K``, the bands that are not the identity; ``coef`` (float64 [K, 5]: b0 b1
    b2 a1 a2 per band); ``mats`` (float64 [32 K + 36 K^2]: per band its own 2 x 2 block of T^(16 * 2^j), j < 8, then the coupled
    2K x 2K T^4096 and T^(65536 * 2^j), j < 8, all in the coordinates (u[i-1], u[i-1] - u[i-2]) per band); the signals' CSR
    ``in_off`` (int64 [n + 1]) and the tile table ``tiles`` (int32 [n_tiles, 2]: signal, tile of the signal); ``blob`` holds them
    back to back for one upload."""
    sr: int
    n: int
    bands: tuple
    K: int
    coef: np.ndarray
    mats: np.ndarray
    in_off: np.ndarray
    tiles: np.ndarray
    BLOB = ("in_off", "coef", "mats", "tiles")                 # device_tables: these four, in this order

    @property
    def section_mats(self) -> np.ndarray:
        """[K, 8, 2, 2]: band k's own T^(16 * 2^j)"""
        return self.mats[:4 * LEVELS * self.K].reshape(self.K, LEVELS, 2, 2)

    @property
    def carry_mats(self) -> np.ndarray:
        """[9, 2K, 2K]: T^4096, then T^(65536 * 2^j), j < 8, of the cascade"""
        return self.mats[4 * LEVELS * self.K:].reshape(1 + LEVELS, 2 * self.K, 2 * self.K)


def plan(sr, lengths, bands) -> EqPlan:
    """goofer_host_eq_plan for signals of ``lengths`` samples lying back to back; ``bands``: whatever ``parse`` takes.  Raises
    ValueError for what the library refuses: a rate that is not a whole number of Hz in [8000, 192000], a band with f0 outside
    [sr / 600, 0.45 sr] or with settings outside their ranges, a negative length, a signal of 2^31 samples or more."""
    lib = _lib.load()
    bands = parse(bands)
    in_off = SP.offsets("eq.plan", lengths, sr)
    n = len(in_off) - 1
    kind = np.array([KINDS.index(b.kind) for b in bands], dtype=np.int32)
    f0, gain, q = (np.array([getattr(b, k) for b in bands], dtype=np.float64) for k in ("f0_hz", "gain_db", "q"))
    K, need = C.c_int(0), (C.c_int64 * 1)(0)
    coef, mats = np.zeros(5 * MAX_BANDS), np.zeros(n_mats(MAX_BANDS))
    tiles, = SP.fit(lambda tiles: lib.goofer_host_eq_plan(int(sr), kind.ctypes.data, f0.ctypes.data, gain.ctypes.data, q.ctypes.data,
                                                          len(bands), in_off.ctypes.data, n, C.byref(K), coef.ctypes.data,
                                                          mats.ctypes.data, *SP.cap(tiles), need),
                    (np.zeros((0, 2), dtype=np.int32),), lambda: (np.zeros((int(need[0]), 2), dtype=np.int32),),
                    lambda rc: "goofer_host_eq_plan refused %s Hz, %r (%d): a rate in [%d, %d], f0 in [sr / %g, %g sr], signals shorter "
                               "than 2^31 samples" % (sr, [b.astuple() for b in bands], rc, MIN_SR, MAX_SR, F_MIN_DIV, F_MAX_REL))
    k = K.value
    return EqPlan(int(sr), n, bands, k, coef[:5 * k].reshape(k, 5).copy(), mats[:n_mats(k)].copy(), in_off, tiles)


def response(bands, sr, freqs) -> np.ndarray:
    """The complex frequency response of the cascade of ``bands`` (whatever ``parse`` takes) at ``sr``, at the frequencies
    ``freqs`` in Hz: the product over the bands of (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2) at z = exp(2 pi i f / sr),
    complex128 of ``freqs``' shape.  The coefficients are the planner's, so what it refuses raises ValueError here too.  Host
    numpy: for plots, checks and tests."""
    z1 = np.exp(-2j * np.pi * np.asarray(freqs, dtype=np.float64) / float(sr))
    H = np.ones(z1.shape, dtype=np.complex128)
    for c in plan(sr, [], bands).coef:                         # (the planner's own coefficients; a dropped band is the identity)
        H = H * (c[0] + c[1] * z1 + c[2] * z1 * z1) / (1.0 + c[3] * z1 + c[4] * z1 * z1)
    return H
