"""Loudness metering and normalisation: a signal's integrated loudness measured on the device and the signal scaled to a target,
in front of the look-ahead limiter.

Every other link of the output chain watches peaks; this one watches level.  The measure is ITU-R BS.1770-4 for one channel
(K-weighting, 400 ms blocks with 75 % overlap, the absolute gate at -70 LUFS and the relative one 10 LU under the gated mean),
the definition this project's own (``include/goofer_hip.h``): the filter coefficients, the segment CSR, the tile
table and the powers of the filter's state-transition matrix come from the library's host planner
(``goofer_host_loudness_plan``), the kernels are ``goofer_loudness_measure`` and ``goofer_loudness_apply``
(``Context.loudness``).  ``core.loudness_batch`` is the numpy-in, numpy-out form; ``Renderer.render`` / ``render_phrase`` take
``loudness``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

MIN_SR = 8000                       # GOOFER_LOUDNESS_MIN_SR
MAX_SR = 192000                     # GOOFER_LOUDNESS_MAX_SR
MAX_GAIN_DB = 20.0                  # GOOFER_LOUDNESS_MAX_GAIN_DB
MAX_GAIN_DB_CAP = 60.0              # GOOFER_LOUDNESS_MAX_GAIN_DB_CAP
TILE = 4096                         # GOOFER_LOUDNESS_TILE
SPT = 16                            # GOOFER_LOUDNESS_SPT
MATS = 20                           # GOOFER_LOUDNESS_MATS
SLOTS = 8                           # GOOFER_LOUDNESS_SLOTS


@dataclass
class LoudnessPlan(SP.SignalPlan):
    """What goofer_loudness_measure takes for one ragged batch: the segment length ``S`` in samples, the K-weighting
    coefficients ``coef`` (float64 [10]: shelf b0 b1 b2 a1 a2, high-pass likewise), ``mats`` (float64 [20, 4, 4], the powers
    A^(16 * 2^k) of the state-transition matrix), the signals' CSR ``in_off`` and the segments' ``seg_off`` (int64 [n + 1]) and
    the tile table ``tiles`` (int32 [n_tiles, 2]: signal, tile of the signal); ``blob`` holds them back to back for one
    upload."""
    sr: int
    n: int
    S: int
    coef: np.ndarray
    mats: np.ndarray
    in_off: np.ndarray
    seg_off: np.ndarray
    tiles: np.ndarray
    BLOB = ("in_off", "seg_off", "coef", "mats", "tiles")      # device_tables: these five, in this order

    @property
    def n_segments(self) -> int:
        return int(self.seg_off[-1])


def parse(loudness):
    """``loudness`` as Renderer.render takes it — a target in LUFS, or a (target, max_gain_db) pair — as that pair.  Raises
    ValueError for a target that is not finite and a max_gain_db outside [0, 60]."""
    if isinstance(loudness, (tuple, list)):
        if len(loudness) != 2:
            raise ValueError("loudness is a target in LUFS or a (target, max_gain_db) pair")
        target, cap = float(loudness[0]), float(loudness[1])
    else:
        target, cap = float(loudness), MAX_GAIN_DB
    if not math.isfinite(target):
        raise ValueError("loudness: the target is a finite number of LUFS (None measures only)")
    if not 0.0 <= cap <= MAX_GAIN_DB_CAP:
        raise ValueError("loudness: max_gain_db lies in [0, %g]" % MAX_GAIN_DB_CAP)
    return target, cap


def plan(sr, lengths) -> LoudnessPlan:
    """goofer_host_loudness_plan for signals of ``lengths`` samples lying back to back.  Raises ValueError for what the library
    refuses: a rate that is not a whole number of Hz in [8000, 192000], a negative length, a signal of 2^31 samples or more."""
    lib = _lib.load()
    in_off = SP.offsets("loudness.plan", lengths, sr)
    n = len(in_off) - 1
    S, need = C.c_int(0), (C.c_int64 * 1)(0)
    coef, mats, seg_off = np.zeros(10), np.zeros((MATS, 4, 4)), np.zeros(n + 1, dtype=np.int64)
    tiles, = SP.fit(lambda tiles: lib.goofer_host_loudness_plan(int(sr), in_off.ctypes.data, n, C.byref(S), coef.ctypes.data,
                                                                mats.ctypes.data, seg_off.ctypes.data, *SP.cap(tiles), need),
                    (np.zeros((0, 2), dtype=np.int32),), lambda: (np.zeros((int(need[0]), 2), dtype=np.int32),),
                    lambda rc: "goofer_host_loudness_plan refused %s Hz (%d): a rate in [%d, %d], signals shorter than 2^31 samples"
                               % (sr, rc, MIN_SR, MAX_SR))
    return LoudnessPlan(int(sr), n, S.value, coef, mats, in_off, seg_off, tiles)


def seg_samples(sr) -> int:
    """S of the definition: floor(sr / 10 + 0.5), the samples of a 100 ms segment"""
    return int(math.floor(float(sr) / 10.0 + 0.5))


def momentary(seg_energy, S):
    """The momentary-loudness curve (LUFS per 400 ms block, hop 100 ms) of one signal's segment energies."""
    E = np.asarray(seg_energy, dtype=np.float64)
    kb = max(0, len(E) - 3)
    z = (E[0:kb] + E[1:kb + 1] + E[2:kb + 2] + E[3:kb + 3]) / (4.0 * S)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)
