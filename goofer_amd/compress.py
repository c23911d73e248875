"""The dynamic range compressor: a signal's level evened out on the device, in front of loudness normalisation and the limiter.

Phrase mix, loudness and the limiter are linear or protect peaks; a phrase rendered note by note has consonants, breaths and
sustained vowels 20 dB apart.  This stage is the feed-forward log-domain design with a smooth decoupled peak detector behind
the gain computer (Giannoulis, Massberg and Reiss, 2012), the definition this project's own (``include/goofer_hip.h``;
DESIGN.md): the coefficients, the tile table and the powers of the two one-pole coefficients come from the library's host
planner (``goofer_host_compress_plan``), the kernels are ``goofer_compress`` (``Context.compress``).  ``core.compress_batch``
is the numpy-in, numpy-out form; ``Renderer.render`` / ``render_phrase`` take ``compress``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

MIN_SR = 8000                       # GOOFER_COMPRESS_MIN_SR
MAX_SR = 192000                     # GOOFER_COMPRESS_MAX_SR
KNEE_DB = 6.0                       # GOOFER_COMPRESS_KNEE_DB
ATTACK_MS = 5.0                     # GOOFER_COMPRESS_ATTACK_MS
RELEASE_MS = 100.0                  # GOOFER_COMPRESS_RELEASE_MS
TILE = 4096                         # GOOFER_COMPRESS_TILE
SPT = 16                            # GOOFER_COMPRESS_SPT
COEF = 6                            # GOOFER_COMPRESS_COEF
POWS = 20                           # GOOFER_COMPRESS_POWS
RUN_TILES = 16                      # GOOFER_COMPRESS_RUN_TILES
ROUND_TILES = 4096                  # GOOFER_COMPRESS_ROUND_TILES


@dataclass(frozen=True)
class Compressor:
    """The settings of the definition: threshold T in dB re full scale ([-80, 0]), ratio R ([1, inf]), knee width W in dB
    ([0, 40]), attack and release time constants in ms ([0, 1000], [0, 5000]) and make-up gain M in dB ([-24, 24])."""
    threshold_db: float
    ratio: float
    knee_db: float = KNEE_DB
    attack_ms: float = ATTACK_MS
    release_ms: float = RELEASE_MS
    makeup_db: float = 0.0

    def __post_init__(self):
        for name in ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db"):
            object.__setattr__(self, name, float(getattr(self, name)))
        ok = (-80.0 <= self.threshold_db <= 0.0 and self.ratio >= 1.0 and 0.0 <= self.knee_db <= 40.0 and
              0.0 <= self.attack_ms <= 1000.0 and 0.0 <= self.release_ms <= 5000.0 and -24.0 <= self.makeup_db <= 24.0)
        if not ok:                  # (a NaN fails every comparison)
            raise ValueError("compress: threshold_db in [-80, 0], ratio in [1, inf], knee_db in [0, 40], attack_ms in [0, 1000], "
                             "release_ms in [0, 5000], makeup_db in [-24, 24]; got %r" % (self.astuple(),))

    def astuple(self):
        return (self.threshold_db, self.ratio, self.knee_db, self.attack_ms, self.release_ms, self.makeup_db)


def parse(compress) -> Compressor:
    """``compress`` as Renderer.render takes it — a ``Compressor``, a sequence ``(threshold_db, ratio[, attack_ms, release_ms[,
    knee_db[, makeup_db]]])`` or the command line's string ``T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]`` — as a ``Compressor``.
    Raises ValueError for anything else and for settings outside the definition's ranges."""
    if isinstance(compress, Compressor):
        return compress
    if isinstance(compress, str):
        try:
            compress = [float(v) for v in compress.split(":")]
        except ValueError:
            raise ValueError("compress: T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]], numbers") from None
    if not isinstance(compress, (tuple, list)) or len(compress) not in (2, 4, 5, 6):
        raise ValueError("compress is a Compressor, (threshold_db, ratio[, attack_ms, release_ms[, knee_db[, makeup_db]]]) or "
                         "'T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]'")
    v = [float(c) for c in compress]
    kw = dict(threshold_db=v[0], ratio=v[1])
    if len(v) >= 4:
        kw.update(attack_ms=v[2], release_ms=v[3])
    if len(v) >= 5:
        kw.update(knee_db=v[4])
    if len(v) >= 6:
        kw.update(makeup_db=v[5])
    return Compressor(**kw)


@dataclass
class CompressPlan(SP.SignalPlan):
    """What goofer_compress takes for one ragged batch: ``coef`` (float64 [6]: T, W, s = 1/R - 1, M, aR, aA), ``pows`` (float64
    [2, 20]: aR^(16 * 2^k), then aA^(16 * 2^k)), the signals' CSR ``in_off`` (int64 [n + 1]) and the tile table ``tiles`` (int32
    [n_tiles, 2]: signal, tile of the signal); ``blob`` holds them back to back for one upload."""
    sr: int
    n: int
    settings: Compressor
    coef: np.ndarray
    pows: np.ndarray
    in_off: np.ndarray
    tiles: np.ndarray
    BLOB = ("in_off", "coef", "pows", "tiles")                 # device_tables: these four, in this order


def plan(sr, lengths, settings) -> CompressPlan:
    """goofer_host_compress_plan for signals of ``lengths`` samples lying back to back; ``settings``: whatever ``parse`` takes.
    Raises ValueError for what the library refuses: a rate that is not a whole number of Hz in [8000, 192000], settings
    outside their ranges, a negative length, a signal of 2^31 samples or more."""
    lib = _lib.load()
    settings = parse(settings)
    in_off = SP.offsets("compress.plan", lengths, sr)
    n = len(in_off) - 1
    need = (C.c_int64 * 1)(0)
    coef, pows = np.zeros(COEF), np.zeros((2, POWS))
    tiles, = SP.fit(lambda tiles: lib.goofer_host_compress_plan(int(sr), *settings.astuple(), in_off.ctypes.data, n, coef.ctypes.data,
                                                                pows.ctypes.data, *SP.cap(tiles), need),
                    (np.zeros((0, 2), dtype=np.int32),), lambda: (np.zeros((int(need[0]), 2), dtype=np.int32),),
                    lambda rc: "goofer_host_compress_plan refused %s Hz (%d): a rate in [%d, %d], signals shorter than 2^31 samples"
                               % (sr, rc, MIN_SR, MAX_SR))
    return CompressPlan(int(sr), n, settings, coef, pows, in_off, tiles)


def coefficient(ms, sr) -> float:
    """aA / aR of the definition: 0 for a time constant of 0 ms, else exp(-1 / (ms * 1e-3 * sr))"""
    return 0.0 if ms == 0 else math.exp(-1.0 / (float(ms) * 1e-3 * float(sr)))
