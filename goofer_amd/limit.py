"""Look-ahead peak limiter: finished audio brought under a ceiling on the device, in front of the int16 conversion.

``goofer_pcm16`` hard-clips whatever arrives above full scale, and a finished track can: notes are peak-normalised before their
volume, the phrase mix sums cross-faded neighbours, and the rate converter's windowed sinc overshoots.  The limiter is all FIR
and min / max over a ragged batch, the definition this project's own (``include/goofer_hip.h``): the look-ahead, the
raised-cosine table and the tile table come from the library's host planner (``goofer_host_limit_plan``), the kernel is
``goofer_limit`` (``Context.limit``).  ``core.limit_batch`` is the numpy-in, numpy-out form; ``Renderer.render`` /
``render_phrase`` take ``limit``.

With ``true_peak`` the limiter watches the reconstructed signal between the samples as well (after BS.1770-4 Annex 2; the
header's "true-peak detection"): the plan then carries the oversampling factor ``R`` and the interpolation table of
``goofer_host_true_peak_plan``, the kernel is ``goofer_limit_tp`` and the ceiling is a true-peak ceiling (dBTP).  The meter
alone is ``goofer_true_peak`` (``Context.true_peak``, ``core.true_peak_batch``) on a ``true_peak_plan``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

MAX_LOOK = 1024                     # GOOFER_LIMIT_MAX_LOOK
TILE = 4096                         # GOOFER_LIMIT_TILE
CEILING = 32767.0 / 32768.0         # GOOFER_LIMIT_CEILING
LOOK_MS = 5.0                       # GOOFER_LIMIT_LOOK_MS
TP_ZEROS = 12                       # GOOFER_TP_ZEROS
TP_MIN_SR, TP_MAX_SR = 8000, 192000  # GOOFER_TP_MIN_SR, GOOFER_TP_MAX_SR


@dataclass(frozen=True)
class Limiter:
    """The limiter's settings as ``Renderer.render`` takes them: the ceiling in (0, 1], the look-ahead in ms, and whether the
    ceiling holds for the true peak (the oversampled envelope) or for the samples."""
    ceiling: float = CEILING
    lookahead_ms: float = LOOK_MS
    true_peak: bool = False


@dataclass
class LimitPlan(SP.SignalPlan):
    """What goofer_limit takes for one ragged batch: the look-ahead ``W`` in samples, the ceiling (an fp32 value), the table
    ``taps`` (float32 [2W + 1]), the signals' CSR ``in_off`` (int64 [n + 1]) and the tile table ``tiles`` (int32 [n_tiles, 2]:
    signal, tile of the signal); with ``true_peak`` the factor ``R``, ``Z`` and the table ``tp_taps`` (float32 [R - 1, 2Z]), else
    0, 0 and an empty one; ``blob`` holds offsets, tiles and the two tables back to back for one upload."""
    sr: int
    n: int
    W: int
    ceiling: float
    taps: np.ndarray
    in_off: np.ndarray
    tiles: np.ndarray
    R: int
    Z: int
    tp_taps: np.ndarray
    channels: int = 1                 # 2: signals 2g and 2g + 1 are one group (goofer_limit_linked); ``tiles`` is the groups' table
    BLOB = ("in_off", "tiles", "taps", "tp_taps")

    @property
    def true_peak(self) -> bool:
        return self.R != 0

    def device_tables(self, ctx):
        """(in_off, tiles, taps) on ``ctx``'s device: views of the blob, uploaded on first use."""
        return self._tables(ctx)[:3]

    def device_tp_taps(self, ctx):
        """the true-peak table on ``ctx``'s device: a view of the same blob"""
        return self._tables(ctx)[3]


def parse(limit):
    """``limit`` as Renderer.render takes it, as the arguments of ``plan`` behind the lengths: a ceiling or a (ceiling,
    lookahead_ms) pair as that pair; a ``Limiter`` or a (ceiling, lookahead_ms, true_peak) triple, ``true_peak`` a bool, as
    that triple."""
    if isinstance(limit, Limiter):
        limit = (limit.ceiling, limit.lookahead_ms, bool(limit.true_peak))
    if isinstance(limit, (tuple, list)):
        if len(limit) == 3 and isinstance(limit[2], (bool, np.bool_)):
            return float(limit[0]), float(limit[1]), bool(limit[2])
        if len(limit) != 2:
            raise ValueError("limit is a ceiling, a (ceiling, lookahead_ms) pair, a (ceiling, lookahead_ms, true_peak) triple "
                             "with a bool last, or a Limiter")
        return float(limit[0]), float(limit[1])
    return float(limit), LOOK_MS


def true_peak_table(sr):
    """goofer_host_true_peak_plan: (R, Z, float32 [R - 1, 2Z]) at ``sr``.  Raises ValueError for a rate outside 8000 .. 192000 Hz."""
    lib = _lib.load()
    if int(sr) != sr:
        raise ValueError("limit.true_peak_table: the sample rate is a whole number of Hz")
    R, Z, need = C.c_int(0), C.c_int(0), C.c_int64(0)
    taps, = SP.fit(lambda taps: lib.goofer_host_true_peak_plan(int(sr), C.byref(R), C.byref(Z), *SP.cap(taps), C.byref(need)),
                   (np.zeros(0, dtype=np.float32),), lambda: (np.zeros(int(need.value), dtype=np.float32),),
                   lambda rc: "goofer_host_true_peak_plan refused %s Hz (%d): true-peak detection takes %d to %d Hz" % (sr, rc, TP_MIN_SR, TP_MAX_SR))
    return R.value, Z.value, taps.reshape(R.value - 1, 2 * Z.value)


def group_lengths(who, lengths, channels):
    """The lengths of the groups of ``channels`` consecutive signals, which must agree within a group (``channels`` 1: the
    lengths themselves).  Raises ValueError in ``who``'s name."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    if channels not in (1, 2):
        raise ValueError("%s: channels is 1 or 2" % who)
    if channels == 1:
        return lengths
    if len(lengths) % channels:
        raise ValueError("%s: %d signals are not groups of %d channels" % (who, len(lengths), channels))
    g = lengths.reshape(-1, channels)
    if (g != g[:, :1]).any():
        raise ValueError("%s: the channels of a group have equal lengths" % who)
    return np.ascontiguousarray(g[:, 0])


def true_peak_plan(sr, lengths) -> LimitPlan:
    """The plan of the meter alone (``Context.true_peak``): the limiter's own tile table for these lengths and the true-peak
    table at ``sr``."""
    return plan(sr, lengths, true_peak=True)


def dbtp(x) -> float:
    """a linear peak in dB relative to full scale (-inf for 0): dBTP of a true peak, dBFS of a sample peak"""
    v = float(x)
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def plan(sr, lengths, ceiling=CEILING, lookahead_ms=LOOK_MS, true_peak=False, channels=1) -> LimitPlan:
    """goofer_host_limit_plan for signals of ``lengths`` samples lying back to back.  Raises ValueError for what the library
    refuses: a look-ahead that rounds to less than 1 or more than 1024 samples, a ceiling that is not in (0, 1] as fp32, a rate
    below 1, a signal of 2^31 samples or more.  ``true_peak``: also goofer_host_true_peak_plan's factor and table (a rate of
    8000 to 192000 Hz), in the same blob.  ``channels`` 2: the plan of goofer_limit_linked — signals 2g and 2g + 1 are the
    channels of group g, of equal lengths (anything else is refused), and the tile table is the planner's for the group
    lengths."""
    lib = _lib.load()
    in_off = SP.offsets("limit.plan", lengths, sr)
    n = len(in_off) - 1
    g_off = in_off if channels == 1 else SP.offsets("limit.plan", group_lengths("limit.plan", np.diff(in_off), channels), sr)
    c = float(np.float32(ceiling))
    W, need = C.c_int(0), (C.c_int64 * 2)(0, 0)
    taps, tiles = SP.fit(
        lambda taps, tiles: lib.goofer_host_limit_plan(int(sr), float(lookahead_ms), C.c_float(c), g_off.ctypes.data, len(g_off) - 1, C.byref(W),
                                                       *SP.cap(taps), *SP.cap(tiles), need),
        (np.zeros(0, dtype=np.float32), np.zeros((0, 2), dtype=np.int32)),
        lambda: (np.zeros(int(need[0]), dtype=np.float32), np.zeros((int(need[1]), 2), dtype=np.int32)),
        lambda rc: "goofer_host_limit_plan refused a ceiling of %r and %r ms at %s Hz (%d): a ceiling in (0, 1], a look-ahead of 1 to %d "
                   "samples, a rate >= 1, signals shorter than 2^31 samples" % (ceiling, lookahead_ms, sr, rc, MAX_LOOK))
    R, Z, tp_taps = true_peak_table(sr) if true_peak else (0, 0, np.zeros((0, 0), dtype=np.float32))
    return LimitPlan(int(sr), n, W.value, c, taps, in_off, tiles, R, Z, tp_taps, int(channels))


def look_samples(sr, lookahead_ms=LOOK_MS) -> int:
    """W of the definition: floor(look_ms * sr / 1000 + 0.5) in float64."""
    return int(math.floor(float(lookahead_ms) * float(sr) / 1000.0 + 0.5))


def reduction_db(min_gain) -> float:
    """a gain as the reduction it is, in dB (0 for a gain of 1; inf for 0)"""
    g = float(min_gain)
    return -20.0 * math.log10(g) if g > 0.0 else math.inf
