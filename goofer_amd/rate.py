"""Output-rate conversion: finished audio from the voicebank's rate to another one on the device.

Every note, and since phrase assembly every track, is rendered at the voicebank's own rate; a 44.1 kHz voicebank mixed into a
48 kHz session needs the track at 48 kHz.  The converter is a polyphase Kaiser-windowed sinc over a ragged batch, the
definition this project's own (``include/goofer_hip.h``): the geometry, the tap table and the output offsets come
from the library's host planner (``goofer_host_rate_plan``), the kernel is ``goofer_rate_convert`` (``Context.rate_convert``).
``core.resample_batch`` is the numpy-in, numpy-out form; ``Renderer.render`` / ``render_phrase`` take ``out_sr``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

MAX_PHASES = 1024                   # GOOFER_RATE_MAX_PHASES


@dataclass
class RatePlan(SP.SignalPlan):
    """What goofer_rate_convert takes for one ragged batch: the geometry ``L``, ``M``, ``H``, the table ``taps`` (float32
    [L, 2H]), the signals' CSR ``in_off`` and that of their outputs ``out_off`` (int64 [n + 1]); ``blob`` holds the two offset
    arrays and the table back to back for one upload."""
    sr_in: int
    sr_out: int
    n: int
    L: int
    M: int
    H: int
    taps: np.ndarray
    in_off: np.ndarray
    out_off: np.ndarray
    BLOB = ("in_off", "out_off", "taps")                       # device_tables: these three, in this order

    @property
    def total_in(self) -> int:
        return self.total

    @property
    def total_out(self) -> int:
        return int(self.out_off[-1])


def plan(sr_in, sr_out, lengths) -> RatePlan:
    """goofer_host_rate_plan for signals of ``lengths`` samples lying back to back.  Raises ValueError for what the library
    refuses: a rate below 1, equal rates, more than 1024 phases on either side, a signal of 2^31 samples or more."""
    lib = _lib.load()
    in_off = SP.offsets("rate.plan", lengths)
    n = len(in_off) - 1
    out_off = np.zeros(n + 1, dtype=np.int64)
    L, M, H, need = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    taps, = SP.fit(lambda taps: lib.goofer_host_rate_plan(int(sr_in), int(sr_out), in_off.ctypes.data, n, C.byref(L), C.byref(M),
                                                          C.byref(H), *SP.cap(taps), C.byref(need), out_off.ctypes.data),
                   (np.zeros(0, dtype=np.float32),), lambda: (np.zeros(int(need.value), dtype=np.float32),),
                   lambda rc: "goofer_host_rate_plan refused %s -> %s Hz (%d): rates >= 1 and different, at most %d phases on either side "
                              "(sr / gcd), signals shorter than 2^31 samples" % (sr_in, sr_out, rc, MAX_PHASES))
    return RatePlan(int(sr_in), int(sr_out), n, L.value, M.value, H.value, taps.reshape(L.value, 2 * H.value), in_off, out_off)
