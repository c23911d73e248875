"""The convolution reverb: a signal given a room on the device, behind the compressor and in front of the loudness stage.

Every other link of the finishing chain acts on level, spectrum or peaks.  This one convolves every signal of a ragged batch with
one impulse response (the IR) of up to 2^18 taps, ``y = dry x + wet (h * x delayed by the pre-delay)``, and by default keeps the
decay past the signal's end, the definition this project's own (``include/goofer_hip.h``): the output CSR, the block
CSR and the run table come from the library's host planner (``goofer_host_reverb_plan``), the IR's spectra from
``goofer_reverb_ir`` (``Context.reverb_ir``, once per IR and device), the kernels are ``goofer_reverb`` (``Context.reverb``):
uniformly partitioned overlap-save on the project's own framewise FFT.  No IR file ships with the project: ``Room`` /
``synthetic_ir`` make one in host numpy, and ``ir:PATH`` reads a mono wav.  ``core.reverb_batch`` is the numpy-in, numpy-out
form; ``Renderer.render`` / ``render_phrase`` take ``reverb``, and ``python -m goofer_amd.phrase`` takes ``--reverb room:1.2:-10``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

BLOCK = 1024                        # GOOFER_REVERB_BLOCK
RUN = 32                            # GOOFER_REVERB_RUN
MAX_TAPS = 1 << 18                  # GOOFER_REVERB_MAX_TAPS
MAX_PREDELAY = 1 << 16              # GOOFER_REVERB_MAX_PREDELAY
MIN_SR = 8000                       # GOOFER_REVERB_MIN_SR
MAX_SR = 192000                     # GOOFER_REVERB_MAX_SR
TOL = 2.0 ** -19                    # GOOFER_REVERB_TOL
IR_HEAD = 12800                     # GOOFER_REVERB_IR_HEAD
WET_DB = -12.0


def ir_bytes(L) -> int:
    """GOOFER_REVERB_IR_BYTES(L)"""
    return IR_HEAD + 8 * BLOCK * ((int(L) + BLOCK - 1) // BLOCK)


def db_gain(db) -> float:
    """a gain in dB as the linear factor the library takes; -inf dB is 0"""
    db = float(db)
    return 0.0 if db == -math.inf else 10.0 ** (db / 20.0)


@dataclass(frozen=True)
class Room:
    """A synthetic room (``synthetic_ir``): ``rt60``, the time in seconds its decay takes to fall by 60 dB, where the IR is cut;
    ``seed`` of the noise; ``damping_hz``, the corner of an optional one-pole low-pass over the noise (None: white)."""
    rt60: float
    seed: int = 0
    damping_hz: float = None

    def __post_init__(self):
        object.__setattr__(self, "rt60", float(self.rt60))
        if int(self.seed) != self.seed or int(self.seed) < 0:
            raise ValueError("reverb: a room's seed is a whole number >= 0; got %r" % (self.seed,))
        object.__setattr__(self, "seed", int(self.seed))
        if self.damping_hz is not None:
            object.__setattr__(self, "damping_hz", float(self.damping_hz))
        if not (self.rt60 > 0.0 and math.isfinite(self.rt60)) or (self.damping_hz is not None and
                                                                  not (self.damping_hz > 0.0 and math.isfinite(self.damping_hz))):
            raise ValueError("reverb: a room has rt60 > 0 s and damping_hz > 0 Hz or None; got %r" % ((self.rt60, self.seed, self.damping_hz),))


def _rate(who, sr) -> int:
    if int(sr) != sr or not MIN_SR <= int(sr) <= MAX_SR:
        raise ValueError("%s: the sample rate is a whole number of Hz in [%d, %d]; got %r" % (who, MIN_SR, MAX_SR, sr))
    return int(sr)


def synthetic_ir(sr, room) -> np.ndarray:
    """The IR of ``room`` (a ``Room``, or its rt60 in seconds) at ``sr``, fp32 ``[ceil(rt60 * sr)]``, made in host numpy: normals
    from ``np.random.Generator(np.random.PCG64(seed))``, through a one-pole low-pass at ``damping_hz`` where the room has one,
    under an exponential decay that reaches -60 dB at ``rt60`` and is cut there, scaled to unit energy.  Raises ValueError for a
    rate outside [8000, 192000] and a length outside [1, 2^18] taps."""
    room = room if isinstance(room, Room) else Room(room)
    sr = _rate("synthetic_ir", sr)
    L = int(math.ceil(room.rt60 * sr))
    if not 1 <= L <= MAX_TAPS:
        raise ValueError("synthetic_ir: rt60 %g s at %d Hz is %d taps, 1 to %d are taken" % (room.rt60, sr, L, MAX_TAPS))
    z = np.random.Generator(np.random.PCG64(room.seed)).standard_normal(L)
    if room.damping_hz is not None:
        if not room.damping_hz < 0.5 * sr:
            raise ValueError("synthetic_ir: damping_hz %g lies under sr / 2" % room.damping_hz)
        a = math.exp(-2.0 * math.pi * room.damping_hz / sr)                # y[i] = (1 - a) z[i] + a y[i-1], as one FFT convolution
        K = min(L, int(math.ceil(math.log(1e-18) / math.log(a))) + 1) if a > 0.0 else 1
        m = 1 << int(math.ceil(math.log2(L + K)))
        z = np.fft.irfft(np.fft.rfft(z, m) * np.fft.rfft((1.0 - a) * a ** np.arange(K, dtype=np.float64), m), m)[:L]
    h = z * np.exp(-math.log(1000.0) * np.arange(L, dtype=np.float64) / (room.rt60 * sr))
    e = math.sqrt(float(np.sum(h * h)))
    if not e > 0.0:
        raise ValueError("synthetic_ir: the room's noise is all zero")
    return (h / e).astype(np.float32)


@dataclass(frozen=True, eq=False)
class Reverb:
    """The settings of the stage: ``ir``, the impulse response as a 1-D array (1 to 2^18 finite taps, kept as fp32) or a ``Room``,
    whose IR is made at the rate the stage runs at; ``wet_db`` / ``dry_db``, the gains of the convolved and of the direct signal in
    dB (-inf: none of it; wet -inf runs no transform); ``predelay_ms``, the delay of the convolved signal, rounded to whole
    samples (at most 2^16 of them); ``tail``: keep the decay past the signal's end (the output is pre-delay + taps - 1 samples
    longer).  ``ir_sr``: the rate an array IR was recorded at, or None — a plan at another rate is refused.  The IR's spectra are
    kept per device (and rate, for a room) on the object: a second call does not compute them again."""
    ir: object
    wet_db: float = WET_DB
    dry_db: float = 0.0
    predelay_ms: float = 0.0
    tail: bool = True
    ir_sr: int = None

    def __post_init__(self):
        if not isinstance(self.ir, Room):
            try:
                h = np.array(self.ir, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError("reverb: ir is a 1-D array of taps or a Room") from None
            if h.ndim != 1 or not 1 <= h.size <= MAX_TAPS or not np.all(np.isfinite(h)):
                raise ValueError("reverb: ir is a 1-D array of 1 to %d finite taps (a mono impulse response) or a Room" % MAX_TAPS)
            h.setflags(write=False)
            object.__setattr__(self, "ir", h)
        for name in ("wet_db", "dry_db", "predelay_ms"):
            try:
                object.__setattr__(self, name, float(getattr(self, name)))
            except (TypeError, ValueError):
                raise ValueError("reverb: %s is a number; got %r" % (name, getattr(self, name))) from None
        object.__setattr__(self, "tail", bool(self.tail))
        ok = (all(g == -math.inf or (math.isfinite(g) and db_gain(g) <= float(np.finfo(np.float32).max)) for g in (self.wet_db, self.dry_db))
              and math.isfinite(self.predelay_ms) and self.predelay_ms >= 0.0)
        if not ok:                  # (a NaN fails every comparison)
            raise ValueError("reverb: wet_db and dry_db are finite or -inf, predelay_ms >= 0; got %r" % ((self.wet_db, self.dry_db, self.predelay_ms),))
        if self.ir_sr is not None:
            object.__setattr__(self, "ir_sr", _rate("reverb (the impulse response)", self.ir_sr))
        object.__setattr__(self, "_taps", {})
        object.__setattr__(self, "_spectra", {})

    @property
    def wet(self) -> float:
        return db_gain(self.wet_db)

    @property
    def dry(self) -> float:
        return db_gain(self.dry_db)

    def predelay(self, sr) -> int:
        """the pre-delay in samples at ``sr``; ValueError above 2^16"""
        pre = int(math.floor(self.predelay_ms * float(sr) / 1000.0 + 0.5))
        if not 0 <= pre <= MAX_PREDELAY:
            raise ValueError("reverb: a pre-delay of %g ms at %d Hz is %d samples, at most %d are taken" % (self.predelay_ms, sr, pre, MAX_PREDELAY))
        return pre

    def taps(self, sr) -> np.ndarray:
        """the IR at ``sr``: the array, or the room's ``synthetic_ir`` (made once per rate).  ValueError for an array recorded at
        another rate."""
        sr = _rate("reverb", sr)
        if not isinstance(self.ir, Room):
            if self.ir_sr is not None and self.ir_sr != sr:
                raise ValueError("reverb: the impulse response was recorded at %d Hz and the stage runs at %d Hz" % (self.ir_sr, sr))
            return self.ir
        if sr not in self._taps:
            self._taps[sr] = synthetic_ir(sr, self.ir)
        return self._taps[sr]

    def spectra(self, ctx, sr):
        """``Context.reverb_ir`` of the IR at ``sr`` on ``ctx``'s device, computed on first use and kept; None where wet is 0 (no
        transform runs)."""
        if self.wet == 0.0:
            return None
        key = (ctx.device, int(sr) if isinstance(self.ir, Room) else None)
        if key not in self._spectra:
            self._spectra[key] = ctx.reverb_ir(self.taps(sr))
        return self._spectra[key]


def _read_ir(path):
    from . import trackers
    try:
        y, sr = trackers._read_wav_stdlib(path)
    except Exception as err:        # noqa: BLE001  (wave.Error, EOFError, OSError: one refusal for the command line)
        raise ValueError("reverb: cannot read the impulse response %s: %s" % (path, err)) from None
    if y.ndim != 1:
        raise ValueError("reverb: the impulse response %s has %d channels; the chain is mono" % (path, y.shape[1]))
    return y, sr


def parse(reverb) -> Reverb:
    """``reverb`` as Renderer.render takes it — a ``Reverb``, a tuple ``(ir[, wet_db[, dry_db[, predelay_ms[, tail]]]])`` with
    ``ir`` an array or a ``Room``, or the command line's string, ``room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]]`` for a synthetic
    room or ``ir:PATH[:WET_DB[:PREDELAY_MS]]`` for a mono wav — as a ``Reverb``.  Raises ValueError for anything else and for
    settings outside the definition's ranges."""
    if isinstance(reverb, Reverb):
        return reverb
    if isinstance(reverb, str):
        kind, _, rest = reverb.partition(":")
        toks = rest.split(":") if rest else []
        try:
            if kind == "room" and 1 <= len(toks) <= 4:
                nums = [float(v) for v in toks[:3]]
                seed = int(toks[3]) if len(toks) == 4 else 0
                return Reverb(Room(nums[0], seed), *([nums[1]] if len(nums) > 1 else []), predelay_ms=nums[2] if len(nums) > 2 else 0.0)
            if kind == "ir" and toks:
                nums = []
                while len(nums) < 2 and len(toks) > 1:               # numbers behind the path, which may hold colons of its own
                    try:
                        nums.insert(0, float(toks[-1]))
                    except ValueError:
                        break
                    toks = toks[:-1]
                y, sr = _read_ir(":".join(toks))
                return Reverb(y, *nums[:1], predelay_ms=nums[1] if len(nums) > 1 else 0.0, ir_sr=sr)
        except ValueError as err:
            if str(err).startswith("reverb:"):
                raise
        raise ValueError("reverb: room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]] or ir:PATH[:WET_DB[:PREDELAY_MS]]; got %r" % reverb)
    if isinstance(reverb, Room):
        return Reverb(reverb)
    if isinstance(reverb, (tuple, list)) and 1 <= len(reverb) <= 5 and (isinstance(reverb[0], Room) or np.ndim(reverb[0]) == 1):
        return Reverb(*reverb)
    raise ValueError("reverb is a Reverb, (ir[, wet_db[, dry_db[, predelay_ms[, tail]]]]) with ir an array or a Room, "
                     "'room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]]' or 'ir:PATH[:WET_DB[:PREDELAY_MS]]'")


@dataclass
class ReverbPlan(SP.SignalPlan):
    """What goofer_reverb takes for one ragged batch: the settings (``L`` taps, ``pre`` samples of pre-delay, ``tail``, the linear
    gains ``dry`` and ``wet``); the signals' CSR ``in_off``, the outputs' ``out_off`` and the blocks' ``blk_off`` (int64 [n + 1]
    each) and the run table ``runs`` (int32 [n_runs, 3]: signal, first block, blocks); ``blob`` holds them back to back for one
    upload."""
    sr: int
    n: int
    reverb: Reverb
    L: int
    pre: int
    tail: bool
    dry: float
    wet: float
    in_off: np.ndarray
    out_off: np.ndarray
    blk_off: np.ndarray
    runs: np.ndarray
    BLOB = ("in_off", "out_off", "blk_off", "runs")            # device_tables: these four, in this order

    @property
    def total_out(self) -> int:
        return int(self.out_off[-1])

    @property
    def total_blocks(self) -> int:
        return int(self.blk_off[-1])

    @property
    def n_runs(self) -> int:
        return len(self.runs)

    @property
    def added(self) -> int:
        """samples every signal that has any grows by: pre + L - 1 with the tail, else 0"""
        return self.pre + self.L - 1 if self.tail else 0


def plan(sr, lengths, reverb) -> ReverbPlan:
    """goofer_host_reverb_plan for signals of ``lengths`` samples lying back to back; ``reverb``: whatever ``parse`` takes.
    Raises ValueError for what the library refuses: a rate that is not a whole number of Hz in [8000, 192000], an IR recorded at
    another rate or of more than 2^18 taps, a pre-delay above 2^16 samples, a negative length, an output of 2^31 samples or more."""
    lib = _lib.load()
    reverb = parse(reverb)
    in_off = SP.offsets("reverb.plan", lengths, sr)
    sr = _rate("reverb.plan", sr)
    n = len(in_off) - 1
    L, pre = len(reverb.taps(sr)), reverb.predelay(sr)
    out_off, blk_off, need = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64), (C.c_int64 * 1)(0)
    runs, = SP.fit(lambda runs: lib.goofer_host_reverb_plan(sr, in_off.ctypes.data, n, L, pre, int(reverb.tail), out_off.ctypes.data,
                                                            blk_off.ctypes.data, *SP.cap(runs), need),
                   (np.zeros((0, 3), dtype=np.int32),), lambda: (np.zeros((int(need[0]), 3), dtype=np.int32),),
                   lambda rc: "goofer_host_reverb_plan refused %d Hz, %d taps, %d samples of pre-delay (%d): a rate in [%d, %d], outputs "
                              "shorter than 2^31 samples" % (sr, L, pre, rc, MIN_SR, MAX_SR))
    return ReverbPlan(sr, n, reverb, L, pre, reverb.tail, float(np.float32(reverb.dry)), float(np.float32(reverb.wet)), in_off, out_off,
                      blk_off, runs)
