"""Device context: one libgoofer_hip handle per GPU, PyTorch-ROCm tensors as the buffer currency.

torch is plumbing here (allocation, streams, H2D/D2H); every number is produced by the HIP
kernels behind the C ABI.  Matrices are ``[frames, bins]`` row-major on the device — the transpose
of the reference's ``[bins, frames]`` — with fp32 rows padded to ``ld`` (a multiple of 4 floats).
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from .sampler import check_noise_seed, check_phi_seed


_ROW_ALIGN = int(__import__("os").environ.get("GOOFER_ROW_ALIGN", "4"))
if _ROW_ALIGN < 4 or _ROW_ALIGN & (_ROW_ALIGN - 1):
    raise ValueError("GOOFER_ROW_ALIGN must be a power of two >= 4 (floats per row are rounded up to it; the row kernels load 16 bytes at a time)")


def row_stride(n_bins: int) -> int:
    """floats per row of a [frames x bins] matrix (GOOFER_ROW_ALIGN: experiment knob, floats, a power of two >= 4)"""
    return (n_bins + _ROW_ALIGN - 1) & ~(_ROW_ALIGN - 1)


def spec_stride(n_bins: int) -> int:
    """complex64 slots per row of a [frames x bins] spectrum matrix: 128-byte aligned rows (csrc/common.h:spec_stride)."""
    return (n_bins + 15) & ~15


class GooferError(RuntimeError):
    pass


@functools.lru_cache(maxsize=4096)
def _pcg64_state(seed: int):
    st = np.random.PCG64(seed).state["state"]
    s, inc = int(st["state"]), int(st["inc"])
    m = 0xFFFFFFFFFFFFFFFF
    return s & m, s >> 64, inc & m, inc >> 64


def pcg64_words(seeds) -> np.ndarray:
    """goofer_phase_fill's per-note records, uint64 [n, 4]: (state lo, state hi, inc lo, inc hi) of ``np.random.PCG64(seed)`` —
    the generator ``default_rng(seed)`` starts from; the seeding itself (SeedSequence) stays numpy's.  A ``None`` seed gives
    the zero record: that note is not seeded and the fill leaves its rows alone."""
    w = np.zeros((len(seeds), 4), dtype=np.uint64)
    for i, sd in enumerate(seeds):
        if sd is not None:
            w[i] = _pcg64_state(check_phi_seed(sd))
    return w


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _host(a):
    """a host numpy array as a C pointer"""
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """Owns a ``goofer_ctx`` for one device and the current (sr, n_fft, hop) plan."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise GooferError("no ROCm device visible: goofer_amd needs an MI355X (there is no CPU path)")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        rc = self.lib.goofer_create(device, C.byref(h))
        if rc != 0:
            raise GooferError(f"goofer_create failed ({rc})")
        self.h = h
        self.geom = None
        self._track_settings = None                        # the tracker settings last applied (None: the defaults)

    def close(self):
        self._stem_scratch = None
        if getattr(self, "h", None):
            self.lib.goofer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise GooferError(f"libgoofer_hip error {rc}: {self.lib.goofer_last_error(self.h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch_call(self, fn, args, outs=(), tail=(), check=None):
        """``fn`` by the caller-scratch protocol (include/goofer_hip.h): its query form, NULL outputs and scratch, which fills the
        host offset arrays among ``args``; then the outputs the callables ``outs`` make, a scratch tensor of the reported size and
        the call on the current stream.  ``args`` / ``tail``: fn's arguments before / behind the outputs.  Returns (outputs, call),
        call() running the device call again.  ``Context._scratch_call(None, fn, args, check=check)``: the query alone, no handle."""
        h, check = (None, check) if self is None else (self.h, self._check)
        need = C.c_int64(0)
        check(fn(h, *args, *[None] * len(outs), *tail, None, C.byref(need), None))
        if self is None:
            return None
        res = [make() for make in outs]
        scratch = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=self.device)

        def call():
            self._check(fn(self.h, *args, *map(_ptr, res), *tail, _ptr(scratch), C.byref(need), self._stream()))
        call()
        return res, call

    def tensor(self, a, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device)

    def plan(self, sr: int, n_fft: int, hop: int):
        g = (int(sr), int(n_fft), int(hop))
        if self.geom != g:
            self._check(self.lib.goofer_plan(self.h, *g))
            self.geom = g
            self.lf = (0.02, 1.7, 0.8)
        return self

    def pulse_model(self, Ra: float = 0.02, Rg: float = 1.7, Rk: float = 0.8):
        """gf.pulse_train_numba's Ra, Rg, Rk (GOOFER.py:474) for every pulse this handle makes from now on (the plan's tables
        are rebuilt; a new plan starts from the defaults again)."""
        lf = (float(Ra), float(Rg), float(Rk))
        if getattr(self, "lf", (0.02, 1.7, 0.8)) != lf:
            self._check(self.lib.goofer_pulse_model(self.h, *lf))
            self.lf = lf
        return self

    @property
    def n_bins(self):
        return self.geom[1] // 2 + 1

    def reserve(self, frames: int, samples: int, notes: int):
        self._check(self.lib.goofer_reserve(self.h, frames, samples, notes))

    def table(self, which: int) -> np.ndarray:
        out = np.zeros(8193, dtype=np.float32)
        n = self.lib.goofer_debug_table(self.h, which, out.ctypes.data_as(C.c_void_p), out.size)
        if n < 0:
            self._check(n)
        return out[:n]

    _DBG = {"frame_note": (0, np.int32), "row_src": (1, np.int64), "f0": (2, np.float32), "pulse": (3, np.float32),
            "S_harm": (4, np.complex64), "S_uv": (5, np.complex64), "S_breath": (6, np.complex64), "frames": (7, np.float32),
            "env_harm": (8, np.float32), "env_noise": (9, np.float32), "mask_short": (10, np.float64),
            "note_mag": (11, np.float32), "note_peak": (12, np.float32), "onset_cnt": (13, np.int32),
            "onset_idx": (14, np.int32), "frame_skip": (15, np.uint8),
            "picks": (16, np.float32)}                        # (f0, mask) per frame, interleaved

    def debug_fetch(self, name: str) -> np.ndarray:
        """Intermediate of the last synth_batch (onset_cnt / onset_idx: also of the last pulse_train) as a flat host array
        (tests / debugging only).  onset_idx: every onset slot; note k's onset samples start at sample_off[k] // 2 + 16 k —
        after a batch with the 'sg' layer at sample_off[k] + 16 k, the sub-harmonic onsets of its last ratio."""
        which, dt = self._DBG[name]
        size = self.lib.goofer_debug_fetch(self.h, which, None, 0)
        if size < 0:
            raise GooferError(f"debug_fetch({name}) failed ({size})")
        out = np.empty(size // np.dtype(dt).itemsize, dtype=dt)
        self.lib.goofer_debug_fetch(self.h, which, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def profile_begin(self, max_steps: int):
        self._check(self.lib.goofer_profile_begin(self.h, max_steps))

    def profile_stage_names(self) -> list:
        """Stage names by index for the pipeline the handle ran last (goofer_profile_stage_name_ex); '' = unused."""
        return [self.lib.goofer_profile_stage_name_ex(self.h, i).decode() for i in range(18)]

    def profile_only(self, stage=None):
        """Bracket one stage only from the next profile_begin on (option "prof_only": two event records per step instead of
        twenty); None: every stage again."""
        idx = -1 if stage is None else self.profile_stage_names().index(stage)
        self.set_option("prof_only", idx)

    def profile_end(self) -> dict:
        """{'steps': k, 'ms': {stage: summed milliseconds}} from HIP events on the launch stream."""
        ms = np.zeros(18, dtype=np.float64)
        k = self.lib.goofer_profile_end(self.h, ms.ctypes.data_as(C.c_void_p), 18)
        if k < 0:
            self._check(k)
        names = [self.lib.goofer_profile_stage_name_ex(self.h, i).decode() for i in range(18)]
        return {"steps": k, "ms": {nm: v for nm, v in zip(names, ms.tolist()) if nm}}

    def check(self):
        """Synchronise and raise what the asynchronous batch calls detected on the device (goofer_check)."""
        self._check(self.lib.goofer_check(self.h))

    def set_option(self, name: str, value: int):
        self._check(self.lib.goofer_set_option(self.h, name.encode(), int(value)))

    def pcm16(self, x, out=None, channels=1):
        """The wav samples of fp32 audio on the device (goofer_pcm16: clip, * 32768, round half to even -> int16).  ``channels``
        2: ``x`` is a planar stereo bus, L then R (``bus_mix``), and the frames come back interleaved, int16 ``[N, 2]``
        (goofer_pcm16_planar)."""
        if channels == 1:
            out = torch.empty(x.numel(), dtype=torch.int16, device=x.device) if out is None else out
            self._check(self.lib.goofer_pcm16(self.h, _ptr(x), x.numel(), _ptr(out), self._stream()))
            return out
        if channels != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() % 2:
            raise ValueError("pcm16: channels is 1 or 2, and a stereo bus is a contiguous float32 tensor of 2 N samples")
        n = x.numel() // 2
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int16, device=x.device)
        elif out.dtype != torch.int16 or not out.is_contiguous() or out.numel() != 2 * n:
            raise ValueError("pcm16: out must be a contiguous int16 tensor of the %d frames" % n)
        self._check(self.lib.goofer_pcm16_planar(self.h, _ptr(x), n, 2, _ptr(out), self._stream()))
        return out

    def _mix_out(self, who, out, samples, channels, what):
        """``out`` of a mix onto a time line of ``samples`` samples and ``channels`` planar channels (phrase_mix, bus_mix): a new
        tensor where it is None, else checked, a ValueError in ``who``'s name that calls the samples ``what``."""
        if out is None:
            return torch.empty(channels * samples, dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != channels * samples:
            raise ValueError("%s: out must be a contiguous float32 tensor of the %s samples" % (who, what))
        return out

    def bus_mix(self, xs, plan, out=None):
        """Finished tracks panned and summed onto a planar stereo bus on the device (goofer_bus_mix; the definition:
        include/goofer_hip.h, "stereo bus", restated in tests/bus_ref.py).  ``xs``: the tracks, a list of contiguous fp32 device
        tensors, each wherever it lies (nothing is concatenated), muted ones included (or None for them); ``plan``: the
        ``goofer_amd.bus.BusPlan`` made for these very tensors (it holds their addresses; records and cover table are shipped
        in one upload the first time it is used on this device); ``out``: a contiguous fp32 device tensor of ``2 *
        plan.total_out`` samples (default: a new one; it need not be cleared, every sample is stored).  Returns it: L is
        ``out[:N]``, R is ``out[N:]``.  Asynchronous on the current stream."""
        n, total = plan.n, plan.total_out
        for j, k in enumerate(plan.index):
            x = xs[int(k)]
            if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < int(plan.tracks["len"][j]):
                raise ValueError("bus_mix: track %d must be a contiguous float32 tensor of the plan's %d samples" % (k, plan.tracks["len"][j]))
            if int(plan.tracks["len"][j]) and x.data_ptr() != int(plan.tracks["x"][j]):
                raise ValueError("bus_mix: track %d is not the tensor the plan was made for" % k)
        out = self._mix_out("bus_mix", out, total, 2, "bus's 2 * %d" % total)
        tracks, tile_off, tile_tracks = plan.device_tables(self)
        self._check(self.lib.goofer_bus_mix(self.h, _ptr(tracks), n, _ptr(tile_off), _ptr(tile_tracks), total, _ptr(out), self._stream()))
        return out

    def phrase_mix(self, x, sample_off, plan, out=None):
        """The notes of a batch enveloped and mixed into one track on the device (goofer_phrase_mix; the definition:
        include/goofer_hip.h, restated in tests/phrase_ref.py).  ``x``: the notes' samples back to back, a contiguous fp32 device
        tensor (``out["mix"]`` of a batch); ``sample_off``: their int64 CSR offsets ``[n + 1]``, a device tensor or a host
        sequence; ``plan``: a ``goofer_amd.phrase.PhrasePlan`` for these notes (records and cover table, shipped in one upload the
        first time it is used on this device); ``out``: a contiguous fp32 device tensor of ``plan.total_out`` samples (default: a
        new one; it need not be cleared, every sample is stored).  Asynchronous on the current stream."""
        n, total = plan.n, plan.total_out
        if not isinstance(sample_off, torch.Tensor):
            sample_off = self.tensor(np.ascontiguousarray(sample_off, dtype=np.int64))
        if sample_off.dtype != torch.int64 or not sample_off.is_contiguous() or sample_off.numel() != n + 1:
            raise ValueError("phrase_mix: sample_off is one contiguous int64 CSR of the plan's %d notes" % n)
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("phrase_mix: x must be a contiguous float32 tensor")
        out = self._mix_out("phrase_mix", out, total, 1, "track's %d" % total)
        notes, tile_off, tile_notes = plan.device_tables(self)
        if n and not x.numel():                                # notes without samples: the library still wants an array
            x = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._check(self.lib.goofer_phrase_mix(self.h, _ptr(x), _ptr(sample_off), n, _ptr(notes), _ptr(tile_off),
                                               _ptr(tile_notes), total, _ptr(out), self._stream()))
        return out

    def _signals(self, who, x, d_off, plan, out, n_out=None, make_out=True):
        """The argument checks the stages over a ragged batch share (rate_convert, eq, compress, loudness, limit, true_peak), each a
        ValueError in ``who``'s name: ``d_off`` a device tensor (one contiguous int64 CSR of ``plan.n`` signals), a host sequence
        (equal to the plan's) or None for the plan's own; ``x`` a contiguous fp32 tensor of at least ``plan.total`` samples;
        ``out`` None or a contiguous fp32 tensor of ``n_out`` samples (default: ``plan.total``).  Returns (the offsets on the
        device, ``out``, or with ``make_out`` a new tensor where it is None).  That ``out`` overlaps ``x`` is the library's to
        refuse."""
        n, n_out = plan.n, plan.total if n_out is None else n_out
        d_in = plan.device_tables(self)[0]
        if isinstance(d_off, torch.Tensor):
            if d_off.dtype != torch.int64 or not d_off.is_contiguous() or d_off.numel() != n + 1:
                raise ValueError("%s: the offsets are one contiguous int64 CSR of the plan's %d signals" % (who, n))
            d_in = d_off
        elif d_off is not None and not np.array_equal(np.asarray(d_off, dtype=np.int64), plan.in_off):
            raise ValueError("%s: the offsets are not the CSR the plan was made for" % who)
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < plan.total:
            raise ValueError("%s: x must be a contiguous float32 tensor of the plan's %d samples" % (who, plan.total))
        if out is None:
            out = torch.empty(n_out, dtype=torch.float32, device=self.device) if make_out else None
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n_out:
            raise ValueError("%s: out must be a contiguous float32 tensor of the %d output samples" % (who, n_out))
        return d_in, out

    def rate_convert(self, x, in_off, plan, out=None):
        """The signals of a ragged batch converted to another sample rate on the device (goofer_rate_convert; the definition:
        include/goofer_hip.h, restated in tests/rate_ref.py).  ``x``: the signals' samples back to back, a contiguous fp32 device
        tensor (``out["mix"]`` of a batch, a phrase's track); ``in_off``: their int64 CSR offsets ``[n + 1]``, a device tensor,
        a host sequence (checked against the plan) or None for the plan's own; ``plan``: a ``goofer_amd.rate.RatePlan`` for
        these lengths (offsets and tap table, shipped in one upload the first time it is used on this device); ``out``: a
        contiguous fp32 device tensor of ``plan.total_out`` samples that does not overlap ``x`` (default: a new one; it need
        not be cleared, every sample is stored).  Signal i's output is ``out[plan.out_off[i]:plan.out_off[i + 1]]``.
        Asynchronous on the current stream."""
        n, total = plan.n, plan.total_out
        d_in, out = self._signals("rate_convert", x, in_off, plan, out, n_out=total)
        _, d_out, taps = plan.device_tables(self)
        if total:                                              # (signals without samples have no output: nothing to launch)
            self._check(self.lib.goofer_rate_convert(self.h, _ptr(x), _ptr(d_in), n, plan.L, plan.M, plan.H, _ptr(taps), _ptr(d_out),
                                                     _ptr(out), self._stream()))
        return out

    def limit(self, x, d_off, plan, out=None):
        """The signals of a ragged batch brought under a ceiling by the look-ahead peak limiter on the device (goofer_limit; the
        definition: include/goofer_hip.h, restated in tests/limit_ref.py).  ``x``: the signals' samples back to back, a contiguous
        fp32 device tensor (``out["mix"]`` of a batch, a phrase's track, the output of ``rate_convert``); ``d_off``: their int64
        CSR offsets ``[n + 1]``, a device tensor, a host sequence (checked against the plan) or None for the plan's own;
        ``plan``: a ``goofer_amd.limit.LimitPlan`` for these lengths (offsets, tile table and tap table, shipped in one upload
        the first time it is used on this device); ``out``: a contiguous fp32 device tensor of ``plan.total`` samples that does
        not overlap ``x`` (default: a new one; it need not be cleared).  Returns ``(y, peak_in, min_gain)``, device tensors:
        signal i is ``y[plan.in_off[i]:plan.in_off[i + 1]]``, ``peak_in[i]`` its greatest ``|x|`` and ``min_gain[i]`` the
        smallest gain it was given (fp32 ``[n]``).  A plan made with ``true_peak`` runs goofer_limit_tp: the ceiling holds for
        the oversampled envelope (restated in tests/true_peak_ref.py) and ``peak_in`` is the true peak.  A plan made with
        ``channels=2`` runs goofer_limit_linked: signals 2g and 2g + 1 get one gain (restated in tests/bus_ref.py), and
        ``peak_in`` / ``min_gain`` are fp32 ``[n / 2]``, one pair per group.  Asynchronous on the current stream."""
        n, total = plan.n, plan.total
        d_in, out = self._signals("limit", x, d_off, plan, out)
        _, tiles, taps = plan.device_tables(self)
        if plan.channels != 1:
            groups = n // plan.channels
            peak_in = torch.empty(groups, dtype=torch.float32, device=self.device)
            min_gain = torch.empty(groups, dtype=torch.float32, device=self.device)
            if n:
                self._check(self.lib.goofer_limit_linked(
                    self.h, _ptr(x) if total else None, _ptr(d_in), n, total, plan.channels, plan.W, _ptr(taps), C.c_float(plan.ceiling),
                    _ptr(tiles) if total else None, plan.n_tiles, _ptr(out) if total else None, _ptr(peak_in), _ptr(min_gain), plan.R,
                    _ptr(plan.device_tp_taps(self)) if plan.true_peak else None, self._stream()))
            return out, peak_in, min_gain
        peak_in = torch.empty(n, dtype=torch.float32, device=self.device)
        min_gain = torch.empty(n, dtype=torch.float32, device=self.device)
        if n:
            args = (self.h, _ptr(x) if total else None, _ptr(d_in), n, total, plan.W, _ptr(taps), C.c_float(plan.ceiling),
                    _ptr(tiles) if total else None, plan.n_tiles, _ptr(out) if total else None, _ptr(peak_in), _ptr(min_gain))
            if plan.true_peak:
                self._check(self.lib.goofer_limit_tp(*args, plan.R, plan.Z, _ptr(plan.device_tp_taps(self)), self._stream()))
            else:
                self._check(self.lib.goofer_limit(*args, self._stream()))
        return out, peak_in, min_gain

    def true_peak(self, x, d_off, plan):
        """The true peak of every signal of a ragged batch, measured on the device (goofer_true_peak; the definition:
        include/goofer_hip.h, "true-peak detection", restated in tests/true_peak_ref.py): the greatest magnitude of the signal
        reconstructed at ``plan.R`` times its rate, linear.  ``x``, ``d_off`` as ``limit`` takes them; ``plan``: a
        ``goofer_amd.limit.LimitPlan`` with the true-peak table (``limit.true_peak_plan``, or the plan of a true-peak limiter
        for the same lengths).  Returns fp32 ``[n]`` on the device (0 for a signal without a sample).  Asynchronous on the
        current stream."""
        if not plan.true_peak:
            raise ValueError("true_peak: the plan has no true-peak table (limit.true_peak_plan)")
        n, total = plan.n, plan.total
        d_in, _ = self._signals("true_peak", x, d_off, plan, None, make_out=False)
        tiles = plan.device_tables(self)[1]
        peak = torch.empty(n, dtype=torch.float32, device=self.device)
        if n:
            self._check(self.lib.goofer_true_peak(self.h, _ptr(x) if total else None, _ptr(d_in), n, total, plan.R, plan.Z,
                                                  _ptr(plan.device_tp_taps(self)), _ptr(tiles) if total else None, plan.n_tiles,
                                                  _ptr(peak), self._stream()))
        return peak

    def loudness(self, x, d_off, plan, target=None, max_gain_db=20.0, out=None, channels=1):
        """The integrated loudness of the signals of a ragged batch measured on the device and, with a ``target`` in LUFS, the
        signals scaled to it (goofer_loudness_measure, goofer_loudness_apply; the definition: include/goofer_hip.h, restated in
        tests/loudness_ref.py).  ``x``: the signals' samples back to back, a contiguous fp32 device tensor; ``d_off``: their
        int64 CSR offsets ``[n + 1]``, a device tensor, a host sequence (checked against the plan) or None for the plan's own;
        ``plan``: a ``goofer_amd.loudness.LoudnessPlan`` for these lengths (shipped in one upload the first time it is used on
        this device); ``target``: None measures only; ``max_gain_db``: the cap of the gain; ``out``: a contiguous fp32 device
        tensor of ``plan.total`` samples, which may be ``x`` itself (default: a new one).  Returns ``(y, loud, gain,
        seg_energy)``, device tensors: ``y`` the scaled signals (None when measuring only), ``loud`` float64 ``[n, 2]``
        (integrated loudness and the greatest momentary loudness, LUFS), ``gain`` fp32 ``[n]`` (1 when measuring only; it goes
        from the measurement to the scaling without visiting the host) and ``seg_energy`` float64 ``[plan.n_segments]``, the
        K-weighted energy of every whole 100 ms segment (signal i: ``plan.seg_off[i]:plan.seg_off[i + 1]``).  ``channels`` 2:
        signals 2g and 2g + 1 are the channels of one programme — measure only, then goofer_loudness_link gates the sum of the
        two channels' energies (restated in tests/bus_ref.py), then the scaling: ``loud`` is float64 ``[n / 2, 2]`` and
        ``gain`` holds the group's value for both channels.  Asynchronous on the current stream."""
        from . import loudness as LD
        n, total = plan.n, plan.total
        cap = float(max_gain_db)
        if target is not None:
            target, cap = LD.parse((target, cap))
        elif not 0.0 <= cap <= LD.MAX_GAIN_DB_CAP:
            raise ValueError("loudness: max_gain_db lies in [0, %g]" % LD.MAX_GAIN_DB_CAP)
        if out is not None and target is None:
            raise ValueError("loudness: out, with a target only, must be a contiguous float32 tensor of the %d samples" % total)
        d_in, y = self._signals("loudness", x, d_off, plan, out, make_out=target is not None)
        _, d_seg, coef, mats, tiles = plan.device_tables(self)
        seg_buf = torch.empty(max(plan.n_segments, 1), dtype=torch.float64, device=self.device)     # (never a null pointer)
        seg = seg_buf[:plan.n_segments]
        loud = torch.empty((n, 2), dtype=torch.float64, device=self.device)
        gain = torch.empty(n, dtype=torch.float32, device=self.device)
        if channels != 1:
            if channels != 2 or n % 2:
                raise ValueError("loudness: channels is 1 or 2, and %d signals are not pairs" % n)
            link = torch.empty((n // 2, 2), dtype=torch.float64, device=self.device)
            if n:
                args = (_ptr(x) if total else None, _ptr(d_in), n, total, plan.S, _ptr(coef), _ptr(mats), _ptr(d_seg),
                        _ptr(tiles) if total else None, plan.n_tiles, math.nan, cap, _ptr(seg_buf), _ptr(loud), _ptr(gain))
                self._scratch_call(self.lib.goofer_loudness_measure, args)
                self._check(self.lib.goofer_loudness_link(self.h, _ptr(seg_buf), _ptr(d_seg), n, 2, plan.S, math.nan if target is None else target,
                                                          cap, _ptr(link), _ptr(gain), self._stream()))
                if y is not None and total:
                    self._check(self.lib.goofer_loudness_apply(self.h, _ptr(x), _ptr(d_in), n, total, _ptr(gain), _ptr(y), self._stream()))
            return y, link, gain, seg
        if n:
            args = (_ptr(x) if total else None, _ptr(d_in), n, total, plan.S, _ptr(coef), _ptr(mats), _ptr(d_seg),
                    _ptr(tiles) if total else None, plan.n_tiles, math.nan if target is None else target, cap,
                    _ptr(seg_buf), _ptr(loud), _ptr(gain))
            self._scratch_call(self.lib.goofer_loudness_measure, args)
            if y is not None and total:
                self._check(self.lib.goofer_loudness_apply(self.h, _ptr(x), _ptr(d_in), n, total, _ptr(gain), _ptr(y), self._stream()))
        return y, loud, gain, seg

    def compress(self, x, d_off, plan, out=None, curve=False):
        """The signals of a ragged batch through the dynamic range compressor on the device (goofer_compress; the definition:
        include/goofer_hip.h, restated in tests/compress_ref.py).  ``x``: the signals' samples back to back, a contiguous fp32
        device tensor; ``d_off``: their int64 CSR offsets ``[n + 1]``, a device tensor, a host sequence (checked against the
        plan) or None for the plan's own; ``plan``: a ``goofer_amd.compress.CompressPlan`` for these lengths, which carries the
        settings (shipped in one upload the first time it is used on this device); ``out``: a contiguous fp32 device tensor of
        ``plan.total`` samples, which may be ``x`` itself (default: a new one); ``curve``: also the detector's curve.  Returns
        ``(y, max_reduction, yl)``, device tensors: ``y`` fp32 ``[plan.total]``, ``max_reduction`` float64 ``[n]``, the greatest
        gain reduction of every signal in dB (0 for a signal without a sample), and ``yl`` float64 ``[plan.total]``, the gain
        reduction in dB per sample, or None without ``curve``.  Asynchronous on the current stream."""
        n, total = plan.n, plan.total
        d_in, y = self._signals("compress", x, d_off, plan, out)
        _, coef, pows, tiles = plan.device_tables(self)
        red = torch.zeros(n, dtype=torch.float64, device=self.device)
        yl = torch.empty(total, dtype=torch.float64, device=self.device) if curve else None
        if n:
            args = (_ptr(x) if total else None, _ptr(d_in), n, total, _ptr(coef), _ptr(pows), _ptr(tiles) if total else None,
                    plan.n_tiles, _ptr(y) if total else None, _ptr(red), _ptr(yl) if curve and total else None)
            self._scratch_call(self.lib.goofer_compress, args)
        return y, red, yl

    def eq(self, x, d_off, plan, out=None):
        """The signals of a ragged batch through the parametric equaliser on the device (goofer_eq; the definition:
        include/goofer_hip.h, restated in tests/eq_ref.py).  ``x``: the signals' samples back to back, a contiguous fp32 device
        tensor; ``d_off``: their int64 CSR offsets ``[n + 1]``, a device tensor, a host sequence (checked against the plan) or
        None for the plan's own; ``plan``: a ``goofer_amd.eq.EqPlan`` for these lengths, which carries the bands (shipped in one
        upload the first time it is used on this device); ``out``: a contiguous fp32 device tensor of ``plan.total`` samples
        that does not overlap ``x`` (default: a new one; it need not be cleared).  Returns ``y``, fp32 ``[plan.total]``: signal i
        is ``y[plan.in_off[i]:plan.in_off[i + 1]]``; with a plan whose bands are all the identity, a copy of ``x``.
        Asynchronous on the current stream."""
        n, total = plan.n, plan.total
        d_in, y = self._signals("eq", x, d_off, plan, out)
        _, coef, mats, tiles = plan.device_tables(self)
        if n and total:
            args = (_ptr(x), _ptr(d_in), n, total, plan.K, _ptr(coef) if plan.K else None, _ptr(mats) if plan.K else None, _ptr(tiles),
                    plan.n_tiles, _ptr(y))
            self._scratch_call(self.lib.goofer_eq, args)
        return y

    def reverb_ir(self, h):
        """The spectra of an impulse response on the device (goofer_reverb_ir), once per IR: ``h``, a host array of 1 to 2^18
        finite taps (taken as fp32).  Returns the device buffer (uint8) that ``reverb`` takes for every plan with this IR: the
        transform's tables, a live byte per partition of 1024 taps and the partitions' spectra."""
        from . import reverb as RV
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
        if not 1 <= h.size <= RV.MAX_TAPS or not np.all(np.isfinite(h)):
            raise ValueError("reverb_ir: 1 to %d finite taps" % RV.MAX_TAPS)
        ir = torch.empty(RV.ir_bytes(h.size), dtype=torch.uint8, device=self.device)
        self._check(self.lib.goofer_reverb_ir(self.h, _host(h), h.size, _ptr(ir), ir.numel(), self._stream()))
        return ir

    def reverb(self, x, d_off, plan, ir_spectra, out=None):
        """The signals of a ragged batch through the convolution reverb on the device (goofer_reverb; the definition:
        include/goofer_hip.h, restated in tests/reverb_ref.py).  ``x``: the signals' samples back to back, a contiguous fp32 device
        tensor; ``d_off``: their int64 CSR offsets ``[n + 1]``, a device tensor, a host sequence (checked against the plan) or
        None for the plan's own; ``plan``: a ``goofer_amd.reverb.ReverbPlan`` for these lengths, which carries the settings
        (shipped in one upload the first time it is used on this device); ``ir_spectra``: ``reverb_ir`` of the plan's IR (None is
        taken where the plan's wet gain is 0: no transform runs); ``out``: a contiguous fp32 device tensor of ``plan.total_out``
        samples that does not overlap ``x`` (default: a new one; it need not be cleared).  Returns ``y``, fp32
        ``[plan.total_out]``: signal i is ``y[plan.out_off[i]:plan.out_off[i + 1]]``, ``plan.added`` samples longer than it was.
        Asynchronous on the current stream."""
        from . import reverb as RV
        n, total, total_out = plan.n, plan.total, plan.total_out
        d_in, y = self._signals("reverb", x, d_off, plan, out, n_out=total_out)
        if plan.wet != 0.0 and (not isinstance(ir_spectra, torch.Tensor) or ir_spectra.dtype != torch.uint8 or not ir_spectra.is_contiguous()
                                or ir_spectra.numel() < RV.ir_bytes(plan.L) or ir_spectra.device != x.device):
            raise ValueError("reverb: ir_spectra is Context.reverb_ir of the plan's %d taps, on x's device" % plan.L)
        _, d_out, d_blk, runs = plan.device_tables(self)
        if n and total_out:
            args = (_ptr(x), _ptr(d_in), n, total, None if plan.wet == 0.0 else _ptr(ir_spectra), plan.L, plan.pre, int(plan.tail),
                    C.c_float(plan.dry), C.c_float(plan.wet), _ptr(d_out), _ptr(d_blk), plan.total_blocks, _ptr(runs), plan.n_runs,
                    total_out, _ptr(y))
            self._scratch_call(self.lib.goofer_reverb, args)
        return y

    def normal_fill(self, seed: int, params, lengths_or_offsets, tag: int, note_on=None, growl_scale=None, out=None):
        """float64 standard normals of stream ``tag`` (0 f0 jitter, 1 / 2 harmonic / breath volume jitter, 3 sub-harmonic f0
        jitter, 4 growl) for the notes of a ragged batch, drawn on the device (goofer_normal_fill; the stream's definition:
        include/goofer_hip.h, restated in tests/noise_ref.py).  A note's draws depend on ``seed ^ params[note].seed`` and the
        tag only.  Asynchronous on the current stream.

        ``params``: a NOTE_PARAMS array, or its device copy (``device_offsets(..)["d_par"]``).  ``lengths_or_offsets``: the notes'
        sample counts (host sequence), or the device int64 CSR offsets ``[n + 1]`` — then ``out`` gives the total.
        ``note_on``: per-note switch (host sequence or device uint8 tensor); the samples of the other notes are left as they
        are.  ``growl_scale``: per-note float64 (host or device) — writes ``0.5 * 2 ** (scale * z)`` instead of z.  ``out``:
        a contiguous float64 device tensor of the batch's samples to fill (default: a new one)."""
        keep = []

        def dev(a, dtype):
            if a is None or isinstance(a, torch.Tensor):
                return a
            keep.append(self.tensor(np.ascontiguousarray(np.asarray(a), dtype=dtype)))
            return keep[-1]
        if isinstance(lengths_or_offsets, torch.Tensor):
            d_s = lengths_or_offsets
            if out is None:
                raise ValueError("normal_fill: device offsets need the tensor to fill (out=)")
            n, total = d_s.numel() - 1, out.numel()
        else:
            s_off = self.offsets(lengths_or_offsets)
            n, total = len(s_off) - 1, int(s_off[-1])
            d_s = dev(s_off, np.int64)
        if out is None:
            out = torch.empty(total, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != total:
            raise ValueError("normal_fill: out must be a contiguous float64 tensor of the batch's %d samples" % total)
        if not isinstance(params, torch.Tensor):
            params = dev(self._c_params(params).view(np.uint8), np.uint8)
        if params.numel() * params.element_size() != n * _lib.NOTE_PARAMS.itemsize:
            raise ValueError("normal_fill: one parameter record per note")
        note_on, growl_scale = dev(note_on, np.uint8), dev(growl_scale, np.float64)
        for t, dt, what in ((note_on, torch.uint8, "note_on"), (growl_scale, torch.float64, "growl_scale")):
            if t is not None and (t.dtype != dt or t.numel() != n):
                raise ValueError(f"normal_fill: {what} is one {dt} per note")
        self._check(self.lib.goofer_normal_fill(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(params), _ptr(d_s), n, total, int(tag),
                                                _ptr(note_on), _ptr(growl_scale), _ptr(out), self._stream()))
        self._fill_keep = keep                                  # this call's uploads, until the next call (stream order frees them safely)
        return out

    def phase_fill(self, seeds, frames, out=None, n_bins=None):
        """The aperiodic branch's phases of a seeded reference run for the notes of a ragged batch, drawn on the device
        (goofer_phase_fill; the stream's definition: include/goofer_hip.h, restated in tests/pcg_ref.py): note i's rows are
        ``np.random.default_rng(seeds[i]).uniform(0, 2 pi, (n_bins, T_i)).astype(np.float32).T``, bit for bit — what
        ``synth_batch(phi=)`` takes.  Asynchronous on the current stream.

        ``seeds``: one non-negative int (any size) or None per note — the rows of a None note are not written — or the device
        copy of ``pcg64_words(seeds)`` (int64 [n, 4]).  ``frames``: the notes' frame counts (host sequence), or the device int64
        CSR offsets ``[n + 1]`` — then ``out`` gives the total.  ``out``: the ld-strided fp32 ``[sum T_i, n_bins]`` rows to fill
        (``Context.rows``; default: new ones, of the plan's ``n_bins`` unless given).  Returns the rows."""
        keep = []
        if isinstance(frames, torch.Tensor):
            d_f = frames
            if out is None:
                raise ValueError("phase_fill: device offsets need the rows to fill (out=)")
            n, total = d_f.numel() - 1, out.shape[0]
        else:
            counts = [int(v) for v in frames]
            if any(v < 0 for v in counts):
                raise ValueError("phase_fill: a negative frame count")
            f_off = self.offsets(counts)
            n, total = len(counts), int(f_off[-1])
            keep.append(self.tensor(f_off))
            d_f = keep[-1]
        if d_f.dtype != torch.int64 or not d_f.is_contiguous():
            raise ValueError("phase_fill: the frame offsets are a contiguous int64 tensor")
        if isinstance(seeds, torch.Tensor):
            d_w = seeds
        else:
            if len(seeds) != n:
                raise ValueError(f"phase_fill: {len(seeds)} seeds for {n} notes")
            keep.append(self.tensor(pcg64_words(seeds).view(np.int64)))
            d_w = keep[-1]
        if d_w.dtype != torch.int64 or not d_w.is_contiguous() or d_w.numel() != 4 * n:
            raise ValueError("phase_fill: the seed records are a contiguous int64 [n, 4] tensor (pcg64_words)")
        if out is None:
            out = self.rows(total, self.n_bins if n_bins is None else int(n_bins))
        nb = out.shape[1] if out.dim() == 2 else -1
        if (out.dim() != 2 or out.dtype != torch.float32 or out.device != self.device or out.shape[0] != total
                or (n_bins is not None and nb != int(n_bins)) or (total and (out.stride(1) != 1 or out.stride(0) < nb))):
            raise ValueError("phase_fill: out must be the batch's fp32 [%d, n_bins] rows on this context's device" % total)
        if total and n:
            self._check(self.lib.goofer_phase_fill(self.h, _ptr(d_w), _ptr(d_f), n, total, nb, _ptr(out), out.stride(0), self._stream()))
        self._fill_keep = keep                                  # this call's uploads, until the next call (stream order frees them safely)
        return out

    def legacy_normal_fill(self, seeds, lengths_or_offsets, stream_on, out=None, attempts=False):
        """The sh / sr jitter normals of a seeded reference run for the notes of a ragged batch, drawn on the device
        (goofer_legacy_normal_fill; the stream's definition: include/goofer_hip.h, restated in tests/mt_ref.py): note i draws
        what ``np.random.seed(seeds[i])`` followed by one ``np.random.randn(n_i)`` per enabled stream gives, in the reference's
        order (f0 jitter, harmonic volume, breath volume) — exact up to the last place of ``log``.  Asynchronous on the current
        stream; a note that runs into its block bound is reported by ``check()``.

        ``seeds``: one int in [0, 2**32) per note, or the device copy (int32 [n]: the 32-bit words).  ``lengths_or_offsets``: the
        notes' sample counts (host sequence), or the device int64 CSR offsets ``[n + 1]`` — then ``out`` gives the total.
        ``stream_on``: [n, 3] switches (host, or a device uint8 tensor): which of the three streams each note draws.  ``out``:
        up to three contiguous float64 device tensors of the batch's samples (f0, harmonic volume, breath volume; None: that
        stream's draws are dropped); default: three new ones.  Samples of streams that are off are left as they are.
        Returns ``out`` as a tuple — with ``attempts=True`` also the int64 [n] tensor of attempts each note's normals took."""
        keep = []
        if isinstance(lengths_or_offsets, torch.Tensor):
            d_s = lengths_or_offsets
            if out is None or all(t is None for t in out):
                raise ValueError("legacy_normal_fill: device offsets need the tensors to fill (out=)")
            n, total = d_s.numel() - 1, next(t for t in out if t is not None).numel()
        else:
            counts = [int(v) for v in lengths_or_offsets]
            if any(v < 0 for v in counts):
                raise ValueError("legacy_normal_fill: a negative sample count")
            s_off = self.offsets(counts)
            n, total = len(counts), int(s_off[-1])
            keep.append(self.tensor(s_off))
            d_s = keep[-1]
        if d_s.dtype != torch.int64 or not d_s.is_contiguous():
            raise ValueError("legacy_normal_fill: the sample offsets are a contiguous int64 tensor")
        if isinstance(seeds, torch.Tensor):
            d_seed = seeds
        else:
            if len(seeds) != n:
                raise ValueError(f"legacy_normal_fill: {len(seeds)} seeds for {n} notes")
            if any(sd is None for sd in seeds):
                raise ValueError("legacy_normal_fill: one seed per note")
            words = np.array([check_noise_seed(sd, "seeds[%d]" % i) for i, sd in enumerate(seeds)], dtype=np.uint32)
            keep.append(self.tensor(words.view(np.int32)))
            d_seed = keep[-1]
        if d_seed.dtype != torch.int32 or not d_seed.is_contiguous() or d_seed.numel() != n:
            raise ValueError("legacy_normal_fill: the seeds are one 32-bit word per note (a contiguous int32 tensor)")
        if isinstance(stream_on, torch.Tensor):
            d_on = stream_on
        else:
            keep.append(self.tensor(np.ascontiguousarray(np.asarray(stream_on) != 0, dtype=np.uint8).reshape(-1)))
            d_on = keep[-1]
        if d_on.dtype != torch.uint8 or not d_on.is_contiguous() or d_on.numel() != 3 * n:
            raise ValueError("legacy_normal_fill: stream_on is three uint8 switches per note")
        if out is None:
            out = tuple(torch.empty(total, dtype=torch.float64, device=self.device) for _ in range(3))
        out = tuple(out)
        if len(out) != 3:
            raise ValueError("legacy_normal_fill: out is (f0, harmonic volume, breath volume), None for a stream that is dropped")
        for t in out:
            if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != total or t.device != self.device):
                raise ValueError("legacy_normal_fill: an output must be a contiguous float64 tensor of the batch's %d samples" % total)
        d_att = torch.zeros(n, dtype=torch.int64, device=self.device) if attempts else None
        if n and (d_att is not None or any(t is not None for t in out)):
            self._check(self.lib.goofer_legacy_normal_fill(self.h, _ptr(d_seed), _ptr(d_on), _ptr(d_s), n, total, _ptr(out[0]), _ptr(out[1]),
                                                           _ptr(out[2]), _ptr(d_att), self._stream()))
        self._fill_keep = keep                                  # this call's uploads, until the next call (stream order frees them safely)
        return (out, d_att) if attempts else out

    def legacy_normal_jobs(self, jobs, attempts=False):
        """numpy's legacy normal stream by job table, drawn on the device (goofer_legacy_normal_jobs; the stream's definition:
        include/goofer_hip.h, restated in tests/mt_ref.py and tests/legacy_jobs_ref.py) — every legacy draw of ``gf.synthesize``.
        ``jobs``: a sequence of ``(seed, n, destinations, f32)``: ``seed`` an int in [0, 2**32); ``n`` the samples per destination;
        ``destinations`` up to four ``(tensor, offset)`` pairs in order, or None for a destination whose ``n`` draws are consumed
        and dropped — ``tensor`` a contiguous float64 tensor on this context's device that holds ``offset + n`` elements;
        ``f32`` rounds every normal to float32 and widens it again (``randn(n).astype(np.float32)`` held in float64).  Job j writes
        what ``np.random.seed(seed)`` followed by one ``np.random.randn(n)`` per destination gives, normal p to destination p // n
        at ``offset + p % n`` — exact up to the last place of ``log``.  A job with ``n == 0`` or no destination draws nothing.
        Everything is checked before anything is uploaded or launched (ValueError).  Asynchronous on the current stream; a job
        that runs into its block bound is reported by ``check()``.  Returns None, or with ``attempts=True`` the int64 [len(jobs)]
        tensor of attempts each job's normals took."""
        jobs = list(jobs)
        tab = np.zeros(len(jobs), dtype=_lib.LEGACY_JOB)
        for j, job in enumerate(jobs):
            try:
                seed, n, dsts, f32 = job
                n = int(n)
                dsts = list(dsts)
            except (TypeError, ValueError):
                raise ValueError(f"legacy_normal_jobs: job {j} is (seed, n, destinations, f32)") from None
            if seed is None:
                raise ValueError(f"legacy_normal_jobs: job {j} has no seed")
            seed = check_noise_seed(seed, "the seed of job %d" % j)
            if n < 0 or len(dsts) > 4:
                raise ValueError(f"legacy_normal_jobs: job {j} has {n} samples and {len(dsts)} destinations (at most four)")
            rec = tab[j]
            rec["seed"], rec["flags"], rec["n"], rec["n_dst"] = seed, _lib.LEGACY_F32 if f32 else 0, n, len(dsts)
            for k, d in enumerate(dsts):
                if d is None:
                    continue
                t, off = d
                off = int(off)
                if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device
                        or off < 0 or off + n > t.numel()):
                    raise ValueError(f"legacy_normal_jobs: destination {k} of job {j} must be a contiguous float64 tensor on this "
                                     f"context's device that holds offset + n = {off} + {n} elements")
                rec["dst"][k], rec["off"][k] = t.data_ptr(), off
        if self.lib.goofer_sizeof(9) != _lib.LEGACY_JOB.itemsize:
            raise GooferError("goofer_legacy_job layout mismatch between libgoofer_hip.so and the binding")
        d_att = torch.zeros(len(jobs), dtype=torch.int64, device=self.device) if attempts else None
        if jobs:
            d_tab = self.tensor(tab.view(np.uint8))
            self._check(self.lib.goofer_legacy_normal_jobs(self.h, _ptr(d_tab), len(jobs), _ptr(d_att), self._stream()))
            self._fill_keep = [d_tab]                           # this call's upload, until the next call (stream order frees it safely)
        return d_att

    def counter(self, name: str) -> int:
        """Cumulative device-side counter of the handle (goofer_counter): 'pulse_scanned_notes', 'pulse_fallback_notes', 'pulse_list_notes',
        'mask_flag_segments', 'mask_staged_segments'; and, host-side and not cumulative, the frames per wave of the last launch
        of each frame walker: 'walk_run_noise', 'walk_run_harm', 'walk_run_ola3', 'walk_run_ola1' (option 'walk_run')."""
        v = C.c_int64(0)
        self._check(self.lib.goofer_counter(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    # -- CSR helpers ---------------------------------------------------------------------------
    def offsets(self, lengths):
        off = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
        return off

    def frame_counts(self, sample_lengths, hop=None):
        hop = self.geom[2] if hop is None else int(hop)
        return (1 + np.asarray(sample_lengths, dtype=np.int64) // hop).tolist()

    # -- single-kernel entry points -------------------------------------------------------------
    def rfft_frames(self, x, sample_off, frame_off, total_frames: int, out=None):
        """x fp32 [N_total] -> complex64 [F_total, n_bins] (gf.stft per note)."""
        nb = self.n_bins
        if out is None:
            out = torch.empty((total_frames, spec_stride(nb)), dtype=torch.complex64, device=self.device)
        S, ldc = out, out.stride(0)
        self._check(self.lib.goofer_rfft_frames(self.h, _ptr(x), _ptr(sample_off), _ptr(frame_off), sample_off.numel() - 1,
                                                total_frames, _ptr(S), ldc, self._stream()))
        return S[:, :nb]

    def irfft_ola(self, S, sample_off, frame_off, total_samples: int):
        """complex64 [F_total, >=n_bins] (row stride taken from the tensor) -> fp32 [N_total] (gf.istft)."""
        assert S.dtype == torch.complex64 and S.stride(1) == 1
        y = torch.empty(total_samples, dtype=torch.float32, device=self.device)
        self._check(self.lib.goofer_irfft_ola(self.h, _ptr(S), S.stride(0), _ptr(sample_off), _ptr(frame_off),
                                              sample_off.numel() - 1, S.shape[0], total_samples, _ptr(y), self._stream()))
        return y

    def pulse_train(self, f0, sample_off):
        out = torch.empty_like(f0)
        self._check(self.lib.goofer_pulse_train(self.h, _ptr(f0), _ptr(sample_off), sample_off.numel() - 1, f0.numel(),
                                                _ptr(out), self._stream()))
        return out

    def gauss_bins(self, rows, taps: np.ndarray):
        """rows fp32 [R, ld-strided]; taps fp64 host array of odd length."""
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        out = self.rows_like(rows)
        n_bins = rows.shape[1]
        self._check(self.lib.goofer_gauss_bins(self.h, _ptr(rows), _ptr(out), rows.shape[0], n_bins, rows.stride(0),
                                               taps.ctypes.data_as(C.c_void_p), (taps.size - 1) // 2, self._stream()))
        return out

    def warp_bins(self, rows, formants=None, f_shift=None, ratio: float = 1.0):
        out = self.rows_like(rows)
        fs = None if f_shift is None else np.ascontiguousarray(f_shift, dtype=np.float64)
        self._check(self.lib.goofer_warp_bins(self.h, _ptr(rows), _ptr(out), rows.shape[0], rows.shape[1], rows.stride(0),
                                              _ptr(formants), fs.ctypes.data_as(C.c_void_p) if fs is not None else None,
                                              float(ratio), self._stream()))
        return out

    # -- f0 / formant tracks of the cold-cache analysis (csrc/tracker.hip) --------------------------------------
    def _track_configure(self, settings):
        """The handle's tracker settings for the call that follows (goofer_track_configure): ``settings`` a
        ``trackers.TrackerSettings`` or None, the defaults.  The handle is told only when they differ from the last applied."""
        key = _track_key(settings)
        if key != self._track_settings:
            self._check(self.lib.goofer_track_configure(self.h, None if key is None else C.byref(_lib.TrackSettings(*key))))
            self._track_settings = key

    def track(self, y, lengths, sr: int, hop: int, settings=None):
        """Pitch and formant tracks of a ragged batch of signals: ``y`` a contiguous fp64 device tensor holding
        ``lengths`` samples per signal, ``settings`` a ``trackers.TrackerSettings`` (None: the defaults, whatever ran on
        this context before; the same for every track_* method).  Returns (f0 [frames] fp64, f0 frame_off, formants
        [frames', 5] fp64, formant frame_off), the offsets as host int64 arrays.  Each call's scratch is a tensor of this
        method, released in stream order when it returns."""
        s_off = self._track_input(y, lengths, "track")
        self._track_configure(settings)
        out = []
        for fn, width in ((self.lib.goofer_track_pitch, 1), (self.lib.goofer_track_formants, 5)):
            f_off = np.zeros(len(s_off), dtype=np.int64)
            [res], _ = self._scratch_call(fn, (_ptr(y), _host(s_off), len(s_off) - 1, int(sr), int(hop), _host(f_off)),
                                          [lambda f_off=f_off, width=width: torch.empty((int(f_off[-1]), width), dtype=torch.float64,
                                                                                        device=self.device)])
            out += [res if width > 1 else res[:, 0], f_off]
        return tuple(out)

    # the tracker's stages one at a time (goofer_track_candidates / _path / _resample / _formant_frames): track's parts
    def _track_input(self, y, lengths, what):
        if not (isinstance(y, torch.Tensor) and y.dtype == torch.float64 and y.is_contiguous() and y.device == self.device):
            raise ValueError(f"{what} expects a contiguous fp64 tensor on this context's device")
        lengths = [int(v) for v in lengths]
        if not lengths or any(v < 0 for v in lengths) or sum(lengths) != y.numel():
            raise ValueError(f"{what}: the lengths sum to {sum(lengths)}, the signal has {y.numel()} samples")
        return self.offsets(lengths)

    def track_candidates(self, y, lengths, sr: int, hop: int, settings=None):
        """The pitch candidates of every frame: (cand_f [F, 15], cand_s [F, 15] fp64, cand_n [F] int32, frame_off host int64).
        Slot 0 is the unvoiced candidate; the slots from cand_n on are 0."""
        s_off = self._track_input(y, lengths, "track_candidates")
        self._track_configure(settings)
        f_off = np.zeros(len(s_off), dtype=np.int64)
        cand = lambda: torch.zeros((int(f_off[-1]), 15), dtype=torch.float64, device=self.device)   # noqa: E731
        count = lambda: torch.zeros(int(f_off[-1]), dtype=torch.int32, device=self.device)        # noqa: E731
        (cf, cs, cn), _ = self._scratch_call(self.lib.goofer_track_candidates,
                                             (_ptr(y), _host(s_off), len(s_off) - 1, int(sr), int(hop), _host(f_off)), (cand, cand, count))
        return cf, cs, cn, f_off

    def track_path(self, cand_f, cand_s, cand_n, frame_off, sr: int, hop: int, settings=None):
        """The Viterbi f0 [frame_off[-1]] fp64 of candidates in track_candidates' layout (contiguous device tensors)."""
        self._track_configure(settings)
        frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
        F = int(frame_off[-1])
        for t, dt in ((cand_f, torch.float64), (cand_s, torch.float64), (cand_n, torch.int32)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.device == self.device
                    and t.shape[0] == F and t.numel() == F * (1 if dt == torch.int32 else 15)):
                raise ValueError(f"track_path expects contiguous [{F}, 15] fp64 and [{F}] int32 tensors on this context's device")
        [f0], _ = self._scratch_call(self.lib.goofer_track_path, (_ptr(cand_f), _ptr(cand_s), _ptr(cand_n), _host(frame_off),
                                                                  len(frame_off) - 1, int(sr), int(hop)),
                                     [lambda: torch.empty(F, dtype=torch.float64, device=self.device)])
        return f0

    def track_resample(self, y, lengths, sr: int, settings=None):
        """The signals the formant stage analyses, at 2 x max_formant (11 kHz by default): (x11 fp64 device tensor, x_off
        host int64)."""
        s_off = self._track_input(y, lengths, "track_resample")
        self._track_configure(settings)
        x_off = np.zeros(len(s_off), dtype=np.int64)
        [x11], _ = self._scratch_call(self.lib.goofer_track_resample, (_ptr(y), _host(s_off), len(s_off) - 1, int(sr), _host(x_off)),
                                      [lambda: torch.empty(int(x_off[-1]), dtype=torch.float64, device=self.device)])
        return x11, x_off

    def track_formant_frames(self, x11, lengths11, sr: int, hop: int, settings=None):
        """Formants [F, 5] fp64 of signals at 2 x max_formant (11 kHz by default; ``lengths11`` samples each) placed as a
        signal at ``sr`` with ``hop`` would place them, and their frame_off (host int64).  The columns from n_formants on
        are 0."""
        x_off = self._track_input(x11, lengths11, "track_formant_frames")
        self._track_configure(settings)
        f_off = np.zeros(len(x_off), dtype=np.int64)
        [forms], _ = self._scratch_call(self.lib.goofer_track_formant_frames,
                                        (_ptr(x11), _host(x_off), len(x_off) - 1, int(sr), int(hop), _host(f_off)),
                                        [lambda: torch.empty((int(f_off[-1]), 5), dtype=torch.float64, device=self.device)])
        return forms, f_off

    def per_sample_f0(self, tracks, track_lengths, sample_lengths, sr, f0_min=75, f0_merge_range=2):
        """trackers.per_sample_f0 for a ragged batch in one launch (goofer_per_sample_f0): ``tracks`` a contiguous fp64 device
        tensor holding ``track_lengths`` frames per signal (two at least each), ``sample_lengths`` the signals' sample counts.
        Returns (f0, voicing mask), fp64 device tensors of sum(sample_lengths) values, bit for bit the host function's.  Bad
        offsets or lengths raise ValueError before anything is launched."""
        if not (isinstance(tracks, torch.Tensor) and tracks.dtype == torch.float64 and tracks.is_contiguous() and tracks.device == self.device):
            raise ValueError("per_sample_f0 expects a contiguous fp64 tensor on this context's device")
        t_len, s_len = [int(v) for v in track_lengths], [int(v) for v in sample_lengths]
        if not t_len or len(t_len) != len(s_len):
            raise ValueError(f"per_sample_f0: {len(t_len)} tracks for {len(s_len)} signals")
        if min(t_len) < 2 or min(s_len) < 0 or sum(t_len) != tracks.numel():
            raise ValueError(f"per_sample_f0: track lengths {min(t_len)}.. summing to {sum(t_len)} for {tracks.numel()} frames, "
                             f"sample lengths from {min(s_len)} (every track needs two frames, no length may be negative)")
        t_off, s_off = self.offsets(t_len), self.offsets(s_len)
        samples = lambda: torch.empty(int(s_off[-1]), dtype=torch.float64, device=self.device)   # noqa: E731
        (f0, mask), _ = self._scratch_call(self.lib.goofer_per_sample_f0, (_ptr(tracks), _host(t_off), _host(s_off), len(t_len), float(sr),
                                                                          float(f0_min), int(min(f0_merge_range, 2 ** 31 - 1))),
                                           (samples, samples))
        return f0, mask

    # -- analysis (GOOFER.py:942-946, 97-147) -----------------------------------------------------
    def envelope_knots(self, y32, lengths, want_env: bool = False):
        """The envelope half of gf.extract_features for a ragged batch at the current plan (goofer_envelope_knots_batch):
        ``y32`` a contiguous fp32 device tensor holding ``lengths`` samples per signal.  Returns (knots fp16 [frames, 192]:
        signal i's [T_i, K_i] knots frames-major from row frame_off[i] on, K int32 [n] on the device, frame_off host int64
        [n + 1], the sigma-2 envelope fp64 [frames, n_bins] or None).  Nothing is synchronised: the results are ready when
        the stream is.  The call's scratch is a tensor of this method, released in stream order when it returns."""
        from . import core
        if not (isinstance(y32, torch.Tensor) and y32.dtype == torch.float32 and y32.is_contiguous() and y32.device == self.device):
            raise ValueError("envelope_knots expects a contiguous fp32 tensor on this context's device")
        lengths = [int(v) for v in lengths]
        if not lengths or any(v < 1 for v in lengths) or sum(lengths) != y32.numel():
            raise ValueError(f"envelope_knots: {len(lengths)} lengths summing to {sum(lengths)} for {y32.numel()} samples "
                             "(every signal needs a sample at least)")
        sr, n_fft, _ = self.geom
        tabs = getattr(self, "_knot_tabs", None)
        if tabs is None or tabs[0] != (sr, n_fft):
            tabs = self._knot_tabs = ((sr, n_fft), core.knot_candidate_tables(sr, n_fft), core.gaussian_taps(2.0), core.gaussian_taps(0.5))
        (hz, bins), t_env, t_fit = tabs[1], tabs[2], tabs[3]
        s_off = self.offsets(lengths)
        f_off = np.zeros(len(lengths) + 1, dtype=np.int64)
        nb = self.n_bins
        ld64 = (nb + 1) & ~1
        (knots, K, env), _ = self._scratch_call(
            self.lib.goofer_envelope_knots_batch,
            (_ptr(y32), _host(s_off), len(lengths), _host(t_env), (t_env.size - 1) // 2, _host(t_fit), (t_fit.size - 1) // 2, _host(hz),
             _host(bins), _host(f_off)),
            (lambda: torch.empty((int(f_off[-1]), 192), dtype=torch.float16, device=self.device),
             lambda: torch.empty(len(lengths), dtype=torch.int32, device=self.device),
             lambda: torch.empty((int(f_off[-1]), ld64), dtype=torch.float64, device=self.device) if want_env else None),
            tail=(ld64,))
        return knots, K, f_off, (env[:, :nb] if want_env else None)

    def gauss_bins_f64(self, rows, taps: np.ndarray):
        """fp32 rows -> fp64 rows (the reference's gaussian_filter1d returns float64)."""
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        R, nb = rows.shape
        ld64 = (nb + 1) & ~1
        out = torch.empty((R, ld64), dtype=torch.float64, device=self.device)[:, :nb]
        self._check(self.lib.goofer_gauss_bins_f64(self.h, _ptr(rows), rows.stride(0), _ptr(out), ld64, R, nb,
                                                   taps.ctypes.data_as(C.c_void_p), (taps.size - 1) // 2, self._stream()))
        return out

    def knot_fit_error(self, env64, probe_rows, knot_bin, hz_knots: np.ndarray) -> float:
        hz = np.ascontiguousarray(hz_knots, dtype=np.float32)
        err = C.c_double(0.0)
        self._check(self.lib.goofer_knot_fit_error(self.h, _ptr(env64), env64.stride(0), _ptr(probe_rows), probe_rows.numel(),
                                                   env64.shape[1], _ptr(knot_bin), hz.size, hz.ctypes.data_as(C.c_void_p),
                                                   C.byref(err), self._stream()))
        return float(err.value)

    def knot_gather(self, env64, knot_bin):
        R, K = env64.shape[0], knot_bin.numel()
        out = torch.empty((R, K), dtype=torch.float16, device=self.device)
        self._check(self.lib.goofer_knot_gather(self.h, _ptr(env64), env64.stride(0), R, _ptr(knot_bin), K, _ptr(out), self._stream()))
        return out

    def knot_decode(self, knots_f16, hz_knots: np.ndarray):
        """knots fp16 [rows, K] -> env fp32 [rows, n_bins] (view of an ld-strided buffer)."""
        hz = np.ascontiguousarray(hz_knots, dtype=np.float32)
        rows, K = knots_f16.shape
        nb = self.n_bins
        env = self.rows(rows, nb)
        self._check(self.lib.goofer_knot_decode(self.h, _ptr(knots_f16), K, hz.ctypes.data_as(C.c_void_p), rows, _ptr(env),
                                                nb, env.stride(0), self._stream()))
        return env

    def rows(self, n_rows: int, n_bins: int, dtype=torch.float32):
        """Uninitialised [n_rows, n_bins] view of an ld-strided device buffer."""
        ld = row_stride(n_bins)
        return torch.empty((n_rows, ld), dtype=dtype, device=self.device)[:, :n_bins]

    def rows_like(self, r):
        """Same shape AND same row stride as ``r`` (torch.empty_like would densify a strided view)."""
        return torch.empty((r.shape[0], r.stride(0)), dtype=r.dtype, device=self.device)[:, :r.shape[1]]

    def rows_from(self, a: np.ndarray):
        """Upload a host [n_rows, n_bins] fp32 matrix into an ld-strided buffer."""
        r = self.rows(a.shape[0], a.shape[1])
        r.copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)))
        return r

    def gauss_rows_f64(self, x, taps: np.ndarray, lengths=None):
        """gf.gaussian_filter1d along the last axis of an fp64 [rows, L] device tensor (each row its own reflect padding).
        ``lengths``: ragged rows instead — a contiguous fp64 tensor of sum(lengths) values, row r the next lengths[r] of them."""
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        if lengths is None:
            rows, L = x.shape
            row_off = np.arange(rows + 1, dtype=np.int64) * L
        else:
            row_off = self.offsets(lengths)
            rows = len(lengths)
            if not (x.dtype == torch.float64 and x.is_contiguous() and x.numel() == int(row_off[-1]) and min(lengths, default=1) >= 1):
                raise ValueError("gauss_rows_f64: ragged rows need a contiguous fp64 tensor of sum(lengths) values, no row empty")
        off = self.tensor(row_off)
        out = torch.empty_like(x)
        self._check(self.lib.goofer_gauss_rows_f64(self.h, _ptr(x), _ptr(off), rows, int(row_off[-1]), taps.ctypes.data_as(C.c_void_p),
                                                   (taps.size - 1) // 2, _ptr(out), self._stream()))
        return out

    # -- ragged feature preparation of core.synthesize_batch -----------------------------------------------------------
    def ingest_rows(self, flat, lengths, n_cols: int):
        """to_compute(a).T for a batch of [n_cols, T_i] arrays in one launch (goofer_ingest_rows): ``flat`` a contiguous fp32 or
        fp64 device tensor holding the arrays back to back (C order), ``lengths`` their T_i.  Returns the ld-strided fp32
        [sum T_i, n_cols] rows; fp64 is rounded on the device exactly as numpy's astype(np.float32)."""
        lengths = [int(v) for v in lengths]
        if not (isinstance(flat, torch.Tensor) and flat.dtype in (torch.float32, torch.float64) and flat.is_contiguous()
                and flat.device == self.device):
            raise ValueError("ingest_rows expects a contiguous fp32 or fp64 tensor on this context's device")
        if any(v < 0 for v in lengths) or sum(lengths) * int(n_cols) != flat.numel():
            raise ValueError(f"ingest_rows: {len(lengths)} arrays of {n_cols} x {sum(lengths)} values, the buffer has {flat.numel()}")
        row_off = self.offsets(lengths)
        tile_off = self.offsets([(v + 63) // 64 for v in lengths])
        meta = self.tensor(np.concatenate([row_off, tile_off]))
        out = self.rows(int(row_off[-1]), int(n_cols))
        n = len(lengths)
        self._check(self.lib.goofer_ingest_rows(self.h, _ptr(flat), int(flat.dtype == torch.float64), _ptr(meta[:n + 1]),
                                                _ptr(meta[n + 1:]), n, int(tile_off[-1]), int(n_cols), _ptr(out), out.stride(0),
                                                self._stream()))
        return out

    def warp_bins_ragged(self, rows, lengths, formants, f_shift, ratio, anchor):
        """goofer_warp_bins note by note in one launch (goofer_warp_bins_ragged): ``lengths`` rows per note; per note
        ``f_shift`` [n, 4], ``ratio`` [n] and ``anchor`` [n] (False: no anchor warp, as f_shift=None of warp_bins)."""
        lengths = [int(v) for v in lengths]
        n, R = len(lengths), rows.shape[0]
        if any(v < 0 for v in lengths) or sum(lengths) != R or (formants is not None and tuple(formants.shape) != (R, 4)):
            raise ValueError("warp_bins_ragged: the row lengths do not cover the rows (or the formants do not)")
        args = np.zeros((n, 6), dtype=np.float64)
        args[:, :4] = np.asarray(f_shift, dtype=np.float64).reshape(n, 4)
        args[:, 4] = np.asarray(ratio, dtype=np.float64)
        args[:, 5] = np.asarray(anchor, dtype=bool)
        meta = self.tensor(np.concatenate([self.offsets(lengths), args.ravel().view(np.int64)]))
        out = self.rows_like(rows)
        self._check(self.lib.goofer_warp_bins_ragged(self.h, _ptr(rows), _ptr(out), R, rows.shape[1], rows.stride(0), _ptr(formants),
                                                     _ptr(meta[:n + 1]), n, _ptr(meta[n + 1:].view(torch.float64)), self._stream()))
        return out

    def stretch_ragged(self, env_h, env_n, row_lengths, row_cuts, rows_out, f0, mask, sample_lengths, sample_cuts, samples_out):
        """gf.synthesize's time stretch for every note in one launch (goofer_stretch_ragged): per note concat(x[:a],
        stretch(x[a:b]), x[b:]) of env_h and env_n (ld-strided, the same stride; ``row_cuts`` (a, b) per note, ``rows_out``
        output rows per note) and of f0 and mask (``sample_cuts``, ``samples_out``).  Returns (env_h, env_n, f0, mask)."""
        def axis(lengths, cuts, out_lengths):
            lengths, out_lengths = np.asarray(lengths, dtype=np.int64), np.asarray(out_lengths, dtype=np.int64)
            cuts = np.asarray(cuts, dtype=np.int64).reshape(len(lengths), 2)
            a, b = cuts[:, 0], cuts[:, 1]
            m = out_lengths - a - (lengths - b)
            # the kernel indexes by these: a cut outside its array, or a region stretched from nothing, would read out of bounds
            if np.any(a < 0) or np.any(b < a) or np.any(b > lengths) or np.any(m < 0) or np.any((m > 0) & (b == a)):
                raise ValueError("stretch_ragged: a cut (a, b) outside its array, or an empty region stretched")
            return [self.offsets(lengths), self.offsets(out_lengths), cuts.ravel()]
        n = len(row_lengths)
        if not (len(row_cuts) == len(rows_out) == len(sample_lengths) == len(sample_cuts) == len(samples_out) == n):
            raise ValueError("stretch_ragged: one cut and one output length per note on both axes")
        ra, sa = axis(row_lengths, row_cuts, rows_out), axis(sample_lengths, sample_cuts, samples_out)
        R, N = int(ra[0][-1]), int(sa[0][-1])
        if (env_h.shape[0] != R or env_n.shape != env_h.shape or env_n.stride(0) != env_h.stride(0) or env_h.stride(0) != row_stride(env_h.shape[1])
                or env_h.stride(1) != 1 or env_n.stride(1) != 1 or f0.numel() != N or mask.numel() != N or not (f0.is_contiguous() and mask.is_contiguous())
                or f0.dtype != torch.float32 or mask.dtype != torch.float32):
            raise ValueError("stretch_ragged: the arrays do not match the per-note lengths")
        meta = self.tensor(np.concatenate(ra + sa))
        pieces, o = [], 0
        for k in (n + 1, n + 1, 2 * n, n + 1, n + 1, 2 * n):
            pieces.append(meta[o:o + k])
            o += k
        R2, N2 = int(ra[1][-1]), int(sa[1][-1])
        h2, n2 = self.rows(R2, env_h.shape[1]), self.rows(R2, env_h.shape[1])
        f2 = torch.empty(N2, dtype=torch.float32, device=self.device)
        m2 = torch.empty(N2, dtype=torch.float32, device=self.device)
        self._check(self.lib.goofer_stretch_ragged(self.h, *[_ptr(t) for t in pieces], n, R2, N2, env_h.shape[1], env_h.stride(0),
                                                   _ptr(env_h), _ptr(env_n), _ptr(h2), _ptr(n2), _ptr(f0), _ptr(mask), _ptr(f2),
                                                   _ptr(m2), self._stream()))
        return h2, n2, f2, m2

    def vocal_roughness(self, y, f0, mask, noise_s, k_list, h_list, noise_amp: float, hp_fc: float, alpha_slewed, lengths=None):
        """apply_vocal_roughness (GOOFER.py:901-940) on fp32 device signals; ``noise_s`` fp64 [n_k, N] smoothed noises,
        ``alpha_slewed`` fp32 [N].  Returns the roughened signal (a new tensor)."""
        n_total = y.numel()
        lengths = [n_total] if lengths is None else list(lengths)
        off = self.tensor(self.offsets(lengths))
        k = np.ascontiguousarray(k_list, dtype=np.float64)
        h = np.ascontiguousarray(h_list, dtype=np.float64)
        out = torch.empty_like(y)
        self._check(self.lib.goofer_vocal_roughness(self.h, _ptr(y), _ptr(f0), _ptr(mask), _ptr(noise_s) if len(k) else None, len(k),
                                                    k.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), float(noise_amp),
                                                    float(hp_fc), _ptr(alpha_slewed), _ptr(off), len(lengths), n_total, _ptr(out),
                                                    self._stream()))
        out._keep = off
        return out

    def smooth_mask_ds(self, mask, lengths=None, sigma: float = 100.0, fast_interp: bool = False):
        """gf.smooth_mask_ds (GOOFER.py:556-569) of fp32 device masks (a ragged batch when ``lengths`` is given)."""
        n_total = mask.numel()
        lengths = [n_total] if lengths is None else [int(v) for v in lengths]
        # the kernels index the mask by these lengths: a mismatch would read and write out of bounds on the device
        if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.float32 and mask.is_contiguous() and mask.device == self.device):
            raise ValueError("smooth_mask_ds expects a contiguous fp32 tensor on this context's device")
        if any(v < 0 for v in lengths) or sum(lengths) != n_total:
            raise ValueError(f"smooth_mask_ds: the lengths sum to {sum(lengths)}, the mask has {n_total} samples")
        off = self.tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
        out = torch.empty(n_total, dtype=torch.float32, device=self.device)
        self._check(self.lib.goofer_smooth_mask_ds(self.h, _ptr(mask), _ptr(off), len(lengths), n_total, float(sigma),
                                                   int(bool(fast_interp)), _ptr(out), self._stream()))
        return out

    def stretch_rows(self, x, rows_out: int):
        """gf.stretch_feature along axis 0 (GOOFER.py:597-616): a 1-D fp32 tensor, or an ld-strided [rows, bins] view."""
        if x.dim() == 1:
            y = torch.empty(rows_out, dtype=torch.float32, device=self.device)
            self._check(self.lib.goofer_stretch_rows(self.h, _ptr(x), 1, x.numel(), _ptr(y), 1, rows_out, 1, self._stream()))
            return y
        y = self.rows(rows_out, x.shape[1])
        self._check(self.lib.goofer_stretch_rows(self.h, _ptr(x), x.stride(0), x.shape[0], _ptr(y), y.stride(0), rows_out, x.shape[1],
                                                 self._stream()))
        return y

    def onepole_cascade(self, x, f0, cutoff_factor: float, order: int = 4, btype: str = "lowpass", f0_mode: int = 0, lengths=None):
        """dynamic_butter_filter (SillySampler.py:95-174) on fp32 device signals: every note of ``lengths`` (default:
        the whole array as one note) is filtered with the same settings.  Returns a new tensor."""
        n_total = x.numel()
        lengths = [n_total] if lengths is None else list(lengths)
        off = self.offsets(lengths)
        jobs = np.zeros(len(lengths), dtype=_lib.ONEPOLE_JOB)
        jobs["src_off"] = jobs["dst_off"] = jobs["f0_off"] = off[:-1]
        jobs["n"], jobs["order"], jobs["highpass"] = lengths, order, int(btype != "lowpass")
        jobs["f0_mode"], jobs["cutoff_factor"] = f0_mode, cutoff_factor
        d_jobs = self.tensor(jobs.view(np.uint8))
        y = torch.empty_like(x)
        self._check(self.lib.goofer_onepole_cascade(self.h, _ptr(x), _ptr(y), _ptr(f0), _ptr(d_jobs), len(lengths), self._stream()))
        y._keep = d_jobs
        return y

    # -- the batch ------------------------------------------------------------------------------
    def device_offsets(self, env_lengths, sample_lengths, params: np.ndarray, put=None, hop=None):
        """Upload the CSR offsets and the per-note parameter array once (reused by every step of a resident batch)."""
        params = self._c_params(params)
        s_off = self.offsets(sample_lengths)
        f_off = self.offsets(self.frame_counts(sample_lengths, hop))
        e_off = self.offsets(env_lengths)
        put = put or self.tensor
        return {"s_off": s_off, "f_off": f_off, "e_off": e_off, "d_s": put(s_off), "d_f": put(f_off),
                "d_e": put(e_off), "d_par": put(params.view(np.uint8))}

    def _c_params(self, params: np.ndarray) -> np.ndarray:
        if params.dtype != _lib.NOTE_PARAMS or params.dtype.itemsize != _lib.NOTE_PARAMS.itemsize:
            # numpy re-packs structured dtypes on concatenate/promotion: force the C layout back
            fixed = np.zeros(params.shape, dtype=_lib.NOTE_PARAMS)
            for name in _lib.NOTE_PARAMS.names:
                fixed[name] = params[name]
            params = fixed
        return np.ascontiguousarray(params)

    def synth_batch(self, env, env_lengths, f0, mask, sample_lengths, params: np.ndarray, formants=None, phi=None,
                    seed: int = 0, transition_sigma: float = 100.0, want_rec=True, want_mix=True, offsets=None,
                    noise_f0=None, noise_vol=None, f0_jitter_speed: float = 100.0, vol_jitter_speed: float = 150.0,
                    subharm=None, volume_vibrato: bool = False, env_noise=None, mix_only: bool = False, noise_subharm=None,
                    assembly=None, f0_64=None):
        """Run goofer_synth_batch — or, given the ``assembly`` descriptor that produces this batch's f0 / mask / env,
        goofer_render_batch (assembly + synthesis as one call, the pulse chain forked as soon as f0 exists).

        ``subharm`` = dict(semitones, vibrato, rate, depth, delay) switches the sub-harmonic pulse layer on for the
        notes whose params.subharm_weight > 0 (gf.synthesize's add_subharm, GOOFER.py:1076-1097).

        env fp32 [R_total, n_bins] ld-strided device tensor; env_lengths rows per note;
        f0 / mask fp32 [N_total]; sample_lengths per note; params structured array (NOTE_PARAMS);
        formants fp64 [R_total, 4] or None; phi fp32 [F_total, n_bins] ld-strided or None.
        ``f0_64``: the same f0 as a float64 device tensor (goofer_batch.f0_64: what the reference holds behind its time stretch).
        Returns dict of device tensors harm / uv / bre / rec / mix, plus the CSR offsets.
        """
        nb = self.n_bins
        n = len(sample_lengths)
        o = offsets or self.device_offsets(env_lengths, sample_lengths, params)
        s_off, f_off, e_off = o["s_off"], o["f_off"], o["e_off"]
        d_s, d_f, d_e, d_par = o["d_s"], o["d_f"], o["d_e"], o["d_par"]
        N, F, R = int(s_off[-1]), int(f_off[-1]), int(e_off[-1])
        assert env.shape == (R, nb) and f0.numel() == N and mask.numel() == N and params.shape == (n,)
        if mix_only and want_mix:
            # the three stems are scratch of this call (they hold the stems before the peak gain afterwards): one block per handle,
            # grown as needed and re-used call after call in stream order, instead of 12 N bytes through the allocator per batch
            st = getattr(self, "_stem_scratch", None)
            Np = (N + 63) & ~63                                 # each stem starts on a 256-byte boundary (the finish pass's 16-byte accesses)
            if st is None or st.numel() < 3 * Np:
                st = self._stem_scratch = torch.empty(3 * max(Np, (int(1.25 * N) + 63) & ~63), dtype=torch.float32, device=self.device)
            out = {k: st[i * Np:i * Np + N] for i, k in enumerate(("harm", "uv", "bre"))}
        else:
            out = {k: torch.empty(N, dtype=torch.float32, device=self.device) for k in ("harm", "uv", "bre")}
        if want_rec:
            out["rec"] = torch.empty(N, dtype=torch.float32, device=self.device)
        if want_mix:
            out["mix"] = torch.empty(N, dtype=torch.float32, device=self.device)
        if phi is not None:
            assert phi.shape == (F, nb) and phi.stride(0) == env.stride(0)
        if env_noise is not None:                            # pre-blurred noise envelope rows (gf.synthesize's time stretch)
            assert env_noise.shape == env.shape and env_noise.stride(0) == env.stride(0)
        b = _lib.Batch(n_notes=n, n_bins=nb, ld=env.stride(0), mix_only=int(bool(mix_only and want_mix)), total_frames=F, total_samples=N, total_env_rows=R,
                       sample_off=d_s.data_ptr(), frame_off=d_f.data_ptr(), env_off=d_e.data_ptr(), env=env.data_ptr(),
                       formants=formants.data_ptr() if formants is not None else None, f0=f0.data_ptr(),
                       mask=mask.data_ptr(), phi=phi.data_ptr() if phi is not None else None,
                       env_noise=env_noise.data_ptr() if env_noise is not None else None, params=d_par.data_ptr(),
                       seed=seed, transition_sigma=float(transition_sigma),
                       noise_f0=noise_f0.data_ptr() if noise_f0 is not None else None,
                       noise_vol_h=noise_vol[0].data_ptr() if noise_vol is not None else None,
                       noise_vol_b=noise_vol[1].data_ptr() if noise_vol is not None else None,
                       noise_subharm=noise_subharm.data_ptr() if noise_subharm is not None else None,
                       f0_jitter_sigma=self.geom[0] / (f0_jitter_speed * 6), vol_jitter_sigma=self.geom[0] / (vol_jitter_speed * 6),
                       vol_jitter_speed=float(vol_jitter_speed), volume_vibrato=int(bool(volume_vibrato)),
                       subharm_ratio=_ratios(subharm)[0], subharm_more=(C.c_double * 15)(*_ratios(subharm)[1:16]),
                       subharm_vib_rate=float(subharm.get("rate", 6.0)) if subharm else 0.0,
                       subharm_vib_depth=float(subharm.get("depth", 0.1)) if subharm else 0.0,
                       subharm_vib_delay=float(subharm.get("delay", 0.1)) if subharm else 0.0,
                       subharm_vibrato=int(bool(subharm.get("vibrato", False))) if subharm else 0,
                       unit_pitch_shift=int(bool(np.all(params["pitch_shift"] == 1.0))),
                       no_warp=int(bool(np.all(params["f_shift"] == 1.0) and np.all(params["formant_shift"] == 1.0))),
                       harm=out["harm"].data_ptr(),
                       uv=out["uv"].data_ptr(), bre=out["bre"].data_ptr(),
                       rec=out["rec"].data_ptr() if want_rec else None, mix=out["mix"].data_ptr() if want_mix else None,
                       f0_64=f0_64.data_ptr() if f0_64 is not None else None)
        if f0_64 is not None:
            assert f0_64.dtype == torch.float64 and f0_64.numel() == N and f0_64.is_contiguous()
        if assembly is not None:
            self._check(self.lib.goofer_render_batch(self.h, C.byref(assembly), C.byref(b), self._stream()))
        else:
            self._check(self.lib.goofer_synth_batch(self.h, C.byref(b), self._stream()))
        out["_keep"] = (d_s, d_f, d_e, d_par, f0_64)   # keep device-side descriptors alive until the caller syncs
        out["sample_off"], out["frame_off"] = s_off, f_off
        return out


def _track_key(settings):
    """A ``trackers.TrackerSettings`` (or anything with goofer_track_settings' fields) as the struct's values in order;
    None stays None, the defaults."""
    if settings is None:
        return None
    return tuple(getattr(settings, name) for name, _ in _lib.TrackSettings._fields_)


def track_frame_offsets(lengths, sr: int, hop: int, settings=None):
    """(f0 frame_off, formant frame_off) the tracker gives signals of these lengths under ``settings`` (a
    ``trackers.TrackerSettings``; None: the defaults), from the library's own layout (goofer_track_layout); needs no
    device."""
    lib = _lib.load()
    s_off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=s_off[1:])
    key = _track_key(settings)
    p_off, f_off = np.zeros(len(s_off), dtype=np.int64), np.zeros(len(s_off), dtype=np.int64)
    rc = lib.goofer_track_layout(None if key is None else C.byref(_lib.TrackSettings(*key)), _host(s_off), len(s_off) - 1, int(sr),
                                 int(hop), _host(p_off), None, _host(f_off))
    if rc != 0:
        raise GooferError(f"libgoofer_hip error {rc}: the tracker refuses this batch (settings, sample rate, hop or a signal length)")
    return p_off, f_off


def _ratios(subharm):
    """2^(st/12) for up to sixteen sub-harmonic semitone offsets (a scalar or a list, like gf.add_subharms takes), 0-padded."""
    if not subharm:
        return [0.0] * 16
    st = np.atleast_1d(np.asarray(subharm["semitones"], dtype=np.float64))
    if st.size > 16:
        raise ValueError("at most sixteen sub-harmonic ratios per call")
    r = [float(2.0 ** (v / 12.0)) for v in st]
    return r + [0.0] * (16 - len(r))


_default = {}


def default_context(device: int = 0) -> Context:
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]


def default_params(n: int) -> np.ndarray:
    """NOTE_PARAMS array with gf.synthesize's defaults (GOOFER.py:971-983) and a unity mix."""
    p = np.zeros(n, dtype=_lib.NOTE_PARAMS)
    p["pitch_shift"] = 1.0
    p["formant_shift"] = 1.0
    p["f_shift"] = 1.0
    p["uv_strength"] = 0.75
    p["breath_strength"] = 0.1
    p["normalize"] = 1.0
    p["apply_brightness"] = 1
    p["cut_below_f0"] = 1
    p["mix_harm"] = p["mix_breath"] = p["mix_unvoiced"] = p["volume"] = 1.0
    return p
