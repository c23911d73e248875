"""The cold-cache path: a voicebank sample that has no ``<stem>_features.goofy`` yet.

The reference analyses the wav on the first render and writes the cache (SillySampler.py:425-432; folder mode :214-240).
Half of that analysis is its own arithmetic — STFT magnitude, sigma-2 blur, mel-knot fit — and runs on the GPU here
(``core.envelope_features``).  The other half is Praat's (f0 by autocorrelation, formants by Burg's method,
through ``praat-parselmouth``): third-party, unpinned, not in this image — **parity unpinned** for those tracks (SURVEY §8 c).
This module is the plug for that half and the host logic the reference wraps around it:

* a *tracker* is ``fn(y, sr, hop_length, n_frames) -> (f0_track [frames'], {1..5: formant track [n_frames]})``;
  ``praat_tracker`` makes the reference's very calls when ``parselmouth`` is importable (GOOFER.py:341-353, 768-792);
  ``native_tracker`` computes the same tracks on the GPU from the published methods without Praat (``tracker="native"``
  or ``GOOFER_TRACKER=native``; its numbers are its own, not Praat's); ``TrackerSettings`` are its pitch range, costs and
  formant ceiling, ``native(settings)`` a tracker bound to them (``"native:pitch_floor=40,max_formant=5000"`` by name);
  ``get()`` resolves the tracker to use (argument, ``GOOFER_TRACKER=name`` or ``module:function``, Praat when present);
* ``fix_f0_gaps`` (GOOFER.py:415-435) and ``per_sample_f0`` (GOOFER.py:957-966) — pinned by ``tests/golden/cold_cache.npz``,
  which ``make_golden.py`` generates by running the reference's own ``extract_features`` over a fake ``parselmouth``;
* ``analyse_batch`` / ``ensure_features_batch`` / ``extract_folder``: wav -> features -> byte-compatible ``.goofy`` next to
  the wav, many samples per device pass; ``ensure_features`` is the batch of one.

Nothing here re-implements Praat: the native tracker follows the published methods, not Praat's code.
"""
from __future__ import annotations

import dataclasses
import importlib
import importlib.util
import logging
import math
import os
from pathlib import Path

import numpy as np

AUDIO_SUFFIXES = (".wav", ".flac", ".aiff", ".aif", ".mp3")      # SillySampler.py:211-212


class TrackerUnavailable(NotImplementedError):
    """No f0 / formant tracker can be had: parselmouth is not installed and none was supplied (a RuntimeError)."""


# -- trackers ----------------------------------------------------------------------------------------------------
def praat_tracker(y, sr, hop_length, n_frames):
    """The reference's Praat calls, argument for argument: ``Sound.to_pitch`` with the AC method, time step hop / sr, floor
    75 Hz, ceiling 950 Hz (GOOFER.py:341-353 — extract_features never forwards its own f0_max), and ``Sound.to_formant_burg``
    with the same time step and five formants, read back frame by frame at the frame's own time (GOOFER.py:768-792)."""
    try:
        import parselmouth
    except ImportError as e:                                      # noqa: PERF203
        raise TrackerUnavailable("praat-parselmouth is not installed") from e
    step = hop_length / sr
    snd = parselmouth.Sound(y, sr)
    burg = snd.to_formant_burg(time_step=step, max_number_of_formants=5)
    tracks = {k: [] for k in range(1, 6)}
    for frame in range(1, burg.get_number_of_frames() + 1):       # Praat numbers frames from 1
        t = burg.get_time_from_frame_number(frame)
        for k in tracks:
            try:
                v = burg.get_value_at_time(k, t)
            except Exception:                                     # noqa: BLE001 - "undefined" is a zero in the reference
                v = None
            tracks[k].append(0.0 if v is None else v)
    pitch = parselmouth.Sound(y, sr).to_pitch(method=parselmouth.Sound.ToPitchMethod.AC, time_step=step, pitch_floor=75,
                                              pitch_ceiling=950)
    return pitch.selected_array["frequency"], fit_formants(tracks, n_frames)


NATIVE_SR_RANGE = (8000, 96000)


@dataclasses.dataclass(frozen=True)
class TrackerSettings:
    """The native tracker's settings (``goofer_track_settings`` of include/goofer_hip.h; the defaults are what the reference
    hands to Praat): the pitch range in Hz (``pitch_floor`` an integer in [20, 600] — the pitch window is three of its
    periods —, ``pitch_ceiling`` above it and at most 20000; a call uses min(ceiling, sr / 2)), Boersma's thresholds and
    costs (finite and >= 0, the voicing threshold in (0, 1)), and the formant stage's ceiling ``max_formant`` (an integer in
    [2500, 8000] Hz; Praat's advice is 5000 for a male voice, 5500 for a female one) and count ``n_formants`` (3, 4 or 5).
    A value outside its range raises ValueError naming the field, as ``goofer_track_configure`` refuses it."""
    pitch_floor: int = 75
    pitch_ceiling: float = 950.0
    silence_threshold: float = 0.03
    voicing_threshold: float = 0.45
    octave_cost: float = 0.01
    octave_jump_cost: float = 0.35
    voiced_unvoiced_cost: float = 0.14
    max_formant: int = 5500
    n_formants: int = 5

    def __post_init__(self):
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            try:
                if isinstance(v, bool):
                    raise TypeError
                x = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"TrackerSettings: {f.name} must be a number (got {v!r})") from None
            if f.type in (int, "int"):
                if not (math.isfinite(x) and x == int(x)):
                    raise ValueError(f"TrackerSettings: {f.name} must be an integer (got {v!r})")
                x = int(x)
            object.__setattr__(self, f.name, x)
        if not 20 <= self.pitch_floor <= 600:
            raise ValueError(f"TrackerSettings: pitch_floor {self.pitch_floor} outside [20, 600]")
        if not self.pitch_floor < self.pitch_ceiling <= 20000.0:
            raise ValueError(f"TrackerSettings: pitch_ceiling {self.pitch_ceiling:g} must be above the floor ({self.pitch_floor}) and at "
                             "most 20000")
        for name in ("silence_threshold", "octave_cost", "octave_jump_cost", "voiced_unvoiced_cost"):
            if not (math.isfinite(getattr(self, name)) and getattr(self, name) >= 0.0):
                raise ValueError(f"TrackerSettings: {name} {getattr(self, name):g} must be finite and >= 0")
        if not 0.0 < self.voicing_threshold < 1.0:
            raise ValueError(f"TrackerSettings: voicing_threshold {self.voicing_threshold:g} outside (0, 1)")
        if not 2500 <= self.max_formant <= 8000:
            raise ValueError(f"TrackerSettings: max_formant {self.max_formant} outside [2500, 8000]")
        if self.n_formants not in (3, 4, 5):
            raise ValueError(f"TrackerSettings: n_formants {self.n_formants} is not 3, 4 or 5")

    @classmethod
    def parse(cls, text: str) -> "TrackerSettings":
        """``"key=value,key=value"`` (what follows ``native:`` in a tracker name) -> settings; an unknown key or a value that
        is no number raises ValueError."""
        names = {f.name for f in dataclasses.fields(cls)}
        kw = {}
        for item in text.split(","):
            key, eq, value = (p.strip() for p in item.partition("="))
            if not eq or key not in names or key in kw:
                raise ValueError(f"tracker settings {text!r}: {item.strip()!r} is not one key=value with a key of {sorted(names)}")
            try:
                kw[key] = float(value)
            except ValueError:
                raise ValueError(f"tracker settings {text!r}: {key}={value!r} is not a number") from None
        return cls(**kw)


def native_min_length(sr, settings=None) -> int:
    """Samples in one pitch window of the native tracker: 3 periods of the pitch floor (40 ms at 75 Hz), rounded up."""
    return -(-3 * int(sr) // (settings or TrackerSettings()).pitch_floor)


def native_refusal(n_samples, sr, settings=None):
    """The ValueError native_tracker raises for a mono signal of this length and rate, or None when it takes the signal."""
    sr = int(sr)
    if not NATIVE_SR_RANGE[0] <= sr <= NATIVE_SR_RANGE[1]:
        return ValueError(f"native_tracker: sample rate {sr} Hz is outside {NATIVE_SR_RANGE[0]}..{NATIVE_SR_RANGE[1]} Hz")
    if n_samples < native_min_length(sr, settings):
        floor = (settings or TrackerSettings()).pitch_floor
        return ValueError(f"native_tracker: {n_samples} samples is shorter than one pitch window; at {sr} Hz the minimum length "
                          f"is {native_min_length(sr, settings)} samples ({3000 / floor:g} ms)")
    return None


def native_tracker(y, sr, hop_length, n_frames, ctx=None, settings=None):
    """``praat_tracker``'s contract on the GPU (csrc/tracker.hip): f0 by Boersma's autocorrelation method with a Viterbi
    path and Praat's AC settings as the reference passes them (floor 75 Hz, ceiling 950 Hz, time step hop / sr), formants
    by Burg's method with ``to_formant_burg``'s defaults (5 formants up to 5500 Hz, 50 ms Gaussian, pre-emphasis from 50 Hz);
    ``settings`` (a ``TrackerSettings``) replaces those values.  Written from the published methods: its tracks are not
    Praat's numbers (parity unpinned), and the f0 track has its own frame layout like Praat's does.  Raises ValueError for a
    signal shorter than one pitch window."""
    import torch
    from .device import default_context
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("native_tracker expects a mono signal")
    sr = int(sr)
    refused = native_refusal(len(y), sr, settings)
    if refused is not None:
        raise refused
    c = ctx or default_context()
    f0, _, forms, _ = c.track(torch.as_tensor(y).to(c.device), [len(y)], sr, int(hop_length), settings=settings)
    f0, forms = f0.cpu().numpy(), forms.cpu().numpy()
    return f0, fit_formants({k: forms[:, k - 1].tolist() for k in range(1, 6)}, n_frames)


class NativeTracker:
    """``native_tracker`` bound to settings (``native(settings)``): a tracker like any other, which the batched paths
    recognise (``native_settings``) and serve with one ``Context.track`` call per pass."""

    def __init__(self, settings: TrackerSettings):
        if not isinstance(settings, TrackerSettings):
            raise TypeError("native() expects a TrackerSettings")
        self.settings = settings

    def __call__(self, y, sr, hop_length, n_frames, ctx=None):
        return native_tracker(y, sr, hop_length, n_frames, ctx=ctx, settings=self.settings)

    def __repr__(self):
        return f"native({self.settings!r})"


def native(settings=None):
    """The native tracker bound to ``settings`` (None: ``native_tracker`` itself, the defaults)."""
    return native_tracker if settings is None else NativeTracker(settings)


def native_settings(track_fn):
    """(True, its settings or None) when ``track_fn`` is the native tracker, bound or not; else (False, None)."""
    if track_fn is native_tracker:
        return True, None
    if isinstance(track_fn, NativeTracker):
        return True, track_fn.settings
    return False, None


_REGISTRY = {"praat": praat_tracker, "native": native_tracker}


def register(name: str, fn) -> None:
    _REGISTRY[name] = fn


def get(tracker=None):
    """The tracker to use: the argument if it is callable; else the name given (or ``$GOOFER_TRACKER``) looked up in the
    registry ("praat", "native"), read as ``native:key=value,...`` (the native tracker bound to ``TrackerSettings``, for
    example ``native:pitch_floor=40,pitch_ceiling=1200,max_formant=5000``; a bad key or value is a ValueError) or imported
    as ``module:function``; else Praat when parselmouth is importable.  Raises TrackerUnavailable.  The native tracker is
    used only when named."""
    if callable(tracker):
        return tracker
    name = tracker or os.environ.get("GOOFER_TRACKER")
    if name:
        if name in _REGISTRY:
            return _REGISTRY[name]
        if name.startswith("native:"):
            return native(TrackerSettings.parse(name[len("native:"):]))
        if ":" in name:
            mod, attr = name.split(":", 1)
            return getattr(importlib.import_module(mod), attr)
        raise TrackerUnavailable(f"unknown tracker {name!r} (registered: {sorted(_REGISTRY)}; or module:function)")
    if importlib.util.find_spec("parselmouth") is not None:
        return praat_tracker
    raise TrackerUnavailable("this sample has no _features.goofy and no f0 / formant tracker is available: install "
                             "praat-parselmouth (what the reference uses), set GOOFER_TRACKER=native (the GPU tracker) or module:function, or run the "
                             "reference's extractor once")


# -- the reference's own arithmetic around the tracks -----------------------------------------------------------------
def fit_formants(tracks: dict, n_frames: int) -> dict:
    """Every track zero-padded / cut to the STFT frame count (GOOFER.py:783-790)."""
    out = {}
    for k, v in tracks.items():
        v = list(v)[:n_frames]
        out[k] = v + [0.0] * (n_frames - len(v))
    return out


def fix_f0_gaps(f0_track, max_gap: int = 4):
    """Runs of exact zeros no longer than ``max_gap`` that have a neighbour on both sides are bridged linearly between those
    neighbours (GOOFER.py:415-435); longer runs and runs touching either end stay zero."""
    f0 = np.array(f0_track, dtype=np.float64)
    zero = f0 == 0.0
    edges = np.flatnonzero(np.diff(np.concatenate([[False], zero, [False]]).astype(np.int8)))
    for a, b in zip(edges[0::2], edges[1::2]):                    # zero run [a, b)
        gap = int(b - a)
        if a > 0 and b < f0.size and gap <= max_gap:
            left, right = f0[a - 1], f0[b]
            for j in range(gap):
                r = (j + 1) / (gap + 1)
                f0[a + j] = left * (1 - r) + right * r
    return f0


def per_sample_f0(f0_track, n_samples: int, sr, f0_min=75, f0_merge_range=2):
    """(f0 per sample, voicing mask) from a frame-rate track (GOOFER.py:957-966): NaN -> 0, short gaps bridged, linear
    interpolation over linspace(0, duration) grids of the track and of the samples (0 outside), clip to [1e-5, 2000],
    voiced where the result exceeds ``f0_min``."""
    track = fix_f0_gaps(np.nan_to_num(np.asarray(f0_track, dtype=np.float64)), f0_merge_range)
    dur = n_samples / sr
    t_track, t_samp = np.linspace(0, dur, num=len(track)), np.linspace(0, dur, num=n_samples)
    if len(track) == 0:
        raise ValueError("x cannot be empty")                     # what gf.interp1d says about an empty track
    if len(track) == 1:                                           # a one-point "interpolant": the fill value except AT the point
        f0 = np.zeros(n_samples)
        f0[np.isclose(t_samp, t_track[0])] = track[0]
    else:
        inside = (t_samp >= t_track[0]) & (t_samp <= t_track[-1])
        f0 = np.zeros(n_samples)
        f0[inside] = np.interp(t_samp[inside], t_track, track)
    f0 = np.clip(f0, 1e-5, 2000)
    return f0, (f0 > f0_min).astype(float)


# -- wav in -------------------------------------------------------------------------------------------------------
def read_audio(path):
    """(mono float64 samples, sr).  soundfile when it is installed (what the reference reads with, any format it knows);
    otherwise PCM / float WAV through the standard library.  Channels are averaged like the reference does."""
    try:
        import soundfile as sf
        y, sr = sf.read(str(path))
    except ImportError:
        y, sr = _read_wav_stdlib(path)
    y = np.asarray(y, dtype=np.float64)
    return (y.mean(axis=1) if y.ndim > 1 else y), int(sr)


def _read_wav_stdlib(path):
    import wave
    with wave.open(str(path), "rb") as w:
        ch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 1:
        y = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    elif width == 2:
        y = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        y = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float64) / float(1 << 23)
    elif width == 4:
        y = np.frombuffer(raw, dtype="<i4").astype(np.float64) / float(1 << 31)
    else:
        raise ValueError(f"unsupported WAV sample width {width}")
    return (y.reshape(-1, ch) if ch > 1 else y), sr


# -- analysis -> .goofy --------------------------------------------------------------------------------------------
def features_path(audio_path) -> Path:
    p = Path(audio_path)
    return p.with_name(f"{p.stem}_features.goofy")


def ensure_features(audio_path, n_fft=1024, hop_length=256, tracker=None, ctx=None) -> Path:
    """The sample's ``.goofy``: returned as is when it exists, else analysed from the wav and written the way the reference
    writes it (knots mode, fp16 f0 / mask, formant dict: save_features) — through a temporary file, so a concurrent render
    never loads half a cache.  ``ensure_features_batch`` of this one path; raises the exception it reports for it."""
    feat = features_path(audio_path)
    if feat.exists():
        return feat
    if not Path(audio_path).exists():
        raise FileNotFoundError(f"{audio_path} not found (and no {feat.name} beside it)")
    track_fn = get(tracker)                                      # before any work: the usual reason a cold sample cannot render
    logging.info("Extracting features")
    out = ensure_features_batch([audio_path], n_fft, hop_length, tracker=track_fn, ctx=ctx, workers=1)[audio_path]
    if isinstance(out, BaseException):
        raise out
    return out


def _write_features(feat, knots, f0, vmask, forms, sr, y_len) -> Path:
    """save_features into a temporary file beside ``feat``, then renamed over it: a concurrent render never loads half a cache.
    The temporary name is one of its own per writer (two threads of one process may analyse the same cold sample) and is gone
    again if anything fails."""
    from . import core
    import tempfile
    fd, tmp_name = tempfile.mkstemp(prefix=feat.name + ".tmp", dir=str(feat.parent))
    os.close(fd)
    tmp = Path(tmp_name)
    try:
        core.save_features(tmp, knots, f0, vmask, forms, sr, y_len)
        os.replace(tmp, feat)
    finally:
        if tmp.exists():
            tmp.unlink()
    return feat


def extract_folder(path, tracker=None, ctx=None) -> dict:
    """Folder mode (SillySampler.py:214-240): every audio file under ``path`` (or the file itself) gets its ``.goofy``;
    existing ones are skipped, a failing file is logged and does not stop the others.  The files without a cache are analysed
    together by ``ensure_features_batch`` (device passes of many files each).  Returns the tallies."""
    root = Path(path)
    files = [f for f in (sorted(root.rglob("*")) if root.is_dir() else [root]) if f.is_file() and f.suffix.lower() in AUDIO_SUFFIXES]
    track_fn = get(tracker)                                      # fail before the first file, not at every file
    done = {"extracted": 0, "skipped": 0, "failed": 0}
    todo = []
    for f in files:
        if features_path(f).exists():
            logging.info(f"[SKIP] {features_path(f).name} already exists")
            done["skipped"] += 1
            continue
        logging.info(f"[EXTRACT] {f}")
        todo.append(f)
    try:
        results = ensure_features_batch(todo, tracker=track_fn, ctx=ctx) if todo else {}
    except Exception as e:                                        # noqa: BLE001 - nothing could run: every file failed with it
        results = {f: e for f in todo}
    for f in todo:
        if isinstance(results[f], BaseException):
            logging.error(f"[ERROR] Failed to extract {f.name}: {results[f]}")
            done["failed"] += 1
        else:
            done["extracted"] += 1
    logging.info(f"[DONE] Extracted features from {len(files)} files.")
    return done


# -- batched analysis -------------------------------------------------------------------------------------------------
FRAME_BUDGET = 1 << 16     # STFT frames per device pass: ~6 minutes of 44.1 kHz audio, ~0.6 GB of pass scratch at n_fft 1024
WORKERS = 8                # host threads that read wavs and write .goofy files (a fixed default: the host's CPU count is no guide)


def plan_passes(entries, frame_budget=FRAME_BUDGET):
    """Cut ``entries`` = [(key, sr, n_frames)] into device passes [(sr, [key, ...])].  A key seen before is dropped.  Sample
    rates come in the order they first appear; inside a rate the keys keep their input order and are taken greedily while the
    pass stays within ``frame_budget`` frames.  A signal larger than the budget gets a pass of its own."""
    return plan_keyed_passes([(key, int(sr), frames) for key, sr, frames in entries], frame_budget)


def plan_keyed_passes(entries, frame_budget=FRAME_BUDGET):
    """``plan_passes`` with any hashable pass key in place of the sample rate: [(key, pass_key, n_frames)] -> [(pass_key,
    [key, ...])].  Entries share a pass only when their pass keys are equal."""
    if frame_budget < 1:
        raise ValueError("frame_budget must be at least one frame")
    seen, groups = set(), {}
    for key, pass_key, frames in entries:
        if key in seen:
            continue
        seen.add(key)
        groups.setdefault(pass_key, []).append((key, int(frames)))
    passes = []
    for pass_key, members in groups.items():
        cur, used = [], 0
        for key, frames in members:
            if cur and used + frames > frame_budget:
                passes.append((pass_key, cur))
                cur, used = [], 0
            cur.append(key)
            used += frames
        if cur:
            passes.append((pass_key, cur))
    return passes


def per_sample_f0_batch(c, tracks, n_samples, sr, f0_min=75, f0_merge_range=2):
    """``per_sample_f0`` for many tracks of one sample rate -> (per track (f0, voicing mask) or the exception it raised, the
    launch's (f0, mask) buffers or None, {track: (first, end) sample in them}).  Every 1-D track of two frames or more goes
    through one ``Context.per_sample_f0`` launch and gets fp64 device views of its buffers; a one-frame or empty track
    (np.isclose's special case, gf.interp1d's ValueError) or any other shape stays on the host and gets host arrays.
    ``tracks``: fp64 device tensors (the native tracker's) or host arrays."""
    import torch
    out, tracks = [None] * len(tracks), list(tracks)
    dev, host = [], []
    for j, t in enumerate(tracks):
        if isinstance(t, torch.Tensor) and t.dim() == 1 and t.numel() >= 2:
            dev.append(j)
        elif not isinstance(t, torch.Tensor):
            a = np.asarray(t, dtype=np.float64)
            (host if a.ndim != 1 or a.size < 2 else dev).append(j)
            tracks[j] = a
        else:
            host.append(j)
    for j in host:
        try:
            t = tracks[j]
            out[j] = per_sample_f0(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, n_samples[j], sr, f0_min, f0_merge_range)
        except Exception as e:                                    # noqa: BLE001 - per-signal isolation
            out[j] = e
    if dev:
        parts = [tracks[j] for j in dev]
        if isinstance(parts[0], torch.Tensor):
            flat = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
        else:
            flat = c.tensor(np.concatenate(parts))
        f0, mask = c.per_sample_f0(flat, [p.shape[0] for p in parts], [n_samples[j] for j in dev], sr, f0_min, f0_merge_range)
        off = c.offsets([n_samples[j] for j in dev])
        slots = {j: (int(off[q]), int(off[q + 1])) for q, j in enumerate(dev)}
        for j, (a, b) in slots.items():
            out[j] = (f0[a:b], mask[a:b])
        return out, (f0, mask), slots
    return out, None, {}


def analyse_batch(signals, sr, n_fft=1024, hop_length=256, f0_min=75, f0_merge_range=2, tracker=None, ctx=None, want_env=True,
                  timings=None):
    """gf.extract_features (GOOFER.py:940-969) for many signals at one sample rate: one 5-tuple (env_spec fp64 [bins, T], f0
    per sample, voicing mask, formants, env_knots) per signal, or the exception that signal raised (env_spec is None unless
    ``want_env``); a signal's result does not depend on the others.  Envelope and knots on the GPU; tracks from ``tracker``
    (see ``get``).  ``analyse_device`` does the work; this brings its results to the host.  ``timings``, a dict, collects
    seconds under "device" (upload to results on the host) and "host"."""
    import time
    import torch
    t0 = time.perf_counter()
    res = analyse_device(signals, sr, n_fft, hop_length, f0_min, f0_merge_range, tracker=tracker, ctx=ctx, want_env=want_env,
                         want_knots=True)
    out = [None] * len(signals)
    live = [i for i, r in enumerate(res) if not isinstance(r, BaseException)]
    for i, r in enumerate(res):
        if isinstance(r, BaseException):
            out[i] = r
    if not live:
        return out
    pa = res[live[0]]["pass"]
    env = pa["env"].cpu().numpy() if want_env else None
    knots, K = pa["knots"].cpu().numpy(), pa["K"].cpu().numpy()
    f0_host = pa["f0"].cpu().numpy() if pa["f0"] is not None else None
    # the 0 / 1 mask comes over as bytes (an eighth of the fp64 copy) and is widened on the host: the same values
    mask_host = pa["mask"].to(torch.uint8).cpu().numpy().astype(np.float64) if pa["mask"] is not None else None
    t1 = time.perf_counter()
    f_off = pa["f_off"]
    for i in live:
        r = res[i]
        j = r["slot"]
        a, b = int(f_off[j]), int(f_off[j + 1])
        env_knots = knots_pack(knots, K, f_off, j, sr, n_fft, pa["n_bins"])
        env_spec = np.ascontiguousarray(env[a:b].T) if want_env else None
        if r["f0_slot"] is not None:
            s0, s1 = r["f0_slot"]
            f0_s, vmask = f0_host[s0:s1], mask_host[s0:s1]
        else:
            f0_s, vmask = r["f0"], r["mask"]
        out[i] = (env_spec, f0_s, vmask, r["formants"], env_knots)
    if timings is not None:
        timings["device"] = timings.get("device", 0.0) + (t1 - t0)
        timings["host"] = timings.get("host", 0.0) + (time.perf_counter() - t1)
    return out


def knots_pack(knots, K, f_off, j, sr, n_fft, n_bins):
    """Signal j's knots dict (what compress_env_to_knots returns) from ``Context.envelope_knots``' knots [frames, 192] and K
    as host arrays and its frame offsets ``f_off``: the [T, K] slice of its rows, transposed."""
    from . import core
    sr, a, b = int(sr), int(f_off[j]), int(f_off[j + 1])
    T, Kj = b - a, int(K[j])
    vals = knots[a:b].reshape(-1)[:T * Kj].reshape(T, Kj).T
    return {"mode": "knots", "knot_vals_log": np.ascontiguousarray(vals),
            "hz_knots": core.make_mel_knots(sr, n_fft, Kj)[1].astype(np.float32), "n_bins": int(n_bins), "n_fft": int(n_fft),
            "sr": sr}


def analyse_device(signals, sr, n_fft=1024, hop_length=256, f0_min=75, f0_merge_range=2, tracker=None, ctx=None, want_env=True,
                   want_knots=False):
    """The device half of ``analyse_batch``, results left on the device: per signal the exception it raised, or a dict with
    "env" (the sigma-2 envelope, an fp64 [T, bins] device view, frame-major; None unless ``want_env``), "f0" and "mask" (per
    sample, fp64: device views, or host arrays for a one-frame track), "formants" (host dict, fitted to T frames), "T", and
    "pass" / "slot" / "f0_slot" (the shared pass buffers and the signal's place in them).  The envelope and knots of every
    signal come from one ``Context.envelope_knots`` call; with the native tracker one ``Context.track`` call follows on the
    same stream (with a bound native tracker's settings), and its f0 tracks never leave the device.  Any other tracker is called per signal, in order, on the host and
    its tracks uploaded.  Per-sample f0 and voicing come from one ``Context.per_sample_f0`` launch (``per_sample_f0_batch``).
    Only the formant tracks (and with ``want_knots`` nothing else) are waited for.  A bound native tracker whose pitch floor
    lies below ``f0_min`` lowers ``f0_min`` to its floor, so that what it tracks down there counts as voiced."""
    import torch
    from .device import default_context
    track_fn = get(tracker)
    native, settings = native_settings(track_fn)
    sr, hop = int(sr), int(hop_length)
    if settings is not None:
        f0_min = min(f0_min, settings.pitch_floor)               # voiced is f0 > f0_min: a floor below it would be tracked, then masked
    out = [None] * len(signals)
    ys, live = [], []
    for i, y in enumerate(signals):
        y = np.asarray(y)
        refused = (ValueError("analyse_batch: expected a mono signal") if y.ndim != 1 else
                   ValueError("analyse_batch: empty signal") if y.size == 0 else
                   native_refusal(y.size, sr, settings) if native else None)
        if refused is not None:
            out[i] = refused
        else:
            ys.append(y)
            live.append(i)
    if not live:
        return out
    c = (ctx or default_context()).plan(sr, n_fft, hop)
    lengths = [y.size for y in ys]
    y32 = torch.from_numpy(np.concatenate([np.asarray(y, dtype=np.float32) for y in ys])).to(c.device)
    knots, K, f_off, env = c.envelope_knots(y32, lengths, want_env=want_env)
    tracks, formants = [None] * len(ys), [None] * len(ys)
    if native:
        y64 = torch.from_numpy(np.concatenate([np.asarray(y, dtype=np.float64) for y in ys])).to(c.device)
        f0, p_off, forms, m_off = c.track(y64, lengths, sr, hop, settings=settings)
        forms = forms.cpu().numpy()
        for j in range(len(ys)):
            T = int(f_off[j + 1] - f_off[j])
            tracks[j] = f0[p_off[j]:p_off[j + 1]]
            formants[j] = fit_formants({k: forms[m_off[j]:m_off[j + 1], k - 1].tolist() for k in range(1, 6)}, T)
    else:
        for j, y in enumerate(ys):
            T = int(f_off[j + 1] - f_off[j])
            try:
                f0_track, forms_j = track_fn(y, sr, hop, T)
                tracks[j], formants[j] = f0_track, fit_formants(dict(forms_j), T)
            except Exception as e:                                # noqa: BLE001 - per-signal isolation
                tracks[j] = e
    ok = [j for j in range(len(ys)) if not isinstance(tracks[j], BaseException)]
    per, bufs, slots = per_sample_f0_batch(c, [tracks[j] for j in ok], [lengths[j] for j in ok], sr, f0_min, f0_merge_range)
    pa = {"env": env, "knots": knots, "K": K, "f_off": f_off, "n_bins": c.n_bins, "f0": bufs[0] if bufs else None,
          "mask": bufs[1] if bufs else None}
    results = {j: (r, slots.get(q)) for q, (j, r) in enumerate(zip(ok, per))}
    for j, i in enumerate(live):
        r, slot = results.get(j, (tracks[j], None))
        if isinstance(r, BaseException):
            out[i] = r
            continue
        f0_j, mask_j = r
        a, b = int(f_off[j]), int(f_off[j + 1])
        out[i] = {"env": env[a:b] if want_env else None, "f0": f0_j, "mask": mask_j, "formants": formants[j], "T": b - a,
                  "pass": pa, "slot": j, "f0_slot": slot}
    return out


def _read_or_error(path):
    try:
        return read_audio(path)
    except Exception as e:                                        # noqa: BLE001 - reported per file
        return e


def ensure_features_batch(paths, n_fft=1024, hop_length=256, tracker=None, ctx=None, frame_budget=FRAME_BUDGET, workers=WORKERS,
                          timings=None) -> dict:
    """``ensure_features`` for many samples: ``{path: .goofy Path or the exception for that path}`` in input order, each
    path once.  Existing caches are returned untouched.  The wavs are read on ``workers`` threads, grouped by sample rate and
    analysed in device passes of at most ``frame_budget`` STFT frames (``plan_passes``); the ``.goofy`` files are written on
    the same threads, the way ``ensure_features`` writes them.  With the native tracker a file it would refuse (too short,
    sample rate out of range) fails up front with its ValueError and the rest of its group still goes.  The tracker is
    resolved first: TrackerUnavailable is raised for the whole call.  ``timings``, a dict, collects seconds under "read",
    "device", "host" and "write" (waiting for the writes still running after the last pass)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    order = list(dict.fromkeys(paths))
    out, todo = {}, []
    for p in order:
        feat = features_path(p)
        if feat.exists():
            out[p] = feat
        elif not Path(p).exists():
            out[p] = FileNotFoundError(f"{p} not found (and no {feat.name} beside it)")
        else:
            todo.append(p)
    if todo:
        track_fn = get(tracker)
        native, settings = native_settings(track_fn)
        timings = {} if timings is None else timings
        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
            t0 = time.perf_counter()
            audio = {}
            for p, r in zip(todo, pool.map(_read_or_error, todo)):
                if isinstance(r, BaseException):
                    out[p] = r
                    continue
                refused = native_refusal(len(r[0]), r[1], settings) if native else None
                if refused is not None:
                    out[p] = refused
                else:
                    audio[p] = r
            timings["read"] = timings.get("read", 0.0) + time.perf_counter() - t0
            writes = []
            for sr, keys in plan_passes([(p, sr, 1 + len(y) // hop_length) for p, (y, sr) in audio.items()], frame_budget):
                try:
                    res = analyse_batch([audio[p][0] for p in keys], sr, n_fft, hop_length, tracker=track_fn, ctx=ctx, want_env=False,
                                        timings=timings)
                except Exception as e:                            # noqa: BLE001 - the pass failed as a whole: each of its files did
                    res = [e] * len(keys)
                for p, r in zip(keys, res):
                    y_len = len(audio.pop(p)[0])
                    if isinstance(r, BaseException):
                        out[p] = r
                    else:
                        _, f0, vmask, forms, knots = r
                        writes.append((p, pool.submit(_write_features, features_path(p), knots, f0, vmask, forms, sr, y_len)))
            t0 = time.perf_counter()
            for p, fut in writes:
                try:
                    out[p] = fut.result()
                except Exception as e:                            # noqa: BLE001
                    out[p] = e
            timings["write"] = timings.get("write", 0.0) + time.perf_counter() - t0
    return {p: out[p] for p in order}
