"""The tracker's numpy restatement (tracker_ref.py) at any settings: a private copy of that module, loaded under another name,
with its constants set from a ``TrackerSettings`` (the restatement reads them at call time; tracker_ref itself is not
touched).  Also the settings and signals of tests/test_gpu_tracker_settings.py and the restatement's answers for them, numpy
only, so that they can be computed in worker processes."""
import importlib.util
import os
import sys

import numpy as np

import tracker_cases as C

FIELDS = ("pitch_floor", "pitch_ceiling", "silence_threshold", "voicing_threshold", "octave_cost", "octave_jump_cost",
          "voiced_unvoiced_cost", "max_formant", "n_formants")
DEFAULTS = dict(zip(FIELDS, (75, 950.0, 0.03, 0.45, 0.01, 0.35, 0.14, 5500, 5)))
_LOADED = {}
LONG_WINDOW = 8192


class _Numpy:
    """numpy for the private copies, with one difference: ``correlate(a, a, "full")`` of more than LONG_WINDOW samples.
    numpy's own takes over a minute per call on a 14400-sample window (floor 20 Hz at 96 kHz).  The restatement reads only
    the lags 0 .. W - 1 of it (from index W - 1 on); each is the dot product of the same overlapping slices numpy's correlate
    multiplies, computed here one lag at a time; the negative lags, which nothing reads, are NaN.  At shorter windows
    numpy's correlate runs unchanged (test_tracker_settings.py checks that the two agree to the last bit there)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def correlate(a, v, mode="valid"):
        if len(a) <= LONG_WINDOW:
            return np.correlate(a, v, mode=mode)
        return long_correlate(a, v, mode)


def long_correlate(a, v, mode):
    assert mode == "full" and len(a) == len(v)
    W = len(a)
    out = np.full(2 * W - 1, np.nan)
    for t in range(W):
        out[W - 1 + t] = np.dot(a[t:], v[:W - t])
    return out


def as_dict(settings):
    """A TrackerSettings, a dict of some of its fields, or None -> every field."""
    if settings is None:
        return dict(DEFAULTS)
    if isinstance(settings, dict):
        assert set(settings) <= set(FIELDS), settings
        return {**DEFAULTS, **settings}
    return {k: getattr(settings, k) for k in FIELDS}


def load(settings=None):
    """The restatement with its constants at ``settings``: a module of its own per settings."""
    s = as_dict(settings)
    key = tuple(s[k] for k in FIELDS)
    if key not in _LOADED:
        name = f"tracker_ref_at_settings_{len(_LOADED)}"
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracker_ref.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        m.np = _Numpy()
        m.FLOOR, m.CEILING = int(s["pitch_floor"]), float(s["pitch_ceiling"])
        m.SILENCE, m.VOICING = float(s["silence_threshold"]), float(s["voicing_threshold"])
        m.OCTAVE_COST, m.OCTAVE_JUMP, m.VUV_COST = float(s["octave_cost"]), float(s["octave_jump_cost"]), float(s["voiced_unvoiced_cost"])
        m.FORMANT_SR = 2 * int(s["max_formant"])
        m.FORMANT_WIN = m.FORMANT_SR // 20
        m.N_FORMANTS = int(s["n_formants"])
        m.ORDER = 2 * m.N_FORMANTS
        _LOADED[key] = m
    return _LOADED[key]


# -- the settings matrix of test_gpu_tracker_settings.py: (settings, sr, hop, seconds of the voice) -------------------------
SETTINGS = (
    ({"pitch_floor": 40}, 16000, 128, 0.4),                                    # changed pitch geometry
    ({"pitch_floor": 40}, 96000, 512, 0.3),                                    # LDS above 64 KB
    ({"pitch_floor": 20}, 96000, 512, 0.3),                                    # the largest admitted frame, ~153 KB
    ({"pitch_floor": 150, "pitch_ceiling": 1500.0}, 8000, 64, 0.4),            # W = 160 < workgroup, small lags
    ({"pitch_ceiling": 6000.0}, 8000, 100, 0.4),                               # clamp to sr / 2, min_lag = 2
    ({"silence_threshold": 0.1, "voicing_threshold": 0.6, "octave_cost": 0.03, "octave_jump_cost": 0.5,
      "voiced_unvoiced_cost": 0.2}, 22050, 256, 0.4),                          # thresholds and costs as arguments
    ({"max_formant": 5000, "n_formants": 4}, 44100, 256, 0.4),                 # rate 10000, window 500, order 8
    ({"max_formant": 8000, "n_formants": 5}, 44100, 441, 0.4),                 # window 800, 13 slots per lane
    ({"max_formant": 8000, "n_formants": 3}, 8000, 64, 0.4),                   # upsampling resample, order 6
)


def signals(settings, sr, hop, dur):
    """{name: signal} for one row of SETTINGS: a voice, a glide from just above the floor to just below the ceiling, the
    segments signal (voice, silence, noise, voice) and the two length edges, one pitch window and one sample short of a
    formant window."""
    s = as_dict(settings)
    M = load(s)
    rng = np.random.default_rng(sr + 7 * hop)
    t = np.arange(int(dur * sr)) / sr
    lo, hi = s["pitch_floor"] * 76.0 / 75.0, min(s["pitch_ceiling"], 0.5 * sr) * 940.0 / 950.0
    v = C.voice(sr, dur, 3)                                                    # longer than any admitted pitch window (150 ms)
    q = dur / 4
    n_win = -(-M.FORMANT_WIN * sr // M.FORMANT_SR)                             # the fewest samples with a formant window
    return {"voice": v,
            "glide": C.harmonic(sr, lo * (hi / lo) ** (t / dur), 1),
            "segments": np.concatenate([C.voice(sr, 1.5 * q, 1), np.zeros(int(0.5 * q * sr)), 0.05 * rng.standard_normal(int(0.5 * q * sr)),
                                        C.voice(sr, 1.5 * q, 2)]),
            "len_min": v[:M.min_length(sr)],
            "len_win-1": v[:n_win - 1]}


def matrix():
    """[(settings, sr, hop, name, signal)] over SETTINGS."""
    return [(st, sr, hop, name, y) for st, sr, hop, dur in SETTINGS for name, y in signals(st, sr, hop, dur).items()]


def restate(case):
    """The restatement's answers for one case, stage by stage with its fragility flags (tracker_cases.restate at settings).
    A signal shorter than a pitch window has the formant stages only."""
    settings, sr, hop, _, y = case
    M = load(settings)
    out = {"pitch": len(y) >= M.min_length(sr)}
    if out["pitch"]:
        cands, frag, peaks = M.pitch_candidates(y, sr, hop)
        f0, _, vfrag = M.viterbi_diag(cands, 0.01 * sr / hop)
        out.update(cands=cands, cand_fragile=frag, peaks=peaks, f0=f0, path_fragile=vfrag)
    x = M.resample(y, sr)
    forms, ffrag = M.formants_of_11k(x, sr, hop)
    out.update(x11=x, formants=forms, formant_fragile=ffrag)
    return out
