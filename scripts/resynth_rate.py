"""Wav-to-wav resynthesis rate: three ways to run the reference's extract_features -> synthesize flow over seeded synthetic clips,
two variants per clip, native tracker.

python scripts/resynth_rate.py [--clips 256] [--min-s 0.5] [--max-s 3.0] [--seed 0] [--repeat 2]
  loop     core.extract_features + core.synthesize per clip and variant
  batch    core.extract_features_batch, then core.synthesize_batch over every (clip, variant) note
  resynth  core.resynthesize_batch (features stay on the device)
for the first 16 and all clips, plain and with stretch_factor=1.3 on every other clip's second variant.  Prints one JSON line:
audio-seconds per second (output audio) per path, batch size and case (best of --repeat runs; the loop runs once)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import core  # noqa: E402
from goofer_amd.device import Context  # noqa: E402

SR, N_FFT, HOP = 44100, 1024, 256


def make_clips(n, lo, hi, seed):
    """Harmonic tones with a vibrato and breath noise, lo..hi seconds each (the voicebank of analyse_rate.py)."""
    rng = np.random.default_rng(seed)
    clips = []
    for _ in range(n):
        m = int(rng.uniform(lo, hi) * SR)
        t = np.arange(m) / SR
        f0 = rng.uniform(90, 400) * 2.0 ** (0.03 * np.sin(2 * np.pi * 5.5 * t))
        ph = 2 * np.pi * np.cumsum(f0) / SR
        y = sum(np.sin(h * ph) * rng.uniform(0.2, 1.0) / h for h in range(1, 16))
        clips.append(0.4 * y / np.max(np.abs(y)) + 0.01 * rng.standard_normal(m))
    return clips


def variants_for(case, i):
    second = {"pitch_shift": 1.25, "formant_shift": 0.95}
    if case == "stretch" and i % 2:
        second["stretch_factor"] = 1.3
    return [{}, second]


def run_loop(clips, case, seeds, ctx):
    for i, y in enumerate(clips):
        env, f0, mask, forms, _ = core.extract_features(y, SR, N_FFT, HOP, pitch_tracker="native", ctx=ctx)
        for v, var in enumerate(variants_for(case, i)):
            core.synthesize(env, f0, mask, y, SR, N_FFT, HOP, formants=forms, **var, seed=seeds[2 * i + v], ctx=ctx)


def run_batch(clips, case, seeds, ctx):
    feats = core.extract_features_batch(clips, SR, N_FFT, HOP, pitch_tracker="native", ctx=ctx)
    notes = []
    for i, (y, f) in enumerate(zip(clips, feats)):
        env, f0, mask, forms, _ = f
        for var in variants_for(case, i):
            notes.append({"env_spec": env, "f0_interp": f0, "voicing_mask": mask, "y": y, "formants": forms, **var})
    core.synthesize_batch(notes, SR, N_FFT, HOP, seeds=seeds[:len(notes)], ctx=ctx)


def run_resynth(clips, case, seeds, ctx):
    if case == "plain":
        core.resynthesize_batch(clips, SR, N_FFT, HOP, pitch_tracker="native", variants=variants_for(case, 0),
                                seeds=seeds[:2 * len(clips)], ctx=ctx)
    else:                                                       # the stretched variant on every other clip: two calls
        for par in (0, 1):
            sub = clips[par::2]
            core.resynthesize_batch(sub, SR, N_FFT, HOP, pitch_tracker="native", variants=variants_for(case, par),
                                    seeds=seeds[:2 * len(sub)], ctx=ctx)


def timed(fn, repeat):
    best = float("inf")
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--max-s", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    ctx = Context(0).plan(SR, N_FFT, HOP)
    clips = make_clips(a.clips, a.min_s, a.max_s, a.seed)
    seeds = list(range(2 * len(clips)))
    for fn in (run_loop, run_batch, run_resynth):                # warm-up: library load, plans, allocator, the tracker
        fn(clips[:3], "stretch", seeds, ctx)
    res = {"metric": "resynth_rate", "clips": len(clips), "variants": 2, "audio_s": round(sum(len(y) for y in clips) / SR, 2)}
    for case in ("plain", "stretch"):
        for size in sorted({16, len(clips)}):
            sub = clips[:size]
            audio = sum(len(y) * sum(v.get("stretch_factor", 1.0) for v in variants_for(case, i)) for i, y in enumerate(sub)) / SR
            t = {"loop": timed(lambda: run_loop(sub, case, seeds, ctx), 1),
                 "batch": timed(lambda: run_batch(sub, case, seeds, ctx), a.repeat),
                 "resynth": timed(lambda: run_resynth(sub, case, seeds, ctx), a.repeat)}
            res[f"{case}_{size}"] = {**{f"{k}_audio_s_s": round(audio / v, 1) for k, v in t.items()},
                                     "resynth_vs_loop": round(t["loop"] / t["resynth"], 2),
                                     "resynth_vs_batch": round(t["batch"] / t["resynth"], 2)}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
