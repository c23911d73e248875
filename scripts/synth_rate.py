"""Library synthesis rate: core.synthesize in a loop against core.synthesize_batch, over seeded synthetic clips.

python scripts/synth_rate.py [--clips 256] [--min-s 0.5] [--max-s 3.0] [--seed 0] [--repeat 2]
Builds clips of min-s..max-s seconds from goofer_amd/synthetic.py (knot envelopes decoded once, outside the clock), then times
both paths for the first 1, 16 and all clips, plain and with stretch_factor=1.3 on every other clip.  Prints one JSON line:
clips/s and audio-seconds/s per path, batch size and case (best of --repeat runs)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import core, synthetic as syn  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def make_clips(n, lo, hi, seed, ctx):
    rng = np.random.default_rng(seed)
    clips = []
    for i in range(n):
        s = syn.make_source(seed * 100003 + i, seconds=float(rng.uniform(lo, hi)))
        env = core.decode_env_from_knots(s["env_pack"], ctx=ctx)
        clips.append({"env_spec": env, "f0_interp": s["f0"] * np.float32(rng.uniform(0.6, 1.6)), "voicing_mask": s["mask"],
                      "y": np.zeros(s["y_len"], dtype=np.float32), "formants": s["formants"],
                      "pitch_shift": float(rng.uniform(0.8, 1.25)), "formant_shift": float(rng.uniform(0.9, 1.1))})
    ctx.plan(44100, 1024, 256)
    return clips


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
    ctx = Context(0).plan(44100, 1024, 256)
    clips = make_clips(a.clips, a.min_s, a.max_s, a.seed, ctx)
    seeds = list(range(len(clips)))
    core.synthesize_batch(clips[:4], 44100, seeds=seeds[:4], ctx=ctx)          # warm-up: library load, plan, allocator
    res = {"metric": "synth_rate", "clips": len(clips), "audio_s": round(sum(len(c["y"]) for c in clips) / 44100.0, 2)}
    for case in ("plain", "stretch"):
        notes = [dict(c, stretch_factor=1.3) if case == "stretch" and i % 2 else c for i, c in enumerate(clips)]
        for size in sorted({1, 16, len(notes)}):
            sub = notes[:size]
            audio = sum(len(c["y"]) * (1.3 if c.get("stretch_factor", 1.0) != 1.0 else 1.0) for c in sub) / 44100.0
            t_loop = timed(lambda: [core.synthesize(**c, sr=44100, seed=s, ctx=ctx) for c, s in zip(sub, seeds)], a.repeat)
            t_batch = timed(lambda: core.synthesize_batch(sub, 44100, seeds=seeds[:size], ctx=ctx), a.repeat)
            res[f"{case}_{size}"] = {"loop_clips_s": round(size / t_loop, 1), "loop_audio_s_s": round(audio / t_loop, 1),
                                     "batch_clips_s": round(size / t_batch, 1), "batch_audio_s_s": round(audio / t_batch, 1),
                                     "speedup": round(t_loop / t_batch, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
