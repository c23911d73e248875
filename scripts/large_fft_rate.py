"""Frames per second of core.stft and core.synthesize_batch at n_fft 4096 (the workgroup transform) against 2048 (one wave
per frame), both in one process on one device, after warm-up.

    python scripts/large_fft_rate.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from goofer_amd import core  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = Context(0)
    sr = 96000
    rng = np.random.default_rng(0)
    x = rng.standard_normal(sr * 60).astype(np.float32)            # one minute at 96 kHz
    res = {}
    for n_fft in (2048, 4096):
        hop = n_fft // 4
        frames = 1 + len(x) // hop
        ctx.plan(sr, n_fft, hop)
        dx = ctx.tensor(x)
        off = ctx.tensor(ctx.offsets([len(x)]))
        foff = ctx.tensor(ctx.offsets([frames]))
        t = timed(lambda: ctx.rfft_frames(dx, off, foff, frames), args.steps, args.warmup)
        res[f"stft_{n_fft}_frames_per_s"] = frames / t
        n = sr * 2
        T = 1 + n // hop
        t_ = np.arange(n) / sr
        f0 = 196.0 * 2 ** (0.3 * np.sin(2 * np.pi * 3.1 * t_))
        notes = [dict(env_spec=np.full((n_fft // 2 + 1, T), 0.01, np.float32), f0_interp=f0 * (1 + 0.01 * i),
                      voicing_mask=np.ones(n, np.float32), y=np.empty(n, bool)) for i in range(32)]
        t = timed(lambda: core.synthesize_batch(notes, sr, n_fft, hop, seeds=list(range(32)), ctx=ctx), args.steps, args.warmup)
        res[f"synth_batch_{n_fft}_frames_per_s"] = 32 * T / t
    print(json.dumps({k: round(v, 1) for k, v in res.items()}))
    ctx.close()


if __name__ == "__main__":
    main()
