"""Seconds of audio the native tracker analyses per second of wall time, pitch and formant stages timed apart.

python scripts/tracker_rate.py [--signals 64] [--seconds 1.0] [--sr 44100] [--hop 256] [--reps 5]
Prints one JSON line.  The batch is ground-truth-like signals (harmonics through five resonators) of equal length."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd.device import Context, _host, _ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Context(0)
    n = int(a.seconds * a.sr)
    t = np.arange(n) / a.sr
    rng = np.random.default_rng(0)
    sig = []
    for k in range(a.signals):
        f0 = rng.uniform(90, 300) * 2.0 ** (0.04 * np.sin(2 * np.pi * 5.0 * t))
        ph = 2 * np.pi * np.cumsum(f0) / a.sr
        sig.append(sum(np.cos(h * ph) / h for h in range(1, 20)))
    y = torch.as_tensor(np.concatenate(sig)).to(ctx.device)
    off = ctx.offsets([n] * a.signals)
    times = {}
    for name, fn, width in (("pitch", ctx.lib.goofer_track_pitch, 1), ("formants", ctx.lib.goofer_track_formants, 5)):
        f_off = np.zeros(a.signals + 1, dtype=np.int64)
        # the first call (the helper's) warms up; the timed ones reuse its output and scratch
        _, call = ctx._scratch_call(fn, (_ptr(y), _host(off), a.signals, a.sr, a.hop, _host(f_off)),
                                    [lambda: torch.empty((int(f_off[-1]), width), dtype=torch.float64, device=ctx.device)])
        best = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        times[name] = {"median_s": float(np.median(best)), "frames": int(f_off[-1])}
    audio = a.signals * a.seconds
    res = {"signals": a.signals, "seconds_each": a.seconds, "sr": a.sr, "hop": a.hop,
           "pitch_audio_s_per_s": audio / times["pitch"]["median_s"], "formant_audio_s_per_s": audio / times["formants"]["median_s"],
           "both_audio_s_per_s": audio / (times["pitch"]["median_s"] + times["formants"]["median_s"]), "stages": times}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
