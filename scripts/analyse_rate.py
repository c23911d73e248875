"""Voicebank preparation rate: folder analysis per file (ensure_features in a loop) against the batched path
(ensure_features_batch), both with the native tracker, over fresh copies of one seeded synthetic voicebank.

python scripts/analyse_rate.py [--files 512] [--extra48 16] [--min-s 0.3] [--max-s 3.0] [--seed 0]
Prints one JSON line: files/s and audio-seconds/s of both paths, and for the batched one its time split into reading,
device passes (host clock around a synchronise), host f0 post-processing and waiting for the writes."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import trackers  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def write_bank(root: Path, files: int, extra48: int, lo: float, hi: float, seed: int) -> float:
    """files wavs at 44.1 kHz and extra48 at 48 kHz of lo..hi seconds each (harmonic tone + breath noise); audio seconds."""
    rng = np.random.default_rng(seed)
    total = 0.0
    for i in range(files + extra48):
        sr = 44100 if i < files else 48000
        n = int(rng.uniform(lo, hi) * sr)
        t = np.arange(n) / sr
        f0 = rng.uniform(90, 400) * 2.0 ** (0.03 * np.sin(2 * np.pi * 5.5 * t))
        ph = 2 * np.pi * np.cumsum(f0) / sr
        y = sum(np.sin(h * ph) * rng.uniform(0.2, 1.0) / h for h in range(1, 16))
        y = 0.4 * y / np.max(np.abs(y)) + 0.01 * rng.standard_normal(n)
        with wave.open(str(root / f"s{i:04d}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
            w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
        total += n / sr
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--extra48", type=int, default=16)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--max-s", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    ctx = Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "bank"
        src.mkdir()
        audio_s = write_bank(src, a.files, a.extra48, a.min_s, a.max_s, a.seed)
        n_files = a.files + a.extra48
        # warm-up outside the clock: plans, kernels, the tracker's first call
        warm = Path(tmp) / "warm"
        shutil.copytree(src, warm)
        for f in sorted(warm.glob("*.wav"))[:2] + sorted(warm.glob("*.wav"))[-1:]:
            trackers.ensure_features(f, tracker="native", ctx=ctx)
        trackers.ensure_features_batch(sorted(warm.glob("*.wav"))[2:8], tracker="native", ctx=ctx)

        per = Path(tmp) / "per_file"
        shutil.copytree(src, per)
        t0 = time.perf_counter()
        for f in sorted(per.glob("*.wav")):
            trackers.ensure_features(f, tracker="native", ctx=ctx)
        per_s = time.perf_counter() - t0

        bat = Path(tmp) / "batched"
        shutil.copytree(src, bat)
        timings = {}
        t0 = time.perf_counter()
        res = trackers.ensure_features_batch(sorted(bat.glob("*.wav")), tracker="native", ctx=ctx, timings=timings)
        bat_s = time.perf_counter() - t0
        failed = sum(isinstance(v, BaseException) for v in res.values())
    out = {"files": n_files, "audio_s": round(audio_s, 3),
           "per_file": {"wall_s": per_s, "files_per_s": n_files / per_s, "audio_s_per_s": audio_s / per_s},
           "batched": {"wall_s": bat_s, "files_per_s": n_files / bat_s, "audio_s_per_s": audio_s / bat_s, "failed": failed,
                       "split_s": {k: round(v, 4) for k, v in timings.items()}},
           "speedup": per_s / bat_s}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
