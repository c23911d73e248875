"""What a seeded ``synthesize_batch`` costs: 256 clips with ``f0_jitter``, ``volume_jitter`` and ``add_subharm`` with
``subharm_f0_jitter`` (four legacy streams per clip), their normals drawn on the device from each clip's seed (``noise_seeds``:
goofer_legacy_normal_jobs) against the same call with the host drawing them — ``np.random.seed(s)`` and four
``np.random.randn(n)`` per clip in ``core._prepare_note``, uploaded as fp64 — in one process.

python scripts/synth_seeded_rate.py [--clips 256] [--repeat 2]
Per variant, best of --repeat: "prepare" (the per-clip host half: checks, draws) and "run" (uploads, device passes, stems back on
the host), in milliseconds; then how far the two renders are apart.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import core, synthetic as syn  # noqa: E402
from goofer_amd.device import Context  # noqa: E402

SR, N_FFT, HOP = 44100, 1024, 256
KW = dict(f0_jitter=True, f0_jitter_strength=0.8, volume_jitter=True, volume_jitter_strength_harm=0.5, volume_jitter_strength_breath=1.0,
          add_subharm=True, subharm_f0_jitter=0.6)


def clips(n):
    from oracle import goofer_ref as R
    rng = np.random.default_rng(5)
    notes = []
    for i in range(n):
        src = syn.make_source(9000 + i, seconds=float(rng.uniform(0.3, 1.2)))
        env = np.ascontiguousarray(R.decode_env_from_knots(src["env_pack"]), dtype=np.float32)
        notes.append({"env_spec": env, "f0_interp": 220.0 * src["mask"], "voicing_mask": src["mask"], "y": np.empty(src["y_len"], bool),
                      "formants": src["formants"]})
    return notes


def render(c, notes, legacy, on_host, repeat):
    merged = {**core._synth_defaults(), **KW}
    best, res = None, None
    for _ in range(repeat + 1):                                 # the first pass warms the allocator and the plan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jobs = []
        for i, note in enumerate(notes):
            if on_host:
                np.random.seed(legacy[i])
            kw = {**merged, "formants": note["formants"]}
            jobs.append(core._prepare_note(c, note, kw, i, None, SR, N_FFT, HOP, 100 + i, None if on_host else legacy[i]))
        t1 = time.perf_counter()
        res = [None] * len(jobs)
        core._render(c, jobs, res, SR)
        c.check()
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    return {"total_ms": round(best[0] * 1e3, 2), "prepare_ms": round(best[1] * 1e3, 2), "run_ms": round(best[2] * 1e3, 2)}, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    c = Context(0).plan(SR, N_FFT, HOP)
    notes = clips(a.clips)
    legacy = [(40503 * (i + 1)) % 2 ** 32 for i in range(a.clips)]
    out = {"metric": "synth_seeded_rate", "clips": a.clips, "samples": int(sum(len(n["y"]) for n in notes)), "rocm": torch.version.hip,
           "device": torch.cuda.get_device_name(0)}
    state = np.random.get_state()
    out["device_draws"], dev = render(c, notes, legacy, False, a.repeat)
    out["host_draws"], host = render(c, notes, legacy, True, a.repeat)
    np.random.set_state(state)
    out["rec_max_abs_diff"] = max(float(np.abs(d[0] - h[0]).max()) for d, h in zip(dev, host))
    out["host_over_device"] = round(out["host_draws"]["total_ms"] / out["device_draws"]["total_ms"], 2)
    print(json.dumps(out))
    c.close()


if __name__ == "__main__":
    main()
