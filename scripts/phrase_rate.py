"""What phrase assembly costs: BASELINE config 3's note lengths laid end to end with 10 % overlaps and mixed into one track by
goofer_phrase_mix, timed with HIP events — beside what a caller does without it: every note downloaded, then enveloped and
summed on the host by the numpy restatement (tests/phrase_ref.py, vectorised per note).  The host figure is the baseline, not
the code under test.

python scripts/phrase_rate.py [--notes 1024] [--reps 200] [--no-host]
The notes are random fp32 samples (nothing is rendered).  GB/s is over the bytes the mix must move: 4 per used source sample
(the effective takes) + 4 per track sample.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import phrase_ref  # noqa: E402
from goofer_amd import phrase as P, synthetic as syn  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def phrase(n_notes):
    """config 3's notes (synthetic.config_note_frames: 100 ms of consonant + the request's 1000 ms at 44.1 kHz) as a phrase: each
    note overlaps the one before by a tenth of its length, fading in over the overlap"""
    geo = syn.config_geometry(3)
    sr = geo["sr"]
    n = int(100.0 / 1000.0 * sr) + int(1000.0 / 1000.0 * sr)
    ms = n * 1000.0 / sr
    ovr = ms / 10.0
    entries = [P.Entry(ms, (5.0, ovr - 5.0, ovr, 0.0, 100.0, 100.0, 0.0, ovr if i else 0.0)) for i in range(n_notes)]
    return entries, [n] * n_notes, sr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    entries, lens, sr = phrase(a.notes)
    t0 = time.perf_counter()
    plan = P.plan_phrase(entries, lens, sr)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    g = torch.Generator(device=ctx.device).manual_seed(3)
    x = 0.3 * torch.randn(sum(lens), dtype=torch.float32, device=ctx.device, generator=g)
    d_off = ctx.tensor(ctx.offsets(lens))
    out = torch.empty(plan.total_out, dtype=torch.float32, device=ctx.device)
    eff = sum(hi - lo for lo, hi in (phrase_ref.effective(r, n, plan.total_out) for r, n in zip(plan.notes, lens)))
    nbytes = 4.0 * eff + 4.0 * plan.total_out
    for _ in range(5):                                          # code object, plan upload, clocks
        ctx.phrase_mix(x, d_off, plan, out=out)
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ctx.phrase_mix(x, d_off, plan, out=out)
        e1.record()
        e1.synchronize()
        rounds.append(e0.elapsed_time(e1) / a.reps)
    ctx.check()
    ms = float(np.median(rounds))
    res = {"notes": a.notes, "samples_in": int(sum(lens)), "track_samples": plan.total_out, "tiles": len(plan.tile_off) - 1,
           "cover_entries": int(len(plan.tile_notes)), "MB": round(nbytes / 1e6, 1), "host_plan_ms": round(plan_ms, 2),
           "mix_ms": round(ms, 4), "mix_ms_rounds": [round(v, 4) for v in rounds], "mix_GB_s": round(nbytes / ms / 1e6, 1)}
    # one download of the track (what is left to cross PCIe) against the download of every note
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = out.cpu().numpy()
    res["track_download_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    if not a.no_host:
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t1 = time.perf_counter()
        xs = [xh[o:o + n] for o, n in zip(ctx.offsets(lens)[:-1], lens)]
        ref, B, D = phrase_ref.mix(xs, plan.notes, plan.total_out)
        t2 = time.perf_counter()
        res["host"] = {"notes_download_ms": round(1e3 * (t1 - t0), 2), "numpy_mix_ms": round(1e3 * (t2 - t1), 2),
                       "total_ms": round(1e3 * (t2 - t0), 2)}
        err, lim = np.abs(got.astype(np.float64) - ref), phrase_ref.bound(B, D)
        res["worst_error_over_bound"] = round(float(np.max(err / np.maximum(lim, 1e-300))), 3)
        res["within_bound"] = bool(np.all(err <= lim))
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
