"""What true-peak detection costs: the track of scripts/limit_rate.py (scripts/phrase_rate.py's workload converted from 44.1 to
48 kHz on the device), metered by goofer_true_peak and limited by goofer_limit_tp, timed with HIP events — beside goofer_limit
in the same process, and beside what a caller does without them: the fp32 track downloaded, metered and limited on the host by
the numpy restatement (tests/true_peak_ref.py).  The host figure is the baseline, not the code under test.

python scripts/true_peak_rate.py [--notes 1024] [--reps 20] [--sigma 0.2] [--ceiling C] [--look-ms 5] [--host-samples 200000] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
The limiter's time depends on the values, through the tiles it may copy (option "limit_tp_skip"), so two inputs are timed, as in
limit_rate.py: the track as it is and the same track times 2.  On each, limit_tp_skip 1 (the default) and 0 alternate round by
round in one process, and goofer_limit (limit_skip 1) runs in the same rounds.  The meter always computes.  Structurally, 24 taps
for each of the R - 1 = 3 phases (72 multiply-adds per sample, 81 with the ninth interval a thread of eight samples makes again)
sit in front of the limiter's 2W + 1 = 481-tap sum; a true-peak tile can copy only behind them, and fewer tiles may: one copies
when the oversampled envelope stays under the ceiling, not the samples.  GB/s is over the bytes a kernel must move: 8 per sample
for a limiter (4 in, 4 out), 4 for the meter.  ``--host-samples`` runs the restatement on the track's first N samples only and
scales its time to the whole track (it is linear in the length); the result says so.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(REPO, "scripts"))
import true_peak_ref  # noqa: E402
from limit_rate import timed  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import limit as LM, phrase as P, rate as RT  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.2)
    ap.add_argument("--ceiling", type=float, default=LM.CEILING)
    ap.add_argument("--look-ms", type=float, default=LM.LOOK_MS)
    ap.add_argument("--host-samples", type=int, default=200000, help="run the host restatement on this many samples and scale (0: the whole track)")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    entries, lens, sr = phrase(a.notes)
    n_in = P.plan_phrase(entries, lens, sr).total_out          # the mixed track's length at the voicebank's rate
    sr_out = 48000
    rplan = RT.plan(sr, sr_out, [n_in])
    g = torch.Generator(device=ctx.device).manual_seed(3)
    x_in = a.sigma * torch.randn(n_in, dtype=torch.float32, device=ctx.device, generator=g)
    track = ctx.rate_convert(x_in, None, rplan)                 # what render_phrase(out_sr=48000) hands the limiter
    n = rplan.total_out
    t0 = time.perf_counter()
    plan = LM.plan(sr_out, [n], a.ceiling, a.look_ms, true_peak=True)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    plain = LM.plan(sr_out, [n], a.ceiling, a.look_ms)
    inputs = {"as_rendered": track, "times_2": track * 2.0}
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)
    kinds = ("tp_skip_1", "tp_skip_0", "sample_peak", "meter")

    def run(kind, x):
        if kind == "meter":
            return ctx.true_peak(x, None, plan)
        if kind == "sample_peak":
            return ctx.limit(x, None, plain, out=out)
        ctx.set_option("limit_tp_skip", 1 if kind == "tp_skip_1" else 0)
        return ctx.limit(x, None, plan, out=out)
    rounds = {(k, kind): [] for k in inputs for kind in kinds}
    for k, x in inputs.items():                                 # code objects, plan uploads, clocks
        for kind in kinds:
            for _ in range(2):
                run(kind, x)
    torch.cuda.synchronize()
    for _ in range(5):
        for k, x in inputs.items():
            for kind in kinds:
                rounds[(k, kind)].append(timed(lambda: run(kind, x), a.reps))
    ctx.set_option("limit_tp_skip", 1)
    taps, tp_taps = 2 * plan.W + 1, (plan.R - 1) * 2 * plan.Z
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "W": plan.W, "taps": taps, "R": plan.R, "tp_taps_per_sample": tp_taps,
           "ceiling": plan.ceiling, "sigma": a.sigma, "tiles": plan.n_tiles, "MB_limiter": round(8.0 * n / 1e6, 1), "host_plan_ms": round(plan_ms, 2)}
    for k, x in inputs.items():
        y, peak, gain = ctx.limit(x, None, plan, out=out)
        tp_out = ctx.true_peak(y, None, plan)
        ctx.check()
        res[k] = {"samples_above_ceiling": int((x.abs() > plan.ceiling).sum().item()), "true_peak_in": round(float(peak.cpu()[0]), 4),
                  "min_gain": round(float(gain.cpu()[0]), 4), "true_peak_out_over_c_minus_1": float(tp_out.cpu()[0]) / plan.ceiling - 1.0}
        for kind in kinds:
            ms = float(np.median(rounds[(k, kind)]))
            nbytes = (4.0 if kind == "meter" else 8.0) * n
            res[k][kind] = {"ms": round(ms, 4), "ms_rounds": [round(v, 4) for v in rounds[(k, kind)]], "GB_s": round(nbytes / ms / 1e6, 1)}
        res[k]["meter"]["G_taps_s"] = round(tp_taps * float(n) / res[k]["meter"]["ms"] / 1e6, 1)
    if not a.no_host:
        x = inputs["times_2"]
        y, peak, _ = ctx.limit(x, None, plan, out=out)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        top = true_peak_ref.true_peak(xh[:part], plan.tp_taps)
        t2 = time.perf_counter()
        ref = true_peak_ref.limit(xh[:part], plan.taps, plan.W, np.float32(plan.ceiling), plan.tp_taps)[0]
        t3 = time.perf_counter()
        scale = n / part
        res["host"] = {"input": "times_2", "track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_true_peak_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "numpy_limit_tp_ms": round(1e3 * (t3 - t2) * scale, 1), "numpy_samples": part, "scaled_by": round(scale, 3)}
        # the restatement of a prefix differs from the whole track's only where a window reaches past the prefix's end
        keep = part - (2 * plan.W + plan.Z if part < n else 0)
        res["bit_equal"] = bool(np.array_equal(got[:keep].view(np.int32), ref[:keep].view(np.int32)))
        if part == n:
            res["bit_equal"] = res["bit_equal"] and float(top) == float(peak.cpu()[0])
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("bit_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
