"""What the look-ahead peak limiter costs: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths laid
end to end with 10 % overlaps), converted from 44.1 to 48 kHz on the device, limited by goofer_limit and timed with HIP events —
beside what a caller does without it: the fp32 track downloaded and limited on the host by the numpy restatement
(tests/limit_ref.py).  The host figure is the baseline, not the code under test.

python scripts/limit_rate.py [--notes 1024] [--reps 20] [--sigma 0.2] [--ceiling C] [--look-ms 5] [--host-samples 200000] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
The limiter's time depends on the values, through the tiles it may copy (option "limit_skip"), so two inputs are timed: the
track as it is (at sigma 0.2 a sample above the ceiling is a five-sigma event: a few tiles of the 11 900 hold one) and the same
track times 2 (one sample in 80 is above: every tile does the full arithmetic).  On each, limit_skip 1 (the default) and 0
alternate round by round in one process.  GB/s is over the 8 bytes per sample the limiter must move (4 in, 4 out); taps/s counts
2W + 1 multiply-adds per sample and is given for the runs in which every tile does the arithmetic.  goofer_rate_convert is
timed on the same track in the same process (a kernel with a comparable tap count per sample).  ``--host-samples`` runs the
restatement on the track's first N samples only and scales its time to the whole track (it is linear in the length); the result
says so.  Prints one JSON line."""
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
import limit_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import limit as LM, phrase as P, rate as RT  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


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
    plan = LM.plan(sr_out, [n], a.ceiling, a.look_ms)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    inputs = {"as_rendered": track, "times_2": track * 2.0}
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)
    nbytes, taps = 8.0 * n, 2 * plan.W + 1
    rounds = {(k, s): [] for k in inputs for s in (1, 0)}
    for k, x in inputs.items():                                 # code objects, plan upload, clocks
        for s in (1, 0):
            ctx.set_option("limit_skip", s)
            for _ in range(2):
                ctx.limit(x, None, plan, out=out)
    for _ in range(3):
        ctx.rate_convert(x_in, None, rplan, out=track)
    torch.cuda.synchronize()
    rate_rounds = []
    for _ in range(5):
        for k, x in inputs.items():
            for s in (1, 0):
                ctx.set_option("limit_skip", s)
                rounds[(k, s)].append(timed(lambda: ctx.limit(x, None, plan, out=out), a.reps))
        rate_rounds.append(timed(lambda: ctx.rate_convert(x_in, None, rplan, out=track), a.reps))
    ctx.set_option("limit_skip", 1)
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "W": plan.W, "taps": taps, "ceiling": plan.ceiling, "sigma": a.sigma,
           "tiles": plan.n_tiles, "MB": round(nbytes / 1e6, 1), "host_plan_ms": round(plan_ms, 2)}
    stats = {}
    for k, x in inputs.items():
        y, peak, gain = ctx.limit(x, None, plan, out=out)
        ctx.check()
        stats[k] = (float(peak.cpu()[0]), float(gain.cpu()[0]))
        above = int((x.abs() > plan.ceiling).sum().item())
        res[k] = {"samples_above_ceiling": above, "peak_in": round(stats[k][0], 4), "min_gain": round(stats[k][1], 4),
                  "max_out": float(y.abs().max().item())}
        for s in (1, 0):
            ms = float(np.median(rounds[(k, s)]))
            res[k]["skip_%d" % s] = {"ms": round(ms, 4), "ms_rounds": [round(v, 4) for v in rounds[(k, s)]], "GB_s": round(nbytes / ms / 1e6, 1),
                                     "G_taps_s_if_every_tile_ran": round(taps * float(n) / ms / 1e6, 1)}
    ms = float(np.median(rate_rounds))
    res["rate_convert_44k1_48k"] = {"ms": round(ms, 4), "taps": 2 * rplan.H, "G_taps_s": round(2.0 * rplan.H * n / ms / 1e6, 1),
                                    "GB_s": round((4.0 * n_in + 4.0 * n) / ms / 1e6, 1)}
    if not a.no_host:
        x = inputs["times_2"]
        y, _, _ = ctx.limit(x, None, plan, out=out)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        ref = limit_ref.limit(xh[:part], plan.taps, plan.W, np.float32(plan.ceiling))[0]
        t2 = time.perf_counter()
        pcm = limit_ref.pcm16(ref)
        t3 = time.perf_counter()
        scale = n / part
        res["host"] = {"input": "times_2", "track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_limit_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "numpy_pcm16_ms": round(1e3 * (t3 - t2) * scale, 1), "numpy_samples": part, "scaled_by": round(scale, 3),
                       "total_ms": round(1e3 * ((t1 - t0) + (t3 - t1) * scale), 1)}
        # the restatement of a prefix differs from the whole track's only where a window reaches past the prefix's end
        keep = part - (2 * plan.W if part < n else 0)
        res["bit_equal"] = bool(len(pcm) == part and np.array_equal(got[:keep].view(np.int32), ref[:keep].view(np.int32)))
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("bit_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
