"""What output-rate conversion costs: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths laid end
to end with 10 % overlaps) converted from 44.1 to 48 kHz by goofer_rate_convert, timed with HIP events — beside what a caller
does without it: the fp32 track downloaded and converted on the host by the numpy restatement (tests/rate_ref.py).  The host
figure is the baseline, not the code under test.

python scripts/convert_rate.py [--notes 1024] [--reps 50] [--rates 44100 48000] [--host-samples N] [--no-host]
The track is random fp32 samples (nothing is rendered or mixed: the converter's time does not depend on the values).  GB/s is
over 4 bytes per input sample + 4 per output sample; taps/s counts 2H multiply-adds per output sample.  The kernel is timed with
its tap table staged in LDS (the default) and, alternating in the same process, read from global memory.  ``--host-samples``
runs the restatement on the track's first N samples only and scales its time to the whole track (the restatement is linear in
the length); the result says so.  Prints one JSON line."""
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
import rate_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import phrase as P, rate as RT  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rates", type=int, nargs=2, default=[44100, 48000], metavar=("IN", "OUT"))
    ap.add_argument("--host-samples", type=int, default=0, help="run the host restatement on this many samples and scale (0: the whole track)")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    entries, lens, sr = phrase(a.notes)
    n = P.plan_phrase(entries, lens, sr).total_out             # the track's length: what render_phrase hands the converter
    sr_in, sr_out = a.rates
    t0 = time.perf_counter()
    plan = RT.plan(sr_in, sr_out, [n])
    plan_ms = 1e3 * (time.perf_counter() - t0)
    g = torch.Generator(device=ctx.device).manual_seed(3)
    x = 0.3 * torch.randn(n, dtype=torch.float32, device=ctx.device, generator=g)
    out = torch.empty(plan.total_out, dtype=torch.float32, device=ctx.device)
    nbytes = 4.0 * n + 4.0 * plan.total_out
    # the table staged in LDS (the default) and read from global memory (option "rate_lds" 0), alternating in one process
    rounds = {1: [], 0: []}
    for lds in (1, 0):                                          # code objects, plan upload, clocks
        ctx.set_option("rate_lds", lds)
        for _ in range(3):
            ctx.rate_convert(x, None, plan, out=out)
    torch.cuda.synchronize()
    for _ in range(5):
        for lds in (1, 0):
            ctx.set_option("rate_lds", lds)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                ctx.rate_convert(x, None, plan, out=out)
            e1.record()
            e1.synchronize()
            rounds[lds].append(e0.elapsed_time(e1) / a.reps)
    ctx.set_option("rate_lds", 1)
    ctx.rate_convert(x, None, plan, out=out)                    # what is compared below: the default path
    ctx.check()
    ms, ms_global = float(np.median(rounds[1])), float(np.median(rounds[0]))
    rounds = rounds[1]
    res = {"notes": a.notes, "sr_in": sr_in, "sr_out": sr_out, "L": plan.L, "M": plan.M, "H": plan.H, "samples_in": n,
           "samples_out": plan.total_out, "MB": round(nbytes / 1e6, 1), "host_plan_ms": round(plan_ms, 2), "convert_ms": round(ms, 4),
           "convert_ms_rounds": [round(v, 4) for v in rounds], "convert_GB_s": round(nbytes / ms / 1e6, 1),
           "G_taps_s": round(2.0 * plan.H * plan.total_out / ms / 1e6, 1), "table_in_global_ms": round(ms_global, 4),
           "table_in_global_GB_s": round(nbytes / ms_global / 1e6, 1)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = out.cpu().numpy()
    res["converted_download_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    if not a.no_host:
        t0 = time.perf_counter()
        xh = x.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        ref = rate_ref.convert(xh[:part], plan.taps, plan.L, plan.M, plan.H)
        t2 = time.perf_counter()
        scale = n / part
        res["host"] = {"track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_convert_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "numpy_samples": part, "scaled_by": round(scale, 3), "total_ms": round(1e3 * ((t1 - t0) + (t2 - t1) * scale), 1)}
        # the restatement of a prefix differs from the whole track's only where a window reaches past the prefix's end
        keep = len(ref) - (rate_ref.margin(plan.L, plan.M, plan.H) if part < n else 0)
        res["bit_equal"] = bool(np.array_equal(got[:keep].view(np.int32), ref[:keep].view(np.int32)))
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("bit_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
