"""What the parametric equaliser costs: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths laid end
to end with 10 % overlaps), converted from 44.1 to 48 kHz on the device, through goofer_eq with 1, 2, 4 and 8 bands, each timed
with HIP events — beside goofer_loudness_measure, goofer_loudness_apply and goofer_compress on the same track in the same
process (a 2-band equaliser does the recurrence work of goofer_loudness_measure and writes the signal once as
goofer_loudness_apply does), and beside what a caller does without it: the fp32 track downloaded and filtered on the host by
the numpy restatement (tests/eq_ref.py, sequential float64).  The host figure is the baseline, not the code under test.

python scripts/eq_rate.py [--notes 1024] [--reps 20] [--sigma 0.2] [--host-samples 200000] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
GB/s is over the bytes the call must move, 12 per sample: two reads and a write.  goofer_eq is three launches (k_eq_tile<false>,
k_eq_carry, k_eq_tile<true>); for the share of each, run this script with --no-host under ``rocprofv3 --kernel-trace --stats``.
``--host-samples`` runs the restatement on the track's first N samples only and scales its time to the whole track (it is linear
in the length); the result says so.  Those samples and as many at the track's end are compared with the restatement.  Prints
one JSON line."""
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
import eq_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import compress as CP, eq as EQ, loudness as LD, phrase as P, rate as RT  # noqa: E402
from goofer_amd.device import Context  # noqa: E402

BANDS = {1: "hp:80", 2: "hp:80,peak:3000:3:1", 4: "hp:80,ls:200:3,peak:3000:3:1,hs:10000:4",
         8: "hp:80,ls:200:3,peak:600:-4:1.5,peak:3000:3:1,peak:7000:-6:4,hs:10000:4,lp:18000,hp:120:0:2"}


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
    track = ctx.rate_convert(x_in, None, rplan)                 # what render_phrase(out_sr=48000) hands the equaliser
    n = rplan.total_out
    plans, plan_ms = {}, {}
    for K, spec in BANDS.items():
        t0 = time.perf_counter()
        plans[K] = EQ.plan(sr_out, [n], spec)
        plan_ms[K] = 1e3 * (time.perf_counter() - t0)
        assert plans[K].K == K
    lplan, cplan = LD.plan(sr_out, [n]), CP.plan(sr_out, [n], "-24:3")
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)
    ones = torch.ones(1, dtype=torch.float32, device=ctx.device)
    d_in = lplan.device_tables(ctx)[0]

    def measure():
        return ctx.loudness(track, None, lplan)

    def apply():                                                # goofer_loudness_apply alone, on a gain that is there already
        ctx._check(ctx.lib.goofer_loudness_apply(ctx.h, track.data_ptr(), d_in.data_ptr(), 1, n, ones.data_ptr(), out.data_ptr(), ctx._stream()))

    def compress():
        return ctx.compress(track, None, cplan, out=out)
    fns = {"loudness_measure": measure, "loudness_apply": apply, "compress": compress}
    for K in BANDS:
        fns["eq_%d" % K] = (lambda K: lambda: ctx.eq(track, None, plans[K], out=out))(K)
    for fn in fns.values():                                     # code objects, plan uploads, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            rounds[k].append(timed(fn, a.reps))
    ctx.check()
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "tiles": plans[1].n_tiles, "MB_track": round(4.0 * n / 1e6, 1), "sigma": a.sigma,
           "bands": BANDS, "host_plan_ms": {str(K): round(v, 2) for K, v in plan_ms.items()}}
    moved = {"loudness_measure": 8.0 * n, "loudness_apply": 8.0 * n, "compress": 16.0 * n}
    for k, v in rounds.items():
        ms = float(np.median(v))
        res[k] = {"ms": round(ms, 4), "ms_rounds": [round(t, 4) for t in v], "GB_s": round(moved.get(k, 12.0 * n) / ms / 1e6, 1)}
    res["eq_2_over_loudness_measure_plus_apply"] = round(res["eq_2"]["ms"] / (res["loudness_measure"]["ms"] + res["loudness_apply"]["ms"]), 3)
    if not a.no_host:
        K = 2
        y = ctx.eq(track, None, plans[K], out=out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh = track.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        want = eq_ref.cascade(xh[:part], plans[K].coef, np.float64)
        t2 = time.perf_counter()
        scale = n / part
        res["host"] = {"track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_eq_2_ms": round(1e3 * (t2 - t1) * scale, 1), "numpy_samples": part,
                       "scaled_by": round(scale, 3), "total_ms": round(1e3 * ((t1 - t0) + (t2 - t1) * scale), 1)}
        got = y.cpu().numpy()
        err = eq_ref.error(got[:part], want)
        # the track's end, where the state has come through every tile: the restatement from zero far enough ahead of the window
        warm = int(np.ceil(-110.0 * np.log(10.0) / np.log(eq_ref.pole_radius(plans[K].coef))))
        if n > part + warm:
            tail = eq_ref.cascade(xh[n - part - warm:], plans[K].coef, np.float64)[warm:]
            err = max(err, eq_ref.error(got[n - part:], tail))
            res["host"]["end_window_run_in"] = warm
        res["worst_error_over_peak"] = err
        res["within_bound"] = bool(err <= eq_ref.TOL)
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
