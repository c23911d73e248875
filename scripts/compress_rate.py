"""What the dynamic range compressor costs: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths laid
end to end with 10 % overlaps), converted from 44.1 to 48 kHz on the device and put through goofer_compress, timed with HIP
events — beside goofer_loudness_measure + goofer_loudness_apply and goofer_limit on the same track in the same process, and
beside what a caller does without it: the fp32 track downloaded and compressed on the host by the numpy restatement
(tests/compress_ref.py, ``blocked``).  The host figure is the baseline, not the code under test.

python scripts/compress_rate.py [--notes 1024] [--reps 20] [--sigma 0.2] [--settings -20:4] [--host-samples 2000000] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
GB/s is over the bytes the call must move, 16 per sample: the three passes read the track, the last writes it.  The two
unmeasured choices of the design are options of the library and alternate with the default round by round in one process:
"compress_skip" 0 takes the logarithm of every sample, "compress_store" 1 writes xl in the first pass and reads it in the other
two.  goofer_compress is five launches (k_cp_release_sum, k_cp_release_carry, k_cp_attack_sum, k_cp_attack_carry, k_cp_apply);
for the time of each, run this script with --no-host under ``rocprofv3 --kernel-trace --stats``.  ``--host-samples`` runs the
restatement on the track's first N samples only and scales its time to the whole track (it is linear in the length); the result
says so.  The curve and the output of those samples are compared with the restatement's.  Prints one JSON line."""
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
import compress_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import compress as CP, limit as LM, loudness as LD, phrase as P, rate as RT  # noqa: E402
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
    ap.add_argument("--settings", default="-20:4", help="T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]")
    ap.add_argument("--host-samples", type=int, default=2000000, help="run the host restatement on this many samples and scale (0: the whole track)")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    entries, lens, sr = phrase(a.notes)
    n_in = P.plan_phrase(entries, lens, sr).total_out          # the mixed track's length at the voicebank's rate
    sr_out = 48000
    rplan = RT.plan(sr, sr_out, [n_in])
    g = torch.Generator(device=ctx.device).manual_seed(3)
    x_in = a.sigma * torch.randn(n_in, dtype=torch.float32, device=ctx.device, generator=g)
    track = ctx.rate_convert(x_in, None, rplan)                 # what render_phrase(out_sr=48000) hands the compressor
    n = rplan.total_out
    settings = CP.parse(a.settings)
    t0 = time.perf_counter()
    plan = CP.plan(sr_out, [n], settings)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    dplan, lplan = LD.plan(sr_out, [n]), LM.plan(sr_out, [n])
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)

    def variant(skip, store):
        def run():
            ctx.set_option("compress_skip", skip)
            ctx.set_option("compress_store", store)
            try:
                return ctx.compress(track, None, plan, out=out)
            finally:
                ctx.set_option("compress_skip", 1)
                ctx.set_option("compress_store", 0)
        return run
    fns = {"compress": variant(1, 0), "compress_skip_0": variant(0, 0), "compress_store_1": variant(1, 1),
           "compress_skip_0_store_1": variant(0, 1),
           "loudness_measure": lambda: ctx.loudness(track, None, dplan),
           "loudness_measure_and_apply": lambda: ctx.loudness(track, None, dplan, -16.0, out=out),
           "limit": lambda: ctx.limit(track, None, lplan, out=out)}
    for fn in fns.values():                                     # code objects, plan uploads, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            rounds[k].append(timed(fn, a.reps))
    y, red, yl = ctx.compress(track, None, plan, curve=True)
    ctx.check()
    under = float((track.abs() <= 10.0 ** ((settings.threshold_db - settings.knee_db / 2.0) / 20.0)).float().mean().cpu())
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "tiles": plan.n_tiles, "MB_track": round(4.0 * n / 1e6, 1),
           "host_plan_ms": round(plan_ms, 2), "sigma": a.sigma, "settings": list(settings.astuple()),
           "max_reduction_db": float(red.cpu()[0]), "samples_under_the_knee": round(under, 4)}
    for k, v in rounds.items():
        ms = float(np.median(v))
        moved = 16.0 * n if k.startswith(("compress", "loudness_measure_and")) else 8.0 * n
        res[k] = {"ms": round(ms, 4), "ms_rounds": [round(t, 4) for t in v], "GB_s": round(moved / ms / 1e6, 1)}
    if not a.no_host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh = track.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        _, want = compress_ref.blocked(xh[:part], sr_out, settings.astuple())
        yh = compress_ref.output(xh[:part], want, settings.makeup_db)
        t2 = time.perf_counter()
        scale = n / part
        res["host"] = {"track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_compress_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "numpy_samples": part, "scaled_by": round(scale, 3), "total_ms": round(1e3 * ((t1 - t0) + (t2 - t1) * scale), 1)}
        res["worst_curve_error_db"] = float(np.abs(yl[:part].cpu().numpy() - want).max())
        ok, ratio = compress_ref.within_output_bound(y[:part].cpu().numpy(), compress_ref.product(xh[:part], want, settings.makeup_db))
        res["worst_output_error_over_bound"] = ratio
        res["within_bound"] = bool(ok and res["worst_curve_error_db"] <= compress_ref.TOL_DB and yh.dtype == np.float32)
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
