"""What loudness metering and normalisation cost: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths
laid end to end with 10 % overlaps), converted from 44.1 to 48 kHz on the device, measured by goofer_loudness_measure and scaled
by goofer_loudness_apply, each timed with HIP events — beside goofer_limit on the same track in the same process, and beside what
a caller does without them: the fp32 track downloaded and measured on the host by the numpy restatement
(tests/loudness_ref.py).  The host figure is the baseline, not the code under test.

python scripts/loudness_rate.py [--notes 1024] [--reps 20] [--sigma 0.2] [--target -16] [--host-samples 200000] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
GB/s is over the bytes the two calls must move, 16 per sample: the measurement reads the track twice, the scaling reads and
writes it once.  The measurement is four launches (k_loud_ends, k_loud_carry, k_loud_energy, k_loud_stats); for the share of each, run
this script with --no-host under ``rocprofv3 --kernel-trace --stats``.  ``--host-samples`` runs the restatement on the track's first N samples
only and scales its time to the whole track (it is linear in the length); the result says so.  The segment energies of those
samples and of as many at the track's end are compared with the restatement's (float64 flavour).  Prints one JSON line."""
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
import loudness_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import limit as LM, loudness as LD, phrase as P, rate as RT  # noqa: E402
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
    ap.add_argument("--target", type=float, default=-16.0)
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
    track = ctx.rate_convert(x_in, None, rplan)                 # what render_phrase(out_sr=48000) hands the loudness stage
    n = rplan.total_out
    t0 = time.perf_counter()
    plan = LD.plan(sr_out, [n])
    plan_ms = 1e3 * (time.perf_counter() - t0)
    lplan = LM.plan(sr_out, [n])
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)
    ones = torch.ones(1, dtype=torch.float32, device=ctx.device)
    d_in = plan.device_tables(ctx)[0]

    def measure():
        return ctx.loudness(track, None, plan)

    def apply():                                                # goofer_loudness_apply alone, on a gain that is there already
        ctx._check(ctx.lib.goofer_loudness_apply(ctx.h, track.data_ptr(), d_in.data_ptr(), 1, n, ones.data_ptr(), out.data_ptr(), ctx._stream()))

    def both():
        return ctx.loudness(track, None, plan, a.target, out=out)

    def limit():
        return ctx.limit(track, None, lplan, out=out)
    for fn in (measure, apply, both, limit):                    # code objects, plan uploads, clocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {"measure": [], "apply": [], "measure_and_apply": [], "limit": []}
    for _ in range(5):
        rounds["measure"].append(timed(measure, a.reps))
        rounds["apply"].append(timed(apply, a.reps))
        rounds["measure_and_apply"].append(timed(both, a.reps))
        rounds["limit"].append(timed(limit, a.reps))
    y, loud, gain, seg = both()
    ctx.check()
    loud, gain = loud.cpu().numpy(), gain.cpu().numpy()
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "S": plan.S, "segments": plan.n_segments, "tiles": plan.n_tiles,
           "MB_track": round(4.0 * n / 1e6, 1), "host_plan_ms": round(plan_ms, 2), "sigma": a.sigma, "target": a.target,
           "lufs": float(loud[0, 0]), "momentary_max": float(loud[0, 1]), "gain": float(gain[0])}
    moved = {"measure": 8.0 * n, "apply": 8.0 * n, "measure_and_apply": 16.0 * n, "limit": 8.0 * n}
    for k, v in rounds.items():
        ms = float(np.median(v))
        res[k] = {"ms": round(ms, 4), "ms_rounds": [round(t, 4) for t in v], "GB_s": round(moved[k] / ms / 1e6, 1)}
    if not a.no_host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh = track.cpu().numpy()
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        part -= part % plan.S
        E = loudness_ref.seg_energy(loudness_ref.weighted_squares(xh[:part], sr_out)[0], plan.S)
        t2 = time.perf_counter()
        scale = n / part
        res["host"] = {"track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_measure_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "numpy_samples": part, "scaled_by": round(scale, 3), "total_ms": round(1e3 * ((t1 - t0) + (t2 - t1) * scale), 1)}
        got = seg.cpu().numpy()
        err = float(np.abs(got[:len(E)] - E).max() / E.max())
        # the track's end, where the state has come through every tile: the restatement from zero ten segments ahead of the
        # window (the high-pass's poles have radius 0.995: after 48 000 samples nothing of the state is left)
        warm, k0 = 10, max(0, plan.n_segments - part // plan.S - 10)
        if k0 > 0:
            E2 = loudness_ref.seg_energy(loudness_ref.weighted_squares(xh[k0 * plan.S:], sr_out)[0], plan.S)[warm:]
            err = max(err, float(np.abs(got[k0 + warm:] - E2).max() / E2.max()))
            res["host"]["end_window_segments"] = len(E2)
        res["worst_E_error_over_max_E"] = err
        res["within_bound"] = bool(res["worst_E_error_over_max_E"] <= loudness_ref.TOL)
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
