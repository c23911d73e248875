"""What the convolution reverb costs: the track of scripts/phrase_rate.py's workload (BASELINE config 3's note lengths laid end to
end with 10 % overlaps), converted from 44.1 to 48 kHz on the device, through goofer_reverb with impulse responses of 0.25 s, 1 s
and 4 s (12, 47 and 188 partitions of 1024 taps), each timed with HIP events; goofer_reverb_ir, which runs once per impulse
response, timed on its own; a one-tap impulse response beside them (the two transforms without a multiply-accumulate to speak
of); goofer_eq and goofer_compress on the same track in the same process; and what a caller does without the stage: the fp32
track downloaded and convolved on the host by the numpy restatement (tests/reverb_ref.py, one float64 FFT convolution).  The
host figure is the baseline, not the code under test.

python scripts/reverb_rate.py [--notes 1024] [--reps 10] [--sigma 0.2] [--ir-seconds 0.25,1,4] [--no-host]
The track is random fp32 samples (normal, standard deviation --sigma) through goofer_rate_convert; nothing is rendered or mixed.
goofer_reverb is three launches (k_reverb_fwd, k_reverb_mac, k_reverb_inv); HIP events bracket the call, so the figures derived
for the multiply-accumulate are over the whole call's time: ``mac_per_s``, complex multiply-accumulates (blocks x partitions in
reach x 1024 bins) per second, and ``naive_TB_s``, the 16 bytes a naive multiply-accumulate reads per product (an input and an
impulse-response bin), i.e. what the LDS slice and the register accumulators stand in for.  ``reread``: (T + P - 1) / T for
T = 32, what the scheme reads of every input spectrum per workgroup; for the measured factor and the kernel's own time run
this script with ``--ir-seconds 1 --no-host`` under ``scripts/pmc_script.sh`` with FETCH_SIZE.  Prints one JSON line."""
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
import reverb_ref  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import compress as CP, eq as EQ, phrase as P, rate as RT, reverb as RV  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.2)
    ap.add_argument("--ir-seconds", default="0.25,1,4", help="rt60 of the synthetic rooms, comma separated")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    entries, lens, sr = phrase(a.notes)
    n_in = P.plan_phrase(entries, lens, sr).total_out          # the mixed track's length at the voicebank's rate
    sr_out = 48000
    rplan = RT.plan(sr, sr_out, [n_in])
    g = torch.Generator(device=ctx.device).manual_seed(3)
    x_in = a.sigma * torch.randn(n_in, dtype=torch.float32, device=ctx.device, generator=g)
    track = ctx.rate_convert(x_in, None, rplan)                 # what render_phrase(out_sr=48000) hands the chain
    n = rplan.total_out
    rooms = [float(v) for v in a.ir_seconds.split(",")]
    revs = {"%g s" % s: RV.Reverb(RV.Room(s, 1, 8000.0), wet_db=-12.0) for s in rooms}
    revs["1 tap"] = RV.Reverb(np.ones(1, np.float32), wet_db=-12.0)
    plans, spectra, ir_ms, outs = {}, {}, {}, {}
    for k, rv in revs.items():
        plans[k] = RV.plan(sr_out, [n], rv)
        taps = rv.taps(sr_out)
        ctx.reverb_ir(taps)                                     # code objects
        ir_ms[k] = float(np.median([timed(lambda: ctx.reverb_ir(taps), 3) for _ in range(3)]))
        spectra[k] = rv.spectra(ctx, sr_out)
        outs[k] = torch.empty(plans[k].total_out, dtype=torch.float32, device=ctx.device)
    eplan, cplan = EQ.plan(sr_out, [n], "hp:80,peak:3000:3:1"), CP.plan(sr_out, [n], "-24:3")
    out = torch.empty(n, dtype=torch.float32, device=ctx.device)
    fns = {"eq_2": lambda: ctx.eq(track, None, eplan, out=out), "compress": lambda: ctx.compress(track, None, cplan, out=out)}
    for k in revs:
        fns["reverb " + k] = (lambda k: lambda: ctx.reverb(track, None, plans[k], spectra[k], out=outs[k]))(k)
    for fn in fns.values():                                     # code objects, plan uploads, clocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            rounds[k].append(timed(fn, a.reps))
    ctx.check()
    res = {"notes": a.notes, "sr": sr_out, "samples": n, "MB_track": round(4.0 * n / 1e6, 1), "sigma": a.sigma}
    for k, v in rounds.items():
        ms = float(np.median(v))
        res[k] = {"ms": round(ms, 4), "ms_rounds": [round(t, 4) for t in v]}
        if k.startswith("reverb "):
            p = plans[k[7:]]
            Pn, nb = (p.L + RV.BLOCK - 1) // RV.BLOCK, p.total_blocks
            pairs = sum(min(b + 1, Pn) for b in range(min(nb, Pn))) + max(nb - Pn, 0) * Pn      # (block, partition) products in reach
            res[k].update({"taps": p.L, "partitions": Pn, "blocks": nb, "reverb_ir_ms": round(ir_ms[k[7:]], 4),
                           "samples_per_s": round(n / ms * 1e3), "mac_per_s": round(pairs * 1024 / ms * 1e3),
                           "naive_TB_s": round(16.0 * pairs * 1024 / ms / 1e9, 3), "reread": round((RV.RUN + Pn - 1) / RV.RUN, 3),
                           "spectra_GB": round(16.0 * nb * 1024 / 1e9, 3)})
    if not a.no_host:
        k = "%g s" % rooms[min(1, len(rooms) - 1)]
        y = ctx.reverb(track, None, plans[k], spectra[k], out=outs[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh = track.cpu().numpy()
        t1 = time.perf_counter()
        want = reverb_ref.reference(xh, revs[k].taps(sr_out), plans[k].pre, True, plans[k].dry, plans[k].wet)
        t2 = time.perf_counter()
        res["host"] = {"ir": k, "track_download_ms": round(1e3 * (t1 - t0), 2), "numpy_fft_convolution_ms": round(1e3 * (t2 - t1), 1),
                       "total_ms": round(1e3 * (t2 - t0), 1)}
        err = reverb_ref.error(y.cpu().numpy(), want)
        res["worst_error_over_peak"] = err
        res["within_bound"] = bool(err <= reverb_ref.TOL)
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("within_bound", True) else 1


if __name__ == "__main__":
    sys.exit(main())
