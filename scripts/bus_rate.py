"""What the stereo bus costs: --tracks tracks of scripts/phrase_rate.py's workload's length at 48 kHz, panned across the field
and staggered by 10 ms each, mixed by goofer_bus_mix and finished by the channel-linked stages, each timed with HIP events —
beside what a caller does without them: every track downloaded, then panned, summed, gated and limited on the host by the numpy
restatement (tests/bus_ref.py).  The host figure is the baseline, not the code under test.

python scripts/bus_rate.py [--tracks 8] [--notes 1024] [--reps 20] [--sigma 0.1] [--host-samples 200000] [--no-host]
The tracks are random fp32 samples (normal, standard deviation --sigma); nothing is rendered.  Timed, warmed, in one process:
goofer_bus_mix, in ms and GB/s over the 4 sum len + 8 N bytes it must move, with goofer_phrase_mix on its own workload beside it;
goofer_limit_linked on the bus as mixed and times 2, in both detection modes, with the same two channels through goofer_limit /
goofer_limit_tp as independent signals beside it; the measure + link + apply loudness chain; goofer_pcm16_planar.
``--host-samples`` runs the restatement on the first N samples of the tracks only and scales its time to the whole length (it is
linear in the length); the result says so.  Prints one JSON line."""
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
import bus_ref  # noqa: E402
import limit_ref  # noqa: E402
import loudness_ref  # noqa: E402
from limit_rate import timed  # noqa: E402
from phrase_rate import phrase  # noqa: E402
from goofer_amd import bus as B, limit as LM, loudness as LD, phrase as P, rate as RT  # noqa: E402
from goofer_amd.device import Context  # noqa: E402


def median_ms(fn, reps, rounds=5):
    v = [timed(fn, reps) for _ in range(rounds)]
    return float(np.median(v)), [round(t, 4) for t in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--host-samples", type=int, default=200000, help="run the host restatement on this many samples and scale (0: everything)")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline (and the comparison with it)")
    a = ap.parse_args()
    ctx = Context(0)
    sr = 48000
    entries, lens, sr_in = phrase(a.notes)
    pplan = P.plan_phrase(entries, lens, sr_in)
    n = RT.plan(sr_in, sr, [pplan.total_out]).total_out          # a track of the phrase workload at 48 kHz
    g = torch.Generator(device=ctx.device).manual_seed(3)
    xs = [a.sigma * torch.randn(n, dtype=torch.float32, device=ctx.device, generator=g) for _ in range(a.tracks)]
    pans = np.linspace(-1.0, 1.0, a.tracks) if a.tracks > 1 else [0.0]
    tracks = [B.Track(-3.0, float(p), 10.0 * k) for k, p in enumerate(pans)]
    t0 = time.perf_counter()
    plan = B.plan(xs, [n] * a.tracks, tracks, sr)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    N = plan.total_out
    bus = torch.empty(2 * N, dtype=torch.float32, device=ctx.device)
    res = {"tracks": a.tracks, "sr": sr, "track_samples": n, "bus_samples": N, "tiles": len(plan.tile_off) - 1,
           "cover_entries": int(len(plan.tile_tracks)), "host_plan_ms": round(plan_ms, 2)}

    # the mix, and goofer_phrase_mix on its own workload in the same process
    nbytes = 4.0 * float(np.minimum(plan.tracks["len"], N - plan.tracks["start"]).sum()) + 8.0 * N
    for _ in range(3):
        ctx.bus_mix(xs, plan, out=bus)
    ms, rounds = median_ms(lambda: ctx.bus_mix(xs, plan, out=bus), a.reps)
    res["bus_mix"] = {"ms": round(ms, 4), "ms_rounds": rounds, "MB": round(nbytes / 1e6, 1), "GB_s": round(nbytes / ms / 1e6, 1)}
    xp = 0.3 * torch.randn(sum(lens), dtype=torch.float32, device=ctx.device, generator=g)
    d_off = ctx.tensor(ctx.offsets(lens))
    pout = torch.empty(pplan.total_out, dtype=torch.float32, device=ctx.device)
    pbytes = 4.0 * sum(min(int(r["take"]), ln - int(r["skip"])) for r, ln in zip(pplan.notes, lens)) + 4.0 * pplan.total_out
    for _ in range(3):
        ctx.phrase_mix(xp, d_off, pplan, out=pout)
    ms, rounds = median_ms(lambda: ctx.phrase_mix(xp, d_off, pplan, out=pout), a.reps)
    res["phrase_mix"] = {"ms": round(ms, 4), "ms_rounds": rounds, "MB": round(pbytes / 1e6, 1), "GB_s": round(pbytes / ms / 1e6, 1)}
    res["bus_mix_over_phrase_mix_GB_s"] = round(res["bus_mix"]["GB_s"] / res["phrase_mix"]["GB_s"], 3)
    del xp, pout

    # the limiter: linked on the pair, and the same two channels as independent signals
    out = torch.empty(2 * N, dtype=torch.float32, device=ctx.device)
    inputs = {"as_mixed": bus, "times_2": bus * 2.0}
    res["limit"] = {}
    for tp in (False, True):
        linked = LM.plan(sr, [N, N], LM.CEILING, LM.LOOK_MS, tp, channels=2)
        apart = LM.plan(sr, [N, N], LM.CEILING, LM.LOOK_MS, tp)
        for k, x in inputs.items():
            row = {"samples_above_ceiling": int((x.abs() > linked.ceiling).sum().item())}
            for name, p in (("linked", linked), ("independent", apart)):
                for _ in range(2):
                    ctx.limit(x, None, p, out=out)
                ms, rounds = median_ms(lambda: ctx.limit(x, None, p, out=out), a.reps)
                row[name] = {"ms": round(ms, 4), "ms_rounds": rounds, "GB_s": round(16.0 * N / ms / 1e6, 1)}
            res["limit"][("true_peak" if tp else "sample_peak") + "_" + k] = row

    # loudness: measure, link, apply
    lplan = LD.plan(sr, [N, N])
    for _ in range(2):
        ctx.loudness(bus, None, lplan, -16.0, out=out, channels=2)
    ms, rounds = median_ms(lambda: ctx.loudness(bus, None, lplan, -16.0, out=out, channels=2), a.reps)
    _, loud, gain, _ = ctx.loudness(bus, None, lplan, -16.0, out=out, channels=2)
    res["loudness_measure_link_apply"] = {"ms": round(ms, 4), "ms_rounds": rounds, "lufs": round(float(loud.cpu()[0, 0]), 3),
                                          "gain": round(float(gain.cpu()[0]), 5)}
    ms1, _ = median_ms(lambda: ctx.loudness(bus, None, lplan, -16.0, out=out), a.reps)
    res["loudness_two_independent_signals_ms"] = round(ms1, 4)

    # int16, interleaved
    pcm = torch.empty((N, 2), dtype=torch.int16, device=ctx.device)
    for _ in range(2):
        ctx.pcm16(bus, out=pcm, channels=2)
    ms, rounds = median_ms(lambda: ctx.pcm16(bus, out=pcm, channels=2), a.reps)
    res["pcm16_planar"] = {"ms": round(ms, 4), "ms_rounds": rounds, "GB_s": round(12.0 * N / ms / 1e6, 1)}
    ctx.check()

    if not a.no_host:
        x2 = inputs["times_2"]
        linked = LM.plan(sr, [N, N], LM.CEILING, LM.LOOK_MS, channels=2)
        y, _, _ = ctx.limit(x2, None, linked, out=out)
        got_mix, got_lim = bus.cpu().numpy(), y.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xh = [x.cpu().numpy() for x in xs]
        t1 = time.perf_counter()
        part = min(n, a.host_samples) if a.host_samples > 0 else n
        rec = [(int(r["start"]), r["gl"], r["gr"]) for r in plan.tracks]
        Np = min(N, part)
        ref = bus_ref.mix([x[:part] for x in xh], rec, Np)
        t2 = time.perf_counter()
        S = loudness_ref.seg_len(sr)
        E = [loudness_ref.seg_energy(loudness_ref.weighted_squares(ref[c * Np:(c + 1) * Np], sr)[0], S) for c in (0, 1)]
        bus_ref.loud_linked(E[0], E[1], S, -16.0)
        t3 = time.perf_counter()
        two = [ref[:Np] * np.float32(2.0), ref[Np:] * np.float32(2.0)]
        (yl, yr), _, _, _ = bus_ref.limit_linked(two, linked.taps, linked.W, np.float32(linked.ceiling))
        t4 = time.perf_counter()
        bus_ref.pcm16_planar(np.concatenate([yl, yr]))
        t5 = time.perf_counter()
        scale = N / Np
        res["host"] = {"tracks_download_ms": round(1e3 * (t1 - t0), 1), "numpy_mix_ms": round(1e3 * (t2 - t1) * scale, 1),
                       "python_loudness_ms": round(1e3 * (t3 - t2) * scale, 1), "numpy_limit_ms": round(1e3 * (t4 - t3) * scale, 1),
                       "numpy_pcm16_ms": round(1e3 * (t5 - t4) * scale, 1), "numpy_samples": Np, "scaled_by": round(scale, 3),
                       "total_ms": round(1e3 * ((t1 - t0) + (t5 - t1) * scale), 1)}
        keep = Np - (2 * linked.W if Np < N else 0)               # a window that reaches past the prefix's end sees another signal there
        same = np.array_equal(got_mix[:Np].view(np.int32), ref[:Np].view(np.int32)) and np.array_equal(got_mix[N:N + Np].view(np.int32), ref[Np:].view(np.int32))
        same = same and np.array_equal(got_lim[:keep].view(np.int32), yl[:keep].view(np.int32)) and np.array_equal(got_lim[N:N + keep].view(np.int32), yr[:keep].view(np.int32))
        res["bit_equal"] = bool(same)
    print(json.dumps(res))
    ctx.close()
    return 0 if res.get("bit_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
