"""What the jitter / growl draws cost: BASELINE config 3's batch with sh50sr50 on every note, on one note in 64, and sj30 on
every note, rendered with noise="host" (np.random, note by note, uploaded) and noise="device" (goofer_normal_fill) in one process.

python scripts/jitter_rate.py [--notes 1024] [--repeat 2] [--seed 0]
Per case and noise source: strings -> audio time of the batch (argument strings decoded, planned, uploaded = "prepare"; device work
until the mix exists = "run"; best of --repeat), then the fill kernel alone by HIP events: milliseconds per [total_samples] array
and GB/s of float64 stores, for an aligned batch and for one whose notes start on odd indices.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import sampler as S, synthetic as syn  # noqa: E402
from goofer_amd.device import Context, default_params  # noqa: E402
from goofer_amd.render import Renderer, Source  # noqa: E402

CASES = {"sh50sr50_all": lambda i: "sh50sr50", "sh50sr50_1_in_64": lambda i: "sh50sr50" if i % 64 == 0 else "", "sj30_all": lambda i: "sj30"}


def batch(n):
    srcs, reqs = [], []
    for i in range(n):
        src, req, _ = syn.config_note(3, i)
        srcs.append(Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]))
        reqs.append(req)
    return srcs, reqs


def render_times(r, srcs, args, seed, repeat):
    best = None
    for _ in range(repeat + 1):                                 # the first pass warms the allocator, the arena and the plan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep = r.prepare((srcs, S.decode_request_batch(args)))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = r.run(prep, seed=seed)
        r.ctx.check()
        t2 = time.perf_counter()
        samples = prep["samples"]
        del out, prep
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    return {"total_ms": round(best[0] * 1e3, 2), "prepare_ms": round(best[1] * 1e3, 2), "run_ms": round(best[2] * 1e3, 2)}, samples


def fill_alone(ctx, lens, growl, reps=20):
    par = default_params(len(lens))
    par["seed"][:, 0] = np.arange(len(lens))
    o = ctx.device_offsets([1] * len(lens), lens, par, hop=256)
    total = int(o["s_off"][-1])
    out = torch.empty(total, dtype=torch.float64, device=ctx.device)
    scale = ctx.tensor(np.full(len(lens), 0.09)) if growl else None
    call = lambda: ctx.normal_fill(1, o["d_par"], o["d_s"], 4 if growl else 0, growl_scale=scale, out=out)
    call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / reps
    return {"samples": total, "ms": round(ms, 4), "store_GB_s": round(8.0 * total / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    ctx = Context(0)
    srcs, reqs = batch(a.notes)
    res = {"metric": "jitter_rate", "notes": a.notes, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    for case, flag in CASES.items():
        args = [syn.request_args(dict(q, flags=q["flags"] + flag(i))) for i, q in enumerate(reqs)]
        res[case] = {}
        for noise in ("host", "device"):
            res[case][noise], samples = render_times(Renderer(ctx, noise=noise), srcs, args, a.seed, a.repeat)
        res[case]["audio_s"] = round(samples / 44100.0, 1)
        res[case]["host_over_device"] = round(res[case]["host"]["total_ms"] / res[case]["device"]["total_ms"], 2)
    n = 48510
    res["fill_normals"] = fill_alone(ctx, [n] * a.notes, False)
    res["fill_normals_odd_offsets"] = fill_alone(ctx, [n - 1] + [n] * (a.notes - 1), False)   # every note after the first starts on an odd index
    res["fill_growl"] = fill_alone(ctx, [n] * a.notes, True)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
