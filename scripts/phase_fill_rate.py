"""What a seeded batch costs: BASELINE config 3's batch rendered with phi_seeds, its phases drawn on the device
(goofer_phase_fill), against the same batch with the phase matrix drawn on the host note by note and uploaded — what
Renderer.prepare did before the kernel existed — in one process.

python scripts/phase_fill_rate.py [--notes 1024] [--repeat 2]
Per variant: strings -> audio time of the batch ("prepare": argument strings decoded, planned, uploaded — for the host variant
also the numpy draws and the matrix upload; "run": device work until the mix exists; best of --repeat), a check that both
give the same mix, then the fill kernel alone by HIP events: milliseconds per matrix and GB/s on the bytes it writes
(4 * n_bins per frame).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import sampler as S, synthetic as syn  # noqa: E402
from goofer_amd.device import Context, pcg64_words  # noqa: E402
from goofer_amd.render import Renderer, Source  # noqa: E402


def batch(n):
    srcs, args, seeds = [], [], []
    for i in range(n):
        src, req, phi_seed = syn.config_note(3, i)
        srcs.append(Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]))
        args.append(syn.request_args(req))
        seeds.append(phi_seed)
    return srcs, args, seeds


def host_matrix(r, prep, seeds):
    """the phase rows as the renderer made them on the host: numpy once per note, transposed, concatenated, uploaded"""
    mats = [np.random.default_rng(sd).uniform(0.0, 2.0 * np.pi, size=(r.ctx.n_bins, 1 + n // r.hop)).astype(np.float32).T
            for n, sd in zip(prep["lens"], seeds)]
    return r.ctx.rows_from(np.concatenate(mats))


def render_times(r, srcs, args, seeds, repeat, on_host):
    best, mix = None, None
    for _ in range(repeat + 1):                                 # the first pass warms the allocator, the arena and the plan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep = r.prepare((srcs, S.decode_request_batch(args)), phi_seeds=seeds)
        if on_host:
            prep["phi"], prep["phi_words"] = host_matrix(r, prep, seeds), None
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = r.run(prep, seed=0)
        r.ctx.check()
        t2 = time.perf_counter()
        frames, mix = prep["frames"], out["mix"].clone()
        del out, prep
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    return {"total_ms": round(best[0] * 1e3, 2), "prepare_ms": round(best[1] * 1e3, 2), "run_ms": round(best[2] * 1e3, 2)}, frames, mix


def fill_alone(ctx, frames, seeds, n_bins, reps=20):
    d_w = ctx.tensor(pcg64_words(seeds).view(np.int64))
    d_f = ctx.tensor(ctx.offsets(frames))
    out = ctx.rows(int(sum(frames)), n_bins)
    call = lambda: ctx.phase_fill(d_w, d_f, out=out)            # noqa: E731
    call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / reps
    nbytes = 4.0 * n_bins * int(sum(frames))
    return {"frames": int(sum(frames)), "n_bins": n_bins, "MB": round(nbytes / 1e6, 1), "ms": round(ms, 4), "store_GB_s": round(nbytes / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    ctx = Context(0)
    srcs, args, seeds = batch(a.notes)
    res = {"metric": "phase_fill_rate", "notes": a.notes, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    r = Renderer(ctx)
    res["device_fill"], frames, mix_d = render_times(r, srcs, args, seeds, a.repeat, on_host=False)
    res["host_draw"], _, mix_h = render_times(r, srcs, args, seeds, a.repeat, on_host=True)
    res["same_mix"] = bool(torch.equal(mix_d, mix_h))
    res["frames"] = int(frames)
    res["host_over_device"] = round(res["host_draw"]["total_ms"] / res["device_fill"]["total_ms"], 2)
    per_note = [1 + int(n) // r.hop for n in np.diff(r.prepare((srcs, S.decode_request_batch(args)))["sample_off"])]
    res["fill_batch"] = fill_alone(ctx, per_note, seeds, ctx.n_bins)
    res["fill_one_seed"] = fill_alone(ctx, per_note, [seeds[0]] * len(per_note), ctx.n_bins)
    res["fill_2049_bins"] = fill_alone(ctx, per_note[:max(1, a.notes // 4)], seeds[:max(1, a.notes // 4)], 2049)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
