"""What a seeded sh / sr batch costs: BASELINE config 3's batch with ``sh50sr50`` on every note, its jitter normals drawn on the
device from numpy's legacy stream (noise_seeds: goofer_legacy_normal_fill), against the same batch with the host drawing them
— ``np.random.seed`` and three ``np.random.randn`` per note, concatenated and uploaded: what a seeded comparison needed before
the kernel existed — in one process.

python scripts/legacy_fill_rate.py [--notes 1024] [--repeat 2]
Per variant: strings -> audio time of the batch ("prepare": argument strings decoded, planned, uploaded — for the host variant
also the numpy draws and the upload of 8 bytes per sample and stream; "run": device work until the mix exists; best of
--repeat), how far the two mixes are apart (only ``log`` differs: a few ulps of the normals), then the fill kernel alone by HIP
events, one workgroup per note and one wave per note (option "legacy_wave"): milliseconds per batch, normals per second, and
the time of one 1.1 s note with three streams — the latency of its sequential blocks.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goofer_amd import sampler as S, synthetic as syn  # noqa: E402
from goofer_amd.device import Context  # noqa: E402
from goofer_amd.render import Renderer, Source  # noqa: E402


def batch(n):
    srcs, args, phi, legacy = [], [], [], []
    for i in range(n):
        src, req, phi_seed = syn.config_note(3, i)
        srcs.append(Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]))
        args.append(syn.request_args(dict(req, flags=req["flags"] + "sh50sr50")))
        phi.append(phi_seed)
        legacy.append((40503 * (i + 1)) % 2 ** 32)
    return srcs, args, phi, legacy


def host_draws(r, lens, legacy):
    """the three streams as a seeded reference process per note draws them, uploaded"""
    nf, nh, nb = [], [], []
    for n, sd in zip(lens, legacy):
        np.random.seed(sd)
        nf.append(np.random.randn(n))
        nh.append(np.random.randn(n))
        nb.append(np.random.randn(n))
    return r.ctx.tensor(np.concatenate(nf)), (r.ctx.tensor(np.concatenate(nh)), r.ctx.tensor(np.concatenate(nb)))


def render_times(r, srcs, args, phi, legacy, repeat, on_host):
    best, mix = None, None
    for _ in range(repeat + 1):                                 # the first pass warms the allocator, the arena and the plan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep = r.prepare((srcs, S.decode_request_batch(args)), phi_seeds=phi, noise_seeds=legacy)
        if on_host:
            prep["noise_f0"], prep["noise_vol"] = host_draws(r, prep["lens"], legacy)
            prep["legacy_noise"] = None
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = r.run(prep, seed=0)
        r.ctx.check()
        t2 = time.perf_counter()
        lens, mix = list(prep["lens"]), out["mix"].clone()
        del out, prep
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    return {"total_ms": round(best[0] * 1e3, 2), "prepare_ms": round(best[1] * 1e3, 2), "run_ms": round(best[2] * 1e3, 2)}, lens, mix


def fill_alone(ctx, lens, legacy, wave, reps=100):
    n = len(lens)
    d_seed = ctx.tensor(np.asarray(legacy, dtype=np.uint32).view(np.int32))
    d_s = ctx.tensor(ctx.offsets(lens))
    d_on = ctx.tensor(np.ones(3 * n, dtype=np.uint8))
    out = tuple(torch.empty(int(sum(lens)), dtype=torch.float64, device=ctx.device) for _ in range(3))
    ctx.set_option("legacy_wave", wave)
    try:
        call = lambda: ctx.legacy_normal_fill(d_seed, d_s, d_on, out=out)   # noqa: E731
        call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        ctx.check()
    finally:
        ctx.set_option("legacy_wave", 0)
    ms = a.elapsed_time(b) / reps
    normals = 3 * int(sum(lens))
    return {"notes": n, "normals": normals, "ms": round(ms, 4), "Mnormals_s": round(normals / ms / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--notes", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    ctx = Context(0)
    srcs, args, phi, legacy = batch(a.notes)
    res = {"metric": "legacy_fill_rate", "notes": a.notes, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    r = Renderer(ctx)
    state = np.random.get_state()
    res["device_fill"], lens, mix_d = render_times(r, srcs, args, phi, legacy, a.repeat, on_host=False)
    res["host_draw"], _, mix_h = render_times(r, srcs, args, phi, legacy, a.repeat, on_host=True)
    np.random.set_state(state)
    res["samples"] = int(sum(lens))
    res["mix_max_abs_diff"] = float((mix_d - mix_h).abs().max())
    res["mix_peak"] = float(mix_h.abs().max())
    res["host_over_device"] = round(res["host_draw"]["total_ms"] / res["device_fill"]["total_ms"], 2)
    t0 = time.perf_counter()
    np.random.randn(1 << 22)
    res["host_randn_Mnormals_s"] = round((1 << 22) / (time.perf_counter() - t0) / 1e6, 1)
    np.random.set_state(state)
    one = [int(1.1 * srcs[0].sr)]
    for name, wave in (("workgroup", 0), ("wave", 1)):
        res["fill_batch_" + name] = fill_alone(ctx, lens, legacy, wave)
        res["fill_one_note_" + name] = fill_alone(ctx, one, legacy[:1], wave)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
