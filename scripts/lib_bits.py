#!/usr/bin/env python
"""Do two builds of libgoofer_hip.so compute the same bits?  The before / after check of a refactor of shared kernel code.

usage: scripts/lib_bits.py <libA.so> <libB.so> [--out FILE] [--limit SECONDS] [--set ragged|stages|walkers|mixes|all]

Each library gets one fresh child process (GOOFER_HIP_LIB set, as scripts/lib_ab.sh does) under its own `timeout -k 10`; the
second starts only if the first exited 0.  A child runs a fixed, seeded case list twice and prints {case: {output: sha256}} of
both runs.  Four sets of cases (default: all):
  ragged  the entry points that reach the kernels built on csrc/ragged.h — the post chain, the cascade, the synthesis on its
          spectra routes with the jitter, vibrato and sub-harmonic keyword sets, normal_fill, smooth_mask_ds, irfft_ola
  stages  the stages built on csrc/tile_scan.h, each on its own test batches at its test rates — loudness measured and normalised
          (seg_energy, loud, gain, y), the compressor under the settings of tests/test_gpu_compress.py with the curve and all
          four combinations of compress_skip and compress_store (y, max_reduction, yl), the equaliser at K = 1 .. 8 (y) — and
          each once on loudness_ref.long_signal(), whose 4116 tiles send a round's carry through thread 0 of the carry kernels
  walkers the four frame walkers (csrc/ola_walk.h) on synth_ref.long_batch through tests/test_gpu_walker_runs._walk: every route of
          its WALKERS table at walk_run 0 and at one forced run (95; 256 for k_irfft_ola1), once with injected phases and once
          with Philox — harm, uv, bre, rec, mix, note_mag, note_peak and, where the route has one, the frame_skip view
  mixes   the two gather-sum mixes (csrc/tile_mix.h) on their tests' inputs, by the tests' own builders: goofer_phrase_mix on every
          entry of tests/test_gpu_phrase.CASES, on _phrase() behind leading rests of 0, 1, 2047 and 2048 samples and with `out` and
          `x` off a 16-byte boundary; goofer_bus_mix on one track at every pan and length, the three tracks with edges and an empty
          tile behind source leads 0 and 1, the alignment grid and the order of the sum — the output and, the planner being in the
          library too, the plan's tile_off and tile list

An output whose digest differs between the two runs of one library is listed as non-deterministic and not compared across the
libraries.  Only outputs behind k_note_sumsq are expected there (post chain, notes with tension != 0 that are longer than a
workgroup: float64 atomics across workgroups).  Anything else listed there is a finding: the stages and the walkers use no
floating-point atomic but the exact max of non-negative floats.

Writes {"A": .., "B": .., "nondeterministic": [..], "differ": [..]} to FILE (default: standard output only) and prints the two
lists; exit status 1 if an output differs, the child's if a child failed.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _stage_cases(ctx):
    """{case: {output name: sha256}} of one pass over the stages on csrc/tile_scan.h"""
    import numpy as np
    import compress_ref as CR
    import eq_ref as ER
    import loudness_ref as LR
    from goofer_amd import compress as CP
    from goofer_amd import eq as EQ
    from goofer_amd import loudness as LD
    out = {}

    def dev(xs):
        return ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))[:sum(len(x) for x in xs)]     # (never an empty tensor)

    def loudness(name, xs, sr):
        plan = LD.plan(sr, [len(x) for x in xs])
        _, loud, gain, seg = ctx.loudness(dev(xs), None, plan)                              # measure only
        out[name + "/measure"] = {"seg_energy": _sha(seg.cpu().numpy()), "loud": _sha(loud.cpu().numpy()), "gain": _sha(gain.cpu().numpy())}
        y, loud, gain, seg = ctx.loudness(dev(xs), None, plan, -23.0, 60.0)
        out[name + "/normalise"] = {"seg_energy": _sha(seg.cpu().numpy()), "loud": _sha(loud.cpu().numpy()), "gain": _sha(gain.cpu().numpy()),
                                    "y": _sha(y.cpu().numpy())}

    def compress(name, xs, sr, settings):
        plan = CP.plan(sr, [len(x) for x in xs], CP.Compressor(*settings))
        y, red, yl = ctx.compress(dev(xs), None, plan, curve=True)
        out[name] = {"y": _sha(y.cpu().numpy()), "max_reduction": _sha(red.cpu().numpy()), "yl": _sha(yl.cpu().numpy())}

    def eq(name, xs, sr, K):
        y = ctx.eq(dev(xs), None, EQ.plan(sr, [len(x) for x in xs], ER.chain(sr, K)))
        out[name] = {"y": _sha(y.cpu().numpy())}

    for sr in LR.RATES:
        for b, xs in enumerate(LR.batch(sr)):
            loudness("loudness/%d/%d" % (sr, b), xs, sr)
    for sr in ER.RATES:
        for K in range(1, ER.MAX_BANDS + 1):
            eq("eq/%d/K%d" % (sr, K), ER.batch(sr), sr, K)
    sr, x = LR.long_signal()
    loudness("loudness/long", [x], sr)
    for K in (2, 8):
        eq("eq/long/K%d" % K, [x], sr, K)
    try:
        for skip in (1, 0):
            for store in (0, 1):
                ctx.set_option("compress_skip", skip)
                ctx.set_option("compress_store", store)
                tag = "skip%d_store%d" % (skip, store)
                for rate in CR.RATES:
                    for name, settings in CR.SETS.items():
                        compress("compress/%d/%s/%s" % (rate, name, tag), CR.batch(rate), rate, settings)
                if skip == 1:
                    compress("compress/long/" + tag, [x], sr, CR.SETS["defaults"])
    finally:
        ctx.set_option("compress_skip", 1)
        ctx.set_option("compress_store", 0)
    return out


def _ragged_cases(ctx):
    """{case: {output name: sha256}} of one pass over the kernels on csrc/ragged.h"""
    import numpy as np
    import post_ref as P
    import synth_ref as SR
    import test_gpu_post_chain as PC
    import test_gpu_ragged_tiles as RT
    from goofer_amd.device import default_params, spec_stride
    out = {}

    # the post chain: one flag at a time and all together, the fry ramps, the pd levels, the ragged-tile batch
    sr = 44100
    ctx.plan(sr, 1024, 256)
    post = {"post/" + kind: PC._boundary_batch(kind, sr) for kind in PC.KINDS}
    post.update({"post/fry_ramps": P.fry_cases(sr), "post/pd_levels": P.pd_cases(sr), "post/tiles": RT.post_notes(False),
                 "post/tiles_st": RT.post_notes(True)})
    for name, notes in post.items():
        res = PC.run_post(ctx, notes)
        out[name] = {"%s[%d]" % (k, i): _sha(v) for i, r in enumerate(res) for k, v in zip(("harm", "bre", "mix"), r)}
    xs, f0s = P.cascade_inputs()
    for order, btype, mode, cf in P.CASCADE_SETTINGS[::4]:
        y = ctx.onepole_cascade(ctx.tensor(np.concatenate(xs)), ctx.tensor(np.concatenate(f0s)), cf, order, btype, f0_mode=mode,
                                lengths=[len(x) for x in xs])
        out["cascade/%s%d_mode%d_cf%g" % (btype, order, mode, cf)] = {"y": _sha(y.cpu().numpy())}

    # the synthesis on the spectra routes (fused and separate overlap-add), each keyword set on every second note
    sets = {"plain": ({}, {}), "jitter": (RT.JITTER, dict(noise=True)),
            "vibrato": (RT.JITTER, dict(volume_vibrato=True, vol_jitter_speed=9.0)),
            "subharm": (dict(add_subharm=True, subharm_weight=0.7, subharm_f0_jitter=0.4),
                        dict(noise=True, subharm=dict(semitones=[-12, 7], vibrato=True, rate=40.0, depth=0.2, delay=0.01)))}
    try:
        ctx.set_option("stems", 0)
        for geo in ((44100, 1024, 256), (44100, 768, 192)):
            for batch in ("main", "tiny"):
                base = SR.batches(geo)[batch][1]
                noise = [np.random.default_rng(5 + q).standard_normal(sum(c["n"] for c in base)) for q in range(4)]
                for tag, (kw, call) in sets.items():
                    if batch == "tiny" and tag != "plain":
                        continue
                    cases = [dict(c, kw=dict(c["kw"], **kw)) if k % 2 else c for k, c in enumerate(base)]
                    res = RT.run_synth(ctx, geo, cases, call, noise)
                    out["synth/%d_%d/%s/%s" % (geo[1], geo[2], batch, tag)] = {k: _sha(v) for k, v in res.items()}
        # the tile batch of tests/test_gpu_ragged_tiles.py: boundaries at every offset the tiles treat differently
        for geo in ((RT.SR_HZ, 1024, 256), (RT.SR_HZ, 768, 192)):
            for tag in RT.VARIANTS:
                cases = RT.synth_cases(geo, tag)
                res = RT.run_synth(ctx, geo, cases, RT.VARIANTS[tag][1], RT.synth_noise(cases))
                out["synth/%d_%d/tiles/%s" % (geo[1], geo[2], tag)] = {k: _sha(v) for k, v in res.items()}
    finally:
        ctx.set_option("stems", 1)

    # single kernels over the tile batch
    ctx.plan(44100, 1024, 256)
    lens, n = RT.LENGTHS, len(RT.LENGTHS)
    par = default_params(n)
    par["seed"][:, 0] = np.arange(n) + 11
    on = np.array([k % 3 != 1 for k in range(n)], dtype=np.uint8)
    for tag in range(5):
        import torch
        z = ctx.normal_fill(2026, par, lens, tag, note_on=on if tag % 2 == 0 else None,
                            growl_scale=np.linspace(0.1, 0.9, n) if tag == 4 else None,
                            out=torch.zeros(sum(lens), dtype=torch.float64, device=ctx.device))
        out["normal_fill/tag%d" % tag] = {"z": _sha(z.cpu().numpy())}
    rng = np.random.default_rng(31)
    mask = np.concatenate([np.repeat(rng.random(m // 37 + 1) > 0.4, 37)[:m] for m in lens]).astype(np.float32)
    for fast in (False, True):
        for sigma in (4.0, 100.0):
            m = ctx.smooth_mask_ds(ctx.tensor(mask), lens, sigma=sigma, fast_interp=fast)
            out["smooth_mask_ds/sigma%g_fast%d" % (sigma, fast)] = {"mask": _sha(m.cpu().numpy())}
    for geo in ((44100, 1024, 256), (44100, 768, 192), (44100, 1000, 250)):
        ctx.plan(*geo)
        nb = geo[1] // 2 + 1
        f_off = ctx.offsets(ctx.frame_counts(lens))
        rng = np.random.default_rng(57)
        S = np.zeros((int(f_off[-1]), spec_stride(nb)), dtype=np.complex64)
        S[:, :nb] = (rng.standard_normal((len(S), nb)) + 1j * rng.standard_normal((len(S), nb))).astype(np.complex64)
        y = ctx.irfft_ola(ctx.tensor(S), ctx.tensor(ctx.offsets(lens)), ctx.tensor(f_off), sum(lens))
        out["irfft_ola/%d_%d" % geo[1:]] = {"y": _sha(y.cpu().numpy())}
    ctx.plan(44100, 1024, 256)
    return out


def _walker_cases(ctx):
    """{case: {output name: sha256}} of one pass over the frame walkers on csrc/ola_walk.h"""
    import test_gpu_synth_stages as ST
    import test_gpu_walker_runs as WR
    out = {}
    try:
        for route, (counters, cap) in WR.WALKERS.items():
            has_skip = ST.ROUTES[route][4]
            ST._set(ctx, ST.ROUTES[route][1])
            for run in (0, 256 if "walk_run_ola1" in counters else 95):
                for tag, seed in (("phi", None), ("philox", 20240611)):
                    d = WR._walk(ctx, route, run, seed=seed)
                    if has_skip:
                        d["frame_skip"] = ctx.debug_fetch("frame_skip")
                    out["walkers/%s/run%d/%s" % (route, run, tag)] = {k: _sha(d[k]) for k in WR.OUTS + ("note_mag", "note_peak") +
                                                                      (("frame_skip",) if has_skip else ())}
    finally:
        ctx.set_option("walk_run", 0)
        ST._restore(ctx)
    return out


def _mix_cases(ctx):
    """{case: {output name: sha256}} of one pass over the two mixes on csrc/tile_mix.h"""
    import numpy as np
    import torch
    import test_gpu_bus as BU
    import test_gpu_phrase as PH
    from goofer_amd import bus as B
    from goofer_amd import phrase as P
    out = {}

    def phrase(name, xs, notes, total, **kw):
        plan = P.plan_records(np.array(notes, dtype=PH._lib.PHRASE_NOTE).reshape(-1), [len(x) for x in xs], total)
        out["phrase/" + name] = {"track": _sha(PH._mix(ctx, xs, notes, total, **kw)), "tile_off": _sha(plan.tile_off),
                                 "tile_notes": _sha(plan.tile_notes)}

    def bus(name, xs, tracks, *args):
        got, _, plan = BU._mix(ctx, xs, tracks, *args)
        out["bus/" + name] = {"bus": _sha(got), "tile_off": _sha(plan.tile_off), "tile_tracks": _sha(plan.tile_tracks)}

    for name, (xs, notes, total) in PH.CASES.items():
        phrase(name, xs, notes, total)
    xs, notes, total = PH._phrase(np.random.default_rng(7))
    for lead in (0, 1, 2047, 2048):
        moved = [r.copy() for r in notes]
        for r in moved:
            r["start"] += lead
        phrase("lead %d" % lead, xs, moved, total + lead)
    xs, notes, total = PH.CASES["sources at every alignment"]
    buf = torch.full((total + 1,), float("nan"), dtype=torch.float32, device=ctx.device)
    phrase("misaligned out", xs, notes, total, out=buf[1:])
    x = torch.zeros(sum(len(v) for v in xs) + 1, dtype=torch.float32, device=ctx.device)
    x[1:] = ctx.tensor(np.concatenate(xs))
    phrase("misaligned x", xs, notes, total, x_dev=x[1:])

    for pan in (-1.0, 0.0, 1.0, 0.3):                              # test_one_track_pan_and_length
        rng = np.random.default_rng(11)
        for N in (1, 7, 2047, 2048, 2049, 5000):
            bus("one track/pan %g/%d" % (pan, N), [rng.uniform(-1, 1, N).astype(np.float32)], [B.Track(-3.0, pan)])
    rng = np.random.default_rng(12)                                # test_three_tracks_edges_and_an_empty_tile
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1500, 700, 1000, 2048)]
    tracks = [B.Track(0.0, -0.4), B.Track(-6.0, 0.2, BU._ms(3)), B.Track(2.0, 0.9, BU._ms(2050)), B.Track(-1.0, 0.0, BU._ms(2048))]
    for lead in (0, 1):
        bus("three tracks/lead %d" % lead, xs, tracks, 3 * 2048 + 5, lead)
    rng = np.random.default_rng(14)                                # test_alignment_of_source_and_bus
    xs = [rng.uniform(-1, 1, 4099).astype(np.float32), rng.uniform(-1, 1, 2600).astype(np.float32)]
    for lead in (0, 1, 2, 3):
        for out_lead in (0, 1):
            for total in (4096, 4097, 4099):
                bus("alignment/%d_%d_%d" % (lead, out_lead, total), xs, [B.Track(0.0, -0.2), B.Track(0.0, 0.7, BU._ms(512 + lead))], total,
                    lead, out_lead)
    xs = [np.full(3000, 1e8, np.float32), np.ones(3000, np.float32), np.full(3000, -1e8, np.float32)]      # test_order_of_the_sum
    t = B.Track(0.0, -1.0)
    bus("order/big one minus", xs, [t, t, t])
    bus("order/big minus one", [xs[0], xs[2], xs[1]], [t, t, t])
    return out


def _cases(ctx, which):
    out = _ragged_cases(ctx) if which in ("ragged", "all") else {}
    if which in ("stages", "all"):
        out.update(_stage_cases(ctx))
    if which in ("walkers", "all"):
        out.update(_walker_cases(ctx))
    if which in ("mixes", "all"):
        out.update(_mix_cases(ctx))
    return out


def child(which):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from goofer_amd.device import Context
    ctx = Context(0)
    runs = [_cases(ctx, which), _cases(ctx, which)]
    ctx.close()
    print("LIB_BITS " + json.dumps(runs))


def _flat(d):
    return {"%s:%s" % (case, name): h for case, outs in d.items() for name, h in outs.items()}


def main(argv):
    if argv[:1] == ["--child"]:
        return child(argv[1])
    opts = {"--out": None, "--limit": "600", "--set": "all"}
    libs = []
    it = iter(argv)
    for a in it:
        if a in opts:
            opts[a] = next(it)
        else:
            libs.append(a)
    if len(libs) != 2 or opts["--set"] not in ("ragged", "stages", "walkers", "mixes", "all"):
        sys.exit(__doc__)
    runs = {}
    for tag, lib in zip("AB", libs):
        env = dict(os.environ, GOOFER_HIP_LIB=os.path.abspath(lib))
        p = subprocess.run(["timeout", "-k", "10", opts["--limit"], sys.executable, os.path.abspath(__file__), "--child", opts["--set"]], env=env,
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LIB_BITS ")]
        if p.returncode != 0 or not lines:
            sys.stdout.write(p.stdout[-4000:])
            print("lib_bits: the child of %s exited %d; nothing more is started" % (lib, p.returncode))
            sys.exit(p.returncode or 2)
        runs[tag] = json.loads(lines[-1][len("LIB_BITS "):])
    flat = {tag: [_flat(r) for r in runs[tag]] for tag in runs}
    keys = sorted(flat["A"][0])
    assert all(sorted(f) == keys for tag in flat for f in flat[tag]), "the libraries ran different case lists"
    loose = [k for k in keys if any(flat[tag][0][k] != flat[tag][1][k] for tag in flat)]
    differ = [k for k in keys if k not in loose and flat["A"][0][k] != flat["B"][0][k]]
    report = {"A": runs["A"][0], "B": runs["B"][0], "libs": [os.path.basename(v) for v in libs], "nondeterministic": loose,
              "differ": differ}
    if opts["--out"]:
        with open(opts["--out"], "w") as fh:
            json.dump(report, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print("%d outputs of %d cases; non-deterministic (not compared): %d; differing: %d" % (len(keys), len(runs["A"][0]), len(loose),
                                                                                        len(differ)))
    for k in loose:
        print("  non-deterministic  " + k)
    for k in differ:
        print("  DIFFERS            " + k)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main(sys.argv[1:])
