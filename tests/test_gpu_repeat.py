"""GPU: the same batch rendered again and again on one handle gives the same bits, stage by stage.

A result that is one of two roundings from run to run is a value with two producers or a read of something stale; no comparison
against a float64 truth sees it (both roundings are inside the bound), and a test that renders once sees it one time in N.  Here a
batch is rendered once with its debug views (the baseline), then R more times; the five outputs of every repeat are compared
with the baseline ON THE DEVICE, so a repeat costs one render and five comparisons.  Before every second repeat another batch
(``tiny``) goes through the handle, so the scratch arena holds other contents when the batch comes back.  On the first repeat
that differs the views of that run are fetched and the failure message walks the pipeline in order — f0, pulse, mask_short,
S_harm, S_uv, S_breath, note_mag, frames, harm, uv, bre, note_peak, rec, mix — with, for each, the number of 32-bit words that
differ and the first (note, frame or sample) that does.  One bounded loop in one process, no retry.

``test_stages_repeat_bit_for_bit``: goofer_synth_batch through tests/test_gpu_synth_stages.py's _run on its ``main`` batch, one
route per synthesis pipeline and per transform form.  Bits, not values: the outputs are compared as int32 words.
``test_renderer_repeats_bit_for_bit``: Renderer.run (goofer_render_batch: the assembly in front of the synthesis, the f0 kernel
on the side stream) on the first group of tests/test_gpu_assemble_oracle.py's test_fused_route_equals_split at
(44100, 2046, 512), alternating the fused call with ``split=True`` and, within each, ``overlap`` 1 with 0.  harm, mix and the
envelope rows are compared as words; uv and bre as values (torch.equal), which is what test_fused_route_equals_split holds
``overlap`` 0 to: a skipped transform leaves + 0 where the sum of an all-zero frame leaves - 0.

R is 20 renders a route, and 200 for the two tests at n_fft 2046: docs/HISTORY.md records a harmonic frame of that geometry that
came out as one of two roundings in 5 of 240 renders, and 200 renders miss a fault of that rate with probability 0.98^200 = 1.5 %.
(That one was k_harm_shape at an even bin count: a wave's warp rows had no room for warp_row's pad element, which landed on
bin 0 of the next wave's blur row.  Before the fix test_renderer_repeats_bit_for_bit failed in both fresh processes it was
run in, at render 23 and at render 51 of 200; test_stages_repeat_bit_for_bit[bluestein_2048] passed in both.)
"""
import time

import numpy as np
import pytest

import synth_ref as SR
import test_gpu_assemble_oracle as AO
import test_gpu_synth_stages as ST

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R_DEFAULT, R_FLAKE = 20, 200
FLAKE_GEO = (44100, 2046, 512)
ROUTES = ["walkers", "ola3", "separate", "ola1_skip", "bluestein", "workgroup",
          "bluestein_256", "bluestein_512", "bluestein_2048", "bluestein_wg", "radix3_1536"]
OUTPUTS = ("harm", "uv", "bre", "rec", "mix")
PIPELINE = ("f0", "pulse", "mask_short", "S_harm", "S_uv", "S_breath", "note_mag", "frames", "harm", "uv", "bre", "note_peak", "rec",
            "mix")
PER_SAMPLE = ("f0", "pulse", "harm", "uv", "bre", "rec", "mix")
PER_FRAME = ("S_harm", "S_uv", "S_breath", "frames")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    ST._restore(c)
    c.set_option("overlap", 1)
    c.close()


def _words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint32), a.dtype.itemsize // 4


def _place(stage, elem, cols, s_off, f_off):
    """Where element ``elem`` of a stage's flat array lies: (note, frame or sample[, column])."""
    if stage in PER_SAMPLE:
        k = int(np.searchsorted(s_off, elem, side="right")) - 1
        return "note %d sample %d" % (k, elem - int(s_off[k]))
    if stage in PER_FRAME:
        row, col = divmod(elem, cols)
        k = int(np.searchsorted(f_off, row, side="right")) - 1
        return "note %d frame %d column %d" % (k, row - int(f_off[k]), col)
    if stage == "mask_short":                                  # note k's knots start at s_off[k] // 4 + k
        starts = np.asarray(s_off[:-1]) // SR.MASK_DS + np.arange(len(s_off) - 1)
        k = int(np.searchsorted(starts, elem, side="right")) - 1
        return "note %d knot %d" % (k, elem - int(starts[k]))
    return "note %d" % elem


def staged_report(base, odd, s_off, f_off):
    """The pipeline in order: per stage the words that differ between two runs and the first place that does."""
    lines = []
    n = len(s_off) - 1
    for st in PIPELINE:
        a, b = base.get(st), odd.get(st)
        if a is None or b is None or np.size(a) == 0:
            lines.append("%-10s no view on this route" % st)
            continue
        if st in ("note_mag", "note_peak"):
            a, b = a[:n], b[:n]
        if np.shape(a) != np.shape(b):
            lines.append("%-10s shapes %r / %r" % (st, np.shape(a), np.shape(b)))
            continue
        (wa, per), (wb, _) = _words(a), _words(b)
        diff = np.nonzero(wa != wb)[0]
        if not diff.size:
            lines.append("%-10s equal" % st)
            continue
        elem = int(diff[0]) // per
        cols = np.shape(a)[1] if np.ndim(a) == 2 else 1
        lines.append("%-10s %d of %d words differ, first at %s" % (st, diff.size, wa.size, _place(st, elem, cols, s_off, f_off)))
    return "\n".join(lines)


def _same_words(x, y):
    return x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("route", ROUTES)
def test_stages_repeat_bit_for_bit(ctx, route):
    """MEASURED on the MI355X, seconds per route at its R, uploads included: walkers 0.20, ola3 0.10, separate 0.09,
    ola1_skip 0.15, bluestein 0.11, workgroup 0.17, bluestein_256 0.08, bluestein_512 0.08, bluestein_wg 0.17, radix3_1536 0.14
    (20 repeats each); bluestein_2048 1.2 to 1.5 (200 repeats of the whole main batch: no need to cut it)."""
    geo, opts, names, kind, has_skip = ST.ROUTES[route]
    repeats = R_FLAKE if geo == FLAKE_GEO else R_DEFAULT
    both = ST._batches(geo)
    sigma, notes = both["main"]
    sigma_t, tiny = both["tiny"]
    t0 = time.perf_counter()
    try:
        ST._set(ctx, opts)
        base = ST._run(ctx, geo, notes, sigma, views=True, device=True)
        for r in range(repeats):
            if r % 2 == 1:
                ST._run(ctx, geo, tiny, sigma_t, views=False, device=True)
            got = ST._run(ctx, geo, notes, sigma, views=False, device=True)
            if all(_same_words(got[k], base[k]) for k in OUTPUTS):
                continue
            odd = _fetch_views(ctx, geo, got)
            host = lambda d: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
            pytest.fail("%s: repeat %d of %d differs from the first render\n%s"
                        % (route, r + 1, repeats, staged_report(host(base), host(odd), base["s_off"], base["f_off"])), pytrace=False)
    finally:
        ST._restore(ctx)
    print("%s: %d repeats in %.2f s" % (route, repeats, time.perf_counter() - t0))


def _fetch_views(ctx, geo, res):
    """The debug views of the render that has just run, into ``res`` (the shapes of test_gpu_synth_stages._run)."""
    n_fft = geo[1]
    nb = n_fft // 2 + 1
    F, N, n = int(res["f_off"][-1]), int(res["s_off"][-1]), len(res["s_off"]) - 1
    res = dict(res)
    # The views are those of the handle's LAST synthesis call.  A render whose post chain re-enters the synthesis for a layer
    # ('su', 'sj', 'sa') leaves the views of that smaller call: they have other sizes and are left out (a view of the wrong
    # call compared with itself says "equal" about a stage it never saw).
    for name, size in (("f0", N), ("pulse", N), ("mask_short", N // SR.MASK_DS + n), ("note_mag", n), ("note_peak", n)):
        v = ctx.debug_fetch(name)
        res[name] = v if v.size == size else None
    ldc = ST.SR_STRIDE(nb)
    for name in ("S_harm", "S_uv", "S_breath"):
        v = ctx.debug_fetch(name)
        res[name] = v.reshape(F, ldc)[:, :nb] if v.size == F * ldc else None
    v = ctx.debug_fetch("frames")
    res["frames"] = v.reshape(F, n_fft) if v.size == F * n_fft else None
    return res


def test_renderer_repeats_bit_for_bit(ctx):
    """MEASURED on the MI355X: 200 renders of the twenty notes (222 065 samples, 443 frames) in 0.6 s, the test in 0.8 s.
    Note 16 of the batch carries the 'sa' layer, whose extra synthesis call owns the debug views after a render: the staged
    report of this test has the outputs and the envelope, its intermediate stages read "no view" (_fetch_views).  With the post
    chain taken off the batch (prep["post"] = None) the views are the main call's; that is how the cause of the n_fft 2046
    flake was read off S_harm (docs/HISTORY.md)."""
    from goofer_amd.render import Renderer
    geo = FLAKE_GEO
    cases, _ = AO.cpu(geo)
    plain, _ = AO.A.fused_matrix(*geo)
    shifted = {i: c for i, c in plain}
    idxs = [i for i, _ in plain]
    r = Renderer(ctx, hop=geo[2])
    np.random.seed(11)                                          # as test_fused_route_equals_split: the draws of prepare
    prep = r.prepare(AO._jobs([shifted[i] for i in idxs]), trim_rows=False)
    s_off = np.asarray(prep["sample_off"], dtype=np.int64)
    f_off = np.concatenate([[0], np.cumsum(ctx.frame_counts(prep["lens"]))]).astype(np.int64)
    keys = ("harm", "uv", "bre", "mix")
    words = ("harm", "mix")

    def render(k):
        ctx.set_option("overlap", 1 - (k // 2) % 2)
        out = r.run(prep, seed=5, keep_stems=True, split=bool(k % 2))
        ctx.check()
        return {"harm": out["harm"], "uv": out["uv"], "bre": out["bre"], "mix": out["mix"], "env": prep["env"].clone(),
                "s_off": s_off, "f_off": f_off}

    t0 = time.perf_counter()
    try:
        base = _fetch_views(ctx, geo, render(0))
        for k in range(1, R_FLAKE + 1):
            got = render(k)
            same = all(_same_words(got[q], base[q]) for q in words + ("env",)) and all(torch.equal(got[q], base[q]) for q in keys)
            if same:
                continue
            odd = _fetch_views(ctx, geo, got)
            host = lambda d: {q: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for q, v in d.items()}
            hb, ho = host(base), host(odd)
            env = "env        %d words differ" % int(np.count_nonzero(_words(hb["env"])[0] != _words(ho["env"])[0]))
            pytest.fail("render %d of %d (%s, overlap %d) differs from the first\n%s\n%s"
                        % (k, R_FLAKE, "split" if k % 2 else "fused", 1 - (k // 2) % 2, env, staged_report(hb, ho, s_off, f_off)),
                        pytrace=False)
    finally:
        ctx.set_option("overlap", 1)
    print("renderer: %d renders in %.2f s" % (R_FLAKE, time.perf_counter() - t0))
