"""GPU: what the finishing stages share, at the smallest shapes at which it can go wrong.  ``Renderer.render`` and
``render_phrase`` with the rate conversion, the compressor, the loudness stage and a true-peak limiter all at once against the
same ``Context`` calls made by hand (bit for bit: the chain adds no arithmetic of its own), and the argument checks of the five
stage methods (``Context._signals``) on a batch of two signals, one shorter than a tile and one a sample longer: every refusal
is a ValueError in the stage's name, raised on the host before anything is launched, and the offsets are taken as a device
tensor, as a host list and as None with the same bits."""
import math

import numpy as np
import pytest

from goofer_amd import compress as CP
from goofer_amd import limit as LM
from goofer_amd import loudness as LD
from goofer_amd import rate as RT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SR, OUT_SR = 44100, 48000
LOUDNESS, LIMIT = -16.0, LM.Limiter(0.1, true_peak=True)     # (-20 dBTP under -16 LUFS: the limiter has work to do)
LENS = [5, 4097]
STAGES = ["rate_convert", "limit", "true_peak", "loudness", "compress"]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _jobs():
    """three synthetic notes (goofer_amd.synthetic.make_source, as the compressor's tests make theirs) and a phrase of them"""
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Source
    requests = [("C4", "100", "g-10", "30", "300", "80", "50", "100", "0", "!120", "AA"),
                ("E4", "100", "t30fa20fb-10B30", "30", "300", "80", "50", "120", "0", "!120", "AA#20#AP"),
                ("A3", "120", "vf30sa20pd40", "30", "300", "80", "50", "110", "0", "!120", "AA#10#BA#10#AA")]
    jobs = []
    for i, args in enumerate(requests):
        src = syn.make_source(100 + i, seconds=0.3)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
    return jobs, ["0 250 5 35 40 0 100 100 0 0", "10 240@120+30 5 35 40 20 100 90 10 30", "R 120", "5 200 5 35 40 0 100 100 0 40"]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _compressor(x):
    """a threshold 12 dB under the peak of ``x``, inside the definition's range: the compressor has work to do"""
    peak = float(np.abs(x).max())
    assert peak > 10.0 ** (-60.0 / 20.0)
    return CP.Compressor(max(-80.0, min(0.0, round(20.0 * math.log10(peak) - 12.0, 1))), 4.0, attack_ms=2.0, release_ms=60.0)


def _by_hand(ctx, xs, st):
    """convert, compress, loudness, true-peak limit and the meter behind it over the signals ``xs`` at SR: the five Context
    calls, each on a plan made here; (the signals at OUT_SR, the statistics as the stages return them)"""
    x = ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))
    rplan = RT.plan(SR, OUT_SR, [len(v) for v in xs])
    lens = np.diff(rplan.out_off)
    conv = ctx.rate_convert(x, None, rplan)
    comp, red, _ = ctx.compress(conv, None, CP.plan(OUT_SR, lens, st))
    y, loud, gain, _ = ctx.loudness(comp, None, LD.plan(OUT_SR, lens), LOUDNESS)
    lplan = LM.plan(OUT_SR, lens, LIMIT.ceiling, LIMIT.lookahead_ms, True)
    lim, peak, gmin = ctx.limit(y, None, lplan)
    tp_out = ctx.true_peak(lim, None, lplan)
    ctx.check()
    assert not _same(comp.cpu().numpy(), conv.cpu().numpy()) and float(gmin.min()) < 1.0          # every stage had work to do
    lim = lim.cpu().numpy()
    return [lim[rplan.out_off[i]:rplan.out_off[i + 1]] for i in range(rplan.n)], (red, loud, gain, peak, gmin, tp_out)


def test_render_with_the_four_settings_is_the_four_calls_by_hand(ctx):
    from goofer_amd.render import Renderer
    jobs, _ = _jobs()
    r = Renderer(ctx)
    notes = r.render(jobs, seed=5)
    st = _compressor(np.concatenate(notes))
    want, _ = _by_hand(ctx, notes, st)
    got = r.render(jobs, seed=5, out_sr=OUT_SR, compress=st, loudness=LOUDNESS, limit=LIMIT)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert len(a) > 4096 and _same(a, b)
    # the settings in their other spellings are the same chain
    spelled = r.render(jobs, seed=5, out_sr=OUT_SR, compress=(st.threshold_db, 4, 2, 60), loudness=(LOUDNESS, LD.MAX_GAIN_DB),
                       limit=(LIMIT.ceiling, LIMIT.lookahead_ms, True))
    assert all(_same(a, b) for a, b in zip(spelled, want))


def test_render_phrase_with_the_four_settings_reports_every_statistic(ctx):
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    plain = r.render_phrase(jobs, entries, seed=5)
    st = _compressor(plain)
    (want,), (red, loud, gain, peak, gmin, tp_out) = _by_hand(ctx, [plain], st)
    got, stats = r.render_phrase(jobs, entries, seed=5, out_sr=OUT_SR, compress=st, loudness=LOUDNESS, limit=LIMIT, return_stats=True)
    assert _same(got, want)
    assert sorted(stats) == sorted(["peak_in", "min_gain", "true_peak_in", "true_peak_out", "lufs_in", "momentary_max", "gain",
                                    "max_reduction_db"])
    assert stats == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "true_peak_in": float(peak.cpu()[0]),
                     "true_peak_out": float(tp_out.cpu()[0]), "lufs_in": float(loud.cpu()[0, 0]), "momentary_max": float(loud.cpu()[0, 1]),
                     "gain": float(gain.cpu()[0]), "max_reduction_db": float(red.cpu()[0])}
    assert stats["max_reduction_db"] > 1.0 and stats["min_gain"] < 1.0 and stats["gain"] != 1.0


def _stage(ctx, stage):
    """(the stage's plan for LENS, call(x, d_off, out=None) -> the tensors the stage returns, whether it takes ``out``)"""
    if stage == "rate_convert":
        plan = RT.plan(SR, OUT_SR, LENS)
        return plan, lambda x, d_off, out=None: (ctx.rate_convert(x, d_off, plan, out=out),), plan.total_out
    if stage == "limit":
        plan = LM.plan(OUT_SR, LENS, 0.25)
        return plan, lambda x, d_off, out=None: ctx.limit(x, d_off, plan, out=out), plan.total
    if stage == "true_peak":
        plan = LM.true_peak_plan(OUT_SR, LENS)
        return plan, lambda x, d_off: (ctx.true_peak(x, d_off, plan),), None
    if stage == "loudness":
        plan = LD.plan(OUT_SR, LENS)
        return plan, lambda x, d_off, out=None: ctx.loudness(x, d_off, plan, LOUDNESS, out=out), plan.total
    plan = CP.plan(OUT_SR, LENS, CP.Compressor(-30.0, 4.0))
    return plan, lambda x, d_off, out=None: ctx.compress(x, d_off, plan, out=out, curve=True), plan.total


def _signal(ctx):
    x = (0.3 * np.random.default_rng(11).standard_normal(sum(LENS) + 1)).astype(np.float32)
    return ctx.tensor(x)


@pytest.mark.parametrize("stage", STAGES)
def test_every_stage_refuses_the_same_arguments_in_its_own_name(ctx, stage):
    plan, call, n_out = _stage(ctx, stage)
    total, named = sum(LENS), "^%s: " % stage
    x = _signal(ctx)
    bad = {"a float64 x": (x.double(), None),
           "a non-contiguous x": (torch.zeros(2 * total, dtype=torch.float32, device=ctx.device)[::2], None),
           "an x one sample short": (x[:total - 1], None),
           "a d_off tensor of the wrong length": (x, ctx.tensor(np.array([0, 5, total, total], dtype=np.int64))),
           "a d_off tensor of the wrong type": (x, ctx.tensor(np.array([0, 5, total], dtype=np.int32))),
           "a host d_off that is not the plan's": (x, [0, 6, total])}
    assert bad["a non-contiguous x"][0].numel() == total and not bad["a non-contiguous x"][0].is_contiguous()
    for what, (xx, d_off) in bad.items():
        with pytest.raises(ValueError, match=named):
            call(xx, d_off)
    if n_out is not None:
        for out in (torch.zeros(n_out + 1, dtype=torch.float32, device=ctx.device), torch.zeros(n_out - 1, dtype=torch.float32, device=ctx.device),
                    torch.zeros(n_out, dtype=torch.float64, device=ctx.device)):
            with pytest.raises(ValueError, match=named):
                call(x, None, out=out)
    ctx.check()                                                 # nothing was launched, nothing is flagged


@pytest.mark.parametrize("stage", STAGES)
def test_every_stage_takes_the_offsets_three_ways(ctx, stage):
    plan, call, n_out = _stage(ctx, stage)
    x = _signal(ctx)
    runs = []
    for d_off in (ctx.tensor(plan.in_off), [int(v) for v in plan.in_off], None):
        res = call(x, d_off)
        ctx.check()
        runs.append([t.cpu().numpy() for t in res if t is not None])
    assert len(runs[0]) >= 1 and len(runs[0][0])               # (the segment energies are empty: no signal here has a whole segment)
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(_same(a, b) for a, b in zip(other, runs[0]))
    if n_out is not None:                                       # and writes where it is told to
        out = torch.full((n_out,), 7.0, dtype=torch.float32, device=ctx.device)
        res = call(x, None, out=out)
        ctx.check()
        assert res[0] is out and _same(out.cpu().numpy(), runs[0][0])
