"""CPU: tests/post_ref.py pinned to the oracle, and proof that the inputs of tests/test_gpu_post_chain.py have teeth.

(a) ``oracle.sampler_ref.render`` with ``G.synthesize`` stubbed (canned fp32 stems, a different seeded set per call of one
    render, so the su / sj / sa layers are distinguishable) against ``post_ref.post_chain(exact=False)`` on the same stems:
    bit for bit, for every post flag alone and all together; the fry mask and the pd gain curve array for array.  The fry
    range is the host planner's for the same request (test_planner_native.py holds that to the oracle), the bend is the
    fp32 array the oracle hands to its 10 ms Gaussian.
(b) Mutation checks: with the fry fades' endpoint rule, the percentile's interpolation or the ``prev = y[0]`` start of a
    high-pass section broken in a local copy, the per-sample bound of the GPU tests is exceeded on the GPU tests' inputs."""
import numpy as np
import pytest

import post_ref as P
from goofer_amd import sampler as S
from goofer_amd import synthetic as syn
from oracle import sampler_ref as SR

F32 = np.float32
FLAGS = ["st50", "st-50", "sd30", "vf40", "vf-40vh70vl40", "pd50", "pd-50", "su50", "sj30", "sa30",
         "su40sj30sa20vf-40vh70vl40sd30st50pd-50V90B10U-10"]


class _Stems:
    """Stand-in for G.synthesize: (rec, harm, uv, bre) of len(mask), seeded by the call's position in the render."""

    def __init__(self):
        self.calls = []

    def __call__(self, env, f0, mask, y, sr, **kw):
        harm, uv, bre = P.stems(900 + len(self.calls), len(mask), sr)
        self.calls.append((harm.copy(), uv.copy(), bre.copy()))
        return None, harm, uv, bre


def _fry_range(req_args, src, hop=256):
    req = S.decode_request(*req_args)
    tracks = [S.source_tracks64(src["formants"])]
    rec = S.plan_records([req], [src["sr"]], [src["y_len"]], [1 + src["y_len"] // hop], tracks)
    plan = S.plan_native(rec, hop, True, keep=(tracks, rec))
    assert plan is not None
    g = plan.geo[0]
    return int(g["fry_a"]), int(g["fry_b"]), int(g["fry_fade"])


@pytest.mark.parametrize("flags", FLAGS)
def test_post_chain_equals_the_stubbed_oracle_render(flags, monkeypatch):
    src = syn.make_source(7100, seconds=0.3)
    sr = src["sr"]
    args = syn.request_args(syn.make_request(7100, flags, length_ms=120.0, offset_ms=20.0, consonant_ms=40.0, cutoff_ms=30.0))
    stub, bends, real_gauss = _Stems(), [], SR.G.gauss1d

    def spy(a, sigma, axis=-1):
        arr = np.asarray(a)
        if arr.ndim == 1 and arr.dtype == F32 and sigma == max(1, int(0.010 * sr)):
            bends.append(arr.copy())
        return real_gauss(a, sigma, axis)

    monkeypatch.setattr(SR.G, "synthesize", stub)
    monkeypatch.setattr(SR.G, "gauss1d", spy)
    p = SR.decode_request(*args)
    feats = (src["env_pack"], src["f0"].copy(), src["mask"].copy(), {k: v.copy() for k, v in src["formants"].items()}, sr,
             src["y_len"])
    out, a, stems0 = SR.render(feats, p, seed=5, return_parts=True)
    n = len(a["mask"])
    assert n > int(0.1 * sr) and out.shape == (n,)

    calls = list(stub.calls)
    harm, uv, bre = calls.pop(0)
    assert all(np.array_equal(x, y) for x, y in zip((harm, uv, bre), stems0))
    su = calls.pop(0)[0] if p.subharm_gain > 0.0 else None
    sj = calls.pop(0)[0] if p.growl_mix > 0.0 else None
    sa = calls.pop(0)[1:] if p.aperiodic_mix > 0.0 else (None, None)
    assert not calls
    fa, fb, fade = _fry_range(args, src)
    note = P.note_fields(su_gain=p.subharm_gain, sj_mix=p.growl_mix, sa_mix=p.aperiodic_mix, sd_strength=p.sd_strength,
                         tension=p.tension, pitch_dyn=p.pitch_dyn, fry_a=fa, fry_b=fb, fry_fade=fade)
    mix = P.mix_fields(mix_harm=p.harmonic_mix, mix_breath=p.breathiness_mix, mix_unvoiced=p.unvoiced_mix, volume=p.volume)
    bend = bends[0] if p.pitch_dyn != 0.0 else None
    f0, mask = a["f0"].astype(F32), a["mask"]

    fm = P.fry_mask(n, fa, fb, fade)
    assert (fm is None) == (a["fry_mask"] is None) == ("vf" not in flags)
    if fm is not None:
        assert fm.dtype == a["fry_mask"].dtype and np.array_equal(fm, a["fry_mask"])
        assert 0 < np.count_nonzero(fm) < n
    if p.pitch_dyn != 0.0:
        dg = P.dyn_gain(bend, mask, p.pitch_dyn, sr)
        assert dg.dtype == a["dyn_gain"].dtype and np.array_equal(dg, a["dyn_gain"])
        assert dg.max() - dg.min() > 0.1
    else:
        assert a["dyn_gain"] is None

    _, _, got = P.post_chain(harm, uv, bre, f0, mask, bend, note, mix, sr, su_harm=su, sj_harm=sj, sa_uv=sa[0], sa_bre=sa[1])
    assert got.dtype == out.dtype and np.array_equal(got, out), float(np.max(np.abs(got - out)))
    plain = P.stage_mix(harm, uv, bre, mix)
    assert np.max(np.abs(plain - out)) > 1e-3 * np.max(np.abs(out))      # the flag did something


# ---------------------------------------------------------------------------------------------
# mutation checks: the bound of the GPU tests, the inputs of the GPU tests, the function broken in a local copy
# ---------------------------------------------------------------------------------------------
def _cascade_zero_start(xs, alphas, orders, btype, exact=False):
    """post_ref.cascade with the high-pass's x_{-1} = 0 instead of x_0."""
    dt = P.F64 if exact else P.F32
    out = []
    for x, al, order in zip(xs, alphas, orders):
        y = np.asarray(x, dtype=dt).copy()
        al = np.asarray(al, dtype=dt)
        for _ in range(max(1, int(order))):
            yp, prev = dt(0.0), dt(0.0)
            for i in range(len(y)):
                xp = y[i]
                yp = al[i] * ((yp + xp) - prev) if btype != "lowpass" else yp + al[i] * (xp - yp)
                prev = xp
                y[i] = yp
        out.append(y)
    return out


def test_a_wrong_fry_endpoint_exceeds_the_bound(monkeypatch):
    sr = 44100
    cases = P.fry_cases(sr)
    truth = [P.stage_fry(c["harm"], c["bre"], c["fry_a"], c["fry_b"], c["fry_fade"], sr, exact=True) for c in cases]
    ref = [P.stage_fry(c["harm"], c["bre"], c["fry_a"], c["fry_b"], c["fry_fade"], sr) for c in cases]
    monkeypatch.setattr(P, "ramp", lambda start, stop, m: np.linspace(start, stop, m, endpoint=False))
    caught = 0
    for c, t, r in zip(cases, truth, ref):
        bad = P.stage_fry(c["harm"], c["bre"], c["fry_a"], c["fry_b"], c["fry_fade"], sr)
        ok = all(P.within(*P.errors(b_, r_, t_)) for b_, r_, t_ in zip(bad, r, t))
        assert all(P.within(*P.errors(r_, r_, t_)) for r_, t_ in zip(r, t))
        if c["fry_b"] - c["fry_a"] >= 2:                      # a range of one sample has one-point ramps: 0 under either rule
            assert not ok, (c["fry_a"], c["fry_b"], c["fry_fade"])
            caught += 1
    assert caught >= 9


def test_a_percentile_without_interpolation_exceeds_the_bound(monkeypatch):
    sr = 44100
    cases = P.pd_cases(sr)
    mixf = P.mix_fields()
    run = lambda c, exact: P.post_chain(c["harm"], c["uv"], c["bre"], c["f0"], c["mask"], c["bend"],
                                        P.note_fields(pitch_dyn=c["pitch_dyn"]), mixf, sr, exact=exact)[2]
    truth = [run(c, True) for c in cases]
    ref = [run(c, False) for c in cases]
    monkeypatch.setattr(P, "percentile95", lambda x: float(np.sort(x)[int(np.floor(0.95 * (len(x) - 1)))]))
    caught = 0
    for c, t, r in zip(cases, truth, ref):
        ok = P.within(*P.errors(run(c, False), r, t))
        if c["level_shift"] > 1e-5:                           # moves the gain by 1.4 times as much: far beyond the bound
            assert not ok, c["name"]
            caught += 1
        elif c["level_shift"] == 0.0:                         # ties, 0.95 (n - 1) an integer, n = 1: nothing to interpolate
            assert ok, c["name"]
    assert caught >= 2


def test_a_high_pass_started_from_zero_exceeds_the_bound(monkeypatch):
    sr = 44100
    xs, f0s = P.cascade_inputs()
    keep = [i for i, x in enumerate(xs) if len(x) <= 2049]
    xs, f0s = [xs[i] for i in keep], [f0s[i] for i in keep]
    order, btype, mode, cf = next(s for s in P.CASCADE_SETTINGS if s[1] == "highpass" and s[0] == 4)
    truth = P.dynamic_filter_batch(xs, f0s, sr, cf, order, btype, mode, exact=True)
    ref = P.dynamic_filter_batch(xs, f0s, sr, cf, order, btype, mode)
    monkeypatch.setattr(P, "cascade", _cascade_zero_start)
    bad = P.dynamic_filter_batch(xs, f0s, sr, cf, order, btype, mode)
    for x, b_, r_, t_ in zip(xs, bad, ref, truth):
        assert P.within(*P.errors(r_, r_, t_))
        assert not P.within(*P.errors(b_, r_, t_)), len(x)
