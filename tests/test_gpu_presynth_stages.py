"""GPU: the sample-domain stages in front of the spectra that the sh / sr / sg flags drive — csrc/jitter.hip (k_gauss_samples,
k_note_absmax, k_f0_jitter, k_volume_jitter), the sub-harmonic layer of csrc/pulse.hip (k_subharm_inc, k_pulse_onsets_wrap,
k_subharm_finish, k_subharm_place, k_subharm_add) and their glue in csrc/synth.hip (k_note_flags, k_note_sub_flags, the f0_64
copy, the jitter in front of the forked pulse chain) — sample by sample against the float64 restatement of tests/presynth_ref.py.

One ragged batch (presynth_ref.cases: ten notes of 1 to 6 000 samples, 10 968 in all, at 44100 / 1024 / 256, normalize 0 so the
stems come back raw), every second note with the flag under test, the injected draws of the others filled with NaN.  Inputs go in
through Context.synth_batch, results come out through debug_fetch and the returned stems; the route of every run is asserted
through profile_stage_names.  No RMS, no sample left out, nothing non-finite anywhere.

sh   the f0 view within ONE fp32 ulp of the restatement's cast.  Derived, not measured: the float64 FIR (2 r + 1 products in
     ascending order, fused or not) and the division put the factor within about (2 r + 1) 2^-53 relative of the exact one, so
     only a product within that of an fp32 rounding tie can round the other way, and then by one ulp.  Bit-equal to the scaled
     input where mask == 0, bit-equal to a run without the flag on every unflagged note (all outputs too).  The pulse view equals
     oracle.goofer_ref.pulse_train of the DEVICE's f0 view within the 5e-6 of tests/test_gpu_kernels.py: on the default route the
     pulse chain runs on the side stream behind the jitter on the caller's, and an ordering fault would be O(1).
sg   onset_cnt / onset_idx (at sample_off[k] + 16 k) exactly the restatement's events of the last ratio, none for a weight of 0;
     per sample  |pulse - truth| <= 2^-24 |truth| + c 2^-23 (weight / max) A + 2^-149,  truth = float64(pulse of the same batch
     without the layer) + layer, A = the sum of the covering normalised pulse values times the mask.
     c = 7: a normalised pulse sample is fp32(raw) / fp32(peak) in fp32.  The device's sin / exp / cos differ from numpy's by
     ulps of float64, so fp32(raw) is numpy's or, at a rounding tie, its neighbour: relative 2^-23 at most; the same for the
     peak; the correctly rounded fp32 quotients of the two pairs then differ by 2^-23 + 2^-23 + 2 * 2^-24 = 3 * 2^-23 relative.
     Every sample is >= 0 (Rk = 1), so the float64 sum S <= A carries the same 3 * 2^-23, and so does the note's maximum, which is
     such a sum.  layer = weight S / max: (3 + 3) 2^-23 (weight / max) A; the seventh unit covers the float64 roundings and every
     second-order term (under 2^-44 each); the fp32 store of pulse + layer is the 2^-24 |truth| (2^-149 below the normal range).
     Bit-equal to the run without the layer: notes of weight 0, the flagged all-unvoiced note, every sample no event covers.
     With subharm_f0_jitter the f0 view shows the second jitter (one ulp, as above), applied after the pulse train — the main
     train is bit-equal to the run without the layer — and the restatement tracks the device's own f0 view.
sr   (stems 0 on both runs, so the run without the flag takes the same route) harm and bre within one fp32 ulp of
     fp32(float64(stem without the flag) * factor), uv bit-equal, unflagged notes bit-equal in every output, note_peak exactly
     max |(h + u) + b| in fp32 over the returned stems, rec exactly (h + u) + b.

tests/test_presynth_ref.py shows on the CPU that six wrong variants (half-up rounding, no key cache, end_max without its carry,
the latest event only, 'symmetric' padding, a maximum without + 1e-6) break these bounds by factors of 1e2 to 1e6.

What the batch cannot show: a note's samples from its last frame's hop on are zero in every stem (all of them in a note under
one hop), and the smoothed mask of an all-unvoiced note is zero, so the volume jitter has nothing to move in the notes of 1, 3,
100 and 255 samples; it is judged on 8 704 (flagged notes 0, 2, 4, ...) and 1 280 (1, 3, 5, ...) non-zero harmonic samples.  The
short notes' reflections are judged through the f0 view (radius 294 against 100, 3 and 1 samples), the same kernel.

MEASURED on the MI355X (each test prints its figures):
  sh   samples of the f0 view whose bits differ from the restatement's cast: 0 of 9 172 (flagged notes 0, 2, ..: 7 706 moved by
       the jitter) and 0 of 1 796 (notes 1, 3, ..: 1 094 moved), the same on both routes, with and without f0_64
  sg   worst error / bound, and the share of c the layer's own terms used (the error beyond the store's half ulp, in units of
       2^-23 (weight / max) A):   one 0.841, 0.000   three 0.755, 0.000   vibrato 0.752, 0.000   jitter 0.630, 0.000 (0 f0
       samples differ from the cast)   f0_64 0.753, 0.000 — every error is the fp32 store's own rounding
  sr   harm / bre samples whose bits differ from the cast: 0 / 0 of 9 172 and of 1 796, noise and vibrato form alike
"""
import numpy as np
import pytest

import presynth_ref as P
from oracle import goofer_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
SR0 = P.GEO[0]

_HEAD = ["setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place"]
_TAIL = ["env_edit", "env_rows", "sample_assemble"]
STEMS = _HEAD + ["mask_short", "noise_stems", "", "harm_stem", "", "", "", "note_finish", ""] + _TAIL
OLA = _HEAD + ["rfft_frames", "harm_shape", "", "noise_spectra", "", "", "mask_short", "irfft_ola3", "apply_gain"] + _TAIL
ROUTES = {"walkers": ({}, STEMS), "stems0": ({"stems": 0}, OLA)}
DEFAULTS = {"stems": 1}
OUTS = ("harm", "uv", "bre", "rec", "mix")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    for k, v in DEFAULTS.items():
        c.set_option(k, v)
    c.close()


def _set(ctx, opts):
    for k, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(k, v)


def _restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.plan(*P.GEO)


def _run(ctx, f0s, keep=None, flags=None, nan_parity=None, **call):
    """One goofer_synth_batch over the notes ``keep`` (default: all) of the batch with the f0 arrays ``f0s``; ``flags``: parameter
    name -> per-note values (of all ten notes); ``call``: synth_batch's keyword arguments, per-sample arrays given for the whole
    batch as host arrays (cut to ``keep`` and, with ``nan_parity``, NaN in the notes without the flag).  Returns the outputs, the
    views and the stage names as host arrays."""
    from goofer_amd.device import default_params
    d = P.cases()
    keep = list(range(len(P.LENGTHS))) if keep is None else list(keep)
    notes = [d["notes"][k] for k in keep]
    ctx.plan(*P.GEO)
    par = default_params(len(keep))
    par["normalize"] = 0.0
    par["pitch_shift"] = [c["ps"] for c in notes]
    for name, v in (flags or {}).items():
        par[name] = np.asarray(v)[keep]

    def cut(x):
        if nan_parity is not None:
            x = P.nan_outside(x, d["off"], nan_parity)
        return ctx.tensor(np.concatenate([x[d["off"][k]:d["off"][k + 1]] for k in keep]))
    for name in ("noise_f0", "noise_subharm", "f0_64"):
        if call.get(name) is not None:
            call[name] = cut(call[name]) if name != "f0_64" else ctx.tensor(
                np.concatenate([call[name][d["off"][k]:d["off"][k + 1]] for k in keep]))
    if call.get("noise_vol") is not None:
        call["noise_vol"] = tuple(cut(x) for x in call["noise_vol"])
    env = ctx.rows_from(np.concatenate([c["env"] for c in notes]))
    phi = ctx.rows_from(np.concatenate([c["phi"] for c in notes]))
    ctx.profile_begin(1)
    try:
        out = ctx.synth_batch(env, [c["T"] for c in notes], ctx.tensor(np.concatenate([f0s[k] for k in keep])),
                              ctx.tensor(np.concatenate([c["mask"] for c in notes])), [c["n"] for c in notes], par, phi=phi, **call)
        torch.cuda.synchronize()
    except RuntimeError as e:                                 # GooferError or torch's device error: nothing more is started on this GPU
        pytest.exit("goofer_synth_batch failed on the device: %r" % (e,), returncode=3)
    res = {k: out[k].cpu().numpy() for k in OUTS}
    ctx.profile_end()
    res["names"] = ctx.profile_stage_names()
    ctx.check()
    res["off"] = np.asarray(out["sample_off"], dtype=np.int64)
    for name in ("f0", "pulse", "onset_cnt", "onset_idx", "note_peak"):
        res[name] = ctx.debug_fetch(name)
    for name in OUTS + ("f0", "pulse", "note_peak"):
        assert np.all(np.isfinite(res[name])), name
    return res


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _plain_f0():
    return [c["f0"] for c in P.cases()["notes"]]


def _within_one_ulp(got, want32):
    return np.abs(got.astype(F64) - want32.astype(F64)) <= P.ulp32(want32)


def _unflagged_only_gives_plain_bits(ctx, opts, names, f0s, parity, flags, **call):
    """A batch of the notes without the flag, under the group's call arguments, against the same batch with none of them."""
    d = P.cases()
    keep = [k for k in range(len(P.LENGTHS)) if not P.flagged(k, parity)]
    zero = {name: np.zeros(len(P.LENGTHS)) for name in flags}
    _set(ctx, opts)
    with_args = _run(ctx, f0s, keep=keep, flags=zero, nan_parity=parity, **call)
    plain = _run(ctx, f0s, keep=keep)
    assert with_args["names"] == names
    for name in OUTS + ("f0", "pulse"):
        assert _same_bits(with_args[name], plain[name]), ("unflagged notes only", name)


# ---------------------------------------------------------------------------------------------
# sh: f0 jitter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", (0, 1))
@pytest.mark.parametrize("with64", (False, True), ids=("f32", "f0_64"))
@pytest.mark.parametrize("route", list(ROUTES))
def test_f0_jitter(ctx, route, with64, parity):
    d = P.cases()
    opts, names = ROUTES[route]
    f0s = _plain_f0()
    n_notes = len(P.LENGTHS)
    strength = np.array([P.SH["strength"] if P.flagged(k, parity) else 0.0 for k in range(n_notes)])
    f64 = d["f0_64"]["plain"] if with64 else None
    try:
        _set(ctx, opts)
        got = _run(ctx, f0s, flags={"f0_jitter": strength}, nan_parity=parity, noise_f0=d["noise"]["f0"],
                   f0_jitter_speed=P.SH["speed"], f0_64=f64)
        base = _run(ctx, f0s)
        _unflagged_only_gives_plain_bits(ctx, opts, names, f0s, parity, {"f0_jitter": strength}, noise_f0=d["noise"]["f0"],
                                         f0_jitter_speed=P.SH["speed"], f0_64=f64)
    finally:
        _restore(ctx)
    assert got["names"] == names and base["names"] == names
    sigma = SR0 / (P.SH["speed"] * 6)
    differ = total = changed = 0
    for k, c in enumerate(d["notes"]):
        a, b = int(d["off"][k]), int(d["off"][k + 1])
        scaled = P.scaled_f0(c)
        f0v = got["f0"][a:b]
        assert _same_bits(base["f0"][a:b], scaled), (c["name"], "the scaled input")
        if not P.flagged(k, parity):
            assert _same_bits(f0v, scaled), (c["name"], "f0 of a note without the flag")
            for name in OUTS + ("pulse",):
                assert _same_bits(got[name][a:b], base[name][a:b]), (c["name"], name, "a note without the flag")
        else:
            _, want = P.f0_after_jitter(scaled, c["mask"], d["noise"]["f0"][a:b], P.SH["strength"], sigma,
                                        f0_64=f64[a:b] if with64 else None)
            assert np.all(_within_one_ulp(f0v, want)), (c["name"], "f0 against the restatement's cast")
            off = c["mask"] == 0
            assert _same_bits(f0v[off], scaled[off]), (c["name"], "f0 where mask == 0")
            differ += int(np.sum(_bits(f0v) != _bits(want)))
            changed += int(np.sum(_bits(f0v) != _bits(scaled)))
            total += c["n"]
        ref = R.pulse_train(f0v, SR0)
        assert np.max(np.abs(got["pulse"][a:b] - ref)) < 5e-6, (c["name"], "pulse against the oracle's train of the device's f0")
    print("MEASURED sh %s %s parity %d: %d of %d samples differ from the restatement's cast (%d moved by the jitter)"
          % (route, "f0_64" if with64 else "f32", parity, differ, total, changed))
    assert changed > total // 3


# ---------------------------------------------------------------------------------------------
# sg: the sub-harmonic layer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(P.SG_CASES))
def test_sub_harmonic_layer(ctx, case):
    d = P.cases()
    subharm, sjit, with64 = P.SG_CASES[case]
    f0s = d["sg_f0"]
    n_notes = len(P.LENGTHS)
    on = np.array([P.flagged(k) for k in range(n_notes)])
    flags = {"subharm_weight": np.where(on, P.SG_WEIGHT, 0.0), "subharm_f0_jitter": np.where(on, sjit, 0.0)}
    call = dict(subharm=subharm, f0_64=d["f0_64"]["sg"] if with64 else None, f0_jitter_speed=P.SH["speed"])
    if sjit > 0:
        call["noise_subharm"] = d["noise"]["sub"]
    try:
        _set(ctx, {})
        got = _run(ctx, f0s, flags=flags, nan_parity=0, **call)
        _set(ctx, {"stems": 0})
        base = _run(ctx, f0s)
        _set(ctx, {})
        _unflagged_only_gives_plain_bits(ctx, {"stems": 0}, OLA, f0s, 0, flags, **call)
    finally:
        _restore(ctx)
    assert got["names"] == OLA and base["names"] == OLA       # the layer takes the spectra route whatever `stems` says
    assert got["onset_cnt"].size == n_notes and got["onset_idx"].size == d["N"] + 16 * n_notes + 16
    worst, used, f0_differ = 0.0, 0.0, 0
    for k, c in enumerate(d["notes"]):
        a, b = int(d["off"][k]), int(d["off"][k + 1])
        scaled = P.scaled_f0(c, f0s[k])
        slot = a + 16 * k
        if not on[k]:
            assert got["onset_cnt"][k] == 0, (c["name"], "events under a weight of 0")
            assert _same_bits(got["f0"][a:b], scaled)
            for name in OUTS + ("pulse",):
                assert _same_bits(got[name][a:b], base[name][a:b]), (c["name"], name, "a note of weight 0")
            continue
        f0v = got["f0"][a:b]
        if sjit > 0:
            want = P.sg_jittered_f0(case, k)
            assert np.all(_within_one_ulp(f0v, want)), (c["name"], "f0 after the second jitter")
            assert _same_bits(f0v[c["mask"] == 0], scaled[c["mask"] == 0])
            assert np.any(_bits(f0v) != _bits(scaled)) or not np.any(c["mask"])
            f0_differ += int(np.sum(_bits(f0v) != _bits(want)))
            s = P.sg_note(case, k, f0s=f0v)                     # the layer of the device's own f0
            assert not any(e["fragile"].any() or e["key_edge"].any() for e in s["events"])
        else:
            assert _same_bits(f0v, scaled), (c["name"], "f0 is not the layer's to change")
            s = P.sg_truth(case)[k]
        ev = s["events"][-1]["i"]
        assert got["onset_cnt"][k] == ev.size, (c["name"], "event count of the last ratio")
        assert np.array_equal(got["onset_idx"][slot:slot + ev.size], ev), (c["name"], "events of the last ratio")
        truth = base["pulse"][a:b].astype(F64) + s["layer"]
        err = np.abs(got["pulse"][a:b].astype(F64) - truth)
        bound = P.layer_bound(truth, s)
        worst = max(worst, float(np.max(err / bound)))
        # what of c the layer's own terms used: the error beyond the store's rounding, in units of 2^-23 (weight / max) A
        unit = P.layer_bound(0.0 * truth, s, c=1.0) - 2.0 ** -149
        beyond = np.maximum(err - 2.0 ** -24 * np.abs(truth) - 2.0 ** -149, 0.0)
        used = max(used, float(np.max(np.where(unit > 0, beyond / np.where(unit > 0, unit, 1.0), 0.0))))
        assert np.all(err <= bound), (c["name"], case, "pulse", float(np.max(err / bound)), int(np.argmax(err / bound)))
        uncovered = s["C"] == 0
        assert _same_bits(got["pulse"][a:b][uncovered], base["pulse"][a:b][uncovered]), (c["name"], "samples no event covers")
        if not np.any(c["mask"]):
            assert got["onset_cnt"][k] == 0 and _same_bits(got["pulse"][a:b], base["pulse"][a:b]), (c["name"], "all unvoiced")
        else:
            assert k in (4,) or np.any(_bits(got["pulse"][a:b]) != _bits(base["pulse"][a:b])), (c["name"], "the layer is there")
    print("MEASURED sg %s: worst error / bound %.3f, of c = %g used %.3f%s" % (case, worst, P.C_PULSE, used, ", %d f0 samples differ from the cast" % f0_differ if sjit > 0 else ""))


# ---------------------------------------------------------------------------------------------
# sr: volume jitter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", (0, 1))
@pytest.mark.parametrize("form", ("noise", "vibrato"))
def test_volume_jitter(ctx, form, parity):
    d = P.cases()
    vibrato = form == "vibrato"
    cfg = P.SR_VIB if vibrato else P.SR_NOISE
    f0s = _plain_f0()
    n_notes = len(P.LENGTHS)
    sh = np.array([cfg["harm"] if P.flagged(k, parity) else 0.0 for k in range(n_notes)], dtype=F32)
    sb = np.array([cfg["breath"] if P.flagged(k, parity) and k not in P.HARM_ONLY else 0.0 for k in range(n_notes)], dtype=F32)
    flags = {"vol_jitter_harm": sh, "vol_jitter_breath": sb}
    call = dict(vol_jitter_speed=cfg["speed"], volume_vibrato=vibrato)
    if not vibrato:
        call["noise_vol"] = (d["noise"]["vol_h"], d["noise"]["vol_b"])
    opts = {"stems": 0}
    try:
        _set(ctx, opts)
        got = _run(ctx, f0s, flags=flags, nan_parity=parity, **call)
        base = _run(ctx, f0s)
        _unflagged_only_gives_plain_bits(ctx, opts, OLA, f0s, parity, flags, **call)
    finally:
        _restore(ctx)
    assert got["names"] == OLA and base["names"] == OLA
    differ = {"harm": 0, "bre": 0}
    total = live = moved = 0
    for k, c in enumerate(d["notes"]):
        a, b = int(d["off"][k]), int(d["off"][k + 1])
        h, u, br = got["harm"][a:b], got["uv"][a:b], got["bre"][a:b]
        assert _same_bits(got["f0"][a:b], base["f0"][a:b]) and _same_bits(got["pulse"][a:b], base["pulse"][a:b])
        assert _same_bits(u, base["uv"][a:b]), (c["name"], "uv")
        comb = (h + u) + br                                     # fp32, in this order
        assert _same_bits(got["rec"][a:b], comb), (c["name"], "rec")
        assert _bits(got["note_peak"][k:k + 1])[0] == _bits(np.max(np.abs(comb), keepdims=True))[0], (c["name"], "note_peak")
        if not P.flagged(k, parity):
            for name in OUTS:
                assert _same_bits(got[name][a:b], base[name][a:b]), (c["name"], name, "a note without the flag")
            continue
        gh, gb = P.volume_gains(c["n"], SR0, c["mask"], d["noise"]["vol_h"][a:b], d["noise"]["vol_b"][a:b], sh[k], sb[k],
                                cfg["speed"], vibrato)
        for name, g, x in (("harm", gh, h), ("bre", gb, br)):
            want = (base[name][a:b].astype(F64) * g).astype(F32)
            assert np.all(_within_one_ulp(x, want)), (c["name"], name, form)
            differ[name] += int(np.sum(_bits(x) != _bits(want)))
        if sb[k] == 0:
            assert _same_bits(br, base["bre"][a:b]), (c["name"], "breath under a strength of 0")
        # (a note's samples from its last frame's hop on are zero in every stem — all of them in a note under one hop — and the
        # smoothed mask of an all-unvoiced note is zero: nothing for the jitter to move there)
        live += int(np.count_nonzero(base["harm"][a:b]))
        if np.any(c["mask"]) and np.count_nonzero(base["harm"][a:b]) > 1:
            assert np.any(_bits(h) != _bits(base["harm"][a:b])), (c["name"], "the jitter is there")
            moved += int(np.sum(_bits(h) != _bits(base["harm"][a:b])))
        total += c["n"]
    print("MEASURED sr %s parity %d: harm %d, bre %d of %d samples differ from the restatement's cast (%d non-zero harm samples, %d moved)"
          % (form, parity, differ["harm"], differ["bre"], total, live, moved))
    assert moved > live // 3
