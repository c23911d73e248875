"""CPU: tests/synth_ref.py against the oracle, and its judge against planted faults.

1. The reference arithmetic of the restatement equals ``oracle.goofer_ref.synthesize(..., return_parts=True)`` bit for bit on the
   golden ``synthesize`` cases, the 15 sampler calls of tests/test_gpu_synth.py and every note of the GPU matrix at every geometry.
2. Ten faults, each planted into a copy of the float64 truth of a one-second note through ``given=`` (so that what lies behind
   the faulty stage follows from it), are each REJECTED by the rule tests/test_gpu_synth_stages.py applies (per unit,
   e <= 3 E_ref + 2^-23), on stages that test judges.  The old judgement is whole-note sample-RMS below 2e-5 on rec / harm / uv /
   bre (tests/test_gpu_synth.py's TIGHT).  Measured (RMS: the worst stem):
     fault                    stage      e        E_ref     RMS       the RMS bound
     one_sample_1e-5          harm       1.0e-05  2.0e-07   4.2e-08   accepts
     upsample_i_over_n        uv         1.1e-04  2.2e-07   2.0e-06   accepts   (bre: 1.0e-04)
     hp_one_from_bin_64       S_harm     1.4e-05  2.1e-07   1.7e-07   accepts   (S_breath: 2.7e-06 against 1.4e-07)
     breath_frame_dropped     bre        0.52     2.2e-07   2.0e-09   accepts   (mask 1e-6 throughout: the stem's own peak is the scope)
     first_hop_interior_sum   harm       1.7e-03  2.7e-07   4.9e-05   catches it, at twice the bound
     zero_tail_one_late       harm       0.18     2.8e-07   7.8e-04   catches it: the planted sample repeats its neighbour, a loud one
     last_hop_unflushed       harm       0.14     2.0e-07   1.7e-03   catches it: two hops of the note's end are silent
     blur_clamp_at_bin_0      S_harm     0.25     1.9e-07   7.8e-03   catches it HERE (S_breath: 0.10): the note is mask 1 over f0 = 0
                              with cut_subharm_below_f0 off, the one place where bin 0 carries anything; on an ordinary voiced note
                              the high-pass leaves 4e-18 at bin 0 and neither judgement sees the fault
     env_noise_from_warped    S_uv       0.43     1.1e-07   1.5e-02   catches it (uv: 0.21): a formant shift of 1.25 moves the envelope
     mag_without_1e-8         harm       inf      0         NaN       only shows where the pulse train is all zero: mag = 0 instead
                              of 1e-8, 0 / 0 in every harmonic sample where the truth is an exact zero, and a NaN fails any
                              comparison; on a voiced note it moves note_mag by 1e-9 of itself, which neither judgement can see
   So the RMS bound accepts four of the ten and catches six; the six are kept as they are.  What the new judgement adds over the
   old is the first four rows, and for the caught ones the place: a stage and a unit instead of one figure per note.
3. Printed per geometry: the note-level E_ref of every stage under both yardsticks (the oracle's arithmetic, and the same with the
   plain radix-2 fp32 transform), worst note of the main batch.  These are what the GPU bound is built from.
"""
import json

import numpy as np
import pytest

import synth_ref as SR
from conftest import golden, rms_err
from oracle import goofer_ref as R

F32 = np.float32


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _assert_equals_oracle(case, geo, sigma, tag):
    rec, harm, uv, bre, parts = SR.oracle_note(case, geo, sigma)
    s = SR.synth_note(case, geo, exact=False, sigma=sigma)
    for key, ref in (("rec", rec), ("harm", harm), ("uv", uv), ("bre", bre)):
        assert _same(s[key], ref), (tag, case["name"], key)
    for key in SR.ORACLE_PARTS:
        ref = parts[key]
        if key in ("mag", "peak"):
            assert s[key] == ref, (tag, case["name"], key, s[key], ref)
        else:                                                  # (env_noise: one row per frame in the restatement)
            assert _same(s[key].T if key == "env_noise" else s[key], ref), (tag, case["name"], key)


def _golden_case(g, name):
    sr, n_fft, hop, seed = (int(v) for v in g[f"{name}_geo"])
    kw = {str(k): float(v) for k, v in zip(g[f"{name}_kw_keys"], g[f"{name}_kw_vals"]) if k != "_"}
    sigma = kw.pop("noise_transition_smoothness", 100.0)
    for k in ("apply_brightness", "cut_subharm_below_f0"):
        if k in kw:
            kw[k] = bool(kw[k])
    env = g[f"{name}_env"]
    n = len(g[f"{name}_f0"])
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=(env.shape[0], 1 + n // hop)).astype(F32)
    F = g[f"{name}_formants"]
    return dict(name=name, n=n, env=env, f0=g[f"{name}_f0"], mask=g[f"{name}_mask"], phi=phi, formants={i + 1: F[i] for i in range(4)},
                kw=kw, mix={}), (sr, n_fft, hop), sigma


def test_restatement_equals_oracle_on_the_golden_synthesize_cases():
    g = golden("synthesize")
    for name in g["names"]:
        case, geo, sigma = _golden_case(g, str(name))
        assert set(case["kw"]) <= set(SR.KW_DEFAULT), case["kw"]
        _assert_equals_oracle(case, geo, sigma, "golden")
        rec = SR.synth_note(case, geo, sigma=sigma)["rec"]
        assert rms_err(rec, g[f"{name}_rec"]) < 2e-5          # (and the oracle is the reference's: tests/test_oracle_core.py)


SAMPLER = ["default", "t12g50", "tm12gm50", "formants", "formants_flip", "L0", "L1", "L2", "br_es_neg", "br_es_pos",
           "vel60", "vel150", "R1", "FV1_P50", "negcut"]


def test_restatement_equals_oracle_on_the_sampler_calls():
    for name in SAMPLER:
        g = golden("sampler_" + name)
        kw = json.loads(str(g["kw"]))
        # (the recorded keyword set spells out every default: the layers this restatement leaves out must be off)
        assert not any(kw.get(k) for k in ("f0_jitter", "volume_jitter", "add_subharm", "roughness_on")), kw
        assert kw.get("stretch_factor", 1.0) == 1.0 and kw.get("n_fft", 1024) == 1024 and kw.get("hop_length", 256) == 256
        assert kw.get("noise_transition_smoothness", 100) == 100
        kw = {k: v for k, v in kw.items() if k in SR.KW_DEFAULT}
        env = np.asarray(g["env_new"], dtype=F32)
        n = len(g["mask_new"])
        phi = np.random.default_rng(int(g["seed"][0])).uniform(0.0, 2.0 * np.pi, size=(513, 1 + n // 256)).astype(F32)
        Fm = np.asarray(g["formants_new"], dtype=np.float64)
        case = dict(name=name, n=n, env=env, f0=np.asarray(g["f0_new"], dtype=F32), mask=np.asarray(g["mask_new"], dtype=F32), phi=phi,
                    formants={i + 1: Fm[i] for i in range(4)}, kw=kw, mix={})
        _assert_equals_oracle(case, (44100, 1024, 256), 100.0, "sampler")
        s = SR.synth_note(case, (44100, 1024, 256))
        for key in ("harm", "uv", "bre"):                       # the recorded stems of the reference's own run
            assert rms_err(s[key], g[key]) < 2e-5, (name, key)


@pytest.mark.parametrize("geo", SR.GEOMETRIES, ids=lambda g: "%d-%d-%d" % g)
def test_restatement_equals_oracle_on_the_gpu_matrix(geo):
    """Every note of every batch; no case skipped.  A case the oracle refuses raises here."""
    for tag, (sigma, notes) in SR.batches(geo).items():
        for case in notes:
            _assert_equals_oracle(case, geo, sigma, tag)
    sigma, notes = SR.batches(geo)["sigma2000"]
    assert int(4.0 * (sigma / 4) + 0.5) == 2000


def test_long_batch_covers_every_forced_run():
    """synth_ref.long_batch (tests/test_gpu_walker_runs.py): its frame counts are LONG_FRAMES at every geometry that test uses, and
    every condition of run_coverage holds at every run and halo it forces — with and without the stem walkers' record blocks."""
    for geo in ((44100, 1024, 256), (22050, 512, 128), (44100, 2048, 512), (96000, 2048, 96)):
        notes = SR.long_batch(geo)
        assert [1 + c["n"] // geo[2] for c in notes] == list(SR.LONG_FRAMES)
    assert sum(SR.LONG_FRAMES) < 2000 and SR.LONG_FRAMES.count(1) >= 41
    assert {1, 2, 3, 4, 5, 61, 64, 65, 67, 127, 128, 129, 130, 257} <= set(SR.LONG_FRAMES) and max(SR.LONG_FRAMES) >= 300
    f_off = np.concatenate([[0], np.cumsum(SR.LONG_FRAMES)])
    for run, halo in SR.LONG_RUNS:
        cov = SR.run_coverage(f_off, run, halo, blocks=halo == 3 and run <= 128)
        assert all(cov.values()), (run, halo, [k for k, v in cov.items() if not v])
        assert ("refill_inside" in cov) == (halo == 3 and 61 < run <= 128)
    # ... and the conditions can fail: one long note has no run of three notes, a batch of one-frame notes no note of three runs
    assert not SR.run_coverage([0, 1000], 95, 3, True)["3_notes"]
    assert not SR.run_coverage(np.arange(400), 95, 3, True)["3_runs"]
    assert not SR.run_coverage([0, 189], 128, 3, True)["final_block"]           # the last run starts at fs = 125: its block ends with the batch


def test_restatement_equals_oracle_on_the_long_batch():
    """The long notes too (the main geometry; the 2048 geometries differ by the transform size, which the matrix above covers)."""
    for case in SR.long_batch((44100, 1024, 256)):
        _assert_equals_oracle(case, (44100, 1024, 256), 100.0, "long")


@pytest.mark.parametrize("geo", SR.GEOMETRIES, ids=lambda g: "%d-%d-%d" % g)
def test_print_reference_errors(geo):
    """The note-level E_ref of each stage, worst note of the main batch: oracle arithmetic / plain fp32 transform."""
    worst = {}
    for case in SR.main_batch(geo):
        t = SR.synth_note(case, geo, exact=True)
        a = SR.synth_note(case, geo, exact=False)
        b = SR.synth_note(case, geo, exact=False, fft="plain")
        for st in SR.STAGE_SCOPE:
            ea, eb = SR.e_ref(st, t, a), SR.e_ref(st, t, b)
            w = worst.setdefault(st, [0.0, 0.0])
            w[0], w[1] = max(w[0], ea), max(w[1], eb)
    print("\nE_ref %d / %d / %d" % geo)
    for st, (ea, eb) in worst.items():
        print("  %-10s oracle %.2e   plain fp32 transform %.2e" % (st, ea, eb))
        assert np.isfinite(ea) and np.isfinite(eb), st
        assert max(ea, eb) < 1e-5, st                           # a yardstick this far off would bound nothing


# ---------------------------------------------------------------------------------------------
# planted faults: each a function of (case, truth) that returns the stages to hand synth_note(exact=True, given=...) in place of
# its own, so the fault sits in a copy of the truth and everything behind the faulty stage follows from it
# ---------------------------------------------------------------------------------------------
GEO = (44100, 1024, 256)
HOP = GEO[2]
F64 = np.float64


def _harm(edit):
    def plant(case, truth):
        h = truth["harm_pre"].copy()
        edit(h, case["n"], truth["T"])
        return {"harm_pre": h}
    return plant


def _one_sample(h, n, T):
    h[n // 3] += 1e-5 * np.max(np.abs(h))


def _unflushed(h, n, T):
    h[max(0, HOP * (T - 1) - HOP):] = 0.0


def _tail_late(h, n, T):
    at = HOP * (T - 1)
    assert 0 < at < n, "the note needs a zero tail"
    h[at] = h[at - 1]


def _first_hop(h, n, T):
    n_fft = GEO[1]
    w2 = R.sqrt_hann(n_fft).astype(F64) ** 2
    ws = np.zeros(n_fft + HOP * (T - 1))
    for i in range(T):
        ws[i * HOP:i * HOP + n_fft] += w2
    p = np.arange(HOP) + n_fft // 2
    h[:HOP] *= ws[p] / np.array([w2[q % HOP::HOP].sum() for q in p])


def _upsample(case, truth):
    n = case["n"]
    return {"mask_smooth": SR.mask_upsample(truth["mask_short"], n, True, at=(np.arange(n) / F64(n)).astype(F32))}


def _hp_one(case, truth):
    hp = truth["hp"].copy()
    hp[64:] = 1.0
    return {"hp": hp}


def _clamped_blur(rows, voiced):
    """The sigma-0.5 blur of the voiced rows with bin 0 clamped where numpy reflects."""
    k, r = R.gauss_taps(0.5)
    out = rows.copy()
    v = np.nonzero(voiced > 0)[0]
    pad = np.pad(rows[v], [(0, 0), (r, r)], mode="reflect")
    pad[:, :r] = rows[v, :1]
    out[v] = sum(k[j] * pad[:, j:j + rows.shape[1]] for j in range(k.size))
    return out


def _blur_clamp(case, truth):
    return {st: _clamped_blur(truth[st + "_unblurred"], truth["voiced"]) for st in ("S_harm", "S_breath")}


def _breath_frame(case, truth):
    S = truth["S_breath"].copy()
    S[9] = 0.0
    return {"S_breath": S}


def _env_noise_warped(case, truth):
    return {"env_noise": R.gauss1d(truth["env"], 1.75, axis=0).T}


def _mag(case, truth):
    return {"note_mag": truth["note_mag"] - 1e-8}


N1 = 172 * HOP + 75                                            # one second: the size the RMS bound is applied at elsewhere
PLAIN = dict(mask="blocks")
# fault: (how it is planted, the note, the stages the GPU test's rule is asked about)
FAULTS = {
    "one_sample_1e-5": (_harm(_one_sample), PLAIN, ("harm",)),
    "last_hop_unflushed": (_harm(_unflushed), PLAIN, ("harm",)),
    "zero_tail_one_late": (_harm(_tail_late), PLAIN, ("harm",)),
    "first_hop_interior_sum": (_harm(_first_hop), PLAIN, ("harm",)),
    "upsample_i_over_n": (_upsample, dict(mask=lambda i, n: i >= 9 * HOP), ("uv", "bre")),
    "hp_one_from_bin_64": (_hp_one, dict(mask="one", f0=2700.0), ("S_harm", "S_breath")),
    # (bin 0 of the breath spectrum is only there where the high-pass leaves it: mask 1 over f0 = 0)
    "blur_clamp_at_bin_0": (_blur_clamp, dict(mask="one", f0=lambda i, n, m: np.where(i < n // 2, 0.0, 190.0),
                                              kw=dict(cut_subharm_below_f0=False)), ("S_harm", "S_breath")),
    "breath_frame_dropped": (_breath_frame, dict(mask=lambda i, n: np.full(n, 1e-6), f0=lambda i, n, m: np.full(n, 210.0)), ("bre",)),
    "env_noise_from_warped": (_env_noise_warped, dict(mask="blocks", kw=dict(formant_shift=SR.f32(1.25))), ("S_uv", "uv")),
    "mag_without_1e-8": (_mag, dict(mask="zero"), ("harm",)),
}
RMS_CATCHES = {"first_hop_interior_sum", "zero_tail_one_late", "last_hop_unflushed", "blur_clamp_at_bin_0", "env_noise_from_warped",
               "mag_without_1e-8"}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_judge_rejects_planted_fault_and_the_rms_bound_accepts_it(fault):
    plant, note, stages = FAULTS[fault]
    case = SR.make_case(GEO, 70 + list(FAULTS).index(fault), N1, fault, **note)
    truth = SR.synth_note(case, GEO, exact=True)
    with np.errstate(all="ignore"):
        bad = SR.synth_note(case, GEO, exact=True, given=plant(case, truth))
    a = SR.synth_note(case, GEO, exact=False)
    b = SR.synth_note(case, GEO, exact=False, fft="plain")
    for st in stages:                                          # the rule of tests/test_gpu_synth_stages.py, stage by stage
        ok, e, E = SR.judge(st, bad[st], truth, a, b)
        print("%s %s: e %.3g  E_ref %.3g  %s" % (fault, st, e, E, "accepted" if ok else "rejected"))
        assert not ok, (fault, st, e, E)
        # (and the judge accepts the two yardsticks themselves, as it must)
        assert SR.judge(st, a[st], truth, a, b)[0] and SR.judge(st, b[st], truth, a, b)[0]
    with np.errstate(all="ignore"):
        old = max(rms_err(bad[k], truth[k]) / max(1.0, float(np.max(np.abs(truth[k])))) for k in ("rec", "harm", "uv", "bre"))
    print("%s: worst stem sample-RMS %.3g" % (fault, old))
    if fault in RMS_CATCHES:
        assert not old < 2e-5, (fault, old)
    else:
        assert old < 2e-5, (fault, old)


def test_plain_transform_is_a_transform():
    """The plain fp32 transform against numpy's float64 one, every size of the matrix, and its error next to pocketfft's."""
    rng = np.random.default_rng(5)
    assert {g[1] for g in SR.GEOMETRIES} == {130, 320, 512, 768, 1000, 1024, 1536, 2046, 2048, 3000, 4096}
    for n in (130, 320, 512, 768, 1000, 1024, 1536, 2046, 2048, 3000, 4096):
        x = rng.standard_normal((n, 8)).astype(F32)
        X = np.fft.rfft(x.astype(np.float64), axis=0)
        pk = np.max(np.abs(X), axis=0)
        e_plain = float(np.max(np.abs(SR.rfft_plain(x) - X) / pk))
        e_np = float(np.max(np.abs(np.fft.rfft(x, axis=0) - X) / pk))
        back = SR.irfft_plain(X.astype(np.complex64), n)
        e_back = float(np.max(np.abs(back - x)) / np.max(np.abs(x)))
        print("n_fft %d: plain %.2e  numpy fp32 %.2e  round trip %.2e" % (n, e_plain, e_np, e_back))
        assert e_plain < 2e-6 and e_back < 2e-6
        assert SR.rfft_plain(x).dtype == np.complex64 and back.dtype == F32
