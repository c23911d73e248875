"""CPU: tests/presynth_ref.py — the restatement of the jitter and sub-harmonic stages — against this project's oracle
(oracle/goofer_ref.py, itself pinned to the reference by the golden vectors), the conditions the GPU cases must meet, asserted
from the restatement alone so that a case cannot silently stop exercising its edge, and the sensitivity of the GPU test's bounds:
each of six wrong variants of the restatement breaks the bound tests/test_gpu_presynth_stages.py asserts on at least one sample
of the batch, so that test would notice a kernel doing the same.

Tolerances against the oracle are what float64 summation order allows and nothing else.  The oracle's gauss1d runs np.convolve
over the 2 r + 1 taps, the restatement adds them in ascending order: two sums of nt = 2 r + 1 products each within
nt 2^-53 sum|k_j x_j| <= nt 2^-53 max|x| of the exact one (the taps are positive and sum to 1).  The oracle's subharm_layer adds
the pulses of all ratios in sample order, the restatement ratio by ratio: two float64 sums of at most C terms per sample.
"""
import numpy as np
import pytest

import presynth_ref as P
from oracle import goofer_ref as R

F32, F64 = np.float32, np.float64
SR0 = P.GEO[0]
U = 2.0 ** -53


def _radius(sigma):
    return R.gauss_taps(float(sigma))[1]


def _fir_tol(z, sigma):
    """|difference of two float64 FIR sums in any order|: 2 nt 2^-53 max|z|."""
    return 2 * (2 * _radius(sigma) + 1) * U * float(np.max(np.abs(z)))


def _each(parity):
    d = P.cases()
    for k, c in enumerate(d["notes"]):
        if P.flagged(k, parity):
            yield k, c, int(d["off"][k]), int(d["off"][k + 1])


# ---------------------------------------------------------------------------------------------
# the restatement against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", (0, 1))
def test_f0_jitter_is_the_oracles_curve(parity):
    d = P.cases()
    sigma = SR0 / (P.SH["speed"] * 6)
    for k, c, a, b in _each(parity):
        z = d["noise"]["f0"][a:b]
        s, mx = P.smooth_noise(z, sigma)
        curve = R.f0_jitter_curve(c["n"], SR0, speed=P.SH["speed"], strength=P.SH["strength"], noise=z)
        tol = 2 * P.SH["strength"] * _fir_tol(z, sigma) / mx + 4 * U
        assert np.max(np.abs((1.0 + s * P.SH["strength"]) - curve)) <= tol, c["name"]
        # and the product: the reference's `f0_interp *= 1.0 + ((f0_jitter - 1.0) * voicing_mask)` on its fp32 array
        f0s = P.scaled_f0(c)
        want = (f0s.astype(F64) * (1.0 + (curve - 1.0) * c["mask"].astype(F64)))
        got64, got32 = P.f0_after_jitter(f0s, c["mask"], z, P.SH["strength"], sigma)
        assert np.all(np.abs(got64 - want) <= np.abs(want) * (tol + 2 * U)), c["name"]
        assert np.all(np.abs(got32.astype(F64) - want.astype(F32).astype(F64)) <= P.ulp32(want)), c["name"]
        assert np.array_equal(got32[c["mask"] == 0], f0s[c["mask"] == 0])


@pytest.mark.parametrize("vibrato", (False, True))
@pytest.mark.parametrize("parity", (0, 1))
def test_volume_gains_are_the_oracles_curves(parity, vibrato):
    d = P.cases()
    cfg = P.SR_VIB if vibrato else P.SR_NOISE
    sigma = SR0 / (cfg["speed"] * 6)
    for k, c, a, b in _each(parity):
        zh, zb = d["noise"]["vol_h"][a:b], d["noise"]["vol_b"][a:b]
        sh, sb = float(F32(cfg["harm"])), float(F32(0.0 if k in P.HARM_ONLY else cfg["breath"]))
        gh, gb = P.volume_gains(c["n"], SR0, c["mask"], zh, zb, sh, sb, cfg["speed"], vibrato)
        vjm = R.gauss1d(c["mask"], 20.0)
        assert vjm.dtype == F64
        tol_m = _fir_tol(c["mask"], 20.0) + 2 * U
        assert np.max(np.abs(P.smooth_fir(c["mask"], 20.0) - vjm)) <= tol_m
        for g, z, s in ((gh, zh, sh), (gb, zb, sb)):
            j = R.volume_jitter_curve(c["n"], SR0, speed=cfg["speed"], strength=s, vibrato=vibrato, noise=z)
            tol_j = 0.0 if vibrato else 2 * s * _fir_tol(z, sigma) / P.smooth_noise(z, sigma)[1] + 4 * U
            want = 1.0 + (j - 1.0) * vjm
            assert np.max(np.abs(g - want)) <= tol_j + np.max(np.abs(j - 1.0)) * tol_m + 4 * U, (c["name"], vibrato)
            if s == 0.0:
                assert np.all(g == 1.0)


@pytest.mark.parametrize("case", list(P.SG_CASES))
def test_sub_layer_is_the_oracles(case):
    d = P.cases()
    subharm, _, with64 = P.SG_CASES[case]
    for k, s in P.sg_truth(case).items():
        c = d["notes"][k]
        a, b = int(d["off"][k]), int(d["off"][k + 1])
        f_in = d["f0_64"]["sg"][a:b] if with64 else P.sg_jittered_f0(case, k)
        if subharm.get("vibrato"):
            # (the oracle keeps the array's type: fp32 in, fp32 out — float64 behind the time stretch)
            fm = R.subharm_vibrato(f_in, SR0, rate=subharm["rate"], depth=subharm["depth"], delay=subharm["delay"])
            assert fm.dtype == (F64 if with64 else F32)
            assert np.array_equal(fm.astype(F64), s["fm"]), c["name"]
        else:
            assert np.array_equal(np.asarray(f_in, dtype=F64), s["fm"]), c["name"]
        want = R.subharm_layer(s["fm"], SR0, weight=s["weight"], semitones=subharm["semitones"], vmask=c["mask"])
        scale = s["weight"] / s["max"] if s["max"] > 1e-6 else s["weight"]
        cmax, amax = int(s["C"].max(initial=0)), float(s["A"].max(initial=0.0))
        tol = scale * 4 * max(cmax, 1) * U * amax + 4 * U * s["weight"]
        assert np.max(np.abs(s["layer"] - want), initial=0.0) <= tol, (c["name"], case)
        # the increments: 0 where the reference's loop does `continue`
        for ratio, inc in zip(P.ratios_of(subharm), s["inc"]):
            sub = s["fm"] * ratio
            off = (c["mask"] <= 0) | (s["fm"] <= 0) | (sub < 1e-2)
            assert not np.any(inc[off]) and np.array_equal(inc[~off], (sub / SR0)[~off])


def test_lf_pulse_is_the_oracles_bits():
    for T in (0.125, 1 / 50.026, 1 / 915.3, 1 / 18002.0, 1 / 4500.5):
        n = max(3, int(round(SR0 * T)))
        raw, pk = P.lf_pulse_sub(T, n)
        assert np.array_equal(raw / pk, R.lf_pulse(np.float64(T), Ra=0.02, Rg=1.7, Rk=1, sr=SR0))
        assert np.all(raw >= 0)                               # Rk = 1: no negative lobe, so A = the plain sum


def test_short_notes_reflect_more_than_once():
    """A note shorter than the radius: numpy's 'reflect' goes back and forth, one sample is 'edge'."""
    z = np.arange(1.0, 4.0)
    k, r = R.gauss_taps(20.0)
    idx = [0, 1, 2, 1]
    want = sum(k[j] * z[idx[(j - r) % 4]] for j in range(2 * r + 1))
    assert abs(P.smooth_fir(z, 20.0)[0] - want) <= (2 * r + 1) * U * 3
    assert P.smooth_fir(np.array([2.5]), 20.0)[0] == pytest.approx(2.5, rel=1e-15)
    assert np.allclose(P.smooth_fir(z, 20.0), R.gauss1d(z, 20.0), rtol=0, atol=2 * (2 * r + 1) * U * 3)


# ---------------------------------------------------------------------------------------------
# the conditions on the inputs
# ---------------------------------------------------------------------------------------------
def test_batch_shape():
    d = P.cases()
    assert sorted(P.LENGTHS) == [1, 3, 100, 255, 256, 257, 1023, 1025, 2048, 6000] and d["N"] < 16000
    radii = [_radius(20.0), _radius(SR0 / (150.0 * 6)), _radius(SR0 / (100.0 * 6))]
    # the 100-sample note is shorter than the two noise radii (more than one reflection) and than the sigma-20 window of 161
    # taps (both ends reflect for every sample); shorter than the sigma-20 radius are the notes of 3 samples and of 1
    assert radii == [80, 196, 294] and 100 < radii[1] and 100 < 2 * radii[0] + 1 and 3 < radii[0]
    fade = int(0.1 * SR0)
    assert [n for n in P.LENGTHS if fade < n] == [6000]
    assert [k for k, c in enumerate(d["notes"]) if c["ps"] != 1.0] == [1, 4, 7]
    for parity in (0, 1):
        on = [c for k, c in enumerate(d["notes"]) if P.flagged(k, parity)]
        assert any(not np.any(c["mask"]) for c in on), "an all-unvoiced note with the flag"
        assert any(np.any((c["mask"] > 0) & (c["mask"] < 1)) for c in on), "fractional mask values"
        assert any(np.any(c["mask"] == 0) and np.any(c["mask"] == 1) for c in on), "blocks of 0 and 1"
        assert any(k in P.HARM_ONLY for k in range(len(on) * 2) if P.flagged(k, parity))
    # the vibrato form at strength 1.6 reaches both clip limits
    z = P.vibrato_env(6000, SR0, P.SR_VIB["speed"])
    j = 1.0 + z * float(F32(P.SR_VIB["harm"]))
    assert P.SR_VIB["harm"] == 1.6 and j.max() > 1.5 and j.min() < 0.5
    gh, _ = P.volume_gains(6000, SR0, np.ones(6000, F32), None, None, 1.6, 0.7, P.SR_VIB["speed"], True)
    assert abs(gh.max() - 1.5) < 1e-12 and abs(gh.min() - 0.5) < 1e-12     # (times the smoothed all-ones mask: 1 within an ulp)


def _all_events(case):
    for k, s in P.sg_truth(case).items():
        for ri, e in enumerate(s["events"]):
            yield k, ri, s, e


def test_sub_harmonic_conditions():
    d = P.cases()
    # more than 128 events of one ratio in one note: two strip carries in k_subharm_finish — and it is the LAST ratio, the one
    # the onset view shows
    assert max(len(e["i"]) for k, ri, s, e in _all_events("three") if ri == 2) > 128
    # a sample covered by at least three events
    assert max(int(s["C"].max(initial=0)) for s in P.sg_truth("one").values()) >= 3
    # a sample still covered by an event after at least two later events have ended: end_max must be a running maximum
    e = P.sg_truth("one")[0]["events"][0]
    ends = e["i"] + e["n"]
    k0 = int(np.argmax(e["n"]))
    j = min(int(ends[k0]), 6000) - 1
    assert e["i"][k0] <= j < ends[k0] and np.sum(ends[k0 + 1:] <= j) >= 2
    assert np.all(P.sg_truth("one")[0]["fm"][e["i"][k0 + 1:]] > 10 * P.sg_truth("one")[0]["fm"][e["i"][k0]])   # a low f0 that jumps up
    # n clamped to 3
    assert any(e["clamped"].any() and np.all(e["n"][e["clamped"]] == 3) for _, _, _, e in _all_events("three"))
    # sr T at an exact tie: sub 8 Hz, T 0.125, 44100 T = 5512.5 -> 5512
    tie = e["tie"]
    assert tie.sum() == 1 and e["sub"][tie][0] == 8.0 and SR0 * e["T"][tie][0] == 5512.5 and e["n"][tie][0] == 5512
    assert (SR0 * 0.125) - np.floor(SR0 * 0.125) == 0.5
    # a lent sub that changes n
    e8 = P.sg_truth("one")[8]["events"][0]
    assert e8["lent"].any() and np.all(e8["sub_used"][e8["lent"]] != e8["sub"][e8["lent"]])
    # three ratios: below 1, above 1, irrational
    r = P.ratios_of(P.SG_CASES["three"][0])
    assert len(r) == 3 and r[0] == 0.5 and r[2] == 2.0 and 0.5 < r[1] < 1 and r[1] == 2.0 ** (-7 / 12)
    # vibrato whose fade ends inside one note and exceeds another's length
    fade = int(P.SG_CASES["vibrato"][0]["delay"] * SR0)
    assert fade < 6000 and fade > 2048
    # 0 < sub < 1e-2 on a voiced sample
    s0 = P.sg_truth("one")[0]
    sub = s0["fm"] * 0.5
    hit = (sub > 0) & (sub < 1e-2) & (d["notes"][0]["mask"] > 0)
    assert hit.any() and not np.any(s0["inc"][0][hit])
    # one call with f0_64, whose values are no fp32 numbers
    assert P.SG_CASES["f0_64"][2]
    f64 = d["f0_64"]["sg"]
    assert np.mean(f64.astype(F32).astype(F64) != f64) > 0.9
    # the flagged all-unvoiced note has f0 and no event; a weight of 0.5 on every second note
    assert np.all(d["sg_f0"][6] > 0) and all(len(e["i"]) == 0 for k, _, _, e in _all_events("three") if k == 6)
    # some voiced sample of a flagged note that no event covers
    assert any(np.any((s["C"] == 0) & (d["notes"][k]["mask"] > 0)) for k, s in P.sg_truth("one").items())


@pytest.mark.parametrize("case", list(P.SG_CASES))
def test_no_fragile_event(case):
    """No tracker phase within 1e-9 of 1 at an event or in front of it, and no key at a printing edge: an ulp of the device's sin
    (or of its product 100 sub) cannot move an event or change a lender."""
    for k, ri, s, e in _all_events(case):
        assert not e["fragile"].any() and not e["key_edge"].any(), (case, k, ri)


# ---------------------------------------------------------------------------------------------
# sensitivity: wrong variants break the GPU test's bounds
# ---------------------------------------------------------------------------------------------
def _layer_excess(case, k, **variant):
    """max over the note of |wrong layer - layer| / (the GPU test's bound), the main pulse train taken from the oracle."""
    d = P.cases()
    good, bad = P.sg_truth(case)[k], P.sg_note(case, k, **variant)
    base = R.pulse_train(P.scaled_f0(d["notes"][k], d["sg_f0"][k]), SR0).astype(F64)
    return float(np.max(np.abs(bad["layer"] - good["layer"]) / P.layer_bound(base + good["layer"], good)))


@pytest.mark.parametrize("name,case,k,variant", [
    ("half-up rounding of sr T", "one", 0, dict(rounding="up")),
    ("no key cache", "one", 8, dict(cache=False)),
    ("end_max without the carry", "one", 0, dict(carry=False)),
    ("end_max without the carry, 369 events", "three", 0, dict(carry=False)),
    ("covering set limited to the latest event", "one", 0, dict(covering="latest")),
])
def test_wrong_layer_variants_exceed_the_bound(name, case, k, variant):
    x = _layer_excess(case, k, **variant)
    print("%s: worst error / bound %.3g" % (name, x))
    assert x > 1.0, name


def test_the_search_form_of_the_placement_is_the_restatement():
    """The variants above run the placement as k_subharm_place's search; with the carry and the whole covering set that search
    gives the restatement's sums bit for bit, so what the variants show comes from what they leave out."""
    for k in (0, 2, 8):
        good = P.sg_truth("one")[k]
        e = good["events"][0]
        pulses = []
        for T, n in zip(e["T"], e["n"]):
            raw, pk = P.lf_pulse_sub(T, int(n))
            pulses.append(raw / pk)
        got, cov = P._gather_search(e["i"], e["n"], e["end_max"], pulses, good["fm"].size, False)
        assert np.array_equal(got * P.cases()["notes"][k]["mask"].astype(F64), good["raw"]) and np.array_equal(cov, good["C"])


@pytest.mark.parametrize("name,variant", [("numpy symmetric padding", dict(pad="symmetric")), ("maximum without + 1e-6", dict(eps=0.0))])
def test_wrong_smoothing_variants_exceed_one_ulp(name, variant):
    d = P.cases()
    sigma = SR0 / (P.SH["speed"] * 6)
    worst_f0 = worst_vol = 0.0
    for k, c, a, b in _each(0):
        f0s = P.scaled_f0(c)
        good = P.f0_after_jitter(f0s, c["mask"], d["noise"]["f0"][a:b], P.SH["strength"], sigma)[1]
        bad = P.f0_after_jitter(f0s, c["mask"], d["noise"]["f0"][a:b], P.SH["strength"], sigma, **variant)[1]
        worst_f0 = max(worst_f0, float(np.max(np.abs(bad.astype(F64) - good.astype(F64)) / P.ulp32(good))))
        args = (c["n"], SR0, c["mask"], d["noise"]["vol_h"][a:b], d["noise"]["vol_b"][a:b], P.SR_NOISE["harm"], P.SR_NOISE["breath"],
                P.SR_NOISE["speed"], False)
        stem = np.full(c["n"], 0.37, dtype=F32).astype(F64)   # any stem: the factor is what differs
        for g, w in zip(P.volume_gains(*args), P.volume_gains(*args, **variant)):
            t = (stem * g).astype(F32)
            worst_vol = max(worst_vol, float(np.max(np.abs((stem * w).astype(F32).astype(F64) - t.astype(F64)) / P.ulp32(t))))
    print("%s: f0 off by %.3g ulp, a stem by %.3g ulp" % (name, worst_f0, worst_vol))
    assert worst_f0 > 1.0 and worst_vol > 1.0, name
