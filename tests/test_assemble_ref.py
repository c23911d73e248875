"""CPU: tests/assemble_ref.py against the oracle it restates, and the judge against four planted faults.

- ``stages(exact=False)`` equals ``oracle.sampler_ref.assemble`` bit for bit (env, f0, mask, formants) on the 17 golden requests of
  tests/test_gpu_sampler.py, the 12 hard cases and every case of the GPU matrix at every geometry.  No case is skipped or
  caught: a request the oracle refuses fails here and is replaced by another seed in assemble_ref.matrix.
- ``within`` rejects (a) one bin moved by 1e-5 of its row's peak in a row 40 dB below the note's loudest, (b) two neighbouring
  rows swapped, (c) the F1 bell left out of one 64-bin chunk of one row, (d) the es window one bin off on one row.
- per geometry and flag family the note-level E_ref (reference arithmetic against the float64 truth) is printed: the values the
  bound of tests/test_gpu_assemble_oracle.py is built from.
"""
import numpy as np
import pytest

import assemble_ref as A
from conftest import golden
from goofer_amd import synthetic as syn
from oracle import sampler_ref as SR

F32 = np.float32
SUPPORTED = ["default", "t12g50", "tm12gm50", "formants", "formants_flip", "L0", "L1", "L2", "L0_short", "br_es_neg",
             "br_es_pos", "vel60", "vel150", "R1", "FV1_P50", "negcut", "vol_mix"]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_oracle(src, args, hop, what):
    p = SR.decode_request(*args)
    want = SR.assemble(A.features_of(src), p, hop)
    got = A.stages(A.features_of(src), SR.decode_request(*args), hop)
    assert _same(got["env_fry"].T, want["env"]), what
    assert _same(got["f0"], want["f0"]) and _same(got["mask"], want["mask"]), what
    assert sorted(got["formants"]) == sorted(want["formants"]), what
    for k in want["formants"]:
        assert _same(got["formants"][k], want["formants"][k]), (what, k)
    if want["fry_mask"] is None:
        assert _same(got["env"], got["env_fry"]), what
    assert got["edited"].dtype == F32 and got["edited"].shape[1] == want["env"].shape[0], what
    return got


def test_restatement_equals_oracle_on_golden_requests():
    cases = [str(n) for n in golden("sampler_index")["names"]]
    for name in SUPPORTED:
        g = golden("sampler_" + name)
        src = syn.make_source(2000 + cases.index(name), seconds=0.45)
        assert_equals_oracle(src, [str(a) for a in g["args"]], 256, name)


def test_restatement_equals_oracle_on_hard_cases():
    for i in range(len(golden("sampler_hard_index")["names"])):
        src, req = syn.hard_case(i)
        assert_equals_oracle(src, syn.request_args(req), 256, i)


@pytest.mark.parametrize("sr,n_fft,hop", A.GEOMETRIES, ids=A.GEO_IDS)
def test_restatement_equals_oracle_on_the_gpu_matrix(sr, n_fft, hop):
    """... and the truth differs from it in rounding only: E_ref per flag family, printed."""
    cases = A.matrix(sr, n_fft, hop)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    plain, rest = A.fused_matrix(sr, n_fft, hop)                      # the fused-route notes: the same assembly, shifted formants
    assert len(plain) >= 10 and len(rest) >= 2
    assert not any(A.has_flag(c, k) for _, c in plain for k in ("vf", "sg", "sr"))
    for i, c in plain + rest:
        assert_equals_oracle(c["src"], syn.request_args(c["req"]), hop, ("fused", c["name"]))
        assert SR.decode_request(*syn.request_args(c["req"])).F_shift != (1.0, 1.0, 1.0, 1.0)
    fam = {}
    for c in cases:
        args = syn.request_args(c["req"])
        ref = assert_equals_oracle(c["src"], args, hop, c["name"])
        truth = A.stages(A.features_of(c["src"]), SR.decode_request(*args), hop, exact=True, decisions=ref["decisions"])
        for stage in ("edited", "env", "env_fry"):
            assert truth[stage].dtype == np.float64 and truth[stage].shape == ref[stage].shape
            E_ref = A.errors(ref[stage], ref[stage], truth[stage])[0]
            assert E_ref < 1e-5, (c["name"], stage, E_ref)            # rounding only: a decision taken differently is 1e-3 and up
            key = (c["family"], stage)
            fam[key] = max(fam.get(key, 0.0), E_ref)
        for k in ("f0", "mask"):
            assert _same(ref[k], truth[k]), (c["name"], k)            # float64 in the oracle already
    print("E_ref %s:" % A.GEO_IDS[A.GEOMETRIES.index((sr, n_fft, hop))],
          "  ".join("%s %s" % (f, "/".join("%.1e" % fam[(f, s)] for s in ("edited", "env", "env_fry")))
                    for f in sorted({k[0] for k in fam})))


def test_matrix_reaches_the_code_it_names():
    """The matrix at 513 bins holds what the GPU test's docstring says it holds."""
    seen = set()
    for c in A.matrix(44100, 1024, 256):
        p = SR.decode_request(*syn.request_args(c["req"]))
        d = A.stages(A.features_of(c["src"]), p, 256)
        dec = d["decisions"]
        seen.add(dec["loop"])
        seen.add("vel" if dec["vel_active"] else "novel")
        n = len(d["mask"])
        if n in A.SAMPLE_COUNTS:
            seen.add(n)
        if n < 256:
            seen.add("under_one_hop")
        if dec["fry_rows"]:
            seen.add("fry")
        if c["name"].startswith("L0") and dec["loop"] == "concat" and dec["seg"]["end_frame"] - dec["seg"]["consonant_frame"] < 16:
            seen.add("short_tail")
        if "es_clamp_tail" in dec and dec["es_clamp_tail"].any():
            seen.add("es_clamp")
        if dec["bell_on"].any():
            seen.add("bells")
        if c["name"] == "edge_formants":
            F1 = SR.sanitize_formant(d["formants"]["F1"].copy(), len(d["formants"]["F1"]), 44100, min_hz=120.0, sigma_frames=4)
            assert F1.max() < 140.0
    for need in ("slice", "concat", "avg", "stretch", "vel", "novel", "fry", "short_tail", "bells", "under_one_hop") + A.SAMPLE_COUNTS:
        assert need in seen, need


# ---------------------------------------------------------------------------------------------
# the judge can fail
# ---------------------------------------------------------------------------------------------
def _note(flags, seed=1):
    src = syn.make_source(7900 + seed, seconds=0.35)
    req = syn.make_request(7900 + seed, flags, length_ms=200.0, offset_ms=20.0, consonant_ms=40.0, cutoff_ms=20.0)
    p = lambda: SR.decode_request(*syn.request_args(req))
    ref, truth = A.both(A.features_of(src), p(), 256)
    return src, p, ref, truth


def _judge(x, ref, truth):
    E_ref, e = A.errors(x, ref["env"], truth["env"])
    return A.within(E_ref, e)


def test_judge_rejects_planted_faults():
    src, p, ref, truth = _note("fsta40")
    env = ref["env"].astype(F32)
    assert _judge(env, ref, truth)                                     # the reference arithmetic itself passes

    # (a) one bin of a row 40 dB below the loudest, by 1e-5 of that row's peak
    quiet_src = dict(src, env_pack=dict(src["env_pack"]))
    logk = src["env_pack"]["knot_vals_log"].astype(np.float64)
    t_q = logk.shape[1] // 2
    logk[:, t_q] -= np.log(100.0)
    quiet_src["env_pack"]["knot_vals_log"] = logk.astype(np.float16)
    q_ref, q_truth = A.both(A.features_of(quiet_src), p(), 256)
    peaks = np.abs(q_truth["env"]).max(axis=1)
    t = int(np.argmin(peaks))
    assert peaks[t] <= 0.0101 * peaks.max()
    x = q_ref["env"].astype(F32)
    assert _judge(x, q_ref, q_truth)
    x[t, 100] += F32(1e-5 * peaks[t])
    assert not _judge(x, q_ref, q_truth)

    # (b) two neighbouring rows swapped
    x = env.copy()
    x[[20, 21]] = x[[21, 20]]
    assert not _judge(x, ref, truth)

    # (c) the F1 bell left out of one 64-bin chunk of one row, where its factor differs from 1 by more than 1e-4
    t = 15
    F1 = SR.sanitize_formant(ref["formants"]["F1"].copy(), env.shape[0], 44100, min_hz=120.0, sigma_frames=4)
    fr = np.linspace(0.0, 22050.0, 513)
    factor = 1.0 + 0.4 * np.exp(-0.5 * ((fr - float(F1[t])) / 100.0) ** 2)
    chunk = int(np.argmin(np.abs(fr - float(F1[t]))) // A.CHUNK)        # (sigma is 2.3 bins: the bell lives in one chunk)
    assert np.abs(factor[chunk * A.CHUNK:(chunk + 1) * A.CHUNK] - 1.0).max() > 1e-4
    mut = A.stages(A.features_of(src), p(), 256, _mutate={"bell_skip": (0, t, chunk)})["env"].astype(F32)
    assert np.array_equal(np.nonzero((mut != env).any(axis=1))[0], [t])
    assert not _judge(mut, ref, truth)

    # (d) the es window one bin off on one row
    for flags in ("fsta40es-40", "fsta40es40"):
        src, p, ref, truth = _note(flags, seed=2)
        env = ref["env"].astype(F32)
        assert _judge(env, ref, truth)
        mut = A.stages(A.features_of(src), p(), 256, _mutate={"es_shift_frame": 5})["env"].astype(F32)
        assert np.count_nonzero((mut != env).any(axis=1)) == 1
        assert not _judge(mut, ref, truth)


def test_zero_rows_and_non_finite_values_are_judged():
    truth = np.zeros((3, 8))
    truth[1] = 1.0
    x = truth.astype(F32)
    assert A.within(*A.errors(x, truth, truth))
    y = x.copy()
    y[0, 3] = 1e-30
    assert not A.within(*A.errors(y, truth, truth))                    # a zero row must be exactly zero
    y = x.copy()
    y[1, 2] = np.nan
    assert not A.within(*A.errors(y, truth, truth))
    assert A.ulp_distance(F32([1.0, -0.0, 1.0]), F32([np.nextafter(F32(1.0), F32(2.0)), 0.0, 1.0])).tolist() == [1, 0, 0]
