"""GPU: the note assembly kernels (csrc/assemble.hip: k_env_edit, k_row_recs + k_env_rows, k_env_fry, k_sample_assemble) stage by
stage, row by row and sample by sample against tests/assemble_ref.py, at nine row widths.

HARNESS.  ``Renderer.prepare(jobs, trim_rows=False)``, then the assembly's ``edit_rows`` and ``env_out`` are pointed at tensors
the test owns (the ABI takes a caller's buffer for the edited rows: that makes k_env_edit's output observable), every output is
filled with a bit pattern, ``Renderer.assemble`` (goofer_assemble_batch alone) runs, and the row padding ``[bins, ld)`` and the
guard rows behind the last note must still hold the pattern.  Edited rows are mapped to notes with the plan's ``row_lo`` /
``row_hi`` / edit offsets.  The 'sj' multiplier array is the test's own (assemble_ref.growl_factor).

THE JUDGEMENT for matrices is assemble_ref's: per row, ``e_gpu(t) <= 3 E_ref(note) + 2^-23`` with both errors taken against
the float64 truth and relative to the row's own peak; rows whose truth is zero must be zero.  No RMS, no row and no bin left
out.  Notes with 'vf' are judged after the bin squeeze (the device edits the rows in place); every other note before it.
For samples: ``mask`` equals the fp32 cast of the oracle's bit for bit; ``f0``, ``f0_growl`` and ``bend`` are within one fp32 ulp of
the fp32 cast of the oracle's float64 value and ``f0`` is exactly 0 where the mask is 0.  The whole matrix runs with option
``sa_fast`` 0 and 1 (equal bits, judged once) and with ``value_f64`` 1 (the fp64 value arithmetic of k_env_edit, held to the same
factor 3; this is the only place the suite turns that option on).

THE CASES (assemble_ref.matrix, 49 notes per geometry, plain and hard sources alternating): one flag at a time at both ends of
its range (br, es -80 / -10 / 10 / 80, fw +-80, each formant-strength bell alone at +-40 and all four, vf of either sign with vl 0
and 100, FV, R, L0 with a five-frame tail and with a long one, L1, L2, velocity 0 / 60 / 140 / 200, pd +-, sj), formant tracks at the
sanitiser's limits, six random flag strings, notes of 1023 / 1024 / 1025 / 4097 samples, a note of half a hop, a note without a
consonant.  Sub-batches of 1, 3, 4, 5 and 13 notes must reproduce the full batch's bits.

THE FUSED ROUTE (test_fused_route_equals_split): the hard-source notes with formant shifts that cross anchors (the ratios of
test_warp_bins_crossing_anchors_follow_numpy_interp, 'g' for the uniform stage) render to the same bits through
goofer_render_batch and through the split calls, to the same numbers with overlap 0, and the fused call leaves the envelope
the assemble-alone call left, which is judged against the truth as above.  WHERE THE FUSED KERNELS RUN: goofer_render_batch
hands the assembly a warped-copy destination only on the stem-walker route, and ``stems_supported`` is n_fft 1024 with hop 256.
So k_row_recs<true> / k_env_rows<true, 9> run in the [44100_1024_256] case alone, on its first group (no 'vf': a batch with a
fry edit keeps the warp apart, ``any_fry`` in launch_assemble; no 'sg' / 'sr': Renderer.run assembles on its own for a batch
that mixes them with others), and the CH 17 / CH 0 instantiations of k_env_rows<true> are not reachable through the ABI at all.
That this case does run them was checked once with two seeded changes (the uniform stage's ratio, a sorted segment's offset:
docs/HISTORY.md): both fail it and nothing else.  At the other widths the same two batches hold the route those widths take to
the same comparisons.  The notes with 'vf' / 'sg' / 'sr' are the second group everywhere.

MEASURED on an MI355X.  Per geometry and stage the note whose worst row has the largest (e_gpu - 2^-23) / E_ref: its E_ref / that
row's e_gpu (the ratio).  Every stage holds the factor 3 under either arithmetic; the largest ratio is 1.47.

    sr n_fft hop      default: edited              env                          value_f64: edited            env
    44100 1024 256    3.35e-07 / 4.58e-07 (1.01)   3.35e-07 / 4.58e-07 (1.01)   5.61e-07 / 7.22e-07 (1.07)   5.61e-07 / 7.22e-07 (1.07)
    48000 2048 512    6.07e-07 / 8.82e-07 (1.26)   6.07e-07 / 8.82e-07 (1.26)   6.07e-07 / 8.82e-07 (1.26)   6.07e-07 / 8.82e-07 (1.26)
    22050  512 128    3.24e-07 / 5.95e-07 (1.47)   3.42e-07 / 6.02e-07 (1.41)   3.24e-07 / 5.95e-07 (1.47)   3.42e-07 / 6.02e-07 (1.41)
    44100 1100 275    3.48e-07 / 5.33e-07 (1.19)   3.48e-07 / 5.33e-07 (1.19)   4.10e-07 / 5.98e-07 (1.17)   4.11e-07 / 5.98e-07 (1.17)
    44100 1150 250    5.66e-07 / 6.38e-07 (0.92)   2.74e-07 / 4.17e-07 (1.09)   2.74e-07 / 3.92e-07 (1.00)   2.87e-07 / 3.91e-07 (0.95)
    44100  768 192    3.70e-07 / 4.32e-07 (0.85)   2.43e-07 / 3.63e-07 (1.00)   3.43e-07 / 3.89e-07 (0.78)   2.43e-07 / 3.63e-07 (1.00)
    44100  600 150    2.57e-07 / 3.60e-07 (0.94)   3.52e-07 / 4.70e-07 (1.00)   3.16e-07 / 4.14e-07 (0.93)   2.13e-07 / 3.36e-07 (1.02)
    16000   64  16    1.87e-07 / 3.01e-07 (0.97)   1.97e-07 / 3.02e-07 (0.93)   1.87e-07 / 3.01e-07 (0.97)   1.72e-07 / 3.09e-07 (1.11)
    44100 2046 512    5.60e-07 / 7.28e-07 (1.09)   5.60e-07 / 7.28e-07 (1.09)   6.28e-07 / 7.70e-07 (1.04)   6.28e-07 / 7.70e-07 (1.04)

    (E_ref of the es notes, which the table's rows are not: 1.1e-06 to 2.4e-06 at the widths above 64, tests/test_assemble_ref.py.)
    Samples that differ from the fp32 cast of the oracle's float64 value at all, over the nine geometries: f0 0 of 4 248 715,
    f0_growl 0 of 381 078, bend 0 of 199 870; the mask equals the oracle's in every sample.  So one ulp is never used; it stays
    the bound, since the device's 2^x and its tick interpolation are 1e-16 approximations of numpy's, not the same operations.
"""
import numpy as np
import pytest

import assemble_ref as A
from goofer_amd import synthetic as syn
from oracle import sampler_ref as SR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
PATTERN = 0x7FC0DEAD                                               # a quiet NaN with a payload no kernel produces
GUARD_ROWS = 3
FACTOR = {"edited": 3.0, "env": 3.0}
SAMPLE_ULP = 1

_CPU, _DEV = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def cpu(geo):
    """(cases, [(reference arithmetic, truth)]) of a geometry's matrix: computed once, shared, never written to."""
    if geo not in _CPU:
        cases = A.matrix(*geo)
        res = []
        for i, c in enumerate(cases):
            ref, truth = A.both(A.features_of(c["src"]), SR.decode_request(*syn.request_args(c["req"])), geo[2])
            ref["f0_growl"] = ref["f0"] * A.growl_factor(i, len(ref["f0"]))
            res.append((ref, truth))
        _CPU[geo] = (cases, res)
    return _CPU[geo]


def _jobs(cases):
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    return [(Source.from_pack(c["src"]["env_pack"], c["src"]["f0"], c["src"]["mask"], c["src"]["formants"], c["src"]["sr"],
                              c["src"]["y_len"]), S.decode_request(*syn.request_args(c["req"]))) for c in cases]


def _fill(t):
    t.view(torch.int32).fill_(PATTERN)


def _is_pattern(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.int32) == PATTERN))


def assemble(ctx, geo, cases, idxs):
    """goofer_assemble_batch alone over the notes ``idxs`` of ``cases``.  Returns what the device left, per note."""
    from goofer_amd.render import Renderer
    sr, n_fft, hop = geo
    r = Renderer(ctx, hop=hop)
    prep = r.prepare(_jobs([cases[i] for i in idxs]), trim_rows=False)
    a = prep["assembly"]
    B, ld, t_off, e_off = n_fft // 2 + 1, int(a.ld), int(a.total_out_rows), int(a.total_edit_rows)
    assert a.n_bins == B and e_off == prep["edit_rows"]
    edit = torch.empty((e_off + GUARD_ROWS, ld), dtype=torch.float32, device=ctx.device)
    env = torch.empty((t_off + GUARD_ROWS, ld), dtype=torch.float32, device=ctx.device)
    a.edit_rows, a.env_out = edit.data_ptr(), env.data_ptr()
    prep["env"] = env[:t_off, :B]
    so = prep["sample_off"]
    if prep["growl"]:                                              # the sj multiplier: the test's own array
        mul = np.ones(int(so[-1]))
        for k in prep["growl"]:
            mul[int(so[k]):int(so[k + 1])] = A.growl_factor(idxs[k], int(so[k + 1] - so[k]))
        prep["keep"]["f0_mul"].copy_(ctx.tensor(mul))
    outs = [edit, env, prep["f0"], prep["mask"]] + [t for t in (prep["bend_out"], prep["f0_growl"]) if t is not None]
    for t in outs:
        _fill(t)
    r.assemble(prep)
    ctx.check()
    edit_h, env_h = edit.cpu().numpy(), env.cpu().numpy()
    assert _is_pattern(edit_h[:, B:]) and _is_pattern(edit_h[e_off:]), "k_env_edit wrote outside its rows"
    assert _is_pattern(env_h[:, B:]) and _is_pattern(env_h[t_off:]), "the row kernels wrote outside their rows"
    geo_p = prep["planned"].geo
    n_edit = (geo_p["row_hi"] - geo_p["row_lo"]).astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(n_edit)])
    assert eo[-1] == e_off
    host = {k: prep[k].cpu().numpy() for k in ("f0", "mask")}
    host["bend"] = prep["bend_out"].cpu().numpy() if prep["bend_out"] is not None else None
    host["f0_growl"] = prep["f0_growl"].cpu().numpy() if prep["f0_growl"] is not None else None
    notes = []
    for k in range(len(idxs)):
        sl = slice(int(so[k]), int(so[k + 1]))
        notes.append({"edited": edit_h[eo[k]:eo[k + 1], :B], "row_lo": int(geo_p["row_lo"][k]),
                      "env": env_h[int(prep["env_off"][k]):int(prep["env_off"][k + 1]), :B],
                      "f0": host["f0"][sl], "mask": host["mask"][sl],
                      "bend": None if host["bend"] is None else host["bend"][sl],
                      "f0_growl": None if host["f0_growl"] is None else host["f0_growl"][sl]})
    return notes, prep, r


def _same_bits(x, y):
    if x is None or y is None:
        return x is None and y is None
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def judge(label, cases, idxs, res, notes, factor, samples=True):
    """Every note of the batch, every stage; prints the worst figures, then asserts."""
    worst = {s: [0.0, 0.0, 0.0] for s in ("edited", "env")}             # E_ref, e_gpu, (e_gpu - 2^-23) / E_ref of the worst rows
    off_by_one = {k: [0, 0] for k in ("f0", "f0_growl", "bend")}
    bad = []
    for k, i in enumerate(idxs):
        (ref, truth), d, name = res[i], notes[k], cases[i]["name"]
        lo = d["row_lo"] - ref["edit_lo"]
        assert lo >= 0 and lo + d["edited"].shape[0] <= ref["edited"].shape[0], name
        rows = slice(lo, lo + d["edited"].shape[0])
        env_stage = "env_fry" if ref["fry_mask"] is not None else "env"
        for stage, gpu, rf, tr in (("edited", d["edited"], ref["edited"], truth["edited"][rows]),
                                   ("env", d["env"], ref[env_stage], truth[env_stage])):
            assert gpu.dtype == F32
            E_ref = A.errors(rf, rf, truth["edited"] if stage == "edited" else tr)[0]
            e_gpu = A.row_errors(gpu, tr)
            w = float(np.max(e_gpu)) if e_gpu.size else 0.0
            ratio = (w - A.EPS32) / E_ref if E_ref > 0 else (0.0 if w <= A.EPS32 else np.inf)
            if not (ratio <= worst[stage][2]):
                worst[stage] = [E_ref, w, ratio]
            if not A.within(E_ref, e_gpu, factor[stage]):
                t = int(np.argmax(np.where(np.isnan(e_gpu), np.inf, e_gpu)))
                bad.append((name, stage, "row %d of %d" % (t, e_gpu.size), "E_ref %.3g e_gpu %.3g ratio %.2f" % (E_ref, w, ratio)))
        if not samples:
            continue
        if not _same_bits(d["mask"], ref["mask"].astype(F32)):
            bad.append((name, "mask", int(np.count_nonzero(d["mask"] != ref["mask"].astype(F32)))))
        if np.any(d["f0"][d["mask"] == 0.0] != 0.0):
            bad.append((name, "f0 where the mask is 0"))
        for key in ("f0", "f0_growl", "bend"):
            want = ref[key] if key != "f0_growl" or A.has_flag(cases[i], "sj") else None
            if want is None:
                if key == "bend" and d["bend"] is not None and not _is_pattern(d["bend"]):
                    bad.append((name, "bend written for a note without pd"))
                if key == "f0_growl" and d["f0_growl"] is not None and not _same_bits(d["f0_growl"], d["f0"]):
                    bad.append((name, "f0_growl of a note without sj is not its f0"))
                continue
            if d[key] is None:
                bad.append((name, key, "not written"))
                continue
            dist = A.ulp_distance(d[key], want.astype(F32))
            off_by_one[key][0] += int(np.count_nonzero(dist))
            off_by_one[key][1] += dist.size
            if dist.size and dist.max() > SAMPLE_ULP:
                j = int(np.argmax(dist))
                bad.append((name, key, "sample %d: %d ulp (%r, oracle %r)" % (j, int(dist[j]), float(d[key][j]), float(want[j]))))
    print("%-34s" % label + "  ".join("%s E_ref %.2e e_gpu %.2e ratio %.2f" % (s, *worst[s]) for s in worst) +
          ("  off by one ulp: " + " ".join("%s %d/%d" % (k, *v) for k, v in off_by_one.items()) if samples else ""))
    assert not bad, bad[:12]
    return worst


def full_batch(ctx, geo):
    """The whole matrix as one ragged batch under the default options (shared by the tests of a geometry)."""
    if geo not in _DEV:
        cases, _ = cpu(geo)
        _DEV[geo] = assemble(ctx, geo, cases, list(range(len(cases))))[0]
    return _DEV[geo]


def _equal_notes(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        for key in ("edited", "env", "f0", "mask", "bend", "f0_growl"):
            if key in ("bend", "f0_growl") and (x[key] is None or y[key] is None):
                continue                                            # (a batch without a pd / sj note has no such output)
            assert _same_bits(x[key], y[key]), (what, k, key)


@pytest.mark.parametrize("geo", A.GEOMETRIES, ids=A.GEO_IDS)
def test_assembly_stages_against_the_truth(ctx, geo):
    """The full matrix: default arithmetic judged; sa_fast 0 gives the same bits; value_f64 1 judged at factor 3 as well."""
    cases, res = cpu(geo)
    idxs = list(range(len(cases)))
    notes = full_batch(ctx, geo)
    tag = A.GEO_IDS[A.GEOMETRIES.index(geo)]
    try:
        ctx.set_option("sa_fast", 0)
        slow = assemble(ctx, geo, cases, idxs)[0]
        ctx.set_option("sa_fast", 1)
        ctx.set_option("value_f64", 1)
        v64 = assemble(ctx, geo, cases, idxs)[0]
    finally:
        ctx.set_option("sa_fast", 1)
        ctx.set_option("value_f64", 0)
    _equal_notes(notes, slow, "sa_fast 0 against 1")
    for x, y in zip(notes, v64):
        for key in ("f0", "mask", "bend", "f0_growl"):
            assert _same_bits(x[key], y[key]), ("value_f64 moved a sample output", key)
    failures = []
    for label, got, factor, samples in (("%s default" % tag, notes, FACTOR, True),
                                        ("%s value_f64" % tag, v64, {"edited": 3.0, "env": 3.0}, False)):
        try:
            judge(label, cases, idxs, res, got, factor, samples)
        except AssertionError as e:                                 # (both arithmetics are printed before either fails the test)
            failures.append((label, e.args[0] if e.args else ""))
    assert not failures, failures


@pytest.mark.parametrize("geo", A.GEOMETRIES, ids=A.GEO_IDS)
def test_small_batches_reproduce_the_full_batch(ctx, geo):
    """1, 3, 4, 5 and 13 notes (A_ROWS = 4: last workgroups with one to four live waves; a k_sample_assemble grid that ends inside
    a tile): a note's bits do not depend on the batch around it."""
    cases, _ = cpu(geo)
    notes = full_batch(ctx, geo)
    for start, count in ((3, 1), (0, 3), (17, 4), (24, 5), (30, 13)):
        idxs = list(range(start, start + count))
        got = assemble(ctx, geo, cases, idxs)[0]
        _equal_notes([notes[i] for i in idxs], got, (start, count))


@pytest.mark.parametrize("geo", A.GEOMETRIES, ids=A.GEO_IDS)
def test_fused_route_equals_split(ctx, geo):
    """goofer_render_batch against the split calls, bit for bit in harm / uv / bre / mix, and against overlap 0 (equal numbers);
    the envelope the fused call leaves equals the assemble-alone one, which is judged against the truth.  The first group takes
    the fused warp (k_row_recs<true> / k_env_rows<true, 9>) where the product has one, at n_fft 1024 with hop 256; the second
    (notes with 'vf', 'sg' or 'sr') never does: module docstring."""
    from goofer_amd.render import Renderer
    cases, res = cpu(geo)
    plain, rest = A.fused_matrix(*geo)
    assert len(plain) >= 10 and len(rest) >= 2
    assert all(res[i][0]["fry_mask"] is None for i, _ in plain) and any(res[i][0]["fry_mask"] is not None for i, _ in rest)
    for label, group in (("fused", plain), ("vf / sg / sr", rest)):
        idxs = [i for i, _ in group]
        shifted = {i: c for i, c in group}
        batch = [shifted.get(i, cases[i]) for i in range(len(cases))]
        for i, c in group:                                          # the shifts do not reach the assembly: same request otherwise
            p0, p1 = SR.decode_request(*syn.request_args(cases[i]["req"])), SR.decode_request(*syn.request_args(c["req"]))
            assert p1.F_shift != (1.0, 1.0, 1.0, 1.0) and p0.formant_strength == p1.formant_strength and p0.env_shape == p1.env_shape
        alone, _, _ = assemble(ctx, geo, batch, idxs)
        judge("%s %s, assemble alone" % (A.GEO_IDS[A.GEOMETRIES.index(geo)], label), batch, idxs, res, alone, FACTOR)
        r = Renderer(ctx, hop=geo[2])
        np.random.seed(11)                                          # (the sh / sr draws of the random flag strings: made once, in prepare)
        prep = r.prepare(_jobs([batch[i] for i in idxs]), trim_rows=False)
        keys = ("harm", "uv", "bre", "mix")
        try:
            out = r.run(prep, seed=5, keep_stems=True)
            ctx.check()
            fused = {k: out[k].cpu().numpy() for k in keys}
            env_fused = prep["env"].cpu().numpy()
            out = r.run(prep, seed=5, keep_stems=True, split=True)
            ctx.check()
            split = {k: out[k].cpu().numpy() for k in keys}
            env_split = prep["env"].cpu().numpy()
            ctx.set_option("overlap", 0)
            out = r.run(prep, seed=5, keep_stems=True)
            ctx.check()
            serial = {k: out[k].cpu().numpy() for k in keys}
        finally:
            ctx.set_option("overlap", 1)
        for k in keys:
            assert np.isfinite(fused[k]).all(), (label, k)
            assert _same_bits(fused[k], split[k]), (label, k, "fused against split")
            # overlap 0: the same numbers.  At n_fft 2048 the spectra route decides the noise stems' sparsity per frame only with
            # overlap on (synth_route_of: skip_frames), and a transform that is skipped leaves + 0.0 where the sum of an all-zero
            # frame leaves - 0.0: uv and bre then differ in the sign of zeros (measured: 10 010 and 29 238 samples of this batch, no
            # other sample, mix in none).  So equal values here, as torch.equal in test_render_batch_equals_separate_calls.
            assert np.array_equal(fused[k], serial[k]), (label, k, "overlap 1 against 0")
        assert _same_bits(fused["mix"], serial["mix"]) and _same_bits(fused["harm"], serial["harm"]), label
        assert float(np.abs(fused["mix"]).max()) > 0.0
        assert _same_bits(env_fused, env_split), label
        eo = prep["env_off"]
        for k in range(len(idxs)):
            assert _same_bits(env_fused[int(eo[k]):int(eo[k + 1])], alone[k]["env"]), (label, batch[idxs[k]]["name"])
