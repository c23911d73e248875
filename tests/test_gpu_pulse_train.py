"""GPU: the main pulse train of csrc/pulse.hip — k_pulse_onsets_par / k_pulse_onsets_scan, k_onset_finish, k_pulse_tiles,
k_pulse_place over the plan's k_pulse_peak / k_pulse_shape_table — sample by sample against the float64 truth of
tests/pulse_ref.py, at the period clamps, the exact rounding ties, the ends of the shape table and the dense tiles.

The judge (pulse_ref.judge): the onset lists are exactly the restatement's; |pulse - truth| <= c 2^-24 A + 2^-149 at every
sample, c = (C + 2)(1 + 2^-20) + t derived in pulse_ref's docstring from the operations (A = sum |v_k| over the C covering
pulses, t the term for tabulating the shape at the nominal period); a sample no pulse covers is an exact +0.0; nothing is
non-finite.  The batches (pulse_ref.cases) are the smallest that reach each path:
  a   one-onset notes for T0 = 3 .. 8192: one table row each, first to last sample (pulse_tab_row up to 2^25)
  b   both clamps of T0 = clip(rint(sr T), 3, 8192), overlapping three-sample pulses, a tie that rounds up     44100, 96000
  c   exact ties sr * (1 / f0) = k + 0.5: half-even against half-up and truncation              22050, 44100, 48000, 96000
  d   covering lists of 510 .. 513, 615 and 976 onsets in interior tiles: the LDS list at its fullest (512), the step to the
      per-sample search, that search on whole tiles
  e   one 7350-sample pulse in front of dense onsets: the look-back held open over five tiles, covering lists up to 1834
  f   a ragged batch of notes of 1 .. 2049 voiced samples: pulses cut at the note's end, boundary tiles, `live < PP_SPT` tails
  g   rows 3, 2049, 8192 under three other LF models and back at the default: the rebuilt table's far end
tests/test_pulse_ref.py shows on the CPU that ten planted faults (T0 by half-up or by truncation, the clamps at 2048 and at 2, a
row offset one off, a row one sample short, only the latest three onsets summed, the covering list cut to 512, a look-back that
stops at an onset's own end, a pulse not cut at the note's end) each fall outside this bound by factors above 1e6.

Every rate is planned once: the 44100 tests come first, the other rates behind them in ascending order; the three pulse_scan
modes of a batch run once per module and serve the truth test and the mode test.

MEASURED on the MI355X (each test prints its figures; the table is in docs/HISTORY.md, "The pulse train at its clamps, table ends
and dense tiles"): worst error / bound 0.759 (a), 0.748 (b), 0.675 (c), 0.278 (d), 0.434 (e), 0.544 (f), 0.749 (g) at 44100, 0.675
(c at 22050), 0.563 (c at 48000), 0.746 and 0.552 (b, c at 96000) — batch for batch the figure of pulse_ref.table_row placed on the
CPU.  Samples whose bits differ from the reference arithmetic: none except where T0 is far from sr / f0 — 371 of 31 600 (b), 2 972
of 6 244 (d, 21 kHz), 371 of 6 250 (f), 2 of 16 624 (c), 427 of 61 600 (b at 96000): the table holds the shape of the nominal
period.  In mode 1 every note whose phase comes within two bands of an integer was walked.
"""
import numpy as np
import pytest

import pulse_ref as P
from test_gpu_kernels import _onset_lists, _pulse_scan_modes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
GEO = (1024, 256)
AT_44100 = list(P.cases(44100))
ELSEWHERE = [(sr, name) for sr in sorted(P.RATES) if sr != 44100 for name in P.cases(sr)]
DENSE = [("d%d" % f, 0) for f in P.D_F0] + [("e", 0)]         # (batch, note) of the (d) and (e) notes


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _off(c, lengths):
    return c.tensor(c.offsets(lengths))


def _stop(e):
    pytest.exit("the pulse train failed on the device: %r" % (e,), returncode=3)   # nothing more is started on this GPU


_RUNS = {}


def _modes(ctx, sr, name):
    """{pulse_scan mode: (pulse, onset lists, notes scanned, notes walked)} of a batch of pulse_ref.cases, run once per module"""
    if (sr, name) not in _RUNS:
        b = P.cases(sr)[name]
        ctx.plan(sr, *GEO)
        try:
            ctx.pulse_model(*b["model"])
            _RUNS[sr, name] = _pulse_scan_modes(ctx, b["f0s"])
            ctx.check()
        except RuntimeError as e:
            _stop(e)
        finally:
            ctx.pulse_model()
    return _RUNS[sr, name]


def _train(ctx, f0s):
    lens = [len(f) for f in f0s]
    try:
        out = ctx.pulse_train(ctx.tensor(np.concatenate(f0s)), _off(ctx, lens)).cpu().numpy()
        ctx.check()
    except RuntimeError as e:
        _stop(e)
    return out, _onset_lists(ctx, lens)


def _same_bits(a, b):
    return np.array_equal(P.bits(a), P.bits(b))


def _truth(ctx, sr, name):
    b, tr = P.cases(sr)[name], P.truth(sr, name)
    pulse, lists = _modes(ctx, sr, name)[1][:2]
    for k, (t, got) in enumerate(zip(tr, lists)):
        assert np.array_equal(got, t["oi"]), (name, b["names"][k], "onset samples")
    v = P.judge(pulse, tr)
    ref = np.concatenate([t["pulse32"] for t in tr])
    print("MEASURED pulse train %d %-7s worst error / bound %.3f; %d of %d samples differ in bits from the reference arithmetic"
          % (sr, name, v["worst"], int(np.sum(P.bits(pulse) != P.bits(ref))), pulse.size))
    assert v["finite"], (name, "non-finite")
    assert v["first"] is None, (name, "outside the bound: (note, sample)", v["first"], b["names"][v["first"][0]], v["worst"])
    assert v["zeros"], (name, "a sample no pulse covers is not +0.0")


def _scan_modes(ctx, sr, name):
    b = P.cases(sr)[name]
    res = _modes(ctx, sr, name)
    n = len(b["f0s"])
    verdict = [P.scan_verdict(f, sr) for f in b["f0s"]]
    must, may = verdict.count("walk"), verdict.count("either")
    print("MEASURED pulse_scan %d %-7s %d notes: %d must be walked, %d may be; walked in mode 1: %d" % (sr, name, n, must, may, res[1][3]))
    assert res[0][2:] == (0, 0)                                # the walk kernel: no scan at all
    assert res[2][2:] == (n, n)                                # forced: every note walked inside the scan kernel
    assert res[1][2] == n and must <= res[1][3] <= must + may, (res[1][2:], must, may)
    for mode in (1, 2):
        assert _same_bits(res[mode][0], res[0][0]), (name, mode)
        for k, (x, y) in enumerate(zip(res[mode][1], res[0][1])):
            assert np.array_equal(x, y), (name, mode, b["names"][k])


@pytest.mark.parametrize("name", AT_44100)
def test_truth(ctx, name):
    _truth(ctx, 44100, name)


@pytest.mark.parametrize("name", AT_44100)
def test_pulse_scan_modes(ctx, name):
    _scan_modes(ctx, 44100, name)


def test_integer_phase_notes_are_walked(ctx):
    """the constant-f0 notes whose crossings land on integer phases (14 700, 11 025 Hz, fp32(sr / 2^k)): the scan must hand
    every one to the walk, and a batch of one shows which note the counter counted"""
    for name in ("d11025", "d13230", "d21000"):
        (f,) = P.cases(44100)[name]["f0s"]
        assert P.scan_verdict(f, 44100) == "walk" and _modes(ctx, 44100, name)[1][2:] == (1, 1), name
    b = P.cases(44100)["a"]
    walk = [k for k, f in enumerate(b["f0s"]) if P.scan_verdict(f, 44100) == "walk"]
    assert [P.A_T0[k] for k in walk] == [3, 4, 5, 64, 256, 2048, 4096, 8192]
    ctx.plan(44100, *GEO)
    try:
        s0, w0 = ctx.counter("pulse_scanned_notes"), ctx.counter("pulse_fallback_notes")
        _train(ctx, [b["f0s"][k] for k in walk])
        assert (ctx.counter("pulse_scanned_notes") - s0, ctx.counter("pulse_fallback_notes") - w0) == (len(walk), len(walk))
    except RuntimeError as e:
        _stop(e)


def test_peak_table_rows(ctx):
    ctx.plan(44100, *GEO)
    peak = ctx.table(5)
    assert peak.size == 8193
    for T0 in P.A_T0:
        assert P.bits(peak[T0:T0 + 1])[0] == P.bits(np.array([P.table_peak(T0, 44100)]))[0], T0


def test_notes_alone_and_in_company(ctx):
    """(d) and (e) as batches of one, behind a 1 000-sample neighbour (tiles no longer start at the note's start: other covering
    lists, the first tile across the boundary) and inside the ragged batch (f): the same bits all three times"""
    ctx.plan(44100, *GEO)
    neighbour = np.full(1000, 523.25, dtype=F32)
    ragged = P.cases(44100)["f"]["f0s"]
    for name, k in DENSE:
        f = P.cases(44100)[name]["f0s"][k]
        t = P.truth(44100, name)[k]
        alone = _modes(ctx, 44100, name)[1]
        behind, lists_b = _train(ctx, [neighbour, f])
        inside, lists_i = _train(ctx, ragged[:5] + [f] + ragged[5:])
        a = sum(len(x) for x in ragged[:5])
        assert np.array_equal(alone[1][0], t["oi"]) and np.array_equal(lists_b[1], t["oi"]) and np.array_equal(lists_i[5], t["oi"]), name
        assert _same_bits(behind[1000:], alone[0]), (name, "behind a neighbour")
        assert _same_bits(inside[a:a + len(f)], alone[0]), (name, "inside the ragged batch")
        # ... and the company is left as it is alone
        rag = _modes(ctx, 44100, "f")[1][0]
        assert _same_bits(inside[:a], rag[:a]) and _same_bits(inside[a + len(f):], rag[a:]), (name, "the ragged batch around it")


def test_batch_driver_makes_the_same_train(ctx):
    """goofer_synth_batch carves its own tile table and onset slots (csrc/synth.hip): its pulse / onset_cnt / onset_idx views
    against goofer_pulse_train's on the notes of (d), (e) and rows 2049 and 8192 of (a), bit for bit, on both routes"""
    from goofer_amd.device import default_params
    from test_gpu_presynth_stages import DEFAULTS, ROUTES
    sr = 44100
    a = P.cases(sr)["a"]["f0s"]
    f0s = [P.cases(sr)[name]["f0s"][k] for name, k in DENSE] + [a[P.A_T0.index(2049)], a[P.A_T0.index(8192)]]
    lens = [len(f) for f in f0s]
    N = sum(lens)
    ctx.plan(sr, *GEO)
    want, _ = _train(ctx, f0s)
    cnt, idx = ctx.debug_fetch("onset_cnt"), ctx.debug_fetch("onset_idx")
    Ts = [1 + n // GEO[1] for n in lens]
    nb = GEO[0] // 2 + 1
    par = default_params(len(lens))
    par["normalize"] = 0.0
    env = ctx.rows_from(np.ones((sum(Ts), nb), dtype=F32))
    phi = ctx.rows_from(np.zeros((sum(Ts), nb), dtype=F32))
    d_f0, d_mask = ctx.tensor(np.concatenate(f0s)), ctx.tensor(np.ones(N, dtype=F32))
    try:
        for route, (opts, names) in ROUTES.items():
            for k, v in dict(DEFAULTS, **opts).items():
                ctx.set_option(k, v)
            ctx.profile_begin(1)
            try:
                out = ctx.synth_batch(env, Ts, d_f0, d_mask, lens, par, phi=phi)
                torch.cuda.synchronize()
                mix = out["mix"].cpu().numpy()
            except RuntimeError as e:
                _stop(e)
            ctx.profile_end()
            ran = ctx.profile_stage_names()
            assert ran[:6] == names[:6] and ("harm_stem" in ran) == (route == "walkers") and ("irfft_ola3" in ran) == (route == "stems0"), (route, ran)
            ctx.check()
            assert mix.size == N
            assert _same_bits(ctx.debug_fetch("f0"), np.concatenate(f0s)), route
            assert _same_bits(ctx.debug_fetch("pulse"), want), (route, "pulse")
            assert np.array_equal(ctx.debug_fetch("onset_cnt"), cnt), (route, "onset_cnt")
            got = ctx.debug_fetch("onset_idx")
            assert got.size == idx.size == N // 2 + 16 * len(lens) + 16
            off = np.concatenate([[0], np.cumsum(lens)])
            for k in range(len(lens)):
                s = off[k] // 2 + 16 * k
                assert np.array_equal(got[s:s + cnt[k]], idx[s:s + cnt[k]]), (route, "onset_idx", k)
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


@pytest.mark.parametrize("sr,name", ELSEWHERE)
def test_truth_at_other_rates(ctx, sr, name):
    _truth(ctx, sr, name)


@pytest.mark.parametrize("sr,name", ELSEWHERE)
def test_pulse_scan_modes_at_other_rates(ctx, sr, name):
    _scan_modes(ctx, sr, name)
