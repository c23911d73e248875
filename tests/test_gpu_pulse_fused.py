"""GPU: k_pulse_note (csrc/pulse.hip; option pulse_fused = 1, the default) — scan, periods and placement in one pass per note —
against the four-kernel chain it replaces (pulse_fused = 0: k_pulse_onsets_par, k_onset_finish, k_pulse_tiles, k_pulse_place).

The judge is np.array_equal on the bits (pulse_ref.bits): the fused kernel runs the same operations on the same values in the
same order, so there is no tolerance.  Beside the pulse: the onset lists, onset_cnt and the counters pulse_scanned_notes /
pulse_fallback_notes are equal, and pulse_list_notes says which notes were placed from the onset list in global memory.

  cases    every batch of pulse_ref.cases(44100) and batches b, c at 96000, under pulse_scan 1 and 2: both clamps of T0, the
           half-even ties, covering lists of 510 - 513 / 615 / 976 / 1834, the 7350-sample pulse held open over five rounds, notes
           of 1 - 2049 samples cut at the note's end
  ring     notes whose window of live onsets is PN_RING - 1, PN_RING and PN_RING + 1 (an 8192-sample pulse in front of dense
           onsets, the windows counted on the CPU as the kernel counts them): 0, 0 and 1 notes in list mode
  edges    a ragged batch (1 .. 4097 samples, an empty note, first notes of 1, 3 and 5 samples so that later notes start off the
           16-byte grid) and longer notes — voiced from sample 0, an unvoiced head, 50 ms gaps of f0 == 0, a gap of f0 = 1e-6 in
           which an onset falls (its own f0 is not a valid one: the look-back runs), a glide 80 -> 900 Hz, 11 000.3 Hz (dense covering lists from
           the ring), 441 Hz from phase 0 (walked), a negative and a NaN increment (walked) — each note alone and in the batch
  driver   eight notes of config 3 and eight of config 4 through the renderer: mix and the pulse view

Each batch runs once per option setting; the module stops at the first device error.
"""
import numpy as np
import pytest

import pulse_ref as P
from test_gpu_kernels import _onset_lists

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
GEO = (1024, 256)
RING, ROUND = 2048, 2048                                       # PN_RING, PAR_ROUND of csrc/pulse.hip
CASES = [(44100, name) for name in P.cases(44100)] + [(96000, "b"), (96000, "c")]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.set_option("pulse_fused", 1)
    c.set_option("pulse_scan", 1)
    c.close()


def _stop(e):
    pytest.exit("the fused pulse kernel failed on the device: %r" % (e,), returncode=3)   # nothing more is started on this GPU


COUNTERS = ("pulse_scanned_notes", "pulse_fallback_notes", "pulse_list_notes")


def _run(ctx, f0s, scan=1, fused=1):
    """one goofer_pulse_train of the batch under the two options: pulse, onset lists, onset_cnt, the counters' increments"""
    lens = [len(f) for f in f0s]
    try:
        ctx.set_option("pulse_scan", scan)
        ctx.set_option("pulse_fused", fused)
        before = [ctx.counter(c) for c in COUNTERS]
        d_f0 = ctx.tensor(np.concatenate(f0s).astype(F32))
        pulse = ctx.pulse_train(d_f0, ctx.tensor(ctx.offsets(lens))).cpu().numpy()
        ctx.check()
        res = {"pulse": pulse, "lists": _onset_lists(ctx, lens), "cnt": ctx.debug_fetch("onset_cnt").copy()}
        res.update({c: ctx.counter(c) - b for c, b in zip(COUNTERS, before)})
    except RuntimeError as e:
        _stop(e)
    finally:
        ctx.set_option("pulse_scan", 1)
        ctx.set_option("pulse_fused", 1)
    return res


def _assert_same(a, b, what):
    assert np.array_equal(P.bits(a["pulse"]), P.bits(b["pulse"])), (what, "pulse bits",
                                                                    int(np.argmax(P.bits(a["pulse"]) != P.bits(b["pulse"]))))
    assert np.array_equal(a["cnt"], b["cnt"]), (what, "onset_cnt")
    for k, (x, y) in enumerate(zip(a["lists"], b["lists"])):
        assert np.array_equal(x, y), (what, "onset list", k)
    for c in COUNTERS[:2]:
        assert a[c] == b[c], (what, c, a[c], b[c])


@pytest.mark.parametrize("sr,name", CASES)
def test_cases_fused_equals_chain(ctx, sr, name):
    b = P.cases(sr)[name]
    ctx.plan(sr, *GEO)
    try:
        ctx.pulse_model(*b["model"])
        for scan in (1, 2):
            fused, chain = _run(ctx, b["f0s"], scan, 1), _run(ctx, b["f0s"], scan, 0)
            _assert_same(fused, chain, (sr, name, scan))
            assert chain["pulse_list_notes"] == 0
            assert fused["pulse_list_notes"] >= fused["pulse_fallback_notes"]
            if scan == 2:
                assert fused["pulse_list_notes"] == len(b["f0s"])
            print("MEASURED pulse_fused %d %-7s pulse_scan %d: %d notes, %d walked, %d in list mode"
                  % (sr, name, scan, len(b["f0s"]), fused["pulse_fallback_notes"], fused["pulse_list_notes"]))
    except RuntimeError as e:
        _stop(e)
    finally:
        ctx.pulse_model()


# ---------------------------------------------------------------------------------------------
# the ring at its limit
# ---------------------------------------------------------------------------------------------
def _window(f0, sr):
    """the largest window of live onsets over the rounds of a note, counted as k_pulse_note counts it: per round of 2048 samples
    from sample c0, hi = the onsets (that have a slot) up to the round's end, live = the first onset whose running end_max
    passes c0, no further than the round's first new onset"""
    oi, _, T0, _ = P.onsets(f0, sr)
    cap = len(f0) // 2 + 16
    end_max = np.maximum.accumulate(oi + T0)
    worst = 0
    for c0 in range(0, len(f0), ROUND):
        lo = min(int(np.searchsorted(oi, c0, "left")), cap)
        hi = min(int(np.searchsorted(oi, c0 + ROUND, "left")), cap)
        live = min(int(np.searchsorted(end_max, c0, "right")), lo)
        worst = max(worst, hi - live)
    return worst


def _ring_note(window, sr=44100):
    """one 8192-sample pulse from sample 100 (its end, 8292, lies in the fifth round: samples 8192 .. 10239), then an onset every
    4.9 samples until `window` onsets are live in that round, silence to the round's end, and dense onsets again behind it"""
    n = 5 * ROUND + 700
    f0 = np.full(n, 9001.7, dtype=F32)
    head = F32(sr * 0.99995 / 100)
    f0[:100] = head                                           # phase 0.99995 in front of sample 100 ...
    f0[100] = 5.0                                             # ... which crosses 1 on an f0 of 5 Hz: T0 = clip(8820) = 8192
    oi, _, T0, _ = P.onsets(f0, sr)
    assert oi[0] == 100 and T0[0] == 8192 and oi.size > window and oi[window] < 5 * ROUND
    f0[oi[window - 1] + 1:5 * ROUND + 60] = 0.0               # onset number `window` and those behind it wait for the next round
    return f0


def test_ring_at_its_limit(ctx):
    sr = 44100
    ctx.plan(sr, *GEO)
    notes = [_ring_note(w) for w in (RING - 1, RING, RING + 1)]
    assert [_window(f, sr) for f in notes] == [RING - 1, RING, RING + 1]
    assert all(P.scan_verdict(f, sr) == "scan" for f in notes)  # none is walked: list mode can only come from the ring
    chain = _run(ctx, notes, 1, 0)
    for k, f in enumerate(notes):
        assert np.array_equal(chain["lists"][k], P.onsets(f, sr)[0]), k
    for k, f in enumerate(notes):
        alone = _run(ctx, [f], 1, 1)
        print("MEASURED ring window %d: %d notes in list mode, %d walked" % (RING - 1 + k, alone["pulse_list_notes"], alone["pulse_fallback_notes"]))
        assert alone["pulse_fallback_notes"] == 0
        assert (alone["pulse_list_notes"] == 0) if k < 2 else (alone["pulse_list_notes"] >= 1), (k, alone["pulse_list_notes"])
        o = sum(len(x) for x in notes[:k])
        assert np.array_equal(P.bits(alone["pulse"]), P.bits(chain["pulse"][o:o + len(f)])), k
        assert np.array_equal(alone["lists"][0], chain["lists"][k]), k
    _assert_same(_run(ctx, notes, 1, 1), chain, "ring batch")


# ---------------------------------------------------------------------------------------------
# round and alignment edges
# ---------------------------------------------------------------------------------------------
def _voiced(n, f=233.7):
    return np.full(n, f, dtype=F32)


def _head(n):
    f = _voiced(n, 311.3)
    f[:int(0.3 * n)] = 0.0
    return f


def _gaps(n, sr=44100):
    f = _voiced(n, 523.9)
    g = int(0.05 * sr)
    for s in range(g, n, 3 * g):
        f[s:s + g] = 0.0
    return f


def _glide(n):
    return (80.0 * (900.0 / 80.0) ** (np.arange(n) / max(n - 1, 1))).astype(F32)


def _subthreshold_gap(sr=44100):
    """100 voiced samples that leave the phase less than 6.9e-8 (one ulp of the f0) under 1, then 100 ms of f0 = 1e-6 (2.3e-11 of
    phase per sample: 1e-7 in all), then voiced again: the first onset falls in the gap, on a sample whose own f0 is not > 1e-6"""
    f = F32(F64(sr) / 100)
    while np.cumsum(np.full(100, f, dtype=F32).astype(F64) / F64(sr))[-1] >= 1.0:
        f = np.nextafter(f, F32(0))
    g = int(0.1 * sr)
    f0 = np.concatenate([np.full(100, f, dtype=F32), np.full(g, 1e-6, dtype=F32), np.full(3000, 402.3, dtype=F32)])
    oi = P.onsets(f0, sr)[0]
    assert 100 <= oi[0] < 100 + g and not f0[oi[0]] > F32(1e-6)
    return f0


def _edge_notes(sr=44100):
    tiny = lambda n: _voiced(n, 9001.7)                        # (an onset on sample 4)
    ragged = [tiny(1), tiny(3), tiny(5),                      # 9 samples in front: what follows starts off the 16-byte grid
              tiny(1), tiny(7), tiny(8), _voiced(2047), np.zeros(0, dtype=F32), _head(2048), _gaps(2049), _glide(4096), _voiced(4097, 1234.5)]
    neg = _voiced(5000, 180.3)
    neg[2100] = -50.0
    nan = _voiced(5000, 191.9)
    nan[2500] = np.nan
    dense = _voiced(3 * ROUND + 100, 11000.3)                 # covering lists of some 615 onsets, from the ring (pulse_ref's (d) is walked)
    long = [_voiced(6500), _head(7000), _gaps(9000), _glide(20000), dense, _subthreshold_gap(sr), _voiced(6300, 441.0), neg, nan]
    names = (["n%d" % len(f) for f in ragged]
             + ["voiced", "unvoiced_head", "gaps", "glide", "dense", "subthreshold_gap", "441Hz", "negative", "nan"])
    return names, ragged + long


def test_round_and_alignment_edges(ctx):
    sr = 44100
    ctx.plan(sr, *GEO)
    names, notes = _edge_notes(sr)
    walked = {"441Hz", "negative", "nan"}
    assert P.scan_verdict(notes[names.index("441Hz")], sr) != "scan"   # every hundredth sample lies 1e-16 from an integer: inside any band
    assert all(P.scan_verdict(f, sr) == "scan" for nm, f in zip(names, notes) if nm not in walked | {"subthreshold_gap"})
    fused, chain = _run(ctx, notes, 1, 1), _run(ctx, notes, 1, 0)
    _assert_same(fused, chain, "edges")
    assert fused["pulse_scanned_notes"] == len(notes)
    extra = 0 if P.scan_verdict(notes[names.index("subthreshold_gap")], sr) == "scan" else 1
    assert len(walked) <= fused["pulse_fallback_notes"] <= len(walked) + extra
    assert fused["pulse_list_notes"] == fused["pulse_fallback_notes"]
    for k, (nm, f) in enumerate(zip(names, notes)):            # the restatement's onsets, wherever it has an opinion
        if nm not in ("negative", "nan"):
            assert np.array_equal(fused["lists"][k], P.onsets(f, sr)[0]), nm
    off = np.concatenate([[0], np.cumsum([len(f) for f in notes])])
    for k, (nm, f) in enumerate(zip(names, notes)):
        if len(f) == 0:
            continue
        alone = _run(ctx, [f], 1, 1)
        assert np.array_equal(P.bits(alone["pulse"]), P.bits(fused["pulse"][off[k]:off[k + 1]])), (nm, "alone against the batch")
        assert np.array_equal(alone["lists"][0], fused["lists"][k]), nm
        assert alone["pulse_fallback_notes"] == (1 if nm in walked else alone["pulse_list_notes"]), nm
    # forced walks: every note through list mode
    _assert_same(_run(ctx, notes, 2, 1), _run(ctx, notes, 2, 0), "edges, pulse_scan 2")


# ---------------------------------------------------------------------------------------------
# through the batch driver
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", (3, 4))
def test_batch_driver_fused_equals_chain(config):
    from goofer_amd.device import Context
    from goofer_amd.workload import SamplerWorkload
    c = Context(0)
    try:
        wl = SamplerWorkload(c, config, list(range(8)))
        got = {}
        for fused in (1, 0):
            c.set_option("pulse_fused", fused)
            l0 = c.counter("pulse_list_notes")
            mix = wl.step()["mix"]
            torch.cuda.synchronize()
            c.check()
            got[fused] = (mix.cpu().numpy().copy(), c.debug_fetch("pulse").copy(), c.debug_fetch("onset_cnt").copy(), c.counter("pulse_list_notes") - l0)
        assert got[1][0].size == wl.samples and np.abs(got[1][1]).max() > 0
        assert np.array_equal(P.bits(got[1][1]), P.bits(got[0][1])), "pulse view"
        assert np.array_equal(got[1][2], got[0][2]), "onset_cnt"
        assert np.array_equal(P.bits(got[1][0]), P.bits(got[0][0])), "mix"
        assert got[0][3] == 0
        print("MEASURED batch driver config %d: 8 notes, %d samples, %d in list mode" % (config, wl.samples, got[1][3]))
    except RuntimeError as e:
        _stop(e)
    finally:
        c.close()
