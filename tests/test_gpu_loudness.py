"""GPU: loudness metering and normalisation (goofer_loudness_measure / _apply, csrc/loudness.hip) against the numpy restatement
(tests/loudness_ref.py), on the library's own tables.

The bound for the segment energies is the definition's: |E_gpu[k] - E_ld[k]| <= 2^-26 max_k E_ld[k] per signal, E_ld by the
long-double flavour of the restatement — an error e in the gated energy moves the gain by e / 2, so this keeps the fp32 gain
within one ulp.  tests/test_loudness_plan.py shows that the float64 flavour leaves that bound unspent on these very inputs and
that wrong variants (an fp32 state, a state lost at a tile boundary, a counted trailing segment, misplaced gates, history from
the neighbour) break it.  Measured on an MI355X: worst |E_gpu - E_ld| / max E = 2.9e-11 (96 kHz), 5.9e-12 at 48 kHz,
3.2e-12 at 44.1 kHz, 1.0e-13 at 8 kHz: 500 times inside the bound.

The kernels cut a signal into tiles of 4096 samples and carry the filter state across them, and sum v^2 per segment of
S = sr / 10 samples; so the rates put several segments into a tile (8 kHz), a segment over two tiles (44.1 and 48 kHz) and over
three (96 kHz), and the lengths sit around a segment, a block of four segments and the tile.  The state goes from tile to
tile in runs of 16 tiles per thread and rounds of 4096 tiles: one signal at 8 kHz is over 16 tiles, one over 4096.  The lengths do not fit one batch
of 100 000 samples from 44.1 kHz on: loudness_ref.batch cuts them into several."""
import numpy as np
import pytest

import loudness_ref as R
from goofer_amd import loudness as LD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BATCHES = [(sr, b) for sr in R.RATES for b in range(len(R.batch(sr)))]
TARGET, CAP = -23.0, 60.0           # (a cap that no signal of the batches reaches)


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _run(ctx, xs, sr, target=None, max_gain_db=LD.MAX_GAIN_DB, in_place=False):
    """the kernels on the signals xs: (ys or None, loud [n, 2], gain [n], list of E) on the host"""
    plan = LD.plan(sr, [len(x) for x in xs])
    x = ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))[:plan.total]     # (never an empty tensor)
    y, loud, gain, seg = ctx.loudness(x, None, plan, target, max_gain_db, out=x if in_place else None)
    torch.cuda.synchronize()
    assert (y is None) == (target is None) and (not in_place or y is x)
    seg = seg.cpu().numpy()
    if y is not None:
        y = y.cpu().numpy()
        y = [y[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)]
    return y, loud.cpu().numpy(), gain.cpu().numpy(), [seg[plan.seg_off[i]:plan.seg_off[i + 1]] for i in range(plan.n)]


_cache = {}


def _batch(ctx, sr, b):
    """the batch measured and normalised to TARGET, once per module"""
    if (sr, b) not in _cache:
        _cache[(sr, b)] = _run(ctx, R.batch(sr)[b], sr, TARGET, CAP)
    return _cache[(sr, b)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(R.words(a), R.words(b))


def _ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(R.words(np.array([a]))[0]) - int(R.words(np.array([b]))[0]))


@pytest.mark.parametrize("sr,b", BATCHES)
def test_segment_energies_loudness_and_gain_against_the_restatement(ctx, sr, b):
    xs, S = R.batch(sr)[b], R.seg_len(sr)
    ys, loud, gain, Es = _batch(ctx, sr, b)
    assert loud.dtype == np.float64 and loud.shape == (len(xs), 2) and gain.dtype == np.float32 and gain.shape == (len(xs),)
    worst = 0.0
    for i, x in enumerate(xs):
        E_ld, L, mm = R.reference((sr, b, i))
        E = Es[i]
        assert E.dtype == np.float64 and len(E) == len(x) // S == len(E_ld), i
        if len(E):
            top = float(np.abs(E_ld).max())
            err = float(np.abs(E.astype(np.longdouble) - E_ld).max())
            if top > 0:
                worst = max(worst, err / top)
            assert err <= R.TOL * top, (i, len(x), err / top if top else err)
        want_g = R.stats(E_ld, S, TARGET, CAP)[2]
        if len(E) < 4:                                                     # no block
            assert loud[i, 0] == -np.inf and loud[i, 1] == -np.inf and gain[i] == 1.0, (i, loud[i], gain[i])
        elif not np.any(x):                                                # the all-zero signal
            assert np.all(R.words(E) == 0) and loud[i, 0] == -np.inf and loud[i, 1] == -np.inf and gain[i] == 1.0, i
        else:
            assert abs(loud[i, 0] - L) <= 1e-6 and abs(loud[i, 1] - mm) <= 1e-6, (i, loud[i], L, mm)
            assert 0.0 < gain[i] < np.float32(10.0 ** (CAP / 20.0)) and _ulp_apart(gain[i], want_g) <= 1, (i, gain[i], want_g)
    print(sr, b, "worst |E_gpu - E_ld| / max E = %.3e (bound %.3e)" % (worst, R.TOL))
    if b == R.trio(sr)[0]:
        i = R.trio(sr)[1]
        assert len(xs[i]) > 4 * R.TILE and len(Es[i]) >= 5 and np.isfinite(loud[i, 0])           # the signal over four tiles
        assert len(Es[i + 2]) >= 2 and np.all(R.words(Es[i + 2]) == 0)                             # the all-zero signal, exactly 0.0
        assert max(float(e.max()) for e in Es if len(e)) == float(Es[i + 1].max())               # ... directly behind the loudest


@pytest.mark.parametrize("sr,b", BATCHES)
def test_output_is_the_fp32_product_and_remeasures_at_the_target(ctx, sr, b):
    xs = R.batch(sr)[b]
    ys, loud, gain, Es = _batch(ctx, sr, b)
    for i, x in enumerate(xs):
        assert ys[i].dtype == np.float32 and _same(ys[i], x * gain[i]), i
    ys2, loud2, gain2, Es2 = _run(ctx, xs, sr, TARGET, CAP, in_place=True)                  # out == x
    assert _same(loud2, loud) and _same(gain2, gain)
    for i in range(len(xs)):
        assert _same(ys2[i], ys[i]) and _same(Es2[i], Es[i]), i
    _, again, _, _ = _run(ctx, ys, sr)
    for i in range(len(xs)):
        if np.isfinite(loud[i, 0]):
            assert abs(again[i, 0] - TARGET) <= 1e-4, (i, again[i, 0], loud[i, 0], gain[i])
        else:
            assert again[i, 0] == -np.inf and gain[i] == 1.0, i


@pytest.mark.parametrize("sr,b", BATCHES)
def test_measure_only_alone_and_twice(ctx, sr, b):
    """Measuring only gives the same statistics, gain 1 and no y; every signal alone gives the words it has inside the batch; a
    second run gives the same words."""
    xs = R.batch(sr)[b]
    ys, loud, gain, Es = _batch(ctx, sr, b)
    y0, loud0, gain0, Es0 = _run(ctx, xs, sr)
    assert y0 is None and _same(loud0, loud) and np.all(gain0 == 1.0) and all(_same(a, c) for a, c in zip(Es0, Es))
    _, loud1, gain1, Es1 = _run(ctx, xs, sr, TARGET, CAP)
    assert _same(loud1, loud) and _same(gain1, gain) and all(_same(a, c) for a, c in zip(Es1, Es))
    for i, x in enumerate(xs):
        _, la, ga, Ea = _run(ctx, [x], sr, TARGET, CAP)
        assert _same(la[0], loud[i]) and _same(ga, gain[i:i + 1]) and _same(Ea[0], Es[i]), (i, len(x))


def test_the_state_crosses_from_one_run_of_tiles_to_the_next(ctx):
    """k_loud_carry gives a thread 16 consecutive tiles and scans the threads: only a signal over 16 tiles has a state that the
    scan carries.  The batch tests above hold this signal to the restatement, alone and in its batch; here: that it is what
    they take it for, and the segments on either side of the boundary by themselves."""
    sr, b, i = R.runs_signal()
    x, S = R.batch(sr)[b][i], R.seg_len(sr)
    assert i > 0 and R.RUN_TILES * R.TILE < len(x) <= 100000 - len(R.batch(sr)[b][i - 1])
    E_ld = R.reference((sr, b, i))[0]
    E = _batch(ctx, sr, b)[3][i]
    k = R.RUN_TILES * R.TILE // S
    err = np.abs(E.astype(np.longdouble) - E_ld)[k - 2:k + 6]
    print("segments %d .. %d around sample %d: worst error / max E = %.3e" % (k - 2, k + 5, R.RUN_TILES * R.TILE, float(err.max() / E_ld.max())))
    assert np.all(err <= R.TOL * E_ld.max())


def test_a_signal_over_4096_tiles(ctx):
    """k_loud_carry takes 4096 tiles a round and carries the state into the next round.  16.9 M samples are too many for the
    restatement, which is started from zero ten segments ahead of each window instead (loudness_ref.window_energy): the
    signal's start, the round boundary (a DC step 300 samples in front of it), and the end, where the second round's thread 0
    hands over to its thread 1 (tests/test_loudness_plan.py: a state lost at the round boundary breaks the bound on the second
    window).  The bound is taken from each window's own largest segment, which is not above the signal's."""
    sr, x = R.long_signal()
    S = R.seg_len(sr)
    n_tiles = -(-len(x) // R.TILE)
    assert n_tiles > 4096 + R.RUN_TILES
    _, loud, gain, (E,) = _run(ctx, [x], sr)
    kn = len(x) // S
    assert len(E) == kn and np.isfinite(loud).all() and gain[0] == 1.0
    kr, kt = 4096 * R.TILE // S, (4096 + R.RUN_TILES) * R.TILE // S
    for k0, k1 in ((0, 12), (kr - 4, kr + 12), (kt - 4, kn)):
        want = R.window_energy(x, sr, k0, k1)
        err = np.abs(E[k0:k1].astype(np.longdouble) - want)
        print("segments %d .. %d: worst error / max E of the window = %.3e" % (k0, k1 - 1, float(err.max() / want.max())))
        assert len(want) == k1 - k0 and np.all(err <= R.TOL * want.max()), (k0, k1)
    _, loud2, _, (E2,) = _run(ctx, [x], sr)
    assert _same(E2, E) and _same(loud2, loud)


@pytest.mark.parametrize("sr", R.RATES)
def test_a_signal_with_a_nan_and_its_neighbours(ctx, sr):
    xs, S = list(R.batch(sr)[0]), R.seg_len(sr)
    bad = R.nan_signal(sr)
    at = 4
    ys, loud, gain, Es = _batch(ctx, sr, 0)
    ysn, loudn, gainn, Esn = _run(ctx, xs[:at] + [bad] + xs[at:], sr, TARGET, CAP)
    assert np.isnan(loudn[at]).all() and np.isnan(gainn[at]) and np.isnan(ysn[at]).all()
    E_ld = R.reference(("nan", sr))[0]
    first = (len(bad) // 2) // S                                           # the segment that holds the NaN
    assert len(Esn[at]) == 5 and np.isnan(Esn[at][first:]).all() and np.isnan(E_ld[first:]).all()
    good = E_ld[:first]
    assert first >= 1 and np.all(np.abs(Esn[at][:first].astype(np.longdouble) - good) <= R.TOL * np.abs(good).max())
    keep = [k for k in range(len(xs) + 1) if k != at]
    assert _same(loudn[keep], loud) and _same(gainn[keep], gain)
    for k, i in enumerate(keep):
        assert _same(Esn[i], Es[k]) and _same(ysn[i], ys[k]), k


def test_gating_fixtures(ctx):
    sr, xs = R.gating_fixtures()
    S = R.seg_len(sr)
    _, loud, gain, Es = _run(ctx, xs, sr)
    for k in range(len(xs)):
        E_ld, L, mm = R.reference(("gate", k))
        assert np.all(np.abs(Es[k].astype(np.longdouble) - E_ld) <= R.TOL * np.abs(E_ld).max()), k
        assert abs(loud[k, 0] - L) <= 1e-6 and abs(loud[k, 1] - mm) <= 1e-6, (k, loud[k], L, mm)
        assert abs(loud[k, 0] - R.ungated(Es[k], S)) > 1.0, k
        curve = LD.momentary(Es[k], S)
        assert curve.shape == (len(Es[k]) - 3,) and abs(curve.max() - loud[k, 1]) <= 1e-9


def test_under_the_absolute_gate_and_the_cap(ctx):
    sr, x = R.under_gate_signal()
    y, loud, gain, Es = _run(ctx, [x], sr, -16.0)
    E_ld, L, mm = R.reference(("under",))
    assert loud[0, 0] == -np.inf and abs(loud[0, 1] - mm) <= 1e-6 and gain[0] == 1.0 and _same(y[0], x)
    sr, x = R.quiet_tone()
    E_ld, L, mm = R.reference(("tone",))
    assert abs(L + 60.0) < 0.5
    y, loud, gain, Es = _run(ctx, [x], sr, -16.0, 20.0)
    assert abs(loud[0, 0] - L) <= 1e-6 and R.words(gain)[0] == R.words(np.array([10.0], np.float32))[0] and _same(y[0], x * np.float32(10.0))
    y, loud, gain, Es = _run(ctx, [x], sr, -16.0, 0.0)                      # a cap of 0 dB never amplifies
    assert gain[0] == 1.0
    y, loud, gain, Es = _run(ctx, [x], sr, -16.0, 60.0)
    assert _ulp_apart(gain[0], R.stats(E_ld, R.seg_len(sr), -16.0, 60.0)[2]) <= 1 and gain[0] > 100.0


def test_refusals(ctx):
    import ctypes as C
    from goofer_amd import core
    plan = LD.plan(48000, [100, 200])
    x = torch.zeros(300, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.loudness(x, [0, 100, 301], plan)
    with pytest.raises(ValueError):
        ctx.loudness(x[:299], None, plan)
    with pytest.raises(ValueError):
        ctx.loudness(x, None, plan, out=x)                                  # out without a target
    for bad in (dict(target=float("nan")), dict(target=float("inf")), dict(target=-16.0, max_gain_db=-1.0), dict(max_gain_db=61.0)):
        with pytest.raises(ValueError):
            ctx.loudness(x, None, plan, **bad)
    y, loud, gain, seg = ctx.loudness(x, ctx.tensor(plan.in_off), plan, -16.0)
    assert y.shape == (300,) and seg.numel() == 0 and np.all(loud.cpu().numpy() == -np.inf) and gain.tolist() == [1.0, 1.0]
    y, loud, gain, seg = ctx.loudness(x, None, LD.plan(48000, [0, 0, 0]), -16.0)            # signals without a sample
    assert y.numel() == 0 and gain.tolist() == [1.0] * 3 and np.all(loud.cpu().numpy() == -np.inf)
    lib, p, size = ctx.lib, C.c_void_p(x.data_ptr()), C.c_int64(1 << 20)

    def measure(S=4800, target=-16.0, cap=20.0, n=2, total=300, n_tiles=2, scratch=p):
        return lib.goofer_loudness_measure(ctx.h, p, p, n, total, S, p, p, p, p, n_tiles, target, cap, p, p, p, scratch, C.byref(size), None)
    for bad in (dict(S=799), dict(S=19201), dict(target=float("inf")), dict(cap=-1.0), dict(cap=61.0), dict(cap=float("nan")), dict(n=-1),
                dict(total=-1), dict(n_tiles=0), dict(n_tiles=4)):
        assert measure(**bad) == -1, bad
        assert b"goofer_loudness_measure" in lib.goofer_last_error(ctx.h)
    need = C.c_int64(0)
    assert lib.goofer_loudness_measure(ctx.h, None, None, 2, 300, 4800, None, None, None, None, 2, -16.0, 20.0, None, None, None, None,
                                       C.byref(need), None) == 0 and need.value > 0           # the size query
    size = C.c_int64(need.value - 1)
    assert measure() == -1 and b"scratch" in lib.goofer_last_error(ctx.h)
    size = C.c_int64(1 << 20)
    assert lib.goofer_loudness_apply(ctx.h, p, p, 2, 300, p, C.c_void_p(x.data_ptr() + 4), None) == -1
    assert b"overlaps" in lib.goofer_last_error(ctx.h)
    assert lib.goofer_loudness_apply(ctx.h, p, p, 2, 300, None, p, None) == -1
    torch.cuda.synchronize()
    assert not x.any()                                                     # nothing was launched
    with pytest.raises(ValueError):
        core.loudness_batch([np.zeros(10)], 7999, ctx=ctx)
    with pytest.raises(ValueError):
        core.loudness_batch([np.zeros(10)], 48000, target=float("nan"), ctx=ctx)


def test_loudness_batch(ctx):
    from goofer_amd import core
    sr, b = 8000, 0
    xs = R.batch(sr)[b]
    ys, loud, gain, Es = _batch(ctx, sr, b)
    got = core.loudness_batch(xs, sr, TARGET, CAP, ctx=ctx)
    assert _same(got[1], loud) and _same(got[2], gain) and all(_same(a, c) for a, c in zip(got[0], ys)) and all(_same(a, c) for a, c in zip(got[3], Es))
    got = core.loudness_batch(xs, sr, ctx=ctx)
    assert got[0] is None and _same(got[1], loud) and np.all(got[2] == 1.0)
    assert core.loudness_batch([], sr, ctx=ctx)[0] is None and core.loudness_batch([], sr, -16.0, ctx=ctx)[0] == []


def _jobs(seconds=0.3, length="300"):
    """the four notes of examples/render_phrase.py"""
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Source
    requests = [("C4", "100", "g-10", "30", length, "80", "50", "100", "0", "!120", "AA"),
                ("E4", "100", "t30fa20fb-10B30", "30", length, "80", "50", "120", "0", "!120", "AA#20#AP"),
                ("G4", "80", "L1sg40st-30", "30", length, "80", "50", "100", "0", "!120", "AA"),
                ("A3", "120", "vf30sa20pd40", "30", length, "80", "50", "110", "0", "!120", "AA#10#BA#10#AA")]
    jobs = []
    for i, args in enumerate(requests):
        src = syn.make_source(100 + i, seconds=seconds)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
    entries = ["0 250 5 35 40 0 100 100 0 0", "10 240@120+30 5 35 40 20 100 90 10 30", "R 120",
               "0 250 5 35 40 0 110 100 0 25 10 30 80", "5 200 5 35 40 0 100 100 0 40"]
    return jobs, entries


def test_render_phrase_with_loudness_is_the_chain_done_by_hand(ctx, monkeypatch):
    from goofer_amd import limit as LM
    from goofer_amd import rate as RT
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    plain = r.render_phrase(jobs, entries, seed=5)
    conv = ctx.rate_convert(ctx.tensor(plain), None, RT.plan(44100, 48000, [len(plain)]))
    assert _same(conv.cpu().numpy(), r.render_phrase(jobs, entries, seed=5, out_sr=48000))
    n = conv.numel()
    y, loud, gain, _ = ctx.loudness(conv, None, LD.plan(48000, [n]), -16.0)
    lim, peak, gmin = ctx.limit(y, None, LM.plan(48000, [n], 0.5))
    want = ctx.pcm16(lim).cpu().numpy()
    got, st = r.render_phrase(jobs, entries, seed=5, out_sr=48000, loudness=-16, limit=0.5, return_stats=True, pcm16=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert st == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "lufs_in": float(loud.cpu()[0, 0]),
                  "momentary_max": float(loud.cpu()[0, 1]), "gain": float(gain.cpu()[0])}
    assert np.isfinite(st["lufs_in"]) and st["gain"] != 1.0 and st["peak_in"] == float(y.abs().max().cpu())
    # loudness alone: return_stats is accepted, the statistics are the loudness stage's
    got, st2 = r.render_phrase(jobs, entries, seed=5, out_sr=48000, loudness=(-16, 20.0), return_stats=True)
    assert _same(got, y.cpu().numpy()) and set(st2) == {"lufs_in", "momentary_max", "gain"} and st2["gain"] == st["gain"]
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, return_stats=True)
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, loudness=float("nan"))
    # loudness None: the bits of a call without the keyword, and Context.loudness never runs
    track48 = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    pcm_plain = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    lim_plain, st_plain = r.render_phrase(jobs, entries, seed=5, limit=0.5, return_stats=True)
    notes = r.render(jobs, seed=5)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("loudness reached")
    monkeypatch.setattr(Context, "loudness", never)
    assert _same(r.render_phrase(jobs, entries, seed=5, loudness=None), plain)
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, loudness=None), track48)
    assert np.array_equal(r.render_phrase(jobs, entries, seed=5, pcm16=True, loudness=None), pcm_plain)
    got, st3 = r.render_phrase(jobs, entries, seed=5, limit=0.5, return_stats=True, loudness=None)
    assert _same(got, lim_plain) and st3 == st_plain and set(st3) == {"peak_in", "min_gain"}
    for a, c in zip(r.render(jobs, seed=5, loudness=None), notes):
        assert _same(a, c)
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, loudness=-20)
    assert len(calls) == 1


def test_render_with_loudness_gives_loudness_batchs_gains(ctx):
    from goofer_amd import core
    from goofer_amd.render import Renderer
    jobs, _ = _jobs(seconds=0.8, length="700")
    r = Renderer(ctx)
    notes = r.render(jobs, seed=5)
    assert min(len(y) for y in notes) >= 4 * 4410
    ys, loud, gain, _ = core.loudness_batch(notes, 44100, -20.0, ctx=ctx)
    assert np.all(np.isfinite(loud[:, 0])) and np.all(gain != 1.0)
    got = r.render(jobs, seed=5, loudness=-20)
    for i, (a, c) in enumerate(zip(got, ys)):
        assert _same(a, c) and _same(a, notes[i] * gain[i]), i
    conv = r.render(jobs, seed=5, out_sr=48000)
    ys, loud, gain, _ = core.loudness_batch(conv, 48000, -20.0, 6.0, ctx=ctx)
    for a, c in zip(r.render(jobs, seed=5, out_sr=48000, loudness=(-20, 6.0)), ys):
        assert _same(a, c)


def test_job_file_front_end_with_loudness(ctx, tmp_path, capsys):
    """python -m goofer_amd.phrase --loudness -16 --rate 48000 job.txt out.wav (its main(), in process): the wav re-measures at
    -16 LUFS within 0.05 LU, the int16 rounding included, and the measured loudness and the gain are reported on stderr."""
    import wave
    from goofer_amd import core
    from goofer_amd import phrase as P
    from goofer_amd import synthetic as syn
    for i in range(2):
        src = syn.make_source(300 + i, seconds=0.3)
        core.save_features(tmp_path / f"v{i}_features.goofy", src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
    res = ["C4 100 g-10 30 300 80 50 100 0 !120 AA", "E4 100 B30 30 300 80 50 110 0 !120 AA#20#AP"]
    tool = ["0 250 5 35 40 0 100 100 0", "0 240@120 5 35 40 0 100 100 0 30"]
    job = tmp_path / "job.txt"
    job.write_text("".join(f"{tmp_path}/v{k}.wav {tmp_path}/n{k}.wav {r} | {t}\n" for k, (r, t) in enumerate(zip(res, tool))))
    out = tmp_path / "loud.wav"
    assert P.main(["--loudness", "-16", "--rate", "48000", str(job), str(out)]) == 0
    err = capsys.readouterr().err
    assert "Loudness: measured" in err and "LUFS" in err and "gain" in err
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert int(np.abs(pcm.astype(np.int32)).max()) < 32767                  # nothing was clipped on the way to int16
    L = R.measure(pcm.astype(np.float32) / np.float32(32768.0), 48000)[1]
    assert abs(L + 16.0) <= 0.05, L
    assert P.main(["--loudness", "-16", "--limit", "-1", str(job), str(out)]) == 0
    err = capsys.readouterr().err
    assert "Loudness: measured" in err and "Limiter:" in err
    assert P.main(["--loudness", "loud", str(job), str(out)]) == 1
