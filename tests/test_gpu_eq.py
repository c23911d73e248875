"""GPU: the parametric equaliser (goofer_eq, csrc/eq.hip) against the numpy restatement (tests/eq_ref.py), on the library's own
tables.

The bound is the definition's: |y[i] - t[i]| <= 2^-24 |t[i]| + TOL max |t| per signal, t the long-double flavour of the
restatement and TOL = 2^-26.  tests/test_eq_ref.py shows that a float64 model of the kernels' scheme stays within TOL / 4 on the
corners of the accepted range and on these very inputs, and that wrong variants (a state or an input history lost at a tile
boundary, an fp32 state) break the bound.  Measured on an MI355X: worst (|y - t| - 2^-24 |t|) / max |t| = 2.9e-13 (48 kHz,
eight bands) on the ordinary chains, under the fp32 rounding alone at 8 kHz and in the window of the signal over 4096 tiles;
on the worst corners of the range 2^-29.52 (96 kHz; the model: 2^-29.44), eleven times inside the bound.

The kernels cut a signal into tiles of 4096 samples and a tile into runs of 16, and carry the cascade's state across both; the
state goes from tile to tile in runs of 16 tiles per thread and rounds of 4096 tiles.  So the lengths sit around a run, around a
tile, over two tiles and over 16, and one signal at 8 kHz is over 4096 tiles.  A DC step sits 300 samples in front of a tile
boundary: the low-frequency state is large there."""
import ctypes as C
import math

import numpy as np
import pytest

import eq_ref as R
from goofer_amd import eq as EQ

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = R.TILE


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _run(ctx, xs, sr, bands):
    """the kernels on the signals xs: a list of fp32 arrays on the host"""
    plan = EQ.plan(sr, [len(x) for x in xs], bands)
    x = ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))[:plan.total]     # (never an empty tensor)
    y = ctx.eq(x, None, plan)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == (plan.total,) and y.data_ptr() != x.data_ptr()
    y = y.cpu().numpy()
    return [y[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)]


_cache = {}


def _batch(ctx, sr, K):
    """batch(sr) through chain(sr, K), once per module"""
    if (sr, K) not in _cache:
        _cache[(sr, K)] = _run(ctx, R.batch(sr), sr, R.chain(sr, K))
    return _cache[(sr, K)]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(R.words(a), R.words(b))


@pytest.mark.parametrize("K", R.CHAINS)
@pytest.mark.parametrize("sr", R.RATES)
def test_batch_against_the_restatement(ctx, sr, K):
    xs, ys, ts = R.batch(sr), _batch(ctx, sr, K), R.reference(sr, K)
    assert [len(x) for x in xs] == [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 1, 16 * 4096 + 100, 0]
    worst = -math.inf
    for i, (x, y, t) in enumerate(zip(xs, ys, ts)):
        assert y.dtype == np.float32 and len(y) == len(x) == len(t), i
        if len(x):
            e = R.error(y, t)
            worst = max(worst, e)
            assert e <= R.TOL, (sr, K, i, len(x), e)
    print("%d Hz, K = %d: worst (|y - t| - 2^-24 |t|) / max |t| = %.3e (TOL %.3e)" % (sr, K, worst, R.TOL))


@pytest.mark.parametrize("K", [2, 4, 5, 6, 7])
def test_the_other_chain_lengths_against_the_restatement(ctx, K):
    """The tile-to-tile kernel is compiled once per K and R.CHAINS runs three of the eight: the others, on the first K bands of
    the chain of eight at 48 kHz.  The signal of 16 * 4096 + 100 samples puts 17 tiles through that kernel, one more than a
    thread walks, so the second thread's state comes through the scan."""
    sr = 48000
    xs, ys, ts = R.batch(sr), _batch(ctx, sr, K), R.reference(sr, K)
    assert K not in R.CHAINS and R.chain(sr, K) == R.chain(sr, 8)[:K] and max(len(x) for x in xs) == 16 * TILE + 100
    worst = -math.inf
    for i, (x, y, t) in enumerate(zip(xs, ys, ts)):
        assert y.dtype == np.float32 and len(y) == len(x) == len(t), i
        if len(x):
            e = R.error(y, t)
            worst = max(worst, e)
            assert e <= R.TOL, (K, i, len(x), e)
    print("48000 Hz, K = %d: worst (|y - t| - 2^-24 |t|) / max |t| = %.3e (TOL %.3e)" % (K, worst, R.TOL))


@pytest.mark.parametrize("sr", [48000, 96000])
def test_the_worst_corners_of_the_range(ctx, sr):
    """The corner run's input through the corners that do worst in the float64 model (tests/test_eq_ref.py), on the device: one
    notch and then seven peaks of the greatest gain at the lowest f0 and the highest q, two notches and six such peaks, three
    high-passes and five low shelves.  This ties the model, which fixed the range with a factor of 4 for the kernel's other sum
    order, to the kernel."""
    x = R.hazard_input(sr)
    cs = R.corners(sr)
    for i, kinds in ((50, ["notch"] + ["peak"] * 7), (44, ["notch"] * 2 + ["peak"] * 6), (55, ["highpass"] * 3 + ["lowshelf"] * 5)):
        bands = cs[i]
        assert [b[0] for b in bands] == kinds and bands[7][2] == R.MAX_GAIN_DB and all(b[1] * R.F_MIN_DIV >= sr for b in bands)
        y = _run(ctx, [x], sr, bands)[0]
        e = R.error(y, R.cascade(x, R.cascade_coefficients(bands, sr)))
        print("%d Hz, corner %d (%s): %.3e = 2^%.2f (TOL 2^-26)" % (sr, i, " ".join(k[:2] for k in kinds), e, math.log2(max(e, 1e-300))))
        assert e <= R.TOL


@pytest.mark.parametrize("sr", R.RATES)
def test_a_signal_alone_and_a_second_run_give_the_same_bits(ctx, sr):
    xs, K = R.batch(sr), 3
    ys = _batch(ctx, sr, K)
    again = _run(ctx, xs, sr, R.chain(sr, K))
    for i, x in enumerate(xs):
        assert _same(again[i], ys[i]), i
        if len(x):
            assert _same(_run(ctx, [x], sr, R.chain(sr, K))[0], ys[i]), i
    # ... and at another position, behind other neighbours, with eight bands
    ys8 = _batch(ctx, sr, 8)
    order = [10, 0, 9, 3, 8, 7]
    got = _run(ctx, [xs[i] for i in order], sr, R.chain(sr, 8))
    for j, i in enumerate(order):
        assert _same(got[j], ys8[i]), i


def test_a_signal_over_4096_tiles(ctx):
    """The state crosses from one round of the tile-to-tile kernel to the next.  The signal is too long for the restatement as a
    whole: a window around tile 4096 is restated from zero, so far ahead that what is left of the true state there is under
    1e-100 of it — the distance comes from the pole radii and is checked on the power of the transition matrix."""
    import loudness_ref
    sr, x = loudness_ref.long_signal()
    assert sr == 8000 and len(x) > (4096 + 20) * TILE
    bands = [("highpass", 200.0, 0.0, R.Q_DEFAULT), ("peak", 1000.0, 6.0, 1.0)]
    coef = R.cascade_coefficients(bands, sr)
    r = R.pole_radius(coef)
    assert 0.5 < r < 0.95
    m = int(math.ceil(-110.0 * math.log(10.0) / math.log(r)))
    assert np.abs(np.linalg.matrix_power(np.array(R.transition(coef)), m)).max() <= 1e-100 and m < 4 * TILE
    at = 4096 * TILE
    a, b = at - TILE // 2, at + 2 * TILE                                 # compared: half a tile in front of the boundary, two behind
    y = _run(ctx, [x], sr, bands)[0]
    t = R.cascade(x[a - m:b], coef)[m:]
    e = R.error(y[a:b], t)
    print("window around tile 4096: %.3e (TOL %.3e), %d samples of run-in" % (e, R.TOL, m))
    assert e <= R.TOL
    lost = np.concatenate([R.cascade(x[a - m:at], coef)[m:], R.cascade(x[at:b], coef)]).astype(np.float32)
    assert R.error(lost, t) > R.TOL                                      # (the state lost at that boundary would show)
    assert np.all(np.isfinite(y))


def test_no_band_and_zero_gain_bands_copy_the_input(ctx):
    sr = 48000
    xs = R.batch(sr)
    for bands in ([], [("peak", 1000.0, 0.0, 2.0), ("lowshelf", 200.0, 0.0), ("highshelf", 9000.0, 0.0, 1.0)]):
        assert EQ.plan(sr, [1], bands).K == 0
        for x, y in zip(xs, _run(ctx, xs, sr, bands)):
            assert _same(x, y)
    odd = np.array([0.0, -0.0, 1e-45, -1e-40, 3.4e38, -1.0, np.inf, -np.inf], dtype=np.float32)      # denormals and signed zeros too
    assert _same(_run(ctx, [odd], sr, [])[0], odd)


def test_a_nan_stays_in_its_own_signal(ctx):
    sr, K = 48000, 3
    xs = [x.copy() for x in R.batch(sr)]
    ys = _batch(ctx, sr, K)
    for i, at in ((9, TILE + 7), (10, 5 * TILE - 1), (6, 0)):
        bad = [x.copy() for x in xs]
        bad[i][at] = np.nan
        got = _run(ctx, bad, sr, R.chain(sr, K))
        assert np.all(np.isfinite(got[i][:at])) and _same(got[i][:at], ys[i][:at]) and np.all(np.isnan(got[i][at:])), (i, at)
        for j in range(len(xs)):
            if j != i:
                assert _same(got[j], ys[j]), (i, j)


def test_a_sine_at_the_centre_of_a_bell_has_the_responses_amplitude(ctx):
    sr, f, n = 48000, 1000.0, 48000
    w = 2.0 * np.pi * f / sr * np.arange(n)
    x = (0.5 * np.sin(w)).astype(np.float32)
    y = _run(ctx, [x], sr, "peak:1000:6:2")[0].astype(np.float64)
    q = n - n // 4                                                       # the last quarter: 250 whole periods
    amp = 2.0 / (n - q) * abs(np.sum(y[q:] * np.exp(-1j * w[q:])))
    want = 0.5 * abs(complex(EQ.response("peak:1000:6:2", sr, f)))
    assert abs(want / 0.5 - 10.0 ** (6.0 / 20.0)) <= 1e-9 and abs(amp - want) <= 1e-4 * want, (amp, want)


def test_refusals(ctx):
    from goofer_amd import core
    from goofer_amd.device import GooferError
    sr = 48000
    plan = EQ.plan(sr, [100, 5000], "hp:100,peak:1000:3:1")
    x = ctx.tensor(np.zeros(5200, np.float32))
    for bad in (dict(x=x[:5099]), dict(x=x.double()), dict(x=x[::2]), dict(out=x[:5000]), dict(out=torch.zeros(5100, dtype=torch.float64, device=x.device)),
                dict(d_off=[0, 100, 5099]), dict(d_off=ctx.tensor(plan.in_off)[:2]), dict(d_off=ctx.tensor(plan.in_off).int())):
        args = dict(x=x, d_off=None, out=None)
        args.update(bad)
        with pytest.raises(ValueError):
            ctx.eq(args["x"], args["d_off"], plan, out=args["out"])
    with pytest.raises(GooferError, match="overlaps"):
        ctx.eq(x, None, plan, out=x[:5100])                                 # in place: the library's to refuse
    with pytest.raises(GooferError, match="overlaps"):
        ctx.eq(x, None, plan, out=x[50:5150])
    y = ctx.eq(x, ctx.tensor(plan.in_off), plan, out=torch.ones(5100, dtype=torch.float32, device=x.device))
    assert y.shape == (5100,) and not y.any()
    assert ctx.eq(x, None, EQ.plan(sr, [0, 0, 0], "hp:100")).numel() == 0   # signals without a sample
    assert ctx.eq(x, None, EQ.plan(sr, [], "hp:100")).numel() == 0
    lib, size = ctx.lib, C.c_int64(1 << 20)
    big = ctx.tensor(np.zeros(1 << 18, np.float32))                        # x at 0, out at 64 KiB, tables and scratch behind
    p = C.c_void_p(big.data_ptr())
    o, tb, sc = (C.c_void_p(big.data_ptr() + k * 65536) for k in (1, 2, 3))

    def eq(n=2, total=5100, K=2, n_tiles=3, xp=p, off=tb, coef=tb, mats=tb, tiles=tb, out=o, scratch=sc):
        return lib.goofer_eq(ctx.h, xp, off, n, total, K, coef, mats, tiles, n_tiles, out, scratch, C.byref(size), None)
    plus = lambda q, k: C.c_void_p(q.value + k)
    for bad in (dict(n=-1), dict(total=-1), dict(n_tiles=-1), dict(n_tiles=1), dict(n_tiles=6), dict(K=-1), dict(K=9),
                dict(xp=None), dict(off=None), dict(coef=None), dict(mats=None), dict(tiles=None), dict(out=None),
                dict(xp=plus(p, 2)), dict(out=plus(o, 2)), dict(tiles=plus(tb, 2)), dict(off=plus(tb, 4)), dict(coef=plus(tb, 4)),
                dict(mats=plus(tb, 4)), dict(scratch=plus(sc, 4)),
                dict(out=p), dict(out=plus(p, 4)), dict(out=plus(p, 4 * 5099)), dict(xp=plus(o, 4 * 5099))):
        assert eq(**bad) == -1, bad
        assert b"goofer_eq" in lib.goofer_last_error(ctx.h)
    assert eq(out=plus(p, 4)) == -1 and b"overlaps" in lib.goofer_last_error(ctx.h)
    need = C.c_int64(0)
    assert lib.goofer_eq(ctx.h, None, None, 2, 5100, 2, None, None, None, 3, None, None, C.byref(need), None) == 0 and need.value > 0
    assert lib.goofer_eq(ctx.h, p, tb, 2, 5100, 2, tb, tb, tb, 3, o, sc, None, None) == -1                 # no scratch_bytes
    size = C.c_int64(need.value - 1)
    assert eq() == -1 and b"scratch" in lib.goofer_last_error(ctx.h)
    size = C.c_int64(1 << 20)
    assert eq(n=0, total=0, n_tiles=0, xp=None, off=None, coef=None, mats=None, tiles=None, out=None) == 0   # nothing to do: nothing launched
    assert eq(total=0, n_tiles=0, xp=None, tiles=None, out=None) == 0
    torch.cuda.synchronize()
    assert not big.any()                                                   # nothing was launched
    for bad_sr, bands in ((7999, "hp:100"), (48000, "hp:79"), (48000, "hp:100:3"), (48000, "peak:1000:25"), (48000, "bell:1000:3")):
        with pytest.raises(ValueError):
            core.eq_batch([np.zeros(10)], bad_sr, bands, ctx=ctx)


def test_eq_batch(ctx):
    from goofer_amd import core
    sr, K = 8000, 8
    xs, ys = R.batch(sr), _batch(ctx, sr, K)
    got = core.eq_batch(xs, sr, R.chain(sr, K), ctx=ctx)
    assert len(got) == len(xs) and all(_same(a, c) for a, c in zip(got, ys))
    got = core.eq_batch([x.astype(np.float64) for x in xs[:9]], sr, [EQ.Band(*b) for b in R.chain(sr, 3)], ctx=ctx)
    assert all(_same(a, c) for a, c in zip(got, _run(ctx, xs[:9], sr, R.chain(sr, 3))))
    assert core.eq_batch([], sr, "hp:100", ctx=ctx) == []
    assert [len(y) for y in core.eq_batch([np.zeros(0), np.zeros(0)], sr, "hp:100", ctx=ctx)] == [0, 0]


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


SPEC = "hp:80,peak:3000:3:1,hs:10000:4"


def test_render_phrase_with_eq_is_the_chain_done_by_hand(ctx, monkeypatch):
    from goofer_amd import compress as CP
    from goofer_amd import limit as LM
    from goofer_amd import loudness as LD
    from goofer_amd import rate as RT
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    plain = r.render_phrase(jobs, entries, seed=5)
    # mix, convert, eq, compress, loudness, limit, int16
    conv = ctx.rate_convert(ctx.tensor(plain), None, RT.plan(44100, 48000, [len(plain)]))
    n = conv.numel()
    flt = ctx.eq(conv, None, EQ.plan(48000, [n], SPEC))
    cmp_, red, _ = ctx.compress(flt, None, CP.plan(48000, [n], "-30:4"))
    y, loud, gain, _ = ctx.loudness(cmp_, None, LD.plan(48000, [n]), -16.0)
    lim, peak, gmin = ctx.limit(y, None, LM.plan(48000, [n], 0.5))
    want = ctx.pcm16(lim).cpu().numpy()
    got, st = r.render_phrase(jobs, entries, seed=5, out_sr=48000, eq=SPEC, compress="-30:4", loudness=-16, limit=0.5, return_stats=True,
                              pcm16=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert st == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "lufs_in": float(loud.cpu()[0, 0]),
                  "momentary_max": float(loud.cpu()[0, 1]), "gain": float(gain.cpu()[0]), "max_reduction_db": float(red.cpu()[0])}
    # eq alone, at the notes' own rate; bands, tuples and the string are one setting
    alone = ctx.eq(ctx.tensor(plain), None, EQ.plan(44100, [len(plain)], SPEC)).cpu().numpy()
    assert not _same(alone, plain)
    assert _same(r.render_phrase(jobs, entries, seed=5, eq=SPEC), alone)
    assert _same(r.render_phrase(jobs, entries, seed=5, eq=EQ.parse(SPEC)), alone)
    assert _same(r.render_phrase(jobs, entries, seed=5, eq=[("hp", 80), ("peak", 3000, 3, 1), ("hs", 10000, 4)]), alone)
    assert _same(r.render_phrase(jobs, entries, seed=5, eq="peak:1000:0"), plain)           # the identity: the track's bits
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, eq=SPEC, return_stats=True)                   # the stage has no statistic
    for bad in ("hp:20", "bell:100", "hp:80:3", [("hp", float("nan"))]):
        with pytest.raises(ValueError):
            r.render_phrase(jobs, entries, seed=5, eq=bad)
        with pytest.raises(ValueError):
            r.render(jobs, seed=5, eq=bad)
    # render: every note through the same bands, the batch in one pass
    notes = r.render(jobs, seed=5)
    from goofer_amd import core
    for a, c in zip(r.render(jobs, seed=5, eq=SPEC), core.eq_batch(notes, 44100, SPEC, ctx=ctx)):
        assert _same(a, c)
    # eq None: the bits of a call without the keyword, and Context.eq never runs
    track48 = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    pcm_plain = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    full, st_full = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress="-30:4", loudness=-16, limit=0.5, return_stats=True)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("eq reached")
    monkeypatch.setattr(Context, "eq", never)
    assert _same(r.render_phrase(jobs, entries, seed=5, eq=None), plain)
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, eq=None), track48)
    assert np.array_equal(r.render_phrase(jobs, entries, seed=5, pcm16=True, eq=None), pcm_plain)
    got, st2 = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress="-30:4", loudness=-16, limit=0.5, return_stats=True, eq=None)
    assert _same(got, full) and st2 == st_full
    for a, c in zip(r.render(jobs, seed=5, eq=None), notes):
        assert _same(a, c)
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, eq=SPEC)
    assert len(calls) == 1


def test_job_file_front_end_with_eq(ctx, tmp_path, capsys, monkeypatch):
    """python -m goofer_amd.phrase --eq hp:80,peak:3000:3:1 job.txt out.wav (its main(), in process; the seed it would draw
    pinned): the wav is render_phrase(eq=...)'s int16 track; a malformed SPEC is the usage error."""
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
    render_job = P.render_job
    monkeypatch.setattr(P, "render_job", lambda *a, **k: render_job(*a, seed=11, **k))
    spec = "hp:80,peak:3000:3:1"
    out = tmp_path / "eq.wav"
    assert P.main(["--eq", spec, str(job), str(out)]) == 0
    err = capsys.readouterr().err
    assert "Equaliser: highpass 80 Hz" in err and "peak 3000 Hz +3 dB" in err
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 44100)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    want = render_job(str(job), str(tmp_path / "want.wav"), seed=11, eq=EQ.parse(spec))
    plain = render_job(str(job), str(tmp_path / "plain.wav"), seed=11)
    assert want.dtype == np.int16 and np.array_equal(pcm, want) and not np.array_equal(pcm, plain)
    assert P.main(["--rate", "48000", "--eq", spec + ",hs:10000:4", "--limit", "-1", str(job), str(out)]) == 0
    capsys.readouterr()
    for bad in ("hp", "hp:80:0:1:2", "bell:100", "hp:eighty", "peak:1000:30"):
        assert P.main(["--eq", bad, str(job), str(out)]) == 1
