"""GPU: the dynamic range compressor (goofer_compress, csrc/compress.hip) against the numpy restatement (tests/compress_ref.py),
on the library's own tables.

The bounds are the definition's, derived and not measured: |yl_gpu - yl_ref| <= 2^-22 dB per sample, which keeps the gain within
2^-25, and with the one fp32 rounding |y_gpu - y_ref| <= 2^-23 |y_ref| + 2^-149, y_ref the restatement's unrounded float64
product.  tests/test_compress_plan.py shows that the float64 restatement is within 2^-40 dB of the long-double one on these very
inputs and that wrong variants (an fp32 state, a state lost at a tile boundary, a state inherited from the neighbour, a hard
knee for a soft one, attack and release swapped, the floor applied after the logarithm) break the bounds on them.  Measured on
an MI355X: worst |yl_gpu - yl_ref| 1.0e-13 dB over the sixteen batches (44.1 kHz, the slow set) and 7.5e-14 dB on the signal of
4116 tiles, against the bound of 2.4e-7 dB; worst output error 0.4999 of its bound, which is the fp32 rounding itself.

The kernels cut a signal into tiles of 4096 samples and a tile into runs of 16, carry the two detector states across the tiles
in runs of 16 tiles per thread and rounds of GOOFER_COMPRESS_ROUND_TILES tiles: the lengths sit around a run and a tile, one
signal is over 16 tiles and one over a round.  Each rate's ten signals make one batch of 86 k samples."""
import ctypes as C
import math

import numpy as np
import pytest

import compress_ref as R
from goofer_amd import compress as CP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(sr, name) for sr in R.RATES for name in R.SETS]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _settings(name):
    return CP.Compressor(*R.SETS[name]) if isinstance(name, str) else name


def _run(ctx, xs, sr, name, in_place=False, curve=True):
    """the kernels on the signals xs: (ys, max_reduction [n], yls or None) on the host"""
    plan = CP.plan(sr, [len(x) for x in xs], _settings(name))
    x = ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))[:plan.total]     # (never an empty tensor)
    y, red, yl = ctx.compress(x, None, plan, out=x if in_place else None, curve=curve)
    torch.cuda.synchronize()
    assert (not in_place or y is x) and (yl is None) == (not curve)
    y, red = y.cpu().numpy(), red.cpu().numpy()
    cut = lambda v: [v[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)]        # noqa: E731
    return cut(y), red, cut(yl.cpu().numpy()) if curve else None


_cache = {}


def _batch(ctx, sr, name):
    """the rate's batch under SETS[name], once per module"""
    if (sr, name) not in _cache:
        _cache[(sr, name)] = _run(ctx, R.batch(sr), sr, name)
    return _cache[(sr, name)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.words(a), R.words(b))


def _check(x, y, yl, red, want_yl, makeup, who):
    """one signal against a reference curve: the two bounds of the definition and the statistic; the worst ratios"""
    assert y.dtype == np.float32 and yl.dtype == np.float64 and len(y) == len(yl) == len(x) == len(want_yl), who
    if not len(x):
        assert red == 0.0, who
        return 0.0, 0.0
    err = float(np.abs(yl - want_yl).max())
    ok, ratio = R.within_output_bound(y, R.product(x, want_yl, makeup))
    assert err <= R.TOL_DB, (who, err)
    assert ok, (who, ratio)
    assert red == yl.max() and abs(red - R.max_reduction(want_yl)) <= R.TOL_DB, (who, red)
    return err, ratio


@pytest.mark.parametrize("sr,name", CASES)
def test_output_curve_and_max_reduction_against_the_restatement(ctx, sr, name):
    xs = R.batch(sr)
    ys, red, yls = _batch(ctx, sr, name)
    assert red.dtype == np.float64 and red.shape == (len(xs),)
    worst = worst_y = 0.0
    for i, x in enumerate(xs):
        e, r = _check(x, ys[i], yls[i], red[i], R.reference(sr, name, i)[1], R.SETS[name][5], (i, len(x)))
        worst, worst_y = max(worst, e), max(worst_y, r)
    print(sr, name, "worst |yl_gpu - yl_ref| = %.3e dB (bound %.3e), worst output error %.4f of its bound" % (worst, R.TOL_DB, worst_y))
    assert red[R.LONG] > 4.0 and red[0] == 0.0                  # compressed at all; the signal without a sample
    # in place, and without the curve: the same words
    ys2, red2, _ = _run(ctx, xs, sr, name, in_place=True, curve=False)
    assert _same(red2, red) and all(_same(a, b) for a, b in zip(ys2, ys))


@pytest.mark.parametrize("name", ["defaults", "hard", "norelease"])
def test_a_signal_under_the_knee_comes_back_bit_for_bit(ctx, name):
    x = R.quiet_signal()
    assert R.SETS[name][5] == 0.0
    for in_place in (False, True):
        ys, red, yls = _run(ctx, [x[:17], x, x[:4097]], 48000, name, in_place=in_place)
        for y, yl, want in zip(ys, yls, (x[:17], x, x[:4097])):
            assert _same(y, want) and not np.any(R.words(yl))   # every yl is +0.0
        assert not np.any(R.words(red))
    # ... with the logarithm taken for every sample too
    ctx.set_option("compress_skip", 0)
    try:
        ys, red, yls = _run(ctx, [x], 48000, name)
    finally:
        ctx.set_option("compress_skip", 1)
    assert _same(ys[0], x) and not np.any(R.words(yls[0])) and red[0] == 0.0


@pytest.mark.parametrize("sr,name", [(8000, "slow"), (48000, "defaults"), (96000, "hard")])
def test_a_signal_alone_elsewhere_and_twice(ctx, sr, name):
    xs = R.batch(sr)
    ys, red, yls = _batch(ctx, sr, name)
    ys1, red1, yls1 = _run(ctx, xs, sr, name)                   # twice
    assert _same(red1, red) and all(_same(a, b) for a, b in zip(ys1, ys)) and all(_same(a, b) for a, b in zip(yls1, yls))
    for i in (1, 4, 7, 8, R.LONG):
        ya, ra, la = _run(ctx, [xs[i]], sr, name)               # alone
        assert _same(ya[0], ys[i]) and _same(la[0], yls[i]) and _same(ra, red[i:i + 1]), i
    other = [xs[8], xs[3], xs[R.LONG], xs[7], xs[5]]            # at another position of another batch
    yo, ro, lo = _run(ctx, other, sr, name)
    for k, i in enumerate((8, 3, R.LONG, 7, 5)):
        assert _same(yo[k], ys[i]) and _same(lo[k], yls[i]) and ro[k] == red[i], i


def test_a_signal_longer_than_a_round_of_the_carry_kernels(ctx):
    """The carry kernels take ROUND_TILES tiles a round and hand the state in front of the next round to its first thread.
    The reference is ``blocked`` (tests/test_compress_plan.py: within 2^-40 dB of the sequential walk)."""
    sr, x = R.long_signal()
    assert len(x) > (CP.ROUND_TILES + CP.RUN_TILES) * CP.TILE
    name = "defaults"
    want = R.blocked(x, sr, R.SETS[name])[1]
    at = CP.ROUND_TILES * CP.TILE
    assert want[at - 1] > 4.0 and want[at:at + 64].min() > 3.0  # the state that crosses the round boundary matters behind it
    ys, red, yls = _run(ctx, [x], sr, name)
    e, r = _check(x, ys[0], yls[0], red[0], want, 0.0, "long")
    print("%d samples, %d tiles: worst |yl_gpu - yl_ref| = %.3e dB (bound %.3e), worst output error %.4f of its bound"
          % (len(x), -(-len(x) // CP.TILE), e, R.TOL_DB, r))
    ys2, red2, _ = _run(ctx, [x], sr, name, curve=False)
    assert _same(ys2[0], ys[0]) and _same(red2, red)


@pytest.mark.parametrize("sr,name", [(44100, "defaults"), (8000, "slow")])
def test_a_signal_with_a_nan_and_its_neighbours(ctx, sr, name):
    xs = list(R.batch(sr))
    ys, red, yls = _batch(ctx, sr, name)
    bad = xs[8].copy()
    bad[len(bad) // 2] = np.nan
    at = 4
    ysn, redn, ylsn = _run(ctx, xs[:at] + [bad] + xs[at:], sr, name)
    assert np.isnan(ysn[at][len(bad) // 2])
    half = len(bad) // 2                                        # ... and its own samples in front of the NaN are what they were
    assert _same(ysn[at][:half], ys[8][:half]) and _same(ylsn[at][:half], yls[8][:half])
    keep = [k for k in range(len(xs) + 1) if k != at]
    assert _same(redn[keep], red)
    for k, i in enumerate(keep):
        assert _same(ysn[i], ys[k]) and _same(ylsn[i], yls[k]), k


def test_empty_input(ctx):
    d = CP.Compressor(-20.0, 4.0)
    ys, red, yls = _run(ctx, [], 48000, d)
    assert ys == [] and red.shape == (0,) and yls == []
    ys, red, yls = _run(ctx, [np.zeros(0, np.float32)] * 3, 48000, d)
    assert [len(y) for y in ys] == [0, 0, 0] and red.tolist() == [0.0] * 3 and [len(v) for v in yls] == [0, 0, 0]
    x = R.batch(8000)[6]
    ys, red, yls = _run(ctx, [np.zeros(0, np.float32), x, np.zeros(0, np.float32)], 8000, "defaults")
    want = _batch(ctx, 8000, "defaults")
    assert _same(ys[1], want[0][6]) and red.tolist() == [0.0, want[1][6], 0.0]


def test_the_two_options(ctx):
    """compress_store 1 (xl written once and read back) gives the bits of the default; compress_skip 0 (the logarithm for every
    sample) stays within the bounds and within a rounding of the default."""
    sr, name = 44100, "defaults"
    xs = R.batch(sr)
    ys, red, yls = _batch(ctx, sr, name)
    ctx.set_option("compress_store", 1)
    try:
        ys1, red1, yls1 = _run(ctx, xs, sr, name)
        ys1p, red1p, _ = _run(ctx, xs, sr, name, in_place=True, curve=False)
    finally:
        ctx.set_option("compress_store", 0)
    assert _same(red1, red) and all(_same(a, b) for a, b in zip(ys1, ys)) and all(_same(a, b) for a, b in zip(yls1, yls))
    assert _same(red1p, red) and all(_same(a, b) for a, b in zip(ys1p, ys))
    ctx.set_option("compress_skip", 0)
    try:
        ys0, red0, yls0 = _run(ctx, xs, sr, name)
    finally:
        ctx.set_option("compress_skip", 1)
    for i, x in enumerate(xs):
        _check(x, ys0[i], yls0[i], red0[i], R.reference(sr, name, i)[1], 0.0, i)
        if len(x):
            assert float(np.abs(yls0[i] - yls[i]).max()) <= 2.0 ** -40
    with pytest.raises(Exception):
        ctx.set_option("compress_nothing", 1)


def test_refusals(ctx):
    from goofer_amd import core
    d = CP.Compressor(-20.0, 4.0)
    plan = CP.plan(48000, [100, 200], d)
    x = torch.zeros(300, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.compress(x, [0, 100, 301], plan)
    with pytest.raises(ValueError):
        ctx.compress(x[:299], None, plan)
    with pytest.raises(ValueError):
        ctx.compress(x, None, plan, out=x[:299])
    with pytest.raises(ValueError):
        ctx.compress(x.double(), None, plan)
    with pytest.raises(ValueError):
        ctx.compress(x, torch.zeros(3, dtype=torch.int32, device=ctx.device), plan)
    y, red, yl = ctx.compress(x, ctx.tensor(plan.in_off), plan)
    assert y.shape == (300,) and yl is None and red.tolist() == [0.0, 0.0]
    # the plan: every parameter outside its range, the rate, the lengths
    for bad in ((-80.1, 4), (0.1, 4), (-20, 0.99), (-20, math.nan), (-20, 4, -1, 100), (-20, 4, 1000.1, 100), (-20, 4, 5, -1), (-20, 4, 5, 5000.1),
                (-20, 4, 5, 100, -0.1), (-20, 4, 5, 100, 40.1), (-20, 4, 5, 100, 6, -24.1), (-20, 4, 5, 100, 6, 24.1)):
        with pytest.raises(ValueError):
            CP.plan(48000, [100], bad)
    for sr in (7999, 192001, 44100.5):
        with pytest.raises(ValueError):
            CP.plan(sr, [100], d)
    with pytest.raises(ValueError):
        CP.plan(48000, [100, -1], d)
    # the entry point: nothing is launched
    lib, size = ctx.lib, C.c_int64(1 << 20)
    big = torch.zeros(1 << 18, dtype=torch.float32, device=ctx.device)
    pb, qb = C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + (1 << 19))

    def call(xp=pb, off=pb, n=2, total=300, coef=pb, pows=pb, tiles=pb, n_tiles=2, out=qb, red=pb, curve=None, scratch=pb, sz=None):
        return lib.goofer_compress(ctx.h, xp, off, n, total, coef, pows, tiles, n_tiles, out, red, curve, scratch, C.byref(sz or size), None)
    for bad in (dict(n=-1), dict(total=-1), dict(n_tiles=-1), dict(n_tiles=0), dict(n_tiles=4), dict(n_tiles=1 << 31)):
        assert call(**bad) == -1, bad
        assert b"goofer_compress" in lib.goofer_last_error(ctx.h)
    for gone in ("xp", "off", "coef", "pows", "tiles", "out", "red"):
        assert call(**{gone: None}) == -1 and b"null" in lib.goofer_last_error(ctx.h), gone
    odd = lambda v, k: C.c_void_p(v.value + k)                  # noqa: E731
    for name, k in (("xp", 2), ("tiles", 2), ("out", 2), ("off", 4), ("coef", 4), ("pows", 4), ("red", 4), ("curve", 4), ("scratch", 4)):
        assert call(**{name: odd(pb, k)}) == -1 and b"aligned" in lib.goofer_last_error(ctx.h), name
    assert call(out=odd(pb, 4)) == -1 and b"overlaps" in lib.goofer_last_error(ctx.h)
    assert call(out=odd(pb, 4 * 299)) == -1 and b"overlaps" in lib.goofer_last_error(ctx.h)
    need = C.c_int64(0)
    assert lib.goofer_compress(ctx.h, None, None, 2, 300, None, None, None, 2, None, None, None, None, C.byref(need), None) == 0 and need.value > 0
    assert call(sz=C.c_int64(need.value - 1)) == -1 and b"scratch" in lib.goofer_last_error(ctx.h)
    assert lib.goofer_compress(ctx.h, pb, pb, 2, 300, pb, pb, pb, 2, qb, pb, None, pb, None, None) == -1          # no place for the size
    assert lib.goofer_compress(None, pb, pb, 2, 300, pb, pb, pb, 2, qb, pb, None, pb, C.byref(size), None) == -1
    torch.cuda.synchronize()
    assert not big.any() and not x.any()                                  # nothing was launched
    with pytest.raises(ValueError):
        core.compress_batch([np.zeros(10)], 7999, -20.0, 4.0, ctx=ctx)
    with pytest.raises(ValueError):
        core.compress_batch([np.zeros(10)], 48000, -20.0, 0.5, ctx=ctx)


def test_compress_batch(ctx):
    from goofer_amd import core
    sr, name = 8000, "slow"
    xs = R.batch(sr)
    ys, red, yls = _batch(ctx, sr, name)
    T, ratio, W, att, rel, M = R.SETS[name]
    got = core.compress_batch(xs, sr, T, ratio, knee_db=W, attack_ms=att, release_ms=rel, makeup_db=M, curve=True, ctx=ctx)
    assert len(got) == 3 and _same(got[1], red) and all(_same(a, b) for a, b in zip(got[0], ys)) and all(_same(a, b) for a, b in zip(got[2], yls))
    got = core.compress_batch([x.astype(np.float64) for x in xs], sr, T, ratio, W, att, rel, M, ctx=ctx)
    assert len(got) == 2 and _same(got[1], red) and all(_same(a, b) for a, b in zip(got[0], ys))
    ys0, red0 = core.compress_batch([], sr, T, ratio, ctx=ctx)
    assert ys0 == [] and red0.shape == (0,)
    sr, name = 48000, "defaults"                                # the defaults are the definition's
    got = core.compress_batch(R.batch(sr), sr, R.THRESHOLD, 4.0, ctx=ctx)
    assert _same(got[1], _batch(ctx, sr, name)[1]) and all(_same(a, b) for a, b in zip(got[0], _batch(ctx, sr, name)[0]))


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


def _threshold_under(track, db=12.0):
    """a threshold `db` under the track's peak, inside the definition's range: the compressor has work to do"""
    peak = float(np.abs(track).max())
    assert peak > 10.0 ** (-60.0 / 20.0)
    return max(-80.0, min(0.0, round(20.0 * math.log10(peak) - db, 1)))


def test_render_phrase_with_compress_is_the_chain_done_by_hand(ctx, monkeypatch):
    from goofer_amd import limit as LM
    from goofer_amd import loudness as LD
    from goofer_amd import rate as RT
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    plain = r.render_phrase(jobs, entries, seed=5)
    conv = ctx.rate_convert(ctx.tensor(plain), None, RT.plan(44100, 48000, [len(plain)]))
    n = conv.numel()
    st = CP.Compressor(_threshold_under(conv.cpu().numpy()), 4.0, attack_ms=2.0, release_ms=60.0)
    comp, red, _ = ctx.compress(conv, None, CP.plan(48000, [n], st))
    y, loud, gain, _ = ctx.loudness(comp, None, LD.plan(48000, [n]), -16.0)
    lim, peak, gmin = ctx.limit(y, None, LM.plan(48000, [n], 0.5))
    want = ctx.pcm16(lim).cpu().numpy()
    got, stats = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress=st, loudness=-16, limit=0.5, return_stats=True, pcm16=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert stats == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "lufs_in": float(loud.cpu()[0, 0]),
                     "momentary_max": float(loud.cpu()[0, 1]), "gain": float(gain.cpu()[0]), "max_reduction_db": float(red.cpu()[0])}
    assert stats["max_reduction_db"] > 1.0 and not _same(comp.cpu().numpy(), conv.cpu().numpy())
    # compress alone: return_stats is accepted, the statistics are the compressor's; the settings in their other spellings
    got, st2 = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress=st, return_stats=True)
    assert _same(got, comp.cpu().numpy()) and st2 == {"max_reduction_db": stats["max_reduction_db"]}
    spelled = "%r:4:2:60" % st.threshold_db
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress=spelled), got)
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress=(st.threshold_db, 4, 2, 60)), got)
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, return_stats=True)
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, compress=(-20, 0.5))
    # compress None: the bits of a call without the keyword, and Context.compress never runs
    track48 = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    both, st_both = r.render_phrase(jobs, entries, seed=5, out_sr=48000, loudness=-16, limit=0.5, return_stats=True)
    notes = r.render(jobs, seed=5)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("compress reached")
    monkeypatch.setattr(Context, "compress", never)
    assert _same(r.render_phrase(jobs, entries, seed=5, compress=None), plain)
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress=None), track48)
    got, st3 = r.render_phrase(jobs, entries, seed=5, out_sr=48000, loudness=-16, limit=0.5, return_stats=True, compress=None)
    assert _same(got, both) and st3 == st_both and "max_reduction_db" not in st3
    for a, c in zip(r.render(jobs, seed=5, compress=None), notes):
        assert _same(a, c)
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, compress=(-20, 4))
    assert len(calls) == 1


def test_render_with_compress_gives_compress_batchs_notes(ctx):
    from goofer_amd import core
    from goofer_amd.render import Renderer
    jobs, _ = _jobs()
    r = Renderer(ctx)
    notes = r.render(jobs, seed=5)
    T = _threshold_under(np.concatenate(notes))
    ys, red = core.compress_batch(notes, 44100, T, 3.0, ctx=ctx)
    assert red.max() > 1.0
    got = r.render(jobs, seed=5, compress=(T, 3.0))
    for a, c in zip(got, ys):
        assert _same(a, c)
    conv = r.render(jobs, seed=5, out_sr=48000)
    ys, red = core.compress_batch(conv, 48000, T, 3.0, knee_db=0.0, attack_ms=1.0, release_ms=30.0, makeup_db=2.0, ctx=ctx)
    for a, c in zip(r.render(jobs, seed=5, out_sr=48000, compress=CP.Compressor(T, 3.0, 0.0, 1.0, 30.0, 2.0)), ys):
        assert _same(a, c)


def test_job_file_front_end_with_compress(ctx, tmp_path, capsys):
    """python -m goofer_amd.phrase --compress ... job.txt out.wav (its main(), in process), on its own and together with --rate,
    --loudness and --limit: the wav is written at the rate asked for and every stage reports on stderr."""
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
    out = tmp_path / "plain.wav"
    assert P.main([str(job), str(out)]) == 0
    capsys.readouterr()
    with wave.open(str(out), "rb") as w:
        plain = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    T = _threshold_under(plain.astype(np.float32) / 32768.0)
    out = tmp_path / "comp.wav"
    assert P.main(["--compress", "%g:8:1:50:0:0" % T, str(job), str(out)]) == 0
    err = capsys.readouterr().err
    assert "Compressor: greatest reduction" in err and "Loudness" not in err and "Limiter" not in err
    reduction = float(err.split("greatest reduction")[1].split("dB")[0])
    assert reduction > 1.0
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 44100)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert len(pcm) == len(plain) and float(np.sum(pcm.astype(np.float64) ** 2)) < float(np.sum(plain.astype(np.float64) ** 2))
    out = tmp_path / "chain.wav"
    assert P.main(["--rate", "48000", "--compress", "%g:4" % T, "--loudness", "-16", "--limit", "-1", str(job), str(out)]) == 0
    err = capsys.readouterr().err
    assert err.index("Compressor:") < err.index("Loudness: measured") < err.index("Limiter:")
    with wave.open(str(out), "rb") as w:
        assert w.getframerate() == 48000 and w.getnframes() > len(plain)
    assert P.main(["--compress", "loud", str(job), str(out)]) == 1
    assert P.main(["--compress", "-20:0.5", str(job), str(out)]) == 1
