"""GPU: the look-ahead peak limiter (goofer_limit, csrc/limit.hip) against its numpy restatement (tests/limit_ref.py), on the
library's own table.

The fp32 restatement performs the definition's arithmetic, so the kernel is held to it bit for bit on y (as int32 words),
peak_in and min_gain.  Against the float64 flavour (the same fp32 r and table, steps 4 to 8 in float64) the tolerance is derived,
not measured: per sample |got - ref| <= (2 (2W + 1) + 4) * 2^-24 * |x[i]|, one rounding per product and per add of the 2W + 1
taps and the roundings of d, s and y, each at most 2^-24 of a gain that is at most 1.

The kernel gives a workgroup a tile of 4096 samples of one signal with 2W samples of halo on either side, so the lengths sit
around W, 2W, 4W and the tile, and the peaks on signal ends, tile ends and as far from a tile edge as the two halos reach.  A
tile with nothing above the ceiling copies its samples (option "limit_skip" 1); every case runs with and without and must give
the same words."""
import functools

import numpy as np
import pytest

import limit_ref as R
from goofer_amd import limit as LM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 4096
SETTINGS = {"W1": (8000, 0.125), "W1024": (8000, 128.0), "44k1": (44100, 5.0), "48k": (48000, 5.0), "96k": (96000, 5.0)}
LOOKS = {"W1": 1, "W1024": 1024, "44k1": 221, "48k": 240, "96k": 480}
CEILINGS = {"default": R.CEILING, "half": np.float32(0.5), "-1dB": np.float32(10.0 ** (-1.0 / 20.0))}


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(params=[1, 0], ids=["skip", "full"])
def skip(ctx, request):
    """with and without the copy of tiles that have nothing above the ceiling (option "limit_skip")"""
    ctx.set_option("limit_skip", request.param)
    yield request.param
    ctx.set_option("limit_skip", 1)


def _quiet(rng, n, c):
    x = (0.2 * float(c) * rng.standard_normal(n)).astype(np.float32)
    return np.clip(x, -0.9 * float(c), 0.9 * float(c))


def _peaks(rng, x, at, c):
    """peaks of 1.5 to 40 c, either sign, at the positions ``at`` that lie in x"""
    at = np.array([p for p in at if 0 <= p < len(x)], dtype=np.int64)
    x[at] = (float(c) * rng.uniform(1.5, 40.0, len(at)) * rng.choice([-1.0, 1.0], len(at))).astype(np.float32)
    return x


def _signals(rng, W, c):
    """The ragged batch of one setting: lengths around W, 2W, 4W and the tile, two empty signals at the ends, one more signal for
    single peaks that a tile sees in its halo only."""
    T, far = TILE, (W, W + 1, 2 * W, 2 * W + 1)
    lens = [0, 1, W, W + 1, 2 * W, 2 * W + 1, 4 * W + 2, T - 1, T, T + 1, 2 * T + 3, 2 * T, 0]
    xs = [_quiet(rng, n, c) for n in lens]
    _peaks(rng, xs[1], [0], c)
    _peaks(rng, xs[2], [0], c)                                              # a signal's first sample
    _peaks(rng, xs[3], [W], c)                                              # ... its last
    _peaks(rng, xs[4], [0, 2 * W - 1], c)
    _peaks(rng, xs[5], [W], c)
    _peaks(rng, xs[6], [W, 2 * W], c)                                       # two peaks inside one window
    _peaks(rng, xs[7], [0, T - 2], c)
    _peaks(rng, xs[8], [T - 1], c)                                          # a tile's (and the signal's) last sample
    xs[8][500:500 + 2 * W + 3] = np.float32(-7.0) * np.float32(c)           # a run of equal peaks longer than 2W + 1
    _peaks(rng, xs[9], [T - 1, T], c)                                       # a tile's last and the next tile's first sample
    _peaks(rng, xs[10], [T - k for k in far] + [T + k for k in far] + [T - 1 - k for k in far] + [T - 1 + k for k in far]
           + [2 * T - k for k in far] + [2 * T - 1 + k for k in far] + [2 * T - 1, 2 * T, 2 * T + 2], c)
    _peaks(rng, xs[11], [T - 1 - W - W // 2, T + W + W // 2], c)            # each reaches across the edge through a halo
    return xs


@functools.lru_cache(maxsize=None)
def _case(setting, ceiling):
    """(xs, plan, fp32 restatement, float64 restatement) of one setting and ceiling"""
    sr, ms = SETTINGS[setting]
    c = CEILINGS[ceiling]
    W = LOOKS[setting]
    rng = np.random.default_rng(20261020 + 16 * W + len(ceiling))
    xs = _signals(rng, W, c)
    plan = LM.plan(sr, [len(x) for x in xs], c, ms)
    assert plan.W == W and plan.ceiling == float(c)
    return xs, plan, R.limit_batch(xs, plan.taps, W, c), R.limit_batch(xs, plan.taps, W, c, np.float64)


def _limit(ctx, xs, plan, out=None):
    """the kernel on the signals xs: (list of outputs, peak_in, min_gain) on the host"""
    flat = np.concatenate(list(xs) + [np.zeros(1, np.float32)])             # (never an empty tensor)
    y, peak, gain = ctx.limit(ctx.tensor(flat), None, plan, out=out)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    return [y[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)], peak.cpu().numpy(), gain.cpu().numpy()


@pytest.mark.parametrize("ceiling", list(CEILINGS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_ragged_batch_bit_for_bit_and_within_the_bound(ctx, setting, ceiling, skip):
    xs, plan, ref32, ref64 = _case(setting, ceiling)
    W, c = plan.W, CEILINGS[ceiling]
    got, peak, gain = _limit(ctx, xs, plan)
    worst, top, tiles = 0.0, 0.0, 0
    for i, (x, g, r32, r64) in enumerate(zip(xs, got, ref32, ref64)):
        assert g.dtype == np.float32 and g.shape == x.shape, i
        diff = R.words(g) != R.words(r32[0])
        assert not diff.any(), (i, len(x), int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
        assert R.words(peak[i:i + 1])[0] == R.words(r32[2])[0] and R.words(gain[i:i + 1])[0] == R.words(r32[3])[0], (i, peak[i], gain[i])
        err, lim = np.abs(g.astype(np.float64) - r64[0]), R.bound(x, W)
        assert np.all(err <= lim), (i, float(err.max()))
        if len(x):
            worst = max(worst, float(np.max(err / np.maximum(lim, 1e-300))))
            top = max(top, float(np.abs(g).max()) / float(c))
            assert float(np.abs(x).max()) >= 1.5 * float(c) and gain[i] < 1.0, i        # every signal of the batch is limited
            tiles += -(-len(x) // TILE)
    assert top <= 1.0 + 2.0 ** -22
    assert peak[0] == 0.0 and gain[0] == 1.0 and peak[-1] == 0.0 and gain[-1] == 1.0      # the empty signals
    assert plan.n_tiles == tiles
    print(setting, ceiling, "W", W, "worst error / bound %.4f, max |y| / c - 1 = %.3e" % (worst, top - 1.0))


@pytest.mark.parametrize("setting", ["W1", "48k", "W1024"])
def test_quiet_between_loud_and_alone(ctx, setting, skip):
    """A quiet signal between two loud ones comes back as its own words (nothing leaks across a signal boundary, although the
    loud samples lie within 2W of it in memory), and a signal alone gives the words it has inside the batch; nothing is written
    outside [0, total) and no sample is left unwritten."""
    sr, ms = SETTINGS[setting]
    W, c = LOOKS[setting], np.float32(0.5)
    xs, _, ref32, _ = _case(setting, "half")
    rng = np.random.default_rng(7 + W)
    loud_a, loud_b = _quiet(rng, TILE + 5, c), _quiet(rng, W + 3, c)
    loud_a[-1], loud_a[-W - 1], loud_b[0], loud_b[W] = 20.0, -3.0, -20.0, 4.0
    quiet = _quiet(rng, TILE + 2 * W + 1, c)
    quiet[0], quiet[-1], quiet[TILE] = c, -c, c                             # at the ceiling is not above it
    plan = LM.plan(sr, [len(loud_a), len(quiet), len(loud_b)], c, ms)
    got, peak, gain = _limit(ctx, [loud_a, quiet, loud_b], plan)
    assert np.array_equal(R.words(got[1]), R.words(quiet)) and gain[1] == 1.0 and peak[1] == c
    assert gain[0] < 1.0 and gain[2] < 1.0 and peak[0] == 20.0 and peak[2] == 20.0
    want = R.limit_batch([loud_a, loud_b], plan.taps, W, c)
    assert np.array_equal(R.words(got[0]), R.words(want[0][0])) and np.array_equal(R.words(got[2]), R.words(want[1][0]))
    for at in (10, 11, 6):                                                  # 2T + 3, 2T and 4W + 2 samples
        x, want = xs[at], ref32[at]
        empty = np.zeros(0, np.float32)
        for batch, k in (([x], 0), ([loud_a, x, loud_b], 1), ([x, loud_b], 0), ([empty, loud_a, x, empty], 2)):
            p = LM.plan(sr, [len(v) for v in batch], c, ms)
            buf = torch.full((p.total + 16,), float("nan"), dtype=torch.float32, device=ctx.device)
            g, pk, gn = _limit(ctx, batch, p, out=buf[8:8 + p.total])
            assert np.array_equal(R.words(g[k]), R.words(want[0])), (at, k)
            assert R.words(pk[k:k + 1])[0] == R.words(want[2])[0] and R.words(gn[k:k + 1])[0] == R.words(want[3])[0]
            host = buf.cpu().numpy()
            assert np.all(np.isnan(host[:8])) and np.all(np.isnan(host[8 + p.total:]))
            assert not np.any(np.isnan(host[8:8 + p.total]))


def test_a_signal_below_the_ceiling_comes_back_bit_for_bit(ctx, skip):
    rng = np.random.default_rng(11)
    c = R.CEILING
    x = rng.uniform(-1.0, 1.0, 3 * TILE + 17).astype(np.float32)
    np.clip(x, -float(c), float(c), out=x)
    x[5], x[TILE], x[-1], x[9] = c, -c, c, -0.0
    plan = LM.plan(48000, [len(x)])
    (got,), peak, gain = _limit(ctx, [x], plan)
    assert np.array_equal(R.words(got), R.words(x)) and gain[0] == 1.0 and peak[0] == c


def test_refusals(ctx):
    import ctypes as C
    from goofer_amd.device import GooferError
    lib, z = ctx.lib, C.c_void_p(0)
    t = torch.zeros(3 * TILE, dtype=torch.int64, device=ctx.device)
    out = torch.zeros(2 * TILE, dtype=torch.float32, device=ctx.device)
    p, odd, o = C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 4), C.c_void_p(out.data_ptr())
    c = C.c_float(0.5)

    def call(x=p, off=p, n=1, total=5000, W=240, taps=p, cc=c, tiles=p, n_tiles=2, y=o, peak=p, gain=p):
        return lib.goofer_limit(ctx.h, x, off, n, total, W, taps, cc, tiles, n_tiles, y, peak, gain, None)
    torch.cuda.synchronize()
    before = out.clone()
    for k, bad in enumerate((dict(x=z), dict(off=z), dict(taps=z), dict(tiles=z), dict(y=z), dict(peak=z), dict(gain=z))):
        assert call(**bad) == -1, k
        assert b"null" in lib.goofer_last_error(ctx.h)
    for bad in (dict(off=odd), dict(x=C.c_void_p(t.data_ptr() + 2)), dict(y=C.c_void_p(out.data_ptr() + 1))):
        assert call(**bad) == -1
        assert b"aligned" in lib.goofer_last_error(ctx.h)
    for bad in (dict(W=0), dict(W=1025), dict(cc=C.c_float(0.0)), dict(cc=C.c_float(1.5)), dict(cc=C.c_float(float("nan"))), dict(n=-1),
                dict(total=-1), dict(n_tiles=1), dict(n_tiles=4), dict(n_tiles=-1)):
        assert call(**bad) == -1, bad
        assert b"goofer_limit" in lib.goofer_last_error(ctx.h)
    # out overlaps x: in place, from inside x, ending inside x
    for y in (p, C.c_void_p(t.data_ptr() + 4 * 4999), C.c_void_p(t.data_ptr() - 4 * 4999)):
        assert call(y=y) == -1
        assert b"overlaps" in lib.goofer_last_error(ctx.h)
    with pytest.raises(GooferError, match="overlaps"):
        ctx._check(call(y=p))
    assert call(x=z, off=z, n=0, total=0, taps=z, tiles=z, n_tiles=0, y=z, peak=z, gain=z) == 0      # no signal: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(out, before) and not t.any()                        # nothing was launched
    plan = LM.plan(48000, [100, 200])
    x = torch.zeros(300, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.limit(x, [0, 100, 301], plan)
    with pytest.raises(ValueError):
        ctx.limit(x[:299], None, plan)
    with pytest.raises(ValueError):
        ctx.limit(x, None, plan, out=torch.zeros(301, dtype=torch.float32, device=ctx.device))
    with pytest.raises(GooferError, match="overlaps"):
        ctx.limit(x, None, plan, out=x)
    y, peak, gain = ctx.limit(x, ctx.tensor(plan.in_off), plan)
    assert y.shape == (300,) and peak.tolist() == [0.0, 0.0] and gain.tolist() == [1.0, 1.0]
    y, peak, gain = ctx.limit(x, None, LM.plan(48000, [0, 0, 0]))           # signals without a sample: the statistics alone
    assert y.numel() == 0 and peak.tolist() == [0.0] * 3 and gain.tolist() == [1.0] * 3


def test_limit_batch(ctx):
    from goofer_amd import core
    xs, plan, ref32, _ = _case("48k", "-1dB")
    got, peak, gain = core.limit_batch(xs, 48000, ceiling=CEILINGS["-1dB"], ctx=ctx)
    assert len(got) == len(xs) and peak.dtype == np.float32 and gain.dtype == np.float32
    for g, pk, gn, r in zip(got, peak, gain, ref32):
        assert g.dtype == np.float32 and np.array_equal(R.words(g), R.words(r[0])) and pk == r[2] and gn == r[3]
    got, peak, gain = core.limit_batch([np.zeros(0), np.zeros(0, np.float32)], 44100, ctx=ctx)
    assert [len(g) for g in got] == [0, 0] and peak.tolist() == [0.0, 0.0] and gain.tolist() == [1.0, 1.0]
    assert core.limit_batch([], 44100, ctx=ctx)[0] == []
    with pytest.raises(ValueError):
        core.limit_batch(xs, 48000, ceiling=1.5, ctx=ctx)
    with pytest.raises(ValueError):
        core.limit_batch(xs, 48000, lookahead_ms=0.0, ctx=ctx)


def _jobs():
    """the four notes of examples/render_phrase.py, short, at volumes that put the track well above 0.5"""
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Source
    requests = [("C4", "100", "g-10", "30", "300", "80", "50", "100", "0", "!120", "AA"),
                ("E4", "100", "t30fa20fb-10B30", "30", "300", "80", "50", "120", "0", "!120", "AA#20#AP"),
                ("G4", "80", "L1sg40st-30", "30", "300", "80", "50", "100", "0", "!120", "AA"),
                ("A3", "120", "vf30sa20pd40", "30", "300", "80", "50", "110", "0", "!120", "AA#10#BA#10#AA")]
    jobs = []
    for i, args in enumerate(requests):
        src = syn.make_source(100 + i, seconds=0.3)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
    entries = ["0 250 5 35 40 0 100 100 0 0", "10 240@120+30 5 35 40 20 100 90 10 30", "R 120",
               "0 250 5 35 40 0 110 100 0 25 10 30 80", "5 200 5 35 40 0 100 100 0 40"]
    return jobs, entries


def test_render_and_render_phrase_with_limit(ctx, monkeypatch):
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    c = np.float32(0.5)
    # the phrase: mix, convert to 48 kHz, limit at 48 kHz, int16
    track = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    assert track.dtype == np.float32 and float(np.abs(track).max()) > 0.6          # the unlimited track does exceed the ceiling
    W = R.look(48000)
    taps = LM.plan(48000, [len(track)], c).taps
    want, _, peak, gmin = R.limit(track, taps, W, c)
    got, stats = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=0.5, return_stats=True)
    assert got.dtype == np.float32 and np.array_equal(R.words(got), R.words(want))
    assert stats["peak_in"] == float(np.abs(track).max()) == float(peak) and stats["min_gain"] == float(gmin) < 1.0
    pcm = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=0.5, pcm16=True)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, R.pcm16(want))
    assert int(np.abs(pcm.astype(np.int32)).max()) <= int(np.rint(0.5 * 32768)) < int(np.abs(R.pcm16(track).astype(np.int32)).max())
    # a (ceiling, lookahead_ms) pair, at the notes' own rate
    plain = r.render_phrase(jobs, entries, seed=5)
    got = r.render_phrase(jobs, entries, seed=5, limit=(0.25, 2.0))
    W2 = R.look(44100, 2.0)
    assert np.array_equal(R.words(got), R.words(R.limit(plain, LM.plan(44100, [len(plain)], 0.25, 2.0).taps, W2, np.float32(0.25))[0]))
    # the notes
    notes = r.render(jobs, seed=5)
    assert min(float(np.abs(y).max()) for y in notes) > 0.6
    lim = r.render(jobs, seed=5, limit=0.5)
    W3 = R.look(44100)
    want = R.limit_batch(notes, LM.plan(44100, [len(y) for y in notes], c).taps, W3, c)
    for a, b in zip(lim, want):
        assert np.array_equal(R.words(a), R.words(b[0])) and float(np.abs(a).max()) <= 0.5 * (1.0 + 2.0 ** -22)
    conv = r.render(jobs, seed=5, out_sr=48000)
    lim = r.render(jobs, seed=5, out_sr=48000, limit=0.5)
    want = R.limit_batch(conv, taps, W, c)
    for a, b in zip(lim, want):
        assert np.array_equal(R.words(a), R.words(b[0]))
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, limit=1.5)
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, return_stats=True)
    # limit None: the bits of a call without the keyword, and Context.limit never runs
    pcm_plain = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("limit reached")
    monkeypatch.setattr(Context, "limit", never)
    assert np.array_equal(R.words(r.render_phrase(jobs, entries, seed=5, limit=None)), R.words(plain))
    assert np.array_equal(R.words(r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=None)), R.words(track))
    assert np.array_equal(r.render_phrase(jobs, entries, seed=5, pcm16=True, limit=None), pcm_plain)
    for a, b in zip(r.render(jobs, seed=5, limit=None), notes):
        assert np.array_equal(R.words(a), R.words(b))
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, limit=0.5)
    assert len(calls) == 1


def test_job_file_front_end_with_limit(ctx, tmp_path, capsys):
    """python -m goofer_amd.phrase --limit -6 --rate 48000 job.txt out.wav (its main(), in process): the wav says 48000, its
    samples obey the ceiling, and the input peak and the greatest reduction are reported on stderr."""
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

    def read(path):
        with wave.open(str(path), "rb") as w:
            return (w.getnchannels(), w.getsampwidth(), w.getframerate()), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    plain, lim, bare = tmp_path / "plain.wav", tmp_path / "lim.wav", tmp_path / "bare.wav"
    assert P.main(["--rate", "48000", str(job), str(plain)]) == 0
    capsys.readouterr()
    assert P.main(["--limit", "-6", "--rate", "48000", str(job), str(lim)]) == 0
    err = capsys.readouterr().err
    assert "input peak" in err and "reduction" in err and "dB" in err
    c = np.float32(10.0 ** (-6.0 / 20.0))
    top = int(np.rint(float(c) * (1.0 + 2.0 ** -22) * 32768.0))
    head, a = read(plain)
    assert head == (1, 2, 48000) and int(np.abs(a.astype(np.int32)).max()) > top + 1000      # without the limiter it is well above
    head, b = read(lim)
    assert head == (1, 2, 48000) and len(b) == len(a) and int(np.abs(b.astype(np.int32)).max()) <= top
    assert P.main(["--rate", "48000", "--limit", str(job), str(bare)]) == 0               # bare: the default ceiling
    head, d = read(bare)
    assert head == (1, 2, 48000) and len(d) == len(a) and int(np.abs(d.astype(np.int32)).max()) <= 32767
    assert P.main(["--limit", "3", str(job), str(bare)]) == 1                              # a ceiling above full scale
    assert P.main(["--limit", "-6", "--rate", "fast", str(job), str(bare)]) == 1
