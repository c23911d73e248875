"""GPU: the true-peak meter (goofer_true_peak) and the limiter with true-peak detection (goofer_limit_tp, csrc/limit.hip)
against the numpy restatement (tests/true_peak_ref.py), on the library's own tables.

The fp32 restatement performs the definition's arithmetic, so the kernels are held to it bit for bit: y as int32 words, peak_in,
min_gain and the meter's peaks.  Against the float64 flavour the tolerance is derived, not measured (true_peak_ref.bound):
limit_ref's bound for steps 4 to 8, widened by what the roundings of the 24-tap sums in front of r can move a gain.

A workgroup takes a tile of 4096 samples with 2W samples of halo for r and Z = 12 more for the interpolation, and a thread makes
the envelope of eight consecutive positions.  So the lengths sit around Z, W, the halo and the tile; sample peaks sit on signal
ends, tile ends and as far from a tile edge as the longer halo reaches (2W + Z) and one past it; and bursts whose samples stay
under the ceiling while the signal between them does not (a quarter-rate sine of amplitude 1.3 c sampled at 45 degrees) sit on a
signal's first and last sample, across a tile edge and 2W + Z from one.  A tile whose envelope never exceeds the ceiling copies
its samples (option "limit_tp_skip" 1); every case runs with and without and must give the same words.

Output true peaks are held to c (1 + delta_240), delta_240 = 2 * 7.9e-8 being property (c) of the definition as measured on the
float64 restatement (tests/test_true_peak_plan.py)."""
import functools

import numpy as np
import pytest

import limit_ref as L
import true_peak_ref as TP
from goofer_amd import limit as LM

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE, Z = 4096, TP.ZEROS
SETTINGS = {"W1": (8000, 0.125), "48k": (48000, 5.0), "W1024": (8000, 128.0), "96k": (96000, 5.0)}
LOOKS = {"W1": 1, "48k": 240, "W1024": 1024, "96k": 480}
FACTORS = {"W1": 4, "48k": 4, "W1024": 4, "96k": 2}
CEILINGS = {"default": L.CEILING, "half": np.float32(0.5), "-1dB": np.float32(10.0 ** (-1.0 / 20.0))}      # those of test_gpu_limit.py
DELTA_240 = 2 * 7.9e-8


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(params=[1, 0], ids=["skip", "full"])
def skip(ctx, request):
    """with and without the copy of tiles whose envelope stays at or under the ceiling (option "limit_tp_skip")"""
    ctx.set_option("limit_tp_skip", request.param)
    yield request.param
    ctx.set_option("limit_tp_skip", 1)


def _quiet(rng, n, c):
    """noise whose true peak stays under 0.45 c: samples within 0.2 c, and S = 2.21"""
    x = (0.07 * float(c) * rng.standard_normal(n)).astype(np.float32)
    return np.clip(x, -0.2 * float(c), 0.2 * float(c))


def _peaks(rng, x, at, c):
    """sample peaks of 1.5 to 40 c, either sign, at the positions ``at`` that lie in x"""
    at = np.array([p for p in at if 0 <= p < len(x)], dtype=np.int64)
    x[at] = (float(c) * rng.uniform(1.5, 40.0, len(at)) * rng.choice([-1.0, 1.0], len(at))).astype(np.float32)
    return x


def _burst(x, centre, c):
    """the burst with its middle (between its samples 17 and 18) just in front of position ``centre``; what falls outside x is cut"""
    b = TP.burst(c)
    lo = centre - len(b) // 2
    a, e = max(lo, 0), min(lo + len(b), len(x))
    x[a:e] = b[a - lo:e - lo]
    return x


def _signals(rng, W, c):
    """The ragged batch of one setting; every signal with a sample is limited."""
    T, H = TILE, 2 * W + Z
    lens = [0, 1, Z - 1, Z, 2 * Z + 1, W, 2 * W + Z, 4 * W + 2 * Z + 2, T - 1, T, T + 1, 2 * T + 3, 0]
    xs = [_quiet(rng, n, c) for n in lens]
    _peaks(rng, xs[1], [0], c)
    _peaks(rng, xs[2], [0], c)                                              # a signal's first sample
    _peaks(rng, xs[3], [Z - 1], c)                                          # ... its last
    _peaks(rng, xs[4], [0, 2 * Z], c)
    _peaks(rng, xs[5], [W - 1], c)
    _burst(xs[6], 0, c)                                                     # a burst cut by the signal's start: u[-1] = 0
    _peaks(rng, xs[6], [2 * W + Z - 1], c)
    _peaks(rng, xs[7], [W, 2 * W], c)                                       # two peaks inside one window
    _peaks(rng, xs[8], [0, T - 2], c)
    xs[8][500:500 + 2 * W + 3] = np.float32(-7.0) * np.float32(c)           # a run of equal peaks longer than 2W + 1
    _burst(xs[9], 0, c)                                                     # inter-sample peaks alone: at the start, in the
    _burst(xs[9], T // 2, c)                                                # middle and cut by the end of a signal that is
    _burst(xs[9], T, c)                                                     # one whole tile
    _burst(xs[10], T - H, c)                                                # 2W + Z in front of a tile edge
    _peaks(rng, xs[10], [T - 1, T], c)                                      # a tile's last and the next tile's first sample
    _burst(xs[11], T, c)                                                    # across T - 1 | T: u[T - 1] is made from both tiles
    _burst(xs[11], 2 * T - H, c)
    far = (H - 1, H, H + 1)                                                 # the farthest the halo reaches, and one past it
    _peaks(rng, xs[11], [T - k for k in far] + [T + k for k in far] + [T - 1 - k for k in far] + [T - 1 + k for k in far]
           + [2 * T - k for k in far] + [2 * T + 2], c)
    return xs


@functools.lru_cache(maxsize=None)
def _case(setting, ceiling):
    """(xs, plan, fp32 restatement, float64 restatement, restated true peaks) of one setting and ceiling"""
    sr, ms = SETTINGS[setting]
    c, W = CEILINGS[ceiling], LOOKS[setting]
    rng = np.random.default_rng(20261020 + 16 * W + len(ceiling))
    xs = _signals(rng, W, c)
    plan = LM.plan(sr, [len(x) for x in xs], c, ms, true_peak=True)
    assert plan.W == W and plan.ceiling == float(c) and plan.R == FACTORS[setting] and plan.Z == Z
    tp = plan.tp_taps
    assert np.array_equal(tp, TP.table32(plan.R))
    x9 = xs[9]                                                               # nothing but bursts: the samples obey, the signal does not
    assert float(np.abs(x9).max()) <= 0.95 * float(c) and float(TP.true_peak(x9, tp)) >= 1.2 * float(c)
    return (xs, plan, TP.limit_batch(xs, plan.taps, W, c, tp), TP.limit_batch(xs, plan.taps, W, c, tp, np.float64),
            [TP.true_peak(x, tp) for x in xs])


def _flat(xs):
    return np.concatenate(list(xs) + [np.zeros(1, np.float32)])             # (never an empty tensor)


def _limit(ctx, xs, plan, out=None):
    """the kernel on the signals xs: (list of outputs, peak_in, min_gain) on the host"""
    y, peak, gain = ctx.limit(ctx.tensor(_flat(xs)), None, plan, out=out)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    return [y[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)], peak.cpu().numpy(), gain.cpu().numpy()


def _meter(ctx, xs, plan):
    peak = ctx.true_peak(ctx.tensor(_flat(xs)), None, plan)
    torch.cuda.synchronize()
    return peak.cpu().numpy()


@pytest.mark.parametrize("ceiling", list(CEILINGS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_ragged_batch_bit_for_bit_and_within_the_bound(ctx, setting, ceiling, skip):
    xs, plan, ref32, ref64, peaks = _case(setting, ceiling)
    W, c = plan.W, CEILINGS[ceiling]
    got, peak, gain = _limit(ctx, xs, plan)
    meter = _meter(ctx, xs, plan)
    worst, tiles = 0.0, 0
    for i, (x, g, r32, r64) in enumerate(zip(xs, got, ref32, ref64)):
        assert g.dtype == np.float32 and g.shape == x.shape, i
        diff = L.words(g) != L.words(r32[0])
        assert not diff.any(), (i, len(x), int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
        assert L.words(peak[i:i + 1])[0] == L.words(r32[2])[0] and L.words(gain[i:i + 1])[0] == L.words(r32[3])[0], (i, peak[i], gain[i])
        assert L.words(meter[i:i + 1])[0] == L.words(peaks[i])[0] == L.words(peak[i:i + 1])[0], (i, meter[i], peaks[i])
        err, lim = np.abs(g.astype(np.float64) - r64[0]), TP.bound(x, W, c, plan.tp_taps)
        assert np.all(err <= lim), (i, float(err.max()))
        if len(x):
            worst = max(worst, float(np.max(err / np.maximum(lim, 1e-300))))
            assert gain[i] < 1.0 and peak[i] >= 1.2 * float(c), i           # every signal of the batch is limited
            tiles += -(-len(x) // TILE)
    assert peak[0] == 0.0 and gain[0] == 1.0 and peak[-1] == 0.0 and gain[-1] == 1.0 and meter[0] == 0.0 and meter[-1] == 0.0
    assert plan.n_tiles == tiles
    print(setting, ceiling, "W", W, "R", plan.R, "worst error / bound %.4f" % worst)


def _burst_in_noise(c, n=3000, at=1500):
    rng = np.random.default_rng(77)
    x = _burst(_quiet(rng, n, c), at, c)
    return x


def test_a_peak_between_the_samples_is_limited_and_the_sample_peak_limiter_misses_it(ctx, skip):
    """The samples stay within 0.95 c, the signal between them reaches 1.3 c: goofer_limit returns it bit for bit,
    goofer_limit_tp brings its true peak, as goofer_true_peak measures it, under the ceiling.  Fails without the feature."""
    c = np.float32(0.891)
    x = _burst_in_noise(c)
    plain = LM.plan(48000, [len(x)], c)
    plan = LM.plan(48000, [len(x)], c, true_peak=True)
    assert plan.W == 240 and float(np.abs(x).max()) <= 0.95 * float(c) and float(TP.true_peak(x, plan.tp_taps)) >= 1.2 * float(c)
    (same,), peak, gain = _limit(ctx, [x], plain)
    assert np.array_equal(L.words(same), L.words(x)) and gain[0] == 1.0 and peak[0] == np.abs(x).max()
    (y,), peak, gain = _limit(ctx, [x], plan)
    assert gain[0] < 1.0 and 1.2 * float(c) <= peak[0] <= 1.4 * float(c)
    assert _meter(ctx, [x], plan)[0] == peak[0]
    out = float(_meter(ctx, [y], plan)[0])
    print("true peak in %.4f c, out / c - 1 = %.3e, min gain %.4f" % (peak[0] / c, out / float(c) - 1.0, gain[0]))
    assert out <= float(c) * (1.0 + DELTA_240)
    assert np.array_equal(L.words(y), L.words(TP.limit(x, plan.taps, plan.W, c, plan.tp_taps)[0]))


def test_a_signal_whose_true_peak_obeys_comes_back_bit_for_bit(ctx, skip):
    rng = np.random.default_rng(11)
    c = L.CEILING
    x = rng.uniform(-1.0, 1.0, 3 * TILE + 17).astype(np.float32)
    x[9] = -0.0
    plan = LM.plan(48000, [len(x)], true_peak=True)
    x = (x * np.float32(float(c) / float(TP.true_peak(x, plan.tp_taps)) * (1.0 - 1e-6))).astype(np.float32)
    top = TP.true_peak(x, plan.tp_taps)
    assert 0.99 * float(c) < float(top) <= float(c) and float(np.abs(x).max()) < float(top)
    (got,), peak, gain = _limit(ctx, [x], plan)
    assert np.array_equal(L.words(got), L.words(x)) and gain[0] == 1.0 and peak[0] == top


@pytest.mark.parametrize("setting", ["W1", "48k", "W1024"])
def test_quiet_between_loud_and_alone(ctx, setting, skip):
    """A quiet signal between two loud ones comes back as its own words although the loud samples lie within Z of it in memory
    (nothing crosses a signal boundary through the longer halo), and a signal alone gives the words it has inside a batch;
    nothing is written outside [0, total) and no sample is left unwritten."""
    sr, ms = SETTINGS[setting]
    W, c = LOOKS[setting], np.float32(0.5)
    xs, _, ref32, _, peaks = _case(setting, "half")
    rng = np.random.default_rng(7 + W)
    loud_a, loud_b = _quiet(rng, TILE + 5, c), _quiet(rng, W + Z + 3, c)
    loud_a[-1], loud_a[-Z], loud_b[0], loud_b[Z - 1] = 20.0, -3.0, -20.0, 4.0
    quiet = _quiet(rng, TILE + 2 * W + 1, c)
    plan = LM.plan(sr, [len(loud_a), len(quiet), len(loud_b)], c, ms, true_peak=True)
    tp = plan.tp_taps
    assert float(TP.true_peak(quiet, tp)) <= float(c)
    got, peak, gain = _limit(ctx, [loud_a, quiet, loud_b], plan)
    assert np.array_equal(L.words(got[1]), L.words(quiet)) and gain[1] == 1.0 and peak[1] == TP.true_peak(quiet, tp)
    want = TP.limit_batch([loud_a, loud_b], plan.taps, W, c, tp)
    assert gain[0] < 1.0 and gain[2] < 1.0 and peak[0] == want[0][2] and peak[2] == want[1][2]
    assert np.array_equal(L.words(got[0]), L.words(want[0][0])) and np.array_equal(L.words(got[2]), L.words(want[1][0]))
    meter = _meter(ctx, [loud_a, quiet, loud_b], plan)
    assert np.array_equal(L.words(meter), L.words(peak))
    for at in (11, 10, 7):                                                  # 2T + 3, T + 1 and 4W + 2Z + 2 samples
        x, want = xs[at], ref32[at]
        empty = np.zeros(0, np.float32)
        for batch, k in (([x], 0), ([loud_a, x, loud_b], 1), ([x, loud_b], 0), ([empty, loud_a, x, empty], 2)):
            p = LM.plan(sr, [len(v) for v in batch], c, ms, true_peak=True)
            buf = torch.full((p.total + 16,), float("nan"), dtype=torch.float32, device=ctx.device)
            g, pk, gn = _limit(ctx, batch, p, out=buf[8:8 + p.total])
            assert np.array_equal(L.words(g[k]), L.words(want[0])), (at, k)
            assert L.words(pk[k:k + 1])[0] == L.words(want[2])[0] and L.words(gn[k:k + 1])[0] == L.words(want[3])[0]
            assert L.words(_meter(ctx, batch, p)[k:k + 1])[0] == L.words(peaks[at])[0]
            host = buf.cpu().numpy()
            assert np.all(np.isnan(host[:8])) and np.all(np.isnan(host[8 + p.total:]))
            assert not np.any(np.isnan(host[8:8 + p.total]))


def test_refusals(ctx):
    import ctypes as C
    from goofer_amd.device import GooferError
    lib, z = ctx.lib, C.c_void_p(0)
    t = torch.zeros(3 * TILE, dtype=torch.int64, device=ctx.device)
    out = torch.zeros(2 * TILE, dtype=torch.float32, device=ctx.device)
    p, odd, o = C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr() + 4), C.c_void_p(out.data_ptr())
    half = C.c_void_p(t.data_ptr() + 2)
    c = C.c_float(0.5)

    def limit(x=p, off=p, n=1, total=5000, W=240, taps=p, cc=c, tiles=p, n_tiles=2, y=o, peak=p, gain=p, R=4, ZZ=Z, tp=p):
        return lib.goofer_limit_tp(ctx.h, x, off, n, total, W, taps, cc, tiles, n_tiles, y, peak, gain, R, ZZ, tp, None)

    def meter(x=p, off=p, n=1, total=5000, R=4, ZZ=Z, taps=p, tiles=p, n_tiles=2, peak=o):
        return lib.goofer_true_peak(ctx.h, x, off, n, total, R, ZZ, taps, tiles, n_tiles, peak, None)
    torch.cuda.synchronize()
    before = out.clone()
    for call, name in ((limit, b"goofer_limit_tp"), (meter, b"goofer_true_peak")):
        for bad in (dict(R=0), dict(R=1), dict(R=3), dict(R=8), dict(ZZ=0), dict(ZZ=11), dict(ZZ=32), dict(n_tiles=1), dict(n_tiles=4),
                    dict(n_tiles=-1), dict(n=-1), dict(total=-1)):
            assert call(**bad) == -1, (name, bad)
            assert name in lib.goofer_last_error(ctx.h)
        for bad in (dict(x=z), dict(off=z), dict(taps=z), dict(tiles=z), dict(peak=z)):
            assert call(**bad) == -1, (name, bad)
            assert b"null" in lib.goofer_last_error(ctx.h)
        for bad in (dict(off=odd), dict(x=half), dict(taps=half), dict(tiles=half), dict(peak=half)):
            assert call(**bad) == -1, (name, bad)
            assert b"aligned" in lib.goofer_last_error(ctx.h)
    for bad in (dict(tp=z), dict(y=z), dict(gain=z)):
        assert limit(**bad) == -1
        assert b"null" in lib.goofer_last_error(ctx.h)
    for bad in (dict(tp=half), dict(y=C.c_void_p(out.data_ptr() + 1))):
        assert limit(**bad) == -1
        assert b"aligned" in lib.goofer_last_error(ctx.h)
    for bad in (dict(W=0), dict(W=1025), dict(cc=C.c_float(0.0)), dict(cc=C.c_float(1.5)), dict(cc=C.c_float(float("nan")))):
        assert limit(**bad) == -1, bad
    for y in (p, C.c_void_p(t.data_ptr() + 4 * 4999), C.c_void_p(t.data_ptr() - 4 * 4999)):      # out overlaps x
        assert limit(y=y) == -1
        assert b"overlaps" in lib.goofer_last_error(ctx.h)
    assert limit(x=z, off=z, n=0, total=0, taps=z, tiles=z, n_tiles=0, y=z, peak=z, gain=z, tp=z) == 0      # no signal: nothing to do
    assert meter(x=z, off=z, n=0, total=0, taps=z, tiles=z, n_tiles=0, peak=z) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before) and not t.any()                        # nothing was launched
    plan = LM.plan(48000, [100, 200], true_peak=True)
    x = torch.zeros(300, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.true_peak(x, None, LM.plan(48000, [100, 200]))                  # a plan without the table
    with pytest.raises(ValueError):
        ctx.true_peak(x, [0, 100, 301], plan)
    with pytest.raises(ValueError):
        ctx.true_peak(x[:299], None, plan)
    with pytest.raises(GooferError, match="overlaps"):
        ctx.limit(x, None, plan, out=x)
    y, peak, gain = ctx.limit(x, ctx.tensor(plan.in_off), plan)
    assert y.shape == (300,) and peak.tolist() == [0.0, 0.0] and gain.tolist() == [1.0, 1.0]
    assert ctx.true_peak(x, ctx.tensor(plan.in_off), plan).tolist() == [0.0, 0.0]
    none = LM.plan(48000, [0, 0, 0], true_peak=True)                        # signals without a sample: the statistics alone
    y, peak, gain = ctx.limit(x, None, none)
    assert y.numel() == 0 and peak.tolist() == [0.0] * 3 and gain.tolist() == [1.0] * 3 and ctx.true_peak(x, None, none).tolist() == [0.0] * 3


def test_true_peak_batch_and_limit_batch(ctx):
    from goofer_amd import core
    c = CEILINGS["-1dB"]
    rng = np.random.default_rng(5)
    xs = [_burst(_quiet(rng, 700, c), 300, c), _peaks(rng, _quiet(rng, 50, c), [49], c), np.zeros(0, np.float32),
          _peaks(rng, _quiet(rng, TILE + 30, c), [TILE - 1], c)]
    plan = LM.plan(44100, [len(x) for x in xs], c, true_peak=True)
    peaks = core.true_peak_batch(xs, 44100, ctx=ctx)
    assert peaks.dtype == np.float32 and peaks.shape == (4,)
    assert np.array_equal(L.words(peaks), L.words(np.array([TP.true_peak(x, plan.tp_taps) for x in xs], np.float32)))
    assert 1.2 * float(c) <= peaks[0] <= 1.4 * float(c) and peaks[2] == 0.0
    got, peak, gain = core.limit_batch(xs, 44100, ceiling=c, ctx=ctx, true_peak=True)
    want = TP.limit_batch(xs, plan.taps, plan.W, c, plan.tp_taps)
    assert len(got) == 4 and np.array_equal(L.words(peak), L.words(peaks))
    for g, gn, r in zip(got, gain, want):
        assert g.dtype == np.float32 and np.array_equal(L.words(g), L.words(r[0])) and gn == r[3]
    assert gain[0] < 1.0 and gain[2] == 1.0
    plain, ppeak, pgain = core.limit_batch(xs, 44100, ceiling=c, ctx=ctx)                  # without the keyword: today's limiter
    assert np.array_equal(L.words(plain[0]), L.words(xs[0])) and pgain[0] == 1.0 and ppeak[0] == np.abs(xs[0]).max()
    assert core.true_peak_batch([], 44100, ctx=ctx).shape == (0,)
    assert core.true_peak_batch([np.zeros(0), np.zeros(3)], 96000, ctx=ctx).tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        core.true_peak_batch(xs, 7999, ctx=ctx)
    with pytest.raises(ValueError):
        core.limit_batch(xs, 200000, ctx=ctx, true_peak=True)


def _jobs():
    """the four notes of examples/render_phrase.py, short, at volumes that put the track well above 0.891"""
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


def test_render_phrase_with_a_true_peak_limiter(ctx):
    """The track is the restatement applied to the unlimited track, word for word, and its true peak, metered in fp32 on the
    device, obeys the ceiling within delta_240 plus what fp32 rounding can add (derived below; measured: 2.7e-7 over c, where
    delta_240 alone is 1.6e-7 and one fp32 step at 0.891 is 6.7e-8)."""
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    c = np.float32(0.891)
    track = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    plan = LM.plan(48000, [len(track)], c, true_peak=True)
    assert float(TP.true_peak(track, plan.tp_taps)) > 1.05 * float(c)       # the unlimited track does exceed the ceiling
    want, _, peak, gmin = TP.limit(track, plan.taps, plan.W, c, plan.tp_taps)
    got, stats = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=LM.Limiter(0.891, true_peak=True), return_stats=True)
    assert got.dtype == np.float32 and np.array_equal(L.words(got), L.words(want))
    assert stats["true_peak_in"] == stats["peak_in"] == float(peak) and stats["min_gain"] == float(gmin) < 1.0
    assert stats["true_peak_out"] == float(TP.true_peak(want, plan.tp_taps))
    print("true peak in %.4f, out / c - 1 = %.3e" % (stats["true_peak_in"], stats["true_peak_out"] / float(c) - 1.0))
    # delta for an fp32 track, derived: the float64 flavour keeps c (1 + delta_240); an fp32 sample is within true_peak_ref.bound
    # of it, which moves a reconstructed value by at most S = 2.2064 times the greatest bound; the meter's own 24-tap sums round
    # once per product and per add, 25 * 2^-24 * S max |y|
    S = 2.2064
    slack = S * float(TP.bound(track, plan.W, c, plan.tp_taps).max()) + 25.0 * 2.0 ** -24 * S * float(np.abs(want).max())
    assert slack < 1e-3 * float(c)
    assert stats["true_peak_out"] <= float(c) * (1.0 + DELTA_240) + slack
    same = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=(0.891, 5.0, True))
    assert np.array_equal(L.words(same), L.words(want))
    pcm = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=LM.Limiter(0.891, true_peak=True), pcm16=True)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, L.pcm16(want))
    # a scalar still runs today's limiter: the words of Context.limit with a plain plan, and no true-peak statistics
    plain = LM.plan(48000, [len(track)], c)
    y, pk, gn = ctx.limit(ctx.tensor(np.concatenate([track, np.zeros(1, np.float32)])), None, plain)
    got, stats = r.render_phrase(jobs, entries, seed=5, out_sr=48000, limit=0.891, return_stats=True)
    assert np.array_equal(L.words(got), L.words(y.cpu().numpy())) and np.array_equal(L.words(got), L.words(L.limit(track, plain.taps, plain.W, c)[0]))
    assert set(stats) == {"peak_in", "min_gain"} and stats["peak_in"] == float(np.abs(track).max())
    # the notes of render
    notes = r.render(jobs, seed=5)
    lim = r.render(jobs, seed=5, limit=LM.Limiter(0.5, true_peak=True))
    nplan = LM.plan(44100, [len(v) for v in notes], 0.5, true_peak=True)
    for a, b in zip(lim, TP.limit_batch(notes, nplan.taps, nplan.W, np.float32(0.5), nplan.tp_taps)):
        assert np.array_equal(L.words(a), L.words(b[0]))


def test_job_file_front_end_with_a_true_peak_limit(ctx, tmp_path, capsys):
    """python -m goofer_amd.phrase --limit -1 --true-peak --rate 48000 job.txt out.wav (its main(), in process): the wav is
    written and stderr reports the true peak in front of and behind the limiter in dBTP, and the greatest reduction."""
    import re
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
    out = tmp_path / "tp.wav"
    assert P.main(["--limit", "-1", "--true-peak", "--rate", "48000", str(job), str(out)]) == 0
    err = capsys.readouterr().err
    m = re.search(r"input true peak (-?[\d.]+) dBTP, output true peak (-?[\d.]+) dBTP, greatest reduction ([\d.]+) dB \(ceiling -1\.00 dBTP\)", err)
    assert m, err
    assert float(m.group(1)) > -1.0 and float(m.group(2)) <= -1.0 + 0.005 and float(m.group(3)) > 0.0
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    assert len(pcm) and int(np.abs(pcm.astype(np.int32)).max()) <= int(np.rint(10.0 ** (-1.0 / 20.0) * 32768.0))
    assert P.main(["--true-peak", "--rate", "48000", str(job), str(tmp_path / "no.wav")]) == 1      # the flag without --limit
    assert not (tmp_path / "no.wav").exists()
