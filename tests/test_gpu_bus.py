"""The stereo bus on the device against its restatement (tests/bus_ref.py), bit for bit unless said otherwise: goofer_bus_mix at
tile, wave and alignment edges; goofer_limit_linked, the skip decision across channels and the true-peak form included;
goofer_loudness_link on the device's own segment energies; goofer_pcm16_planar; and render_song / python -m goofer_amd.bus
against the same chain made by hand.  Every test here fails on a tree without the bus: the symbols do not exist."""
import ctypes as C
import wave

import numpy as np
import pytest

import bus_ref as R
import limit_ref as L
import loudness_ref as LD
import true_peak_ref as TP
from goofer_amd import bus as B
from goofer_amd import limit as LM
from goofer_amd import loudness as LDP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = -1
DELTA_240 = 2 * 7.9e-8              # tests/test_gpu_true_peak.py's bound on the output true peak: c (1 + DELTA_240)


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _dev(ctx, x, lead=0):
    """x on the device behind ``lead`` floats of padding (lead 1: a source that is not 16-byte aligned), one pad float behind"""
    t = ctx.tensor(np.concatenate([np.zeros(lead, np.float32), np.asarray(x, np.float32), np.zeros(1, np.float32)]))
    return t[lead:lead + len(x)] if len(x) else t[lead:lead + 1][:0]


def _mix(ctx, xs, tracks, total_out=None, lead=0, out_lead=0):
    """(device bus as numpy [2N], restatement) of the host signals ``xs`` with ``tracks``; out is prefilled with NaN"""
    ds = [_dev(ctx, x, lead) for x in xs]
    plan = B.plan([d if d.numel() else 0 for d in ds], [len(x) for x in xs], tracks, 48000, total_out)
    N = plan.total_out
    buf = torch.full((2 * N + out_lead + 1,), float("nan"), dtype=torch.float32, device=ctx.device)
    out = ctx.bus_mix(ds, plan, out=buf[out_lead:out_lead + 2 * N])
    ctx.check()
    live = [k for k, t in enumerate(tracks) if not t.mute]
    want = R.mix([xs[k] for k in live], [(B.samples(tracks[k].start_ms, 48000),) + R.gains(tracks[k].gain_db, tracks[k].pan) for k in live], N)
    assert torch.isnan(buf[:out_lead]).all() and torch.isnan(buf[out_lead + 2 * N:]).all()     # nothing outside the bus is written
    return out.cpu().numpy(), want, plan


def _same(a, b):
    return a.shape == b.shape and np.array_equal(L.words(a), L.words(b))


def _ms(samples):
    return samples * 1000.0 / 48000.0


# ---- mix -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pan", [-1.0, 0.0, 1.0, 0.3])
def test_one_track_pan_and_length(ctx, pan):
    rng = np.random.default_rng(11)
    for N in (1, 7, 2047, 2048, 2049, 5000):
        x = rng.uniform(-1, 1, N).astype(np.float32)
        got, want, _ = _mix(ctx, [x], [B.Track(-3.0, pan)])
        gl, gr = R.gains(-3.0, pan)
        zero = np.float32(0.0)                                  # (the sum starts from +0.0f: a product of -0 becomes +0)
        assert _same(got, want) and _same(got[:N], zero + gl * x) and _same(got[N:], zero + gr * x), (pan, N)
        if pan == -1.0:
            assert not got[N:].any() and not np.signbit(got[N:]).any()


def test_three_tracks_edges_and_an_empty_tile(ctx):
    """Starts 0, 3 and 2050: unaligned sources, a track that ends mid-wave, one that covers exactly a tile (2048 .. 4096 is
    tile 1: here start 2048 of a fourth track), and a tile no track reaches, which holds +0.0f in both channels."""
    rng = np.random.default_rng(12)
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1500, 700, 1000, 2048)]
    tracks = [B.Track(0.0, -0.4), B.Track(-6.0, 0.2, _ms(3)), B.Track(2.0, 0.9, _ms(2050)), B.Track(-1.0, 0.0, _ms(2048))]
    for lead in (0, 1):
        got, want, plan = _mix(ctx, xs, tracks, total_out=3 * 2048 + 5, lead=lead)
        assert _same(got, want), lead
        N = plan.total_out
        assert plan.tile_off[3] == plan.tile_off[2] and plan.tile_off[4] == plan.tile_off[3]        # tiles 2 and 3: nobody
        for ch in (got[:N], got[N:]):
            assert not ch[4096:].any() and not np.signbit(ch[4096:]).any()
        assert N % 4 != 0


def test_cut_zeros_empty_tracks_and_no_track(ctx):
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, 3000).astype(np.float32)
    for total in (2500, 2048, 7001):                            # inside the track (cut); a whole tile; past every track (zeros)
        got, want, _ = _mix(ctx, [x, x[:0], x[:9]], [B.Track(0.0, 0.3, _ms(10)), B.Track(), B.Track(0.0, 0.0, 0.0, True)], total_out=total)
        assert _same(got, want) and len(got) == 2 * total, total
    got, want, plan = _mix(ctx, [], [], total_out=2100)         # n == 0: zeros
    assert plan.n == 0 and _same(got, want) and not got.any()
    got, _, plan = _mix(ctx, [x], [B.Track(mute=True)], total_out=9)
    assert plan.n == 0 and not got.any()
    got, _, plan = _mix(ctx, [x], [B.Track()], total_out=0)     # total_out == 0: nothing is launched
    assert len(got) == 0


def test_alignment_of_source_and_bus(ctx):
    rng = np.random.default_rng(14)
    x = rng.uniform(-1, 1, 4099).astype(np.float32)
    y = rng.uniform(-1, 1, 2600).astype(np.float32)
    for lead in (0, 1, 2, 3):
        for out_lead in (0, 1):
            for total in (4096, 4097, 4099):                    # N % 4 != 0: R's base is not 16-byte aligned
                got, want, _ = _mix(ctx, [x, y], [B.Track(0.0, -0.2), B.Track(0.0, 0.7, _ms(512 + lead))], total, lead, out_lead)
                assert _same(got, want), (lead, out_lead, total)


def test_order_of_the_sum(ctx):
    xs = [np.full(3000, 1e8, np.float32), np.ones(3000, np.float32), np.full(3000, -1e8, np.float32)]
    t = B.Track(0.0, -1.0)
    got, want, _ = _mix(ctx, xs, [t, t, t])
    assert _same(got, want) and not got.any()                   # (1e8 + 1) - 1e8 in fp32, in track order: the 1 is lost
    got, want, _ = _mix(ctx, [xs[0], xs[2], xs[1]], [t, t, t])
    assert _same(got, want) and (got[:3000] == 1.0).all()


def test_phrase_mix_and_bus_mix_agree_on_the_same_placement(ctx):
    """The two mixes stand on one walk (csrc/tile_mix.h): three signals at 0, 3 and 2050 summed by both give the same words.
    Derived, not measured: with every val 1 and distinct knots the phrase's gain is 1 + 0 * q = 1 exactly, and at 0 dB and
    pan -1 the bus has gl = 1 and gr = +0 (test_pan_law_exact_positions), so L is the phrase's track and R is +0.0f."""
    from goofer_amd import _lib
    from goofer_amd import phrase as P
    rng = np.random.default_rng(15)
    lens, starts, total = (1500, 700, 5000), (0, 3, 2050), 3 * 2048 + 5
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
    notes = np.zeros(3, dtype=_lib.PHRASE_NOTE)
    for i, (n, s) in enumerate(zip(lens, starts)):
        notes[i] = (s, 0, n, np.linspace(0, n, 7).astype(np.float32), np.ones(7, np.float32))
    pplan = P.plan_records(notes, lens, total)
    tracks = [B.Track(0.0, -1.0, _ms(s)) for s in starts]
    for lead in (0, 1):
        bus, want, plan = _mix(ctx, xs, tracks, total_out=total, lead=lead)
        track = ctx.phrase_mix(_dev(ctx, np.concatenate(xs), lead), ctx.offsets(lens), pplan)
        ctx.check()
        assert plan.total_out == total and list(plan.tracks["start"]) == list(starts) and _same(bus, want), lead
        assert _same(track.cpu().numpy(), bus[:total]) and not L.words(bus[total:]).any(), lead


def test_mix_refusals(ctx):
    from goofer_amd.device import GooferError
    lib, z = ctx.lib, C.c_void_p(0)
    x = _dev(ctx, np.ones(100, np.float32))
    plan = B.plan([x], [100], [B.Track()], 48000)
    rec, tile_off, tile_tracks = plan.device_tables(ctx)
    out = torch.full((200,), float("nan"), dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(r=p(rec), n=1, off=p(tile_off), tt=p(tile_tracks), total=100, o=p(out)):
        return lib.goofer_bus_mix(ctx.h, r, n, off, tt, total, o, None)
    for bad in (dict(r=z), dict(off=z), dict(tt=z), dict(o=z), dict(n=-1), dict(total=-1), dict(o=C.c_void_p(out.data_ptr() + 2)),
                dict(r=C.c_void_p(rec.data_ptr() + 4)), dict(total=2048 * (1 << 31))):
        assert call(**bad) == EINVAL, bad
    ctx.check()
    assert torch.isnan(out).all()                               # nothing was written
    assert call(total=0, o=z) == 0 and call() == 0
    ctx.check()
    assert not torch.isnan(out).any()
    other = _dev(ctx, np.ones(100, np.float32))
    with pytest.raises(ValueError):
        ctx.bus_mix([other], plan)                              # not the tensor the plan was made for
    with pytest.raises(ValueError):
        ctx.bus_mix([x], plan, out=out[:100])
    with pytest.raises(GooferError):
        ctx._check(call(n=-1))


# ---- limiter ---------------------------------------------------------------------------------------------------------------

PAIR_LENGTHS = (1, 4095, 4096, 4097, 9000)
LOOK_MS = {1: 0.125, 7: 0.875, 240: 30.0}                      # at 8 kHz


def _pairs():
    out = []
    for k, n in enumerate(PAIR_LENGTHS):
        out += list(R.burst_pair(n, seed=30 + k))
    return out


def _flat(xs):
    return np.concatenate([np.asarray(x, np.float32) for x in xs] + [np.zeros(1, np.float32)])


def _limit(ctx, xs, plan, prefill=None):
    x = ctx.tensor(_flat(xs))
    out = None if prefill is None else torch.full((plan.total,), prefill, dtype=torch.float32, device=ctx.device)
    y, peak, gain = ctx.limit(x, None, plan, out=out)
    ctx.check()
    y = y.cpu().numpy()
    return [y[plan.in_off[i]:plan.in_off[i + 1]] for i in range(plan.n)], peak.cpu().numpy(), gain.cpu().numpy()


@pytest.fixture(params=[1, 0], ids=["skip", "noskip"])
def skip(ctx, request):
    ctx.set_option("limit_skip", request.param)
    ctx.set_option("limit_tp_skip", request.param)
    yield request.param
    ctx.set_option("limit_skip", 1)
    ctx.set_option("limit_tp_skip", 1)


@pytest.mark.parametrize("W", R.LOOKS)
@pytest.mark.parametrize("c", R.CEILINGS, ids=["-1dB", "half", "default"])
def test_linked_limiter_against_the_restatement(ctx, W, c, skip):
    """Pairs of 1, 4095, 4096, 4097 and 9000 samples in one batch, a burst at 4090 .. 4100 in L only: R is quiet throughout and
    must equal the restatement in tiles 0 and 1 — it does not where the skip is decided per channel."""
    xs = _pairs()
    plan = LM.plan(8000, [len(x) for x in xs], c, LOOK_MS[W], channels=2)
    assert plan.W == W and plan.channels == 2 and len(plan.tiles) == 1 + 1 + 1 + 2 + 3
    ys, peak, gain = _limit(ctx, xs, plan)
    assert peak.shape == gain.shape == (len(PAIR_LENGTHS),)
    bound = float(c) * (1.0 + 2.0 ** -22)
    for g, n in enumerate(PAIR_LENGTHS):
        (wl, wr), gg, wp, wg = R.limit_linked(xs[2 * g:2 * g + 2], plan.taps, W, c)
        assert _same(ys[2 * g], wl) and _same(ys[2 * g + 1], wr), (g, n)
        assert peak[g] == wp and gain[g] == wg
        assert np.abs(ys[2 * g]).max() <= bound and np.abs(ys[2 * g + 1]).max() <= bound
        if n > 4100:
            assert float(np.abs(xs[2 * g + 1]).max()) < float(c) and gain[g] < 1.0
            hit = np.flatnonzero(gg < 1.0)
            assert hit.min() < 4096 <= hit.max() and not _same(ys[2 * g + 1][hit], xs[2 * g + 1][hit])     # the quiet channel is reduced


def test_linked_limiter_one_channel_pair_of_equals_and_alone(ctx, skip):
    xs = _pairs()
    c = np.float32(0.891)
    one = LM.plan(8000, [len(x) for x in xs], c, LOOK_MS[7])
    mono, mpeak, mgain = _limit(ctx, xs, one)
    # ch == 1 through the linked entry point: goofer_limit's bits
    x = ctx.tensor(_flat(xs))
    in_off, tiles, taps = one.device_tables(ctx)
    out = torch.empty(one.total, dtype=torch.float32, device=ctx.device)
    pk, gn = torch.empty(one.n, dtype=torch.float32, device=ctx.device), torch.empty(one.n, dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._check(ctx.lib.goofer_limit_linked(ctx.h, p(x), p(in_off), one.n, one.total, 1, one.W, p(taps), C.c_float(one.ceiling), p(tiles), one.n_tiles,
                                           p(out), p(pk), p(gn), 0, None, None))
    ctx.check()
    assert _same(out.cpu().numpy(), np.concatenate(mono)) and _same(pk.cpu().numpy(), mpeak) and _same(gn.cpu().numpy(), mgain)
    # (x, x): goofer_limit's output in both channels
    big = xs[8]
    two = LM.plan(8000, [len(big)] * 2, c, LOOK_MS[7], channels=2)
    ys, peak, gain = _limit(ctx, [big, big], two)
    assert _same(ys[0], mono[8]) and _same(ys[1], mono[8]) and peak[0] == mpeak[8] and gain[0] == mgain[8]
    # a pair alone gives the words it has as the second pair of a batch of two
    both = LM.plan(8000, [len(xs[6])] * 2 + [len(big)] * 2, c, LOOK_MS[7], channels=2)
    alone = LM.plan(8000, [len(big)] * 2, c, LOOK_MS[7], channels=2)
    yb, pb, gb = _limit(ctx, xs[6:10], both)
    ya, pa, ga = _limit(ctx, xs[8:10], alone)
    assert _same(yb[2], ya[0]) and _same(yb[3], ya[1]) and pb[1] == pa[0] and gb[1] == ga[0]
    # a group under the ceiling comes back bit for bit
    quiet = [(x * np.float32(0.5)).astype(np.float32) for x in R.burst_pair(9000, lo=9000, hi=9000)]
    yq, pq, gq = _limit(ctx, quiet, alone)
    assert _same(yq[0], quiet[0]) and _same(yq[1], quiet[1]) and gq[0] == 1.0


@pytest.mark.parametrize("sr", [48000, 96000])
def test_linked_true_peak_limiter(ctx, sr, skip):
    """R = 4 at 48 kHz, R = 2 at 96 kHz.  Pair 0: a burst whose samples stay under c in L only, R quiet.  Pair 1: the quarter-rate
    sine at 45 degrees in L, noise in R.  Bit for bit against the restatement; both outputs' true peaks, as goofer_true_peak
    reads them, stay under c (1 + DELTA_240)."""
    c = np.float32(0.891)
    rng = np.random.default_rng(40 + sr)
    n = 2 * 4096 + 300
    Lb = (0.2 * rng.uniform(-1, 1, n)).astype(np.float32)
    Lb[4090 - 18:4090 + 18] = TP.burst(c)                       # across the tile edge at 4096
    Rb = (0.2 * rng.uniform(-1, 1, n)).astype(np.float32)
    Ls = TP.burst(c, length=5000, amp=1.0 / float(c))           # unit amplitude: samples at 0.707, true peak 1.0
    Rs = (0.3 * rng.uniform(-1, 1, 5000)).astype(np.float32)
    xs = [Lb, Rb, Ls, Rs]
    plan = LM.plan(sr, [len(x) for x in xs], c, 5.0, true_peak=True, channels=2)
    assert plan.R == (4 if sr == 48000 else 2) and plan.W == sr // 200
    ys, peak, gain = _limit(ctx, xs, plan)
    meter = LM.true_peak_plan(sr, [len(x) for x in xs])
    tp_out = ctx.true_peak(ctx.tensor(_flat(ys)), None, meter).cpu().numpy()
    for g in (0, 1):
        (wl, wr), gg, wp, wg = R.limit_linked(xs[2 * g:2 * g + 2], plan.taps, plan.W, c, plan.tp_taps)
        assert _same(ys[2 * g], wl) and _same(ys[2 * g + 1], wr), g
        assert peak[g] == wp and gain[g] == wg and gain[g] < 1.0 and peak[g] > c
        print(sr, "pair", g, "true peak in %.4f, out / c - 1 = %.3e %.3e" % (peak[g], tp_out[2 * g] / float(c) - 1.0, tp_out[2 * g + 1] / float(c) - 1.0))
        assert tp_out[2 * g] <= float(c) * (1.0 + DELTA_240) and tp_out[2 * g + 1] <= float(c) * (1.0 + DELTA_240)
    assert float(np.abs(Lb).max()) < float(c) and not _same(ys[1], Rb)     # samples under c, and the quiet channel still reduced
    # ch == 1 with R: goofer_limit_tp's bits
    one = LM.plan(sr, [len(Lb)], c, 5.0, true_peak=True)
    (m,), mp, mg = _limit(ctx, [Lb], one)
    x = ctx.tensor(_flat([Lb]))
    in_off, tiles, taps = one.device_tables(ctx)
    out = torch.empty(one.total, dtype=torch.float32, device=ctx.device)
    pk, gn = torch.empty(1, dtype=torch.float32, device=ctx.device), torch.empty(1, dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx._check(ctx.lib.goofer_limit_linked(ctx.h, p(x), p(in_off), 1, one.total, 1, one.W, p(taps), C.c_float(one.ceiling), p(tiles), one.n_tiles,
                                           p(out), p(pk), p(gn), one.R, p(one.device_tp_taps(ctx)), None))
    ctx.check()
    assert _same(out.cpu().numpy(), m) and pk.cpu()[0] == mp[0] and gn.cpu()[0] == mg[0]


def test_linked_limiter_unequal_lengths_and_refusals(ctx):
    lib = ctx.lib
    xs = [np.full(5000, 2.0, np.float32), np.full(4000, 2.0, np.float32)]
    x = ctx.tensor(_flat(xs))
    grp = LM.plan(8000, [5000], 0.5, 1.0)                       # the table of the group as the longer channel would make it
    in_off = ctx.tensor(np.array([0, 5000, 9000], dtype=np.int64))
    _, tiles, taps = grp.device_tables(ctx)
    out = torch.full((9000,), float("nan"), dtype=torch.float32, device=ctx.device)
    pk, gn = torch.empty(1, dtype=torch.float32, device=ctx.device), torch.empty(1, dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=2, total=9000, ch=2, W=grp.W, c=0.5, n_tiles=grp.n_tiles, R=0, tp=None, xx=p(x), oo=p(out)):
        return lib.goofer_limit_linked(ctx.h, xx, p(in_off), n, total, ch, W, p(taps), C.c_float(c), p(tiles), n_tiles, oo, p(pk), p(gn), R, tp, None)
    assert call() == 0
    ctx.check()
    assert torch.isnan(out).all() and pk.cpu()[0] == 0.0 and gn.cpu()[0] == 1.0     # neither read nor written
    for bad in (dict(ch=0), dict(ch=3), dict(n=1), dict(n=-2), dict(total=-1), dict(W=0), dict(W=1025), dict(c=0.0), dict(c=1.5), dict(n_tiles=9),
                dict(R=3), dict(R=4), dict(xx=C.c_void_p(0)), dict(oo=p(x)), dict(oo=C.c_void_p(out.data_ptr() + 2))):
        assert call(**bad) == EINVAL, bad
    with pytest.raises(ValueError):
        LM.plan(8000, [5000, 4000], 0.5, 1.0, channels=2)


# ---- loudness --------------------------------------------------------------------------------------------------------------

def _ulp_apart(a, b):
    return abs(int(L.words(np.array([a], np.float32))[0]) - int(L.words(np.array([b], np.float32))[0]))


def _loud(ctx, xs, sr, target=-16.0, cap=20.0):
    plan = LDP.plan(sr, [len(x) for x in xs])
    y, loud, gain, seg = ctx.loudness(ctx.tensor(_flat(xs)), None, plan, target, cap, channels=2)
    ctx.check()
    seg = seg.cpu().numpy()
    Es = [seg[plan.seg_off[i]:plan.seg_off[i + 1]] for i in range(plan.n)]
    y = None if y is None else y.cpu().numpy()
    return y, loud.cpu().numpy(), gain.cpu().numpy(), Es, plan


@pytest.mark.parametrize("sr", [8000, 48000])
def test_linked_loudness(ctx, sr):
    """Per rate one batch of pairs: (a, b) of four segments and a remainder, (c, d) of five tiles, (x, 0), (x, x), a pair under
    four segments.  loud within 1e-6 of stats(E0 + E1) on the device's own energies, the gain within one fp32 ulp (the margins
    of tests/test_gpu_loudness.py), the same word for both channels."""
    S = LD.seg_len(sr)
    rng = np.random.default_rng(50 + sr)
    n4, n5 = 4 * S + S // 3, max(5 * 4096, 5 * S) + 77
    a, b = LD._noisy(rng, n4, sr, 0.5), LD._noisy(rng, n4, sr, 0.2)
    c, d = LD._noisy(rng, n5, sr, 0.3), LD._noisy(rng, n5, sr, 0.6)
    x = LD._noisy(rng, n5, sr, 0.4)
    short = LD._noisy(rng, 3 * S + 5, sr, 0.5)
    xs = [a, b, c, d, x, np.zeros_like(x), x, x, short, short]
    y, loud, gain, Es, plan = _loud(ctx, xs, sr)
    assert loud.shape == (5, 2) and loud.dtype == np.float64 and gain.shape == (10,) and plan.S == S
    for g in range(4):
        E0, E1 = Es[2 * g], Es[2 * g + 1]
        assert len(E0) == len(E1) == len(xs[2 * g]) // S >= 4
        Lw, mw, gw = R.loud_linked(E0, E1, S, -16.0, 20.0)
        assert abs(loud[g, 0] - Lw) <= 1e-6 and abs(loud[g, 1] - mw) <= 1e-6, (g, loud[g], Lw, mw)
        assert _ulp_apart(gain[2 * g], gw) <= 1 and L.words(gain[2 * g:2 * g + 1])[0] == L.words(gain[2 * g + 1:2 * g + 2])[0]
    assert loud[4, 0] == -np.inf and loud[4, 1] == -np.inf and gain[8] == 1.0 and gain[9] == 1.0      # under four segments
    for i, xi in enumerate(xs):
        assert _same(y[plan.in_off[i]:plan.in_off[i + 1]], xi * gain[i]), i
    # (x, 0) reads what x alone reads; (x, x) reads that plus 10 log10 2, given every block of x above the absolute gate
    alone = ctx.loudness(ctx.tensor(_flat([x])), None, LDP.plan(sr, [len(x)]))[1].cpu().numpy()
    ctx.check()
    assert LD.gate_classes(LD.blocks(Es[4], S))[0][0].sum() == 0
    assert abs(loud[2, 0] - alone[0, 0]) <= 1e-6 and abs(loud[2, 1] - alone[0, 1]) <= 1e-6
    up = 10.0 * np.log10(2.0)
    assert abs(loud[3, 0] - (alone[0, 0] + up)) <= 1e-6 and abs(loud[3, 1] - (alone[0, 1] + up)) <= 1e-6
    # measure only: a gain of 1 and no output
    y0, loud0, gain0, _, _ = _loud(ctx, xs[:4], sr, target=None)
    assert y0 is None and (gain0 == 1.0).all() and np.array_equal(loud0, loud[:2])


def test_linked_loudness_nan_and_mismatched_segments(ctx):
    sr, S = 8000, 800
    rng = np.random.default_rng(60)
    a, b = LD._noisy(rng, 5 * S + 3, sr, 0.5), LD.nan_signal(sr)
    c, d = LD._noisy(rng, 5 * S + 3, sr, 0.3), LD._noisy(rng, 5 * S + 3, sr, 0.2)
    y, loud, gain, Es, plan = _loud(ctx, [a, b, c, d], sr)
    y1, loud1, gain1, _, _ = _loud(ctx, [c, d], sr)
    assert np.isnan(loud[0]).all() and np.isnan(gain[:2]).all()
    assert np.array_equal(LD.words(loud[1]), LD.words(loud1[0])) and np.array_equal(L.words(gain[2:]), L.words(gain1))
    # channels that differ in segment count: NaN, NaN and a gain of 1 (the C entry point; the Python plan has no such pair)
    seg = ctx.tensor(np.ones(9, dtype=np.float64))
    seg_off = ctx.tensor(np.array([0, 5, 9], dtype=np.int64))
    lo = torch.zeros((1, 2), dtype=torch.float64, device=ctx.device)
    gn = torch.zeros(2, dtype=torch.float32, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=2, ch=2, S_=S, target=-16.0, cap=20.0, e=p(seg)):
        return ctx.lib.goofer_loudness_link(ctx.h, e, p(seg_off), n, ch, S_, target, cap, p(lo), p(gn), None)
    assert call() == 0
    ctx.check()
    assert np.isnan(lo.cpu().numpy()).all() and gn.cpu().tolist() == [1.0, 1.0]
    for bad in (dict(ch=0), dict(ch=3), dict(n=1), dict(n=-2), dict(S_=10), dict(target=float("inf")), dict(cap=-1.0), dict(cap=61.0), dict(e=C.c_void_p(0))):
        assert call(**bad) == EINVAL, bad
    # ch == 1 on the same energies: k_loud_stats' own numbers
    yo, loud_o, gain_o, seg_o = ctx.loudness(ctx.tensor(_flat([c])), None, LDP.plan(sr, [len(c)]), -16.0)
    lo1, gn1 = torch.zeros((1, 2), dtype=torch.float64, device=ctx.device), torch.zeros(1, dtype=torch.float32, device=ctx.device)
    so = ctx.tensor(np.array([0, seg_o.numel()], dtype=np.int64))
    assert ctx.lib.goofer_loudness_link(ctx.h, p(seg_o), p(so), 1, 1, S, -16.0, 20.0, p(lo1), p(gn1), None) == 0
    ctx.check()
    assert torch.equal(lo1, loud_o) and torch.equal(gn1, gain_o)


# ---- pcm16 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 4097])
def test_pcm16_planar(ctx, n):
    rng = np.random.default_rng(70 + n)
    x = rng.uniform(-1.3, 1.3, 2 * n).astype(np.float32)
    special = np.array([1.0, -1.0, 1.0 - 2.0 ** -15, 1.5, -1.5, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768], np.float32)
    k = min(n, len(special))
    x[:k], x[n:n + k] = special[:k], special[::-1][:k]
    for lead in (0, 1):
        d = _dev(ctx, x, lead)
        out = ctx.pcm16(d, channels=2)
        ctx.check()
        assert out.shape == (n, 2) and out.dtype == torch.int16
        assert np.array_equal(out.cpu().numpy(), R.pcm16_planar(x)), (n, lead)
    d = _dev(ctx, x)
    mono = ctx.pcm16(d).cpu().numpy()
    one = torch.empty(2 * n, dtype=torch.int16, device=ctx.device)
    ctx._check(ctx.lib.goofer_pcm16_planar(ctx.h, C.c_void_p(d.data_ptr()), 2 * n, 1, C.c_void_p(one.data_ptr()), None))
    ctx.check()
    assert np.array_equal(one.cpu().numpy(), mono) and np.array_equal(mono, L.pcm16(x))
    assert ctx.lib.goofer_pcm16_planar(ctx.h, C.c_void_p(d.data_ptr()), n, 3, C.c_void_p(one.data_ptr()), None) == EINVAL
    with pytest.raises(ValueError):
        ctx.pcm16(_dev(ctx, x[:2 * n - 1]), channels=2)


# ---- end to end ------------------------------------------------------------------------------------------------------------

REQUESTS = [("C4", "100", "g-10", "30", "300", "80", "50", "100", "0", "!120", "AA"),
            ("E4", "100", "B30", "30", "300", "80", "50", "90", "0", "!120", "AA#20#AP"),
            ("G4", "80", "t10", "30", "300", "80", "50", "100", "0", "!120", "AA"),
            ("A3", "120", "g5", "30", "300", "80", "50", "100", "0", "!120", "AA"),
            ("D4", "100", "B40", "30", "300", "80", "50", "100", "0", "!120", "AA")]
TOOL = ["0 250 5 35 40 0 100 100 0", "0 240@120 5 35 40 0 100 100 0 30", "4 200 5 35 40 0 100 100 0 25"]


@pytest.fixture(scope="module")
def song(ctx):
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Renderer, Source
    jobs = []
    for i, args in enumerate(REQUESTS):
        src = syn.make_source(400 + i, seconds=0.3)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]), S.decode_request(*args)))
    tracks = [(jobs[:2], TOOL[:2], B.Track(-3.0, -0.5)), (jobs[2:], TOOL, B.Track(0.0, 0.5, 100.0, eq="hp:120"))]
    return Renderer(ctx), tracks


def test_render_song_is_the_chain_made_by_hand(ctx, song):
    r, tracks = song
    limit = (0.891, 5.0, True)
    got, st = r.render_song(tracks, seed=7, out_sr=48000, loudness=-16, limit=limit, return_stats=True)
    got16 = r.render_song(tracks, seed=7, pcm16=True, out_sr=48000, loudness=-16, limit=limit)
    xs = [r.render_phrase(jobs, entries, seed=7 + k, out_sr=48000, eq=t.eq) for k, (jobs, entries, t) in enumerate(tracks)]
    ds = [ctx.tensor(x) for x in xs]
    plan = B.plan(ds, [len(x) for x in xs], [t for _, _, t in tracks], 48000)
    N = plan.total_out
    assert N == max(len(xs[0]), 4800 + len(xs[1])) and got.shape == (N, 2) and got.dtype == np.float32
    bus = ctx.bus_mix(ds, plan)
    assert _same(bus.cpu().numpy(), R.mix(xs, [(B.samples(t.start_ms, 48000),) + R.gains(t.gain_db, t.pan) for _, _, t in tracks], N))
    bus, loud, gain, _ = ctx.loudness(bus, None, LDP.plan(48000, [N, N]), -16.0, channels=2)
    lplan = LM.plan(48000, [N, N], *limit, channels=2)
    y, peak, gmin = ctx.limit(bus, None, lplan)
    tp_out = ctx.true_peak(y, None, LM.true_peak_plan(48000, [N, N]))
    want16 = ctx.pcm16(y, channels=2)
    ctx.check()
    y = y.cpu().numpy()
    assert _same(got[:, 0], y[:N]) and _same(got[:, 1], y[N:]) and np.array_equal(got16, want16.cpu().numpy()) and got16.dtype == np.int16
    assert st == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "true_peak_in": float(peak.cpu()[0]),
                  "true_peak_out": float(tp_out.cpu().max()), "lufs_in": float(loud.cpu()[0, 0]), "momentary_max": float(loud.cpu()[0, 1]),
                  "gain": float(gain.cpu()[0])}
    assert np.isfinite(st["lufs_in"]) and float(np.abs(got).max()) > 0.01
    with pytest.raises(ValueError):
        r.render_song(tracks, return_stats=True)
    with pytest.raises(ValueError):
        r.render_song([(tracks[0][0], tracks[0][1], B.Track(mute=True))])


def test_one_track_in_the_middle_and_core_bus_mix(ctx, song):
    from goofer_amd import core
    r, tracks = song
    jobs, entries, _ = tracks[0]
    x = r.render_phrase(jobs, entries, seed=3)
    got = r.render_song([(jobs, entries, B.Track()), (tracks[1][0], tracks[1][1], B.Track(mute=True))], seed=3)
    m = np.float32(np.sqrt(0.5))
    assert got.shape == (len(x), 2) and _same(got[:, 0], x * m) and _same(got[:, 1], x * m)
    frames, stats = core.bus_mix([x, x[:1000]], 44100, [B.Track(-3.0, -1.0), (0.0, 1.0, 10.0)], loudness=-20.0, limit=0.5, ctx=ctx)
    assert frames.shape == (len(x), 2) and set(stats) == {"lufs_in", "momentary_max", "gain", "peak_in", "min_gain"}
    assert float(np.abs(frames).max()) <= 0.5 * (1.0 + 2.0 ** -22) and not frames[:441, 1].any() and frames[441:1441, 1].any()


def test_song_file_front_end(ctx, song, tmp_path):
    """python -m goofer_amd.bus song.txt out.wav (its main(), in process): two channels, 16 bits, the rate, the frame count, and
    the interleaved int16 of render_song for the same tracks."""
    from goofer_amd import core
    from goofer_amd import phrase as P
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Source
    r, _ = song
    for i in range(2):
        src = syn.make_source(500 + i, seconds=0.3)
        core.save_features(tmp_path / f"v{i}_features.goofy", src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
    res = [" ".join(a) for a in REQUESTS[:3]]
    for name, which in (("lead.txt", [0, 1]), ("harm.txt", [1, 0, 1])):
        (tmp_path / name).write_text("".join(f"{tmp_path}/v{w}.wav {tmp_path}/n{k}.wav {res[k]} | {TOOL[k]}\n" for k, w in enumerate(which)))
    song_txt = tmp_path / "song.txt"
    song_txt.write_text("# two tracks and a muted one\nlead.txt -3 -0.5\nharm.txt 0 0.5 100 eq=hp:120\nlead.txt 0 0 0 mute\n")
    out = tmp_path / "out.wav"
    stats = {}
    bus = B.render_file(song_txt, out, renderer=r, seed=9, out_sr=48000, loudness=-16.0, limit=LM.Limiter(0.891, true_peak=True), stats=stats)
    tracks = []
    for job, t in B.read_song(song_txt):
        tracks.append(([], [], t) if t.mute else P.load_job(job, r) + (t,))
    want = r.render_song(tracks, seed=9, pcm16=True, out_sr=48000, loudness=-16.0, limit=LM.Limiter(0.891, true_peak=True))
    assert bus.dtype == np.int16 and bus.shape == want.shape and np.array_equal(bus, want) and int(np.abs(want.astype(np.int32)).max()) > 30
    assert {"lufs_in", "gain", "peak_in", "min_gain", "true_peak_in", "true_peak_out"} <= set(stats)
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, 48000, len(want))
        assert w.readframes(len(want)) == want.astype("<i2").tobytes()
    assert B.main(["--rate", "48000", "--loudness", "-16", "--limit", "-1", "--true-peak", str(song_txt), str(tmp_path / "cli.wav")]) == 0
    with wave.open(str(tmp_path / "cli.wav"), "rb") as w:
        assert (w.getnchannels(), w.getframerate(), w.getnframes()) == (2, 48000, len(want))
    assert B.main([str(tmp_path / "missing.txt"), str(out)]) == 1
