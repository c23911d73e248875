"""GPU: the convolution reverb (goofer_reverb, goofer_reverb_ir, csrc/reverb.hip) against the numpy restatement
(tests/reverb_ref.py).

The bound is the definition's: |y[i] - ref[i]| <= TOL max |ref| per signal, ref the float64 restatement and TOL = 2^-19, four
times what a float32 model of the kernels' scheme loses on these very cases (tests/test_reverb_ref.py).  The kernels cut a signal
into blocks of B = 1024 samples counted from its own start, the impulse response into partitions of B taps, and give a workgroup
runs of 32 blocks; so the lengths sit around a block, the impulse responses around one, two and three partitions, the pre-delays
around a block, and two cases have more partitions than a run has blocks: 41, and all 256."""
import ctypes as C
import math

import numpy as np
import pytest

import reverb_ref as R
from goofer_amd import reverb as RV

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, TOL = R.B, R.TOL


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _db(g):
    return -math.inf if g == 0.0 else 20.0 * math.log10(g)


def _reverb(h, pre=0, tail=True, dry=1.0, wet=1.0, sr=48000):
    """the settings with the pre-delay in samples and the gains linear, as the restatement takes them"""
    rv = RV.Reverb(h, wet_db=_db(wet), dry_db=_db(dry), predelay_ms=1000.0 * pre / sr, tail=tail)
    assert rv.predelay(sr) == pre
    return rv


def _run(ctx, xs, rv, sr=48000):
    """the kernels on the signals xs (fp32 arrays on the host) -> (the outputs, the plan)"""
    plan = RV.plan(sr, [len(x) for x in xs], rv)
    x = ctx.tensor(np.concatenate(list(xs) + [np.zeros(1, np.float32)]))[:plan.total]      # (never an empty tensor)
    y = ctx.reverb(x, None, plan, rv.spectra(ctx, sr))
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == (plan.total_out,) and (y.numel() == 0 or y.data_ptr() != x.data_ptr())
    y = y.cpu().numpy()
    return [y[plan.out_off[i]:plan.out_off[i + 1]] for i in range(plan.n)], plan


def _same(a, b):
    return a.shape == b.shape and np.array_equal(R.words(a), R.words(b))


@pytest.mark.parametrize("L", R.IR_LENGTHS)
def test_batch_against_the_restatement(ctx, L):
    xs, h = R.signals(), R.ir(L)
    assert [len(x) for x in xs] == [0, 1, B - 1, B, B + 1, 3 * B + 17, 700] and (L + B - 1) // B == {1: 1, B: 1, B + 1: 2, 2 * B + 5: 3}[L]
    worst = 0.0
    for pre in R.PREDELAYS:
        for tail in (True, False):
            ys, plan = _run(ctx, xs, _reverb(h, pre, tail, R.DRY, R.WET))
            out_off, blk_off, runs = R.tables([len(x) for x in xs], L, pre, tail)
            assert np.array_equal(plan.out_off, out_off) and np.array_equal(plan.blk_off, blk_off) and np.array_equal(plan.runs, runs)
            for i, (x, y) in enumerate(zip(xs, ys)):
                ref = R.reference(x, h, pre, tail, R.DRY, R.WET)
                assert y.dtype == np.float32 and len(y) == len(ref) == (0 if len(x) == 0 else len(x) + (pre + L - 1 if tail else 0)), (pre, tail, i)
                e = R.error(y, ref)
                worst = max(worst, e)
                assert e <= TOL, (L, pre, tail, i, e)
    print("L = %d: worst max|y - ref| / max|ref| = %.3e = 2^%.2f (TOL 2^-19)" % (L, worst, math.log2(max(worst, 1e-300))))


@pytest.mark.parametrize("pre", R.IMPULSE_PRE)
def test_an_impulse_at_every_block_edge(ctx, pre):
    """a unit sample at q, dry 0, wet 1: the output is h shifted to q + pre, zero elsewhere — the overlap-save indexing"""
    h = R.ir(R.IMPULSE_LEN)
    peak = float(np.max(np.abs(h)))
    xs = [R.impulse(q) for q in R.IMPULSE_AT]
    ys, plan = _run(ctx, xs, _reverb(h, pre, True, 0.0, 1.0))
    for q, y in zip(R.IMPULSE_AT, ys):
        want = np.zeros(R.IMPULSE_LEN + pre + len(h) - 1)
        want[q + pre:q + pre + len(h)] = h
        assert len(y) == len(want)
        assert np.max(np.abs(y - want)) <= TOL * peak, (pre, q, int(np.argmax(np.abs(y - want))))


def test_more_partitions_than_a_run_has_blocks_and_the_most_there_are(ctx):
    (x1, h1), (x2, h2) = R.long_cases()
    assert len(h1) == 40 * B + 3 and len(x1) == 8 * B and len(h2) == 2 ** 18 and len(x2) == 2000
    for x, h, blocks in ((x1, h1, 49), (x2, h2, 258)):
        (y,), plan = _run(ctx, [x], _reverb(h))
        assert plan.total_blocks == blocks and plan.n_runs == (blocks + 31) // 32
        e = R.error(y, R.reference(x, h))
        print("L = %d over %d samples: %.3e = 2^%.2f (TOL 2^-19)" % (len(h), len(x), e, math.log2(e)))
        assert e <= TOL


def test_dead_partitions_are_skipped_to_the_same_bits(ctx):
    h = R.ir(5 * B)
    h[B:2 * B] = 0.0
    h[3 * B:4 * B] = 0.0
    rv = _reverb(h, 3, True, R.DRY, R.WET)
    live = rv.spectra(ctx, 48000)[RV.IR_HEAD - 256:RV.IR_HEAD].cpu().numpy()
    assert live[:5].tolist() == [1, 0, 1, 0, 1] and not live[5:].any()
    xs = R.signals()
    on, _ = _run(ctx, xs, rv)
    ctx.set_option("reverb_skip", 0)
    try:
        off, _ = _run(ctx, xs, rv)
    finally:
        ctx.set_option("reverb_skip", 1)
    for i, (a, b, x) in enumerate(zip(on, off, xs)):
        assert _same(a, b), i
        assert R.error(a, R.reference(x, h, 3, True, R.DRY, R.WET)) <= TOL


def test_a_dead_partition_among_seventy(ctx):
    """More than 64 partitions take the kernel's other shape, whose steady rows go through a register ring when every partition
    takes part and through the tested path when one is dead: 70 partitions, number 33 all zero, with the skip (tested path) and
    without (ring) give the same bits; so does an impulse response without a dead partition, which takes the ring either way."""
    x, h = R.dead_case()
    full, _ = _run(ctx, x, _reverb(R.ir(69 * B + 11, 3), 2, True, R.DRY, R.WET))
    rv = _reverb(h, 2, True, R.DRY, R.WET)
    live = rv.spectra(ctx, 48000)[RV.IR_HEAD - 256:RV.IR_HEAD].cpu().numpy()
    assert live[:70].tolist() == [1] * 33 + [0] + [1] * 36 and not live[70:].any()
    on, _ = _run(ctx, x, rv)
    ctx.set_option("reverb_skip", 0)
    try:
        off, _ = _run(ctx, x, rv)
    finally:
        ctx.set_option("reverb_skip", 1)
    for i, (a, b, c, xi) in enumerate(zip(on, off, full, x)):
        assert _same(a, b), i
        assert not _same(a, c)
        assert R.error(a, R.reference(xi, h, 2, True, R.DRY, R.WET)) <= TOL, i


def test_alone_in_a_batch_and_again_give_the_same_bits_and_a_nan_stays_at_home(ctx):
    xs, h = R.signals(), R.ir(2 * B + 5)
    rv = _reverb(h, B + 3, True, R.DRY, R.WET)
    ys, _ = _run(ctx, xs, rv)
    again, _ = _run(ctx, xs, rv)
    for i, x in enumerate(xs):
        assert _same(again[i], ys[i]), i
        if len(x):
            assert _same(_run(ctx, [x], rv)[0][0], ys[i]), i
    order = [5, 0, 6, 3, 2]
    got, _ = _run(ctx, [xs[i] for i in order], rv)
    for j, i in enumerate(order):
        assert _same(got[j], ys[i]), i
    for i, at in ((5, B + 7), (3, 0), (1, 0)):
        bad = [x.copy() for x in xs]
        bad[i][at] = np.nan
        got, _ = _run(ctx, bad, rv)
        assert np.isnan(got[i]).any()
        for j in range(len(xs)):
            if j != i:
                assert _same(got[j], ys[j]), (i, j)


def test_wet_zero_copies_and_zeros_give_zeros(ctx):
    xs, h = R.signals(), R.ir(B + 1)
    odd = np.array([0.0, -0.0, 1e-45, -1e-40, 3.4e38, -1.0], dtype=np.float32)             # denormals and signed zeros too
    xs = xs + [odd]
    calls = []
    reverb_ir = ctx.reverb_ir
    ctx.reverb_ir = lambda taps: calls.append(len(taps)) or reverb_ir(taps)
    try:
        ys, plan = _run(ctx, xs, RV.Reverb(h, wet_db=-math.inf, dry_db=0.0, predelay_ms=0.25))
    finally:
        del ctx.reverb_ir
    assert plan.wet == 0.0 and plan.dry == 1.0 and plan.pre == 12 and not calls          # no transform, not even the IR's
    for x, y in zip(xs, ys):
        assert len(y) == (len(x) + 12 + B if len(x) else 0)
        assert _same(y[:len(x)], x) and _same(y[len(x):], np.zeros(len(y) - len(x), np.float32))      # bit for bit; the tail +0
    ys, _ = _run(ctx, xs[:7], RV.Reverb(h, wet_db=-math.inf, dry_db=-6.0, tail=False))
    for x, y in zip(xs, ys):
        assert _same(y, (np.float32(10.0 ** (-6.0 / 20.0)) * x).astype(np.float32))
    for rv in (_reverb(h, 5, True, R.DRY, R.WET), _reverb(R.ir(2 * B + 5), 0, False, 1.0, 1.0)):
        ys, _ = _run(ctx, [np.zeros(n, np.float32) for n in (1, B, 3 * B + 17)], rv)
        assert all(len(y) and not y.any() for y in ys)                                   # compares equal to 0 everywhere


def test_refusals(ctx):
    from goofer_amd import core
    from goofer_amd.device import GooferError
    sr, h = 48000, R.ir(B + 1)
    rv = _reverb(h, 7, True, R.DRY, R.WET)
    plan = RV.plan(sr, [100, 5000], rv)
    ir = rv.spectra(ctx, sr)
    assert plan.total_out == 5100 + 2 * (7 + B) and ir.dtype == torch.uint8 and ir.numel() == RV.ir_bytes(B + 1) == 12800 + 2 * 8192
    x = ctx.tensor(np.zeros(8000, np.float32))
    n_out = plan.total_out
    for bad in (dict(x=x[:5099]), dict(x=x.double()), dict(x=x[::2]), dict(out=x[:5100]), dict(out=torch.zeros(n_out, dtype=torch.float64, device=x.device)),
                dict(d_off=[0, 100, 5099]), dict(d_off=ctx.tensor(plan.in_off)[:2]), dict(d_off=ctx.tensor(plan.in_off).int()),
                dict(ir=None), dict(ir=ir[:-1]), dict(ir=ir.float()), dict(ir=ir.cpu())):
        args = dict(x=x, d_off=None, out=None, ir=ir)
        args.update(bad)
        with pytest.raises(ValueError):
            ctx.reverb(args["x"], args["d_off"], plan, args["ir"], out=args["out"])
    with pytest.raises(GooferError, match="overlaps"):
        ctx.reverb(x, None, plan, ir, out=x[100:100 + n_out])                  # the library's to refuse
    with pytest.raises(GooferError, match="overlaps"):
        ctx.reverb(x[:5100], None, plan, ir, out=x[:n_out])
    y = ctx.reverb(x, ctx.tensor(plan.in_off), plan, ir, out=torch.ones(n_out, dtype=torch.float32, device=x.device))
    assert y.shape == (n_out,) and not y.any()
    assert ctx.reverb(x, None, RV.plan(sr, [0, 0, 0], rv), ir).numel() == 0   # signals without a sample
    assert ctx.reverb(x, None, RV.plan(sr, [], rv), ir).numel() == 0
    # the C ABI: x at 0, out at 64 KiB, tables behind, scratch at 256 KiB of a zeroed block
    lib, size = ctx.lib, C.c_int64(1 << 20)
    big = ctx.tensor(np.zeros(1 << 19, np.float32))
    p = C.c_void_p(big.data_ptr())
    o, tb, sc = (C.c_void_p(big.data_ptr() + k * 65536) for k in (1, 3, 4))
    irp = C.c_void_p(ir.data_ptr())
    L, blocks, runs = B + 1, plan.total_blocks, plan.n_runs
    assert (blocks, runs) == (8, 2)                                         # 1131 and 6031 samples: 2 + 6 blocks, a run each

    def rvb(n=2, total=5100, irp=irp, L=L, pre=7, tail=1, dry=0.75, wet=0.5, off=tb, ooff=tb, boff=tb, blocks=blocks, rt=tb, runs=runs,
            total_out=n_out, xp=p, out=o, scratch=sc):
        return lib.goofer_reverb(ctx.h, xp, off, n, total, irp, L, pre, tail, C.c_float(dry), C.c_float(wet), ooff, boff, blocks, rt, runs,
                                 total_out, out, scratch, C.byref(size), None)
    plus = lambda q, k: C.c_void_p(q.value + k)
    for bad in (dict(L=0), dict(L=2 ** 18 + 1), dict(pre=-1), dict(pre=2 ** 16 + 1), dict(dry=math.nan), dict(dry=math.inf), dict(wet=math.nan),
                dict(wet=-math.inf), dict(n=-1), dict(total=-1), dict(runs=-1), dict(runs=0), dict(runs=4), dict(blocks=6), dict(blocks=10),
                dict(total_out=5099), dict(total_out=n_out + 1), dict(tail=0), dict(xp=None), dict(off=None), dict(ooff=None), dict(boff=None),
                dict(rt=None), dict(out=None), dict(irp=None), dict(xp=plus(p, 2)), dict(out=plus(o, 2)), dict(rt=plus(tb, 2)),
                dict(off=plus(tb, 4)), dict(ooff=plus(tb, 4)), dict(boff=plus(tb, 4)), dict(irp=plus(irp, 4)), dict(scratch=plus(sc, 4)),
                dict(out=p), dict(out=plus(p, 4 * 5099)), dict(xp=plus(o, 4 * (n_out - 1)))):
        assert rvb(**bad) == -1, bad
        assert b"goofer_reverb" in lib.goofer_last_error(ctx.h), bad
    assert rvb(out=plus(p, 4)) == -1 and b"overlaps" in lib.goofer_last_error(ctx.h)
    need = C.c_int64(0)
    assert lib.goofer_reverb(ctx.h, None, None, 2, 5100, None, L, 7, 1, C.c_float(0.75), C.c_float(0.5), None, None, blocks, None, runs, n_out,
                             None, None, C.byref(need), None) == 0 and need.value == 2 * blocks * B * 8        # the query: 16 bytes a block sample
    assert lib.goofer_reverb(ctx.h, p, tb, 2, 5100, irp, L, 7, 1, C.c_float(0.75), C.c_float(0.5), tb, tb, blocks, tb, runs, n_out, o, sc, None,
                             None) == -1                                                                       # no scratch_bytes
    size = C.c_int64(need.value - 1)
    assert rvb() == -1 and b"scratch" in lib.goofer_last_error(ctx.h)
    size = C.c_int64(1 << 20)
    assert rvb(n=0, total=0, total_out=0, blocks=0, runs=0, xp=None, off=None, ooff=None, boff=None, rt=None, out=None) == 0   # nothing to do
    assert rvb(total=0, total_out=0, blocks=0, runs=0, xp=None, rt=None, out=None) == 0
    # the IR's entry point
    buf = torch.zeros(RV.ir_bytes(L), dtype=torch.uint8, device=x.device)
    hp = h.ctypes.data_as(C.c_void_p)
    nan = h.copy()
    nan[77] = np.nan
    for args in ((hp, 0, buf.data_ptr(), buf.numel()), (hp, 2 ** 18 + 1, buf.data_ptr(), buf.numel()), (None, L, buf.data_ptr(), buf.numel()),
                 (hp, L, None, buf.numel()), (hp, L, buf.data_ptr(), buf.numel() - 1), (hp, L, buf.data_ptr() + 4, buf.numel()),
                 (nan.ctypes.data_as(C.c_void_p), L, buf.data_ptr(), buf.numel())):
        assert lib.goofer_reverb_ir(ctx.h, args[0], args[1], None if args[2] is None else C.c_void_p(args[2]), args[3], None) == -1, args
        assert b"goofer_reverb_ir" in lib.goofer_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not big.any() and not buf.any()                                     # nothing was launched
    # the same through Python
    for bad_h in (np.zeros(0, np.float32), nan, np.zeros(2 ** 18 + 1, np.float32)):
        with pytest.raises(ValueError):
            ctx.reverb_ir(bad_h)
    for bad_sr, rvs in ((7999, (h,)), (192001, (h,)), (48000.5, (h,)), (sr, (nan,)), (sr, (h, math.nan)), (sr, (h, -6, math.inf)),
                        (sr, (h, -6, 0, 1000.0 * (2 ** 16 + 1) / sr)), (sr, (h, -6, 0, -1.0)), (sr, "room:6"), (sr, "hall:1")):
        with pytest.raises(ValueError):
            core.reverb_batch([np.zeros(10)], bad_sr, rvs, ctx=ctx)


def test_reverb_batch(ctx):
    from goofer_amd import core
    xs, h = R.signals(), R.ir(2 * B + 5)
    rv = RV.Reverb(h, wet_db=-9.0, dry_db=-1.0, predelay_ms=2.0)
    got = core.reverb_batch(xs, 48000, rv, ctx=ctx)
    assert len(got) == len(xs)
    for x, y in zip(xs, got):
        ref = R.reference(x, h, 96, True, rv.dry, rv.wet)
        assert y.dtype == np.float32 and len(y) == len(ref) and R.error(y, ref) <= TOL
    assert all(_same(a, b) for a, b in zip(core.reverb_batch([x.astype(np.float64) for x in xs], 48000, (h, -9, -1, 2.0), ctx=ctx), got))
    room = core.reverb_batch(xs[2:4], 48000, "room:0.05:-6:1:3", ctx=ctx)
    hr = RV.synthetic_ir(48000, RV.Room(0.05, 3))
    for x, y in zip(xs[2:4], room):
        assert R.error(y, R.reference(x, hr, 48, True, 1.0, 10.0 ** (-6.0 / 20.0))) <= TOL
    assert core.reverb_batch([], 48000, rv, ctx=ctx) == []
    assert [len(y) for y in core.reverb_batch([np.zeros(0), np.zeros(0)], 48000, rv, ctx=ctx)] == [0, 0]


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


def test_render_phrase_with_reverb_is_the_chain_done_by_hand(ctx, monkeypatch):
    from goofer_amd import compress as CP
    from goofer_amd import core
    from goofer_amd import eq as EQ
    from goofer_amd import limit as LM
    from goofer_amd import loudness as LD
    from goofer_amd import rate as RT
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    rv = RV.Reverb(RV.Room(0.2, 4, 6000.0), wet_db=-8.0, predelay_ms=10.0)
    plain = r.render_phrase(jobs, entries, seed=5)                            # phrase_mix's track, no stage behind it
    # mix, convert, eq, compress, reverb, loudness, limit, int16
    conv = ctx.rate_convert(ctx.tensor(plain), None, RT.plan(44100, 48000, [len(plain)]))
    n = conv.numel()
    flt = ctx.eq(conv, None, EQ.plan(48000, [n], "hp:80"))
    cmp_, red, _ = ctx.compress(flt, None, CP.plan(48000, [n], "-30:4"))
    plan = RV.plan(48000, [n], rv)
    assert plan.L == 9600 and plan.pre == 480 and plan.total_out == n + 480 + 9600 - 1
    wet = ctx.reverb(cmp_, None, plan, rv.spectra(ctx, 48000))
    m = wet.numel()
    y, loud, gain, _ = ctx.loudness(wet, None, LD.plan(48000, [m]), -16.0)
    lim, peak, gmin = ctx.limit(y, None, LM.plan(48000, [m], 0.5))
    want = ctx.pcm16(lim).cpu().numpy()
    got, st = r.render_phrase(jobs, entries, seed=5, out_sr=48000, eq="hp:80", compress="-30:4", reverb=rv, loudness=-16, limit=0.5,
                              return_stats=True, pcm16=True)
    assert got.dtype == np.int16 and len(got) == m and np.array_equal(got, want)
    assert st == {"peak_in": float(peak.cpu()[0]), "min_gain": float(gmin.cpu()[0]), "lufs_in": float(loud.cpu()[0, 0]),
                  "momentary_max": float(loud.cpu()[0, 1]), "gain": float(gain.cpu()[0]), "max_reduction_db": float(red.cpu()[0])}
    # the reverb alone, at the notes' own rate: the track is pre + L - 1 samples longer; the forms are one setting
    p44 = RV.plan(44100, [len(plain)], rv)
    alone = ctx.reverb(ctx.tensor(plain), None, p44, rv.spectra(ctx, 44100)).cpu().numpy()
    assert len(alone) == len(plain) + p44.pre + p44.L - 1 and p44.L == 8820 and p44.pre == 441
    assert _same(r.render_phrase(jobs, entries, seed=5, reverb=rv), alone)
    assert _same(r.render_phrase(jobs, entries, seed=5, reverb=(RV.Room(0.2, 4, 6000.0), -8.0, 0.0, 10.0)), alone)
    assert R.error(alone, R.reference(plain, rv.taps(44100), 441, True, 1.0, rv.wet)) <= TOL
    short = r.render_phrase(jobs, entries, seed=5, reverb=RV.Reverb(rv.ir, wet_db=-8.0, predelay_ms=10.0, tail=False))
    assert len(short) == len(plain) and _same(short, alone[:len(plain)])
    # the IR's spectra are kept per device and rate on the Reverb: further calls compute none
    calls = []
    reverb_ir = Context.reverb_ir
    monkeypatch.setattr(Context, "reverb_ir", lambda self, taps: calls.append(len(taps)) or reverb_ir(self, taps))
    assert _same(r.render_phrase(jobs, entries, seed=5, reverb=rv), alone) and not calls
    assert len(r.render_phrase(jobs, entries, seed=5, reverb="room:0.1:-10")) == len(plain) + 4410 - 1 and calls == [4410]
    monkeypatch.setattr(Context, "reverb_ir", reverb_ir)
    with pytest.raises(ValueError):
        r.render_phrase(jobs, entries, seed=5, reverb=rv, return_stats=True)   # the stage has no statistic
    for bad in ("room:0", "hall:1", (np.zeros(0),), "room:7", RV.Reverb(R.ir(10), predelay_ms=2000.0), RV.Reverb(R.ir(10), ir_sr=48000)):
        with pytest.raises(ValueError):
            r.render_phrase(jobs, entries, seed=5, reverb=bad)
        with pytest.raises(ValueError):
            r.render(jobs, seed=5, reverb=bad)
    # render: every note through the same room, the batch in one pass, each note longer by the tail
    notes = r.render(jobs, seed=5)
    wet_notes = r.render(jobs[:2], seed=5, reverb=rv)
    assert [len(a) for a in wet_notes] == [len(c) + 441 + 8820 - 1 for c in notes[:2]]
    for a, c in zip(wet_notes, core.reverb_batch(r.render(jobs[:2], seed=5), 44100, rv, ctx=ctx)):
        assert _same(a, c)
    # reverb None: the bits of a call without the keyword, and Context.reverb never runs
    track48 = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    pcm_plain = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    full, st_full = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress="-30:4", loudness=-16, limit=0.5, return_stats=True)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("reverb reached")
    monkeypatch.setattr(Context, "reverb", never)
    monkeypatch.setattr(Context, "reverb_ir", never)
    assert _same(r.render_phrase(jobs, entries, seed=5, reverb=None), plain)
    assert _same(r.render_phrase(jobs, entries, seed=5, out_sr=48000, reverb=None), track48)
    assert np.array_equal(r.render_phrase(jobs, entries, seed=5, pcm16=True, reverb=None), pcm_plain)
    got, st2 = r.render_phrase(jobs, entries, seed=5, out_sr=48000, compress="-30:4", loudness=-16, limit=0.5, return_stats=True, reverb=None)
    assert _same(got, full) and st2 == st_full
    for a, c in zip(r.render(jobs, seed=5, reverb=None), notes):
        assert _same(a, c)
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, reverb=rv)
    assert len(calls) == 1


def test_job_file_front_end_with_reverb(ctx, tmp_path, capsys, monkeypatch):
    """python -m goofer_amd.phrase --reverb SPEC job.txt out.wav (its main(), in process; the seed it would draw pinned): the wav is
    render_phrase(reverb=...)'s int16 track, for a synthetic room and for a wav the test writes; the IR's length and the tail go
    to stderr; a malformed SPEC is the usage error."""
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
    plain = render_job(str(job), str(tmp_path / "plain.wav"), seed=11)
    irwav = tmp_path / "ir.wav"
    h = (0.9 * R.ir(3000)).astype(np.float32)
    with wave.open(str(irwav), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(44100)
        w.writeframes(np.round(h * 32767.0).astype("<i2").tobytes())
    for spec, taps, pre in (("room:0.3:-10:5:7", 13230, 221), (f"ir:{irwav}:-9:2", 3000, 88)):
        out = tmp_path / "rv.wav"
        assert P.main(["--reverb", spec, str(job), str(out)]) == 0
        err = capsys.readouterr().err
        assert "Reverb: impulse response of %d taps" % taps in err and "the tail adds %d samples" % (pre + taps - 1) in err
        with wave.open(str(out), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 44100)
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        want = render_job(str(job), str(tmp_path / "want.wav"), seed=11, reverb=RV.parse(spec))
        assert want.dtype == np.int16 and np.array_equal(pcm, want) and len(pcm) == len(plain) + pre + taps - 1
        assert not np.array_equal(pcm[:len(plain)], plain)
    assert P.main(["--rate", "48000", "--eq", "hp:80", "--compress", "-30:4", "--reverb", "room:0.2", "--limit", "-1", str(job), str(out)]) == 0
    assert "impulse response of 9600 taps" in capsys.readouterr().err
    assert P.main(["--rate", "48000", "--reverb", f"ir:{irwav}", str(job), str(out)]) == 1          # a wav at another rate than the output's
    capsys.readouterr()
    for bad in ("room", "room:fast", "hall:1", "room:0.3:-10:5:7:9", f"ir:{tmp_path}/none.wav"):
        assert P.main(["--reverb", bad, str(job), str(out)]) == 1
