"""GPU: output-rate conversion (goofer_rate_convert, csrc/rate.hip) against its numpy restatement (tests/rate_ref.py), on the
library's own tap table.

The fp32 restatement performs the definition's arithmetic — one rounded multiply and one rounded add per tap, ascending j —
so the kernel is held to it bit for bit, compared as int32 words.  Against the float64 restatement the tolerance is derived,
not measured: per sample |got - ref| <= (2H + 1) * 2^-24 * sum_j |h_p[j] x[q + j]|, one rounding per product and one per add.

The kernel gives a wave 64 consecutive output samples and a workgroup 1024 (the tap table in LDS) or 256 (a table that does not
fit there, or option "rate_lds" 0), and its fixed grid walks longer batches with a stride of 524 288 samples: those are the
tile edges the lengths below are placed on.  The first output of a signal in a tile has its (q, p) from a 32-bit division
where k M < 2^32 and from a 64-bit one beyond: one long signal crosses that.  Both table paths must give the same bits: every
rate pair runs on both, and 192 -> 44.1 kHz (a table of 167 KB with its padding) has the global path only."""
import functools

import numpy as np
import pytest

import rate_ref as R
from goofer_amd import rate as RT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WAVE_TILE, GROUP_TILES, GRID_TILE = 64, (256, 1024), 512 * 1024
IDS = dict(ids=lambda p: "%d-%d" % p)
BIG_TABLE = (192000, 44100)                                   # L = 147, H = 140: more than 160 KiB in LDS


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _x(rng, n):
    return (0.3 * rng.standard_normal(n)).astype(np.float32)


def _words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _convert(ctx, xs, pair, plan=None, out=None):
    """the kernel on the signals xs: a list of outputs"""
    plan = plan or RT.plan(pair[0], pair[1], [len(x) for x in xs])
    flat = np.concatenate(list(xs) + [np.zeros(1, np.float32)])           # (never an empty tensor)
    got = ctx.rate_convert(ctx.tensor(flat), None, plan, out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    return [got[plan.out_off[i]:plan.out_off[i + 1]] for i in range(plan.n)], plan


@functools.lru_cache(maxsize=None)
def _ragged(pair):
    """the ragged batch of a rate pair, with both restatements: (xs, plan, ref32 list, ref64 list, A list)"""
    L, M, H = R.geometry(*pair)
    rng = np.random.default_rng(20261020 + pair[0] + pair[1])
    xs = [_x(rng, n) for n in (0, 1, H - 1, 2049, 5000, 0)]
    plan = RT.plan(pair[0], pair[1], [len(x) for x in xs])
    ref32 = R.convert_batch(xs, plan.taps, L, M, H, np.float32)
    ref64 = R.convert_batch(xs, plan.taps, L, M, H, np.float64)
    return xs, plan, ref32, [r[0] for r in ref64], [r[1] for r in ref64]


def _length_with(L, M, lo, want, mod):
    """the first n >= lo whose output count m has m % mod == want, or None (22.05 -> 44.1 kHz makes even counts only)"""
    for n in range(lo, lo + 4 * mod):
        if R.out_len(n, L, M) % mod == want:
            return n
    return None


@pytest.fixture(params=[1, 0], ids=["lds", "global"])
def table_path(ctx, request):
    """both places the kernel reads the tap table from (option "rate_lds")"""
    ctx.set_option("rate_lds", request.param)
    yield request.param
    ctx.set_option("rate_lds", 1)


@pytest.mark.parametrize("pair", R.PAIRS + [BIG_TABLE], **IDS)
def test_ragged_batch_bit_for_bit_and_within_the_bound(ctx, pair, table_path):
    xs, plan, ref32, ref64, A = _ragged(pair)
    L, M, H = plan.L, plan.M, plan.H
    assert np.array_equal(plan.out_off, R.out_offsets([len(x) for x in xs], L, M))
    assert (4 * L * 4 * (((2 * H + 3) // 4) | 1) > 160 * 1024) == (pair == BIG_TABLE)
    got, _ = _convert(ctx, xs, pair, plan)
    worst = 0.0
    for i, (g, r32, r64, a) in enumerate(zip(got, ref32, ref64, A)):
        assert g.dtype == np.float32 and g.shape == r32.shape, i
        assert np.array_equal(_words(g), _words(r32)), (i, int((_words(g) != _words(r32)).sum()))
        err, lim = np.abs(g.astype(np.float64) - r64), R.bound(a, H)
        assert np.all(err <= lim), (i, float(err.max()))
        if len(err):
            worst = max(worst, float(np.max(err / np.maximum(lim, 1e-300))))
    print(pair, "L M H", L, M, H, "worst error / bound %.4f" % worst)


@pytest.mark.parametrize("pair", R.PAIRS + [BIG_TABLE], **IDS)
def test_last_output_on_a_tile_edge_and_one_past_it(ctx, pair, table_path):
    L, M, H = R.geometry(*pair)
    rng = np.random.default_rng(3)
    lens = [_length_with(L, M, 700, want, tile) for tile in (WAVE_TILE,) + GROUP_TILES for want in (0, 1)]
    lens = [n for n in lens if n is not None]
    assert len(lens) >= 3
    for n in lens:
        x = _x(rng, n)
        (got,), plan = _convert(ctx, [x], pair)
        want = R.convert(x, plan.taps, L, M, H)
        assert np.array_equal(_words(got), _words(want)), (n, len(want))


def test_a_batch_longer_than_one_pass_of_the_grid(ctx, table_path):
    pair = (44100, 48000)
    L, M, H = R.geometry(*pair)
    rng = np.random.default_rng(4)
    for want in (0, 1):
        n = _length_with(L, M, GRID_TILE * M // L - 8, want, GRID_TILE)
        x = _x(rng, n)
        (got,), plan = _convert(ctx, [x], pair)
        assert len(got) % GRID_TILE == want and len(got) >= GRID_TILE
        assert np.array_equal(_words(got), _words(R.convert(x, plan.taps, L, M, H))), want


def test_outputs_beyond_the_32_bit_division(ctx, table_path):
    """44.1 -> 8 kHz, M = 441: from output 2^32 / 441 = 9 739 270 on, k M needs 64 bits.  The outputs around that index and the
    last ones of the signal against the restatement."""
    pair = (44100, 8000)
    L, M, H = R.geometry(*pair)
    edge = -(-(1 << 32) // M)
    n = (edge + 40000) * M // L
    x = np.tile(_x(np.random.default_rng(5), 1 << 20), -(-n // (1 << 20)))[:n]
    plan = RT.plan(pair[0], pair[1], [n])
    got = ctx.rate_convert(ctx.tensor(x), None, plan)
    m = plan.total_out
    assert m > edge + 30000
    ks = np.concatenate([np.arange(edge - 3000, edge + 3000), np.arange(m - 3000, m)])
    got = got[torch.as_tensor(ks, device=got.device)].cpu().numpy()
    assert np.array_equal(_words(got), _words(R.convert(x, plan.taps, L, M, H, ks=ks)))


@pytest.mark.parametrize("pair", R.PAIRS, **IDS)
def test_impulse(ctx, pair):
    """y[k] = h_p[n0 - q] where that tap exists, 0 elsewhere: the index arithmetic and the table layout"""
    L, M, H = R.geometry(*pair)
    n = 3000
    m, q, p = R.index(n, L, M)
    for n0 in (0, 777, n - 1):
        x = np.zeros(n, dtype=np.float32)
        x[n0] = 1.0
        (got,), plan = _convert(ctx, [x], pair)
        j = n0 - q
        has = (j >= -H + 1) & (j <= H)
        want = np.zeros(m, dtype=np.float32)
        want[has] = plan.taps[p[has], j[has] + H - 1]
        assert has.sum() >= H * L // M and np.array_equal(got, want), n0        # (by value: a tap of -0.0 gives +0.0)
        assert np.all(_words(got)[~has] == 0)
        assert np.array_equal(_words(got), _words(R.convert(x, plan.taps, L, M, H)))


@pytest.mark.parametrize("pair", [(44100, 48000), (44100, 8000), (22050, 44100)], **IDS)
def test_a_signal_alone_and_among_neighbours(ctx, pair, table_path):
    xs, plan, ref32, _, _ = _ragged(pair)
    x, want = xs[3], ref32[3]                                  # the 2049-sample signal
    rng = np.random.default_rng(6)
    a, b = _x(rng, 1234), _x(rng, 333)
    for batch, at in (([x], 0), ([x, a, b], 0), ([a, b, x], 2), ([a, x, b], 1), ([np.zeros(0, np.float32), x, np.zeros(0, np.float32)], 1)):
        p = RT.plan(pair[0], pair[1], [len(v) for v in batch])
        buf = torch.full((p.total_out + 16,), float("nan"), dtype=torch.float32, device=ctx.device)
        got, _ = _convert(ctx, batch, pair, p, out=buf[8:8 + p.total_out])
        assert np.array_equal(_words(got[at]), _words(want)), at
        host = buf.cpu().numpy()
        assert np.all(np.isnan(host[:8])) and np.all(np.isnan(host[8 + p.total_out:]))      # nothing outside [0, out_off[n])
        assert not np.any(np.isnan(host[8:8 + p.total_out]))                               # and no sample left unwritten


@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100), (44100, 8000)], **IDS)
def test_one_nan_sample(ctx, pair, table_path):
    L, M, H = R.geometry(*pair)
    x = _x(np.random.default_rng(7), 4000)
    x[1717] = np.nan
    (got,), plan = _convert(ctx, [x], pair)
    want = R.convert(x, plan.taps, L, M, H)
    bad = ~np.isfinite(want)
    assert 2 * H * L // M - 2 <= bad.sum() <= 2 * H * L // M + 2
    assert np.array_equal(~np.isfinite(got), bad)
    assert np.array_equal(_words(got[~bad]), _words(want[~bad]))


@pytest.mark.parametrize("pair", R.PAIRS, **IDS)
def test_sines_through_the_kernel(ctx, pair):
    sr_in, sr_out = pair
    L, M, H = R.geometry(*pair)
    cut = R.margin(L, M, H)
    for frac in (0.02, 0.5, 0.8):
        f = frac * min(sr_in, sr_out) / 2.0
        x = np.sin(2.0 * np.pi * f * np.arange(6000, dtype=np.float64) / sr_in + 0.3).astype(np.float32)
        (got,), plan = _convert(ctx, [x], pair)
        _, A = R.convert(x, plan.taps, L, M, H, np.float64)
        want = np.sin(2.0 * np.pi * f * np.arange(len(got), dtype=np.float64) / sr_out + 0.3)
        err = np.abs(got.astype(np.float64) - want)[cut:len(got) - cut]
        lim = 1e-6 + R.bound(A, H)[cut:len(got) - cut]
        print(pair, frac, "worst %.3e of %.3e allowed" % (float(err.max()), float(lim.max())))
        assert len(err) > 100 and np.all(err <= lim)


def test_refusals(ctx):
    import ctypes as C
    from goofer_amd.device import GooferError
    lib, z = ctx.lib, C.c_void_p(0)
    t = torch.zeros(64, dtype=torch.int64, device=ctx.device)
    p = C.c_void_p(t.data_ptr())
    odd = C.c_void_p(t.data_ptr() + 4)
    ok = (160, 147, 32)
    assert lib.goofer_rate_convert(ctx.h, z, p, 1, *ok, p, p, p, None) == -1
    assert b"null" in lib.goofer_last_error(ctx.h)
    for k in range(5):
        args = [p, p, 1, *ok, p, p, p]
        args[[0, 1, 6, 7, 8][k]] = z
        assert lib.goofer_rate_convert(ctx.h, *args, None) == -1, k
    assert lib.goofer_rate_convert(ctx.h, p, odd, 1, *ok, p, p, p, None) == -1
    assert b"aligned" in lib.goofer_last_error(ctx.h)
    assert lib.goofer_rate_convert(ctx.h, p, p, 1, *ok, p, odd, p, None) == -1
    assert lib.goofer_rate_convert(ctx.h, p, p, -1, *ok, p, p, p, None) == -1
    for geo in ((160, 147, 31), (0, 147, 32), (160, 0, 32), (1280, 147, 32), (147, 1280, 279), (160, 160, 32)):
        assert lib.goofer_rate_convert(ctx.h, p, p, 1, *geo, p, p, p, None) == -1, geo
    assert lib.goofer_rate_convert(ctx.h, z, z, 0, *ok, z, z, z, None) == 0            # no signal: nothing to do
    with pytest.raises(GooferError):
        ctx._check(lib.goofer_rate_convert(ctx.h, z, p, 1, *ok, p, p, p, None))
    plan = RT.plan(44100, 48000, [100, 200])
    x = torch.zeros(300, dtype=torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.rate_convert(x, [0, 100, 301], plan)
    with pytest.raises(ValueError):
        ctx.rate_convert(x[:299], None, plan)
    with pytest.raises(ValueError):
        ctx.rate_convert(x, None, plan, out=torch.zeros(plan.total_out + 1, dtype=torch.float32, device=ctx.device))
    assert ctx.rate_convert(x, ctx.tensor(plan.in_off), plan).shape == (plan.total_out,)


def test_resample_batch(ctx):
    from goofer_amd import core
    xs, plan, ref32, _, _ = _ragged((44100, 48000))
    got = core.resample_batch(xs, 44100, 48000, ctx=ctx)
    assert len(got) == len(xs)
    for g, r in zip(got, ref32):
        assert g.dtype == np.float32 and np.array_equal(_words(g), _words(r))
    assert [len(g) for g in core.resample_batch([np.zeros(0), np.zeros(0, np.float32)], 48000, 44100, ctx=ctx)] == [0, 0]
    with pytest.raises(ValueError):
        core.resample_batch(xs, 44100, 44100, ctx=ctx)


def _jobs():
    """the four notes of examples/render_phrase.py, short"""
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Source
    requests = [("C4", "100", "g-10", "30", "300", "80", "50", "100", "0", "!120", "AA"),
                ("E4", "100", "t30fa20fb-10B30", "30", "300", "80", "50", "90", "0", "!120", "AA#20#AP"),
                ("G4", "80", "L1sg40st-30", "30", "300", "80", "50", "100", "0", "!120", "AA"),
                ("A3", "120", "vf30sa20pd40", "30", "300", "80", "50", "100", "0", "!120", "AA#10#BA#10#AA")]
    jobs = []
    for i, args in enumerate(requests):
        src = syn.make_source(100 + i, seconds=0.3)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
    entries = ["0 250 5 35 40 0 100 100 0 0", "10 240@120+30 5 35 40 20 100 90 10 30", "R 120",
               "0 250 5 35 40 0 110 100 0 25 10 30 80", "5 200 5 35 40 0 100 100 0 40"]
    return jobs, entries


def test_render_and_render_phrase_with_out_sr(ctx):
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    notes = r.render(jobs, seed=5)
    lens = [len(y) for y in notes]
    plan = RT.plan(44100, 48000, lens)
    conv = r.render(jobs, seed=5, out_sr=48000)
    want, _ = _convert(ctx, notes, (44100, 48000), plan)
    assert [len(y) for y in conv] == np.diff(plan.out_off).tolist() and max(lens) > 5000
    for a, b in zip(conv, want):
        assert np.array_equal(_words(a), _words(b)) and float(np.abs(a).max()) > 1e-3
    track = r.render_phrase(jobs, entries, seed=5)
    (want,), tplan = _convert(ctx, [track], (44100, 48000))
    got = r.render_phrase(jobs, entries, seed=5, out_sr=48000)
    assert got.dtype == np.float32 and np.array_equal(_words(got), _words(want))
    pcm = r.render_phrase(jobs, entries, seed=5, pcm16=True, out_sr=48000)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, ctx.pcm16(ctx.tensor(want)).cpu().numpy())
    assert np.array_equal(pcm, np.round(np.clip(want.astype(np.float64), -1.0, 1.0 - 1.0 / 32768) * 32768.0).astype("<i2"))
    import dataclasses
    other = dataclasses.replace(jobs[1][0], sr=48000)          # notes of two rates: refused before anything is planned
    with pytest.raises(ValueError):
        r.render([jobs[0], (other, jobs[1][1])], seed=5, out_sr=32000)
    with pytest.raises(ValueError):
        r.render(jobs, seed=5, out_sr=0)


def test_job_file_front_end_with_rate(ctx, tmp_path):
    """python -m goofer_amd.phrase --rate 48000 job.txt out.wav (its main(), in process): the wav says 48000 and holds the
    converted track's samples."""
    import wave
    from goofer_amd import core
    from goofer_amd import phrase as P
    from goofer_amd import synthetic as syn
    for i in range(2):
        src = syn.make_source(300 + i, seconds=0.3)
        core.save_features(tmp_path / f"v{i}_features.goofy", src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
    res = ["C4 100 g-10 30 300 80 50 100 0 !120 AA", "E4 100 B30 30 300 80 50 90 0 !120 AA#20#AP"]
    tool = ["0 250 5 35 40 0 100 100 0", "0 240@120 5 35 40 0 100 100 0 30"]
    job = tmp_path / "job.txt"
    job.write_text("".join(f"{tmp_path}/v{k}.wav {tmp_path}/n{k}.wav {r} | {t}\n" for k, (r, t) in enumerate(zip(res, tool))))
    plain, conv = tmp_path / "plain.wav", tmp_path / "conv.wav"
    assert P.main([str(job), str(plain)]) == 0
    assert P.main(["--rate", "48000", str(job), str(conv)]) == 0
    with wave.open(str(plain), "rb") as w:
        assert w.getframerate() == 44100
        n = w.getnframes()
    out_off = RT.plan(44100, 48000, [n]).out_off
    with wave.open(str(conv), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 48000, int(out_off[1]))
    assert P.main(["--rate", "fast", str(job), str(conv)]) == 1
    assert P.main(["--rate", str(job), str(conv)]) == 1


def test_no_conversion_without_the_argument(ctx, monkeypatch):
    """out_sr None, or the sources' own rate: the bits of a call without the argument, and Context.rate_convert never runs."""
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    jobs, entries = _jobs()
    r = Renderer(ctx)
    notes = r.render(jobs, seed=5)
    track = r.render_phrase(jobs, entries, seed=5)
    pcm = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    calls = []

    def never(self, *a, **k):
        calls.append(a)
        raise AssertionError("rate_convert reached")
    monkeypatch.setattr(Context, "rate_convert", never)
    for sr in (None, 44100):
        for a, b in zip(r.render(jobs, seed=5, out_sr=sr), notes):
            assert np.array_equal(_words(a), _words(b))
        assert np.array_equal(_words(r.render_phrase(jobs, entries, seed=5, out_sr=sr)), _words(track))
        assert np.array_equal(r.render_phrase(jobs, entries, seed=5, pcm16=True, out_sr=sr), pcm)
    assert not calls
    with pytest.raises(AssertionError):
        r.render(jobs, seed=5, out_sr=48000)
    assert len(calls) == 1
