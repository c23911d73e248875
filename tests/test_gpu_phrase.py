"""GPU: phrase assembly (goofer_phrase_mix, csrc/phrase.hip) against its float64 restatement (tests/phrase_ref.py).

The notes are random fp32 arrays: nothing is rendered except in the end-to-end test.  The tolerance is derived, not measured:
per sample |got - ref| <= (8 + D) * 2^-24 * B with B = sum_i max_k |val_i[k]| * |x_i| and D the number of notes that reach the
sample — six roundings in the gain, one in the product, D in the sum.  Properties that must hold to the bit (a phrase shifted
by a leading rest, a note alone and in company) are compared as int32 words."""
import numpy as np
import pytest

import phrase_ref as R
from goofer_amd import _lib
from goofer_amd import phrase as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _rec(start, skip, take, rng=None, pos=None, val=None):
    r = np.zeros((), dtype=_lib.PHRASE_NOTE)
    r["start"], r["skip"], r["take"] = start, skip, take
    if pos is None:
        pos = np.sort(rng.uniform(0, take, 7)).astype(np.float32) if rng is not None else np.linspace(0, take, 7).astype(np.float32)
    r["pos"] = np.minimum(np.asarray(pos, dtype=np.float32), np.float32(take))
    r["pos"][0], r["pos"][6] = 0.0, np.float32(take)
    r["val"] = rng.uniform(0, 1, 7).astype(np.float32) if val is None else val
    return r


def _x(rng, n):
    return (0.3 * rng.standard_normal(n)).astype(np.float32)


def _mix(ctx, xs, notes, total_out, out=None, x_dev=None):
    notes = np.array(notes, dtype=_lib.PHRASE_NOTE).reshape(-1)
    lens = [len(x) for x in xs]
    plan = P.plan_records(notes, lens, total_out)
    if x_dev is None:
        x_dev = ctx.tensor(np.concatenate(list(xs) + [np.zeros(0, np.float32)]).astype(np.float32))
    got = ctx.phrase_mix(x_dev, ctx.offsets(lens), plan, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _check(got, xs, notes, total_out, what=""):
    ref, B, D = R.mix(xs, notes, total_out)
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.all(np.isfinite(got))
    err, lim = np.abs(got.astype(np.float64) - ref), R.bound(B, D)
    worst = float(np.max(err / np.maximum(lim, 1e-300))) if len(err) else 0.0
    print(what, "samples", len(ref), "deepest cover", int(D.max()) if len(D) else 0, "worst error / bound %.3f" % worst)
    bad = np.nonzero(err > lim)[0]
    assert bad.size == 0, (what, bad[:8], err[bad[:8]], lim[bad[:8]])
    assert np.all(got[D == 0] == 0.0)                          # silence is exact
    return ref, B, D


def _cases():
    """name -> (xs, notes, total_out) of the plain cases (tile = 2048)"""
    rng = np.random.default_rng(20261019)
    c = {}
    c["one note shorter than a tile"] = ([_x(rng, 1500)], [_rec(0, 0, 1500, rng)], 1500)
    c["5000 samples at 777"] = ([_x(rng, 5000)], [_rec(777, 0, 5000, rng)], 5777)
    c["cross-fade across 2048"] = ([_x(rng, 3000), _x(rng, 2500)], [_rec(0, 0, 3000, rng), _rec(2040, 0, 2500, rng)], 4540)
    inner = [(800, 300), (2300, 900), (4000, 450), (4200, 700), (8000, 600)]       # ends are not monotone
    c["five short notes inside a long one"] = ([_x(rng, 10000)] + [_x(rng, n) for _, n in inner],
                                               [_rec(0, 0, 10000, rng)] + [_rec(s, 0, n, rng) for s, n in inner], 10000)
    c["start -100"] = ([_x(rng, 3000)], [_rec(-100, 0, 3000, rng)], 2900)
    c["past total_out"] = ([_x(rng, 6000)], [_rec(500, 0, 6000, rng)], 4100)
    c["skip + take > len"] = ([_x(rng, 2000), _x(rng, 700)], [_rec(10, 600, 3000, rng), _rec(100, 0, 700, rng)], 3500)
    c["take 0"] = ([_x(rng, 500), _x(rng, 800)], [_rec(40, 0, 0, rng), _rec(60, 0, 800, rng)], 1000)
    c["len 0"] = ([_x(rng, 0), _x(rng, 800)], [_rec(40, 0, 300, rng), _rec(60, 0, 800, rng)], 1000)
    c["only a note without samples"] = ([_x(rng, 0)], [_rec(40, 0, 300, rng)], 1000)
    c["eight notes on the same 100 samples"] = ([_x(rng, 100 + 10 * k) for k in range(8)],
                                                [_rec(2000, 10 * k, 100, rng) for k in range(8)], 2200)    # (across the edge at 2048)
    step = [0, 100, 100, 100, 900, 950, 1000]                  # p2 = 0 (and no p5): a step at 100
    c["coincident knots"] = ([_x(rng, 1000)], [_rec(5, 0, 1000, pos=step, val=[0, 0.2, 1.0, 0.9, 0.8, 0.5, 0])], 1100)
    c["all knots at 0 and at the end"] = ([_x(rng, 1000), _x(rng, 1000)],
                                          [_rec(0, 0, 1000, pos=[0, 0, 0, 0, 0, 0, 1000], val=[0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.1]),
                                           _rec(500, 0, 1000, pos=[0, 1000, 1000, 1000, 1000, 1000, 1000], val=[0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.1])],
                                          1500)
    c["seven distinct knots"] = ([_x(rng, 3000)], [_rec(0, 0, 3000, pos=[0, 200, 450, 1100, 2000, 2600, 3000],
                                                        val=[0, 0.5, 1.0, 0.7, 0.9, 0.3, 0])], 3000)
    c["gains above 1"] = ([_x(rng, 2500)], [_rec(30, 0, 2500, rng, val=[0, 2.5, 1.5, 3.0, 1.0, 2.0, 0.5])], 2600)
    # every source alignment (skip - start mod 4) under notes long enough for whole waves inside them, the last note's source
    # ending where the batch ends; knots inside a wave and waves between two knots
    # (the last note: its source one float off a 16-byte boundary, its last whole wave ending where the batch ends)
    c["sources at every alignment"] = ([_x(rng, 6000 + k) for k in range(4)] + [_x(rng, 5751)],
                                       [_rec(300 + 1000 * k, k, 6000, rng) for k in range(4)] + [_rec(5001, 0, 5751, rng)], 11100)
    return c


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_track_matches_the_restatement(ctx, name):
    xs, notes, total = CASES[name]
    _check(_mix(ctx, xs, notes, total), xs, notes, total, name)


def test_rest_between_notes_is_exact_silence_and_nothing_is_left_unwritten(ctx):
    rng = np.random.default_rng(5)
    xs = [_x(rng, 3000), _x(rng, 2500)]
    notes = [_rec(0, 0, 3000, rng), _rec(8000, 0, 2500, rng)]   # a rest of 5000 samples: tiles 1 and 2 hold no note
    out = torch.full((10500,), float("nan"), dtype=torch.float32, device=ctx.device)
    got = _mix(ctx, xs, notes, 10500, out=out)
    _check(got, xs, notes, 10500, "rest")
    assert np.all(got[3000:8000].view(np.int32) == 0)           # +0.0f


def test_no_note_and_no_track(ctx):
    out = torch.full((3000,), float("nan"), dtype=torch.float32, device=ctx.device)
    got = _mix(ctx, [], [], 3000, out=out)
    assert got.shape == (3000,) and np.all(got.view(np.int32) == 0)
    rng = np.random.default_rng(6)
    got = _mix(ctx, [_x(rng, 100)], [_rec(0, 0, 100, rng)], 0)
    assert got.shape == (0,)
    assert _mix(ctx, [], [], 0).shape == (0,)


def test_misaligned_out_and_misaligned_x(ctx):
    name = "sources at every alignment"
    xs, notes, total = CASES[name]
    want = _mix(ctx, xs, notes, total)
    buf = torch.full((total + 1,), float("nan"), dtype=torch.float32, device=ctx.device)
    got = _mix(ctx, xs, notes, total, out=buf[1:])             # 4 bytes off a 16-byte boundary: the scalar stores
    assert buf[1:].data_ptr() % 16 == 4 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert bool(torch.isnan(buf[0]))
    x = torch.zeros(sum(len(v) for v in xs) + 1, dtype=torch.float32, device=ctx.device)
    x[1:] = ctx.tensor(np.concatenate(xs))
    got = _mix(ctx, xs, notes, total, x_dev=x[1:])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    with pytest.raises(ValueError):
        _mix(ctx, xs, notes, total, out=buf[:-2])


def _phrase(rng):
    lens = [5000, 2600, 900, 3100]
    xs = [_x(rng, n) for n in lens]
    notes = [_rec(0, 3, 5000, rng), _rec(4500, 0, 2600, rng), _rec(4800, 1, 899, rng), _rec(6900, 2, 3000, rng)]
    return xs, notes, 10000


@pytest.mark.parametrize("lead", [1, 2047, 2048])
def test_a_leading_rest_shifts_the_track_bit_for_bit(ctx, lead):
    xs, notes, total = _phrase(np.random.default_rng(7))
    base = _mix(ctx, xs, notes, total)
    moved = [r.copy() for r in notes]
    for r in moved:
        r["start"] += lead
    got = _mix(ctx, xs, moved, total + lead)
    assert np.all(got[:lead].view(np.int32) == 0)
    assert np.array_equal(got[lead:].view(np.int32), base.view(np.int32))


def test_a_note_alone_and_in_company_contributes_the_same_bits(ctx):
    xs, notes, total = _phrase(np.random.default_rng(8))
    together = _mix(ctx, xs, notes, total)
    _, _, D = R.mix(xs, notes, total)
    seen = 0
    for i in range(len(notes)):
        alone = _mix(ctx, [xs[i]], [notes[i]], total)
        _, _, Di = R.mix([xs[i]], [notes[i]], total)
        only = (D == 1) & (Di == 1)
        seen += int(only.sum())
        assert np.array_equal(alone[only].view(np.int32), together[only].view(np.int32)), i
    assert seen > 5000


def test_null_pointers_are_refused(ctx):
    import ctypes as C
    from goofer_amd.device import GooferError
    lib, z = ctx.lib, C.c_void_p(0)
    t = torch.zeros(64, dtype=torch.int64, device=ctx.device)
    p = C.c_void_p(t.data_ptr())
    assert lib.goofer_phrase_mix(ctx.h, p, p, 1, p, p, p, 100, z, None) == -1
    assert lib.goofer_phrase_mix(ctx.h, p, p, 1, p, z, p, 100, p, None) == -1
    assert lib.goofer_phrase_mix(ctx.h, z, p, 1, p, p, p, 100, p, None) == -1
    assert b"null" in lib.goofer_last_error(ctx.h)
    assert lib.goofer_phrase_mix(ctx.h, p, p, -1, p, p, p, 100, p, None) == -1
    assert lib.goofer_phrase_mix(ctx.h, z, z, 0, z, z, z, 0, z, None) == 0        # total_out == 0: nothing to do
    with pytest.raises(GooferError):
        ctx._check(lib.goofer_phrase_mix(ctx.h, p, p, 1, p, p, p, 100, z, None))


def test_render_phrase_end_to_end(ctx):
    """Renderer.render_phrase = Context.phrase_mix over the notes Renderer.render returns for the same seed, bit for bit; the
    track against the restatement; pcm16 = write_wav's arithmetic on the fp32 track."""
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Renderer, Source
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
    r = Renderer(ctx)
    track = r.render_phrase(jobs, entries, seed=5)
    notes = r.render(jobs, seed=5)
    lens = [len(y) for y in notes]
    plan = P.plan_phrase(entries, lens, 44100)
    assert track.dtype == np.float32 and track.shape == (plan.total_out,) and plan.n == 4
    again = ctx.phrase_mix(ctx.tensor(np.concatenate(notes)), ctx.offsets(lens), plan).cpu().numpy()
    assert np.array_equal(track.view(np.int32), again.view(np.int32))
    _, B, D = _check(track, notes, plan.notes, plan.total_out, "render_phrase")
    assert D.max() == 2 and float(np.abs(track).max()) > 1e-3   # the notes cross-fade, and sound
    pcm = r.render_phrase(jobs, entries, seed=5, pcm16=True)
    want = np.round(np.clip(track.astype(np.float64), -1.0, 1.0 - 1.0 / 32768) * 32768.0).astype("<i2")
    assert pcm.dtype == np.int16 and np.array_equal(pcm, want)


def test_job_file_front_end(ctx, tmp_path):
    """python -m goofer_amd.phrase job.txt out.wav (its main(), in process): the wav holds the int16 track render_phrase gives
    for the same notes; the samples are found through their .goofy caches (the wav files themselves are never read)."""
    import wave
    from goofer_amd import core
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Renderer, Source
    srcs = []
    for i in range(2):
        src = syn.make_source(300 + i, seconds=0.3)
        core.save_features(tmp_path / f"v{i}_features.goofy", src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
        srcs.append(Source.from_pack(*core.load_features(str(tmp_path / f"v{i}_features.goofy"))))
    res = ["C4 100 g-10 30 300 80 50 100 0 !120 AA", "E4 100 B30 30 300 80 50 90 0 !120 AA#20#AP", "D4 100 t10 30 300 80 50 100 0 !120 AA"]
    tool = ["0 250 5 35 40 0 100 100 0", "0 240@120 5 35 40 0 100 100 0 30", "4 200 5 35 40 0 100 100 0 25"]
    which = [0, 1, 0]
    job = tmp_path / "job.txt"
    job.write_text("".join(f"{tmp_path}/v{w}.wav {tmp_path}/n{k}.wav {r} | {t}\n" + ("R 100\n" if k == 1 else "")
                           for k, (w, r, t) in enumerate(zip(which, res, tool))))
    out = tmp_path / "out.wav"
    lines = P.read_job(job)
    assert [e.rest for _, e in lines] == [False, False, True, False]
    r = Renderer(ctx)
    track = P.render_job(job, out, renderer=r, seed=9)
    jobs = [(srcs[w], S.decode_request(*a.split())) for w, a in zip(which, res)]
    want = r.render_phrase(jobs, [e for _, e in lines], seed=9, pcm16=True)
    assert track.dtype == np.int16 and np.array_equal(track, want) and int(np.abs(want.astype(np.int32)).max()) > 30
    with wave.open(str(out), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 44100, len(want))
        assert w.readframes(len(want)) == want.astype("<i2").tobytes()
    assert P.main([str(tmp_path / "missing.txt"), str(out)]) == 1
