"""The tile flags of the voicing mask (k_sample_assemble -> k_mask_short, goofer_render_batch).

k_sample_assemble leaves a word per 1024 samples of the concatenated mask it writes, which says one of three things about the
tile: every value == 0.0f (flag 0), every value == 1.0f (flag 1), anything else (flag 2).  k_mask_short decides per quarter (256
knots) of each note segment of its 1024-knot tiles whether the flags over everything the quarter's windows can touch are all 0
or all 1, and then writes 0.0 / the tap sum without loading the mask.  A segment whose quarters are all settled that way stages
nothing ("mask_flag_segments"), any other stages its window ("mask_staged_segments").

Here: both rules restated in numpy.  On the GPU, batches of small notes (n_fft 1024 / hop 256) whose assembled masks have their
edges exactly at, one before and one behind the boundaries of a flag tile, of a smoothing tile and of its window, rendered
with option mask_flags 0 and 1: knots, stems and mix equal bit for bit (a rule that is too liberal), and the two counters
equal the restated counts exactly (a rule that is too conservative, or a path that did not run).  The knot scratch holds
the knots of a mask of 0.37 before every run, so a knot nobody wrote shows up.  Without a GPU: wherever the restatement says
"flat", the oracle's knots are 0 or the tap sum.
"""
import numpy as np
import pytest

from goofer_amd import synthetic as syn

SEED = 23
SA_TILE, MS_TILE, MS_QUART, MASK_DS, MS_MAXWIN = 1024, 1024, 256, 4, 1152
SIGMA = 100.0                                                 # Renderer.run's transition sigma


def radius_of(sigma):
    return int(4.0 * max(1.0, sigma / 4.0) + 0.5)


# ---- the two rules, restated ------------------------------------------------------------------

def tile_flags(mask):
    """The flag of every SA_TILE samples of the concatenated mask: 0 all == 0 (so -0.0 counts), 1 all == 1, 2 anything else."""
    mask = np.asarray(mask, dtype=np.float32)
    out = np.full((mask.size + SA_TILE - 1) // SA_TILE, 2, dtype=np.uint8)
    for t in range(out.size):
        v = mask[t * SA_TILE:(t + 1) * SA_TILE]
        if np.all(v == np.float32(0.0)):
            out[t] = 0
        elif np.all(v == np.float32(1.0)):
            out[t] = 1
    return out


def segments(sample_off, flags, radius):
    """Every note segment of every MS_TILE-knot tile of the short axis (note k's knots start at sample_off[k] // 4 + k):
    (note, first knot inside the note, knots, [per quarter: 0 / 1 when the flags settle it, else None]).  Empty for a radius
    the LDS window does not hold (the per-sample loop ignores the flags)."""
    if 2 * radius + MS_TILE > 4 * MS_MAXWIN:
        return []
    sample_off = np.asarray(sample_off, dtype=np.int64)
    n_notes = sample_off.size - 1
    total_short = int(sample_off[-1]) // MASK_DS + n_notes
    lens = np.diff(sample_off)
    ns_all = (lens + MASK_DS - 1) // MASK_DS
    sb_all = sample_off[:-1] // MASK_DS + np.arange(n_notes)
    out = []
    for g0 in range(0, total_short, MS_TILE):
        g1 = min(g0 + MS_TILE, total_short)
        for k in range(n_notes):
            sb, ns, base = int(sb_all[k]), int(ns_all[k]), int(sample_off[k])
            s0, s1 = max(g0, sb), min(g1, sb + ns)
            if s1 <= s0:
                continue
            q0, ln = s0 - sb, s1 - s0
            quarters = []
            for ql in range(0, ln, MS_QUART):
                qh = min(ql + MS_QUART, ln)
                lo = min(max(q0 + ql - radius, 0), ns - 1)
                hi = min(max(q0 + qh - 1 + radius, 0), ns - 1)
                f = flags[(base + MASK_DS * lo) // SA_TILE:(base + MASK_DS * hi) // SA_TILE + 1]
                quarters.append(0 if np.all(f == 0) else (1 if np.all(f == 1) else None))
            out.append((k, q0, ln, quarters))
    return out


def counts(segs):
    flagged = sum(1 for s in segs if all(q is not None for q in s[3]))
    return flagged, len(segs) - flagged


# ---- CPU: the restatement against the oracle ---------------------------------------------------

def _cpu_masks():
    rng = np.random.default_rng(5)
    masks = []
    for n in (1, 3, 5, 700, 1025, 9000, 30011, 16384):
        m = np.ones(n, dtype=np.float32)
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(0, n))
            m[a:a + int(rng.integers(1, 6000))] = 0.0
        masks.append(m)
    masks[5][4001] = 0.5                                       # never decimated
    masks[6][:8000] = -0.0
    masks.append(np.zeros(40000, dtype=np.float32))
    masks.append(np.ones(40000, dtype=np.float32))
    return masks


@pytest.mark.parametrize("sigma", [SIGMA, 4.0, 1400.0])
def test_restatement_against_oracle(sigma):
    """Wherever the flags settle a quarter, every oracle knot of it is 0.0, or the tap sum up to the order of the additions."""
    from oracle import goofer_ref as R
    masks = _cpu_masks()
    off = np.concatenate([[0], np.cumsum([m.size for m in masks])])
    flags = tile_flags(np.concatenate(masks))
    s4 = max(1.0, sigma / 4.0)
    taps, radius = R.gauss_taps(s4)
    assert radius == radius_of(sigma)
    segs = segments(off, flags, radius)
    assert segs
    knots = [np.asarray(R.gauss1d(m[::MASK_DS].astype(np.float64), s4)) for m in masks]
    tap_sum = 0.0
    for t in taps:
        tap_sum += t * 1.0
    seen = set()
    for k, q0, ln, quarters in segs:
        for i, q in enumerate(quarters):
            got = knots[k][q0 + i * MS_QUART:q0 + min((i + 1) * MS_QUART, ln)]
            seen.add(q)
            if q == 0:
                assert np.all(got == 0.0), (k, q0, i)
            elif q == 1:
                assert np.all(np.abs(got - tap_sum) <= (2 * radius + 1) * 2.0 ** -53), (k, q0, i)
    assert seen == {0, 1, None}
    assert all(c > 0 for c in counts(segs))


def test_flag_rule_on_signed_zero_and_fractions():
    m = np.zeros(3 * SA_TILE + 5, dtype=np.float32)
    m[7] = -0.0
    m[SA_TILE:2 * SA_TILE] = 1.0
    m[2 * SA_TILE + 3] = 0.5
    m[3 * SA_TILE:] = 1.0
    assert tile_flags(m).tolist() == [0, 1, 2, 1]
    m[SA_TILE + 1] = np.nan
    assert tile_flags(m).tolist() == [0, 2, 2, 1]


# ---- GPU ----------------------------------------------------------------------------------------

EDGE_KW = dict(length_ms=150.0)                               # 4410 + 6615 = 11025 samples, no tiled tail


def _edge(kind, delta, rising):
    """A note with one edge of its mask `delta` samples from a boundary of the concatenated axis inside it: kind "flag": a flag
    tile (1024 samples), "seg": a smoothing tile (4096 samples; knot sb + q a multiple of 1024)."""
    def pattern(n, base, sb):
        if kind == "flag":
            at = (-base) % SA_TILE
            at += SA_TILE if at < 2 else 0
        else:
            q = (-sb) % MS_TILE
            q += MS_TILE if q < 256 else 0
            at = MASK_DS * q
        at += delta
        assert 0 < at < n
        m = np.zeros(n, dtype=np.float32)
        m[at:] = 1.0
        return m if rising else np.float32(1.0) - m
    return ("t0", EDGE_KW, pattern)


def _const(v):
    return lambda n, base, sb: np.full(n, v, dtype=np.float32)


def _fraction(n, base, sb):
    m = np.ones(n, dtype=np.float32)
    m[4001] = 0.5                                              # not a multiple of 4: never decimated
    return m


def _minus_zero(n, base, sb):
    m = np.zeros(n, dtype=np.float32)
    m[::3] = -0.0
    m[9000:] = 1.0
    return m


def _source_step(ylen):
    """(the SOURCE mask itself: an edge inside the consonant, which the velocity stretch interpolates)"""
    m = np.ones(ylen, dtype=np.float32)
    m[:4000] = 0.0
    return m


_source_step.raw = True
R4 = MASK_DS * radius_of(SIGMA)
BATCH_EDGES = ([_edge("flag", d, up) for d in (-1, 0, 1) for up in (True, False)] +
               [_edge("seg", d, up) for d in (-1, 0, 1, -R4 - 1, -R4, -R4 + 1, R4 - 1, R4, R4 + 1) for up in (True, False)] +
               [("FV1", EDGE_KW, None), ("t0", EDGE_KW, _const(0.0)), ("t0", EDGE_KW, _const(1.0)), ("t0", EDGE_KW, _fraction),
                ("t0", EDGE_KW, _minus_zero)])
_TINY = lambda ms: dict(length_ms=ms, consonant_ms=0.0)
BATCH_SMALL = [("t0", _TINY(6.81), _const(0.0)), ("t0", _TINY(9.08), _const(1.0)),     # 300 + 400 samples: one flag tile
               ("t0", _TINY(0.03), _const(1.0)), ("t0", _TINY(0.07), _const(0.0)), ("t0", _TINY(0.115), _const(1.0)),   # 1, 3, 5 samples
               ("t0", _TINY(23.25), _edge("flag", 0, True)[2]),                          # 1025 samples
               ("R1", EDGE_KW, _edge("seg", 1, False)[2]), ("L1", dict(length_ms=700.0), _edge("seg", -1, True)[2]),   # reversed; tiled tail
               ("t0", dict(length_ms=150.0, velocity=70.0), _source_step), ("t0", EDGE_KW, _const(1.0))]   # velocity stretch: the slow path


def _requests(spec):
    from goofer_amd import sampler as S
    return [S.decode_request(*syn.request_args(syn.make_request(3100 + i, flags, **kw))) for i, (flags, kw, _) in enumerate(spec)]


def _sources(spec, masks):
    from goofer_amd.render import Source
    out = []
    for i in range(len(spec)):
        src = syn.make_source(3100 + i, seconds=0.45)
        m = src["mask"] if masks[i] is None else masks[i]
        out.append(Source.from_pack(src["env_pack"], src["f0"], m, src["formants"], src["sr"], src["y_len"]))
    return out


def _prepare(r, spec, masks, keep=None):
    idx = list(range(len(spec))) if keep is None else keep
    reqs, srcs = _requests(spec), _sources(spec, masks)
    np.random.seed(SEED)
    return r.prepare([(srcs[i], reqs[i]) for i in idx], note_ids=idx)


def _build(r, spec):
    """(prep, poison prep, source masks): the source masks are made so that the ASSEMBLED mask of each note is its pattern — a
    first assembly of index ramps tells which source sample every output sample is."""
    ylen = syn.make_source(3100, seconds=0.45)["y_len"]
    ramp = np.arange(ylen, dtype=np.float32)
    probe = _prepare(r, spec, [ramp] * len(spec))
    r.assemble(probe)
    r.ctx.check()
    where = probe["mask"].cpu().numpy()
    off = np.asarray(probe["sample_off"], dtype=np.int64)
    masks = []
    for k, (flags, kw, pattern) in enumerate(spec):
        if pattern is None or getattr(pattern, "raw", False):
            masks.append(None if pattern is None else pattern(ylen))
            continue
        n, base = int(off[k + 1] - off[k]), int(off[k])
        want = pattern(n, base, base // MASK_DS + k)
        src_idx = where[base:base + n]
        assert np.all(src_idx == np.round(src_idx))
        m = np.ones(ylen, dtype=np.float32)
        m[src_idx.astype(np.int64)] = want                     # (a tiled tail: the last repeat wins)
        masks.append(m)
    poison_spec = [(f.replace("FV1", "t0"), kw, p) for f, kw, p in spec]
    poison = _prepare(r, poison_spec, [np.full(ylen, 0.37, dtype=np.float32)] * len(spec))
    return _prepare(r, spec, masks), poison, masks


def _render(r, prep, poison, flags, sigma=None):
    """One render under option mask_flags = `flags`, behind a render that leaves the knots of a 0.37 mask in the scratch."""
    ctx = r.ctx

    def go(p):
        if sigma is None:
            return r.run(p, seed=SEED, keep_stems=True)
        return ctx.synth_batch(p["env"], p["env_lens"], p["f0"], p["mask"], p["lens"], p["params"], formants=p["formants"], phi=p["phi"],
                               seed=SEED, want_rec=False, want_mix=True, offsets=p["offsets"], transition_sigma=sigma, assembly=p["assembly"])
    ctx.set_option("mask_flags", flags)
    try:
        go(poison)
        ctx.check()
        c0 = (ctx.counter("mask_flag_segments"), ctx.counter("mask_staged_segments"))
        out = go(prep)
        ctx.check()
        res = {k: out[k].cpu().numpy().copy() for k in ("harm", "uv", "bre", "mix")}
        res["knots"] = _live_knots(ctx.debug_fetch("mask_short"), prep["sample_off"])
        res["counts"] = (ctx.counter("mask_flag_segments") - c0[0], ctx.counter("mask_staged_segments") - c0[1])
        res["mask"] = prep["mask"].cpu().numpy().copy()
    finally:
        ctx.set_option("mask_flags", 1)
    return res


def _same(a, b, what):
    for k in ("knots", "harm", "uv", "bre", "mix"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _live_knots(knots, off):
    """The knots of the notes, without the slack between them."""
    off = np.asarray(off, dtype=np.int64)
    return np.concatenate([knots[int(off[k]) // MASK_DS + k:int(off[k]) // MASK_DS + k + (int(off[k + 1] - off[k]) + 3) // 4]
                           for k in range(off.size - 1)])


@pytest.fixture(scope="module")
def renderer():
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    ctx = Context(0)
    yield Renderer(ctx)
    ctx.close()


def _check_batch(r, spec, keep=None, sigma=None):
    prep, poison, _ = _build(r, spec) if keep is None else _build(r, [spec[i] for i in keep])
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    a, b = _render(r, prep, poison, 0, sigma), _render(r, prep, poison, 1, sigma)
    _same(a, b, "mask_flags 0 against 1")
    assert np.array_equal(a["mask"].view(np.uint32), b["mask"].view(np.uint32))
    assert b["knots"].size == int(np.sum((np.diff(off) + 3) // 4)) and np.all(np.isfinite(b["knots"]))
    segs = segments(off, tile_flags(b["mask"]), radius_of(SIGMA if sigma is None else sigma))
    print("segments", len(segs), "restated (flagged, staged)", counts(segs), "counted", b["counts"], "without flags", a["counts"])
    assert a["counts"] == (0, len(segs))
    assert b["counts"] == counts(segs)
    return prep, poison, a, b


@pytest.mark.gpu
def test_edges_at_every_boundary(renderer):
    """Rising and falling edges at -1 / 0 / +1 from a flag-tile boundary, a smoothing-tile boundary and that boundary -+ the
    window's 4 * radius; force-voiced, all-unvoiced, all-voiced, a 0.5 that is never decimated, -0.0.  Then one stream."""
    r = renderer
    prep, poison, a, b = _check_batch(r, BATCH_EDGES)
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    m = b["mask"]
    # the patterns arrived: note 0's rising edge one sample before sample 1024 of the batch
    assert off[0] == 0 and m[1022] == 0.0 and m[1023] == 1.0
    assert np.all(m[off[24]:off[25]] == 1.0) and np.all(m[off[25]:off[26]] == 0.0) and np.all(m[off[26]:off[27]] == 1.0)
    assert m[off[27] + 4001] == 0.5 and np.count_nonzero(m[off[27]:off[28]] != 1.0) == 1
    assert np.any(np.signbit(m[off[28]:off[28] + 9000])) and np.all(m[off[28]:off[28] + 9000] == 0.0)
    assert b["counts"][0] > 0 and b["counts"][1] > 0           # both paths ran
    r.ctx.set_option("overlap", 0)
    try:
        a1, b1 = _render(r, prep, poison, 0), _render(r, prep, poison, 1)
    finally:
        r.ctx.set_option("overlap", 1)
    _same(a1, b1, "one stream: mask_flags 0 against 1")
    _same(a, b1, "one stream against two")
    assert b1["counts"] == b["counts"]


@pytest.mark.gpu
def test_small_notes_and_slow_paths(renderer):
    """Two notes of 300 and 400 samples with different constant masks in one flag tile; 1, 3, 5 and 1025 samples; a reversed
    note, a tiled tail, a velocity stretch."""
    prep, _, _, b = _check_batch(renderer, BATCH_SMALL)
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    assert np.diff(off)[:6].tolist() == [300, 400, 1, 3, 5, 1025]
    assert tile_flags(b["mask"])[0] == 2                       # 300 zeros and 400 ones (and the 1, 3, 5 behind them) share it
    vel = b["mask"][off[8]:off[9]]
    assert np.any((vel != 0.0) & (vel != 1.0))                 # the stretch interpolates the edge


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [[0, 7, 12, 25, 28], [3, 26, 9]])
def test_sub_batches(renderer, keep):
    _check_batch(renderer, BATCH_EDGES, keep=keep)


@pytest.mark.gpu
def test_large_radius_takes_the_per_sample_loop(renderer):
    """transition_sigma 2000: radius 2000, beyond the LDS window.  The flags are ignored; only the values must match."""
    assert 2 * radius_of(2000.0) + MS_TILE > 4 * MS_MAXWIN
    _, _, a, b = _check_batch(renderer, BATCH_SMALL, sigma=2000.0)
    assert a["counts"] == (0, 0) and b["counts"] == (0, 0)
