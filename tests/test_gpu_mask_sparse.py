"""The sparse voicing mask (option "mask_sparse"; k_sample_assemble -> the frame picks and k_mask_short, goofer_render_batch).

In a mix_only render on the stem walkers the f0 / mask kernel does not store the 256 mask values of a wave that are all 0.0f or all
1.0f: it sets bit 2 of the wave's flag byte, and the only readers of the mask on that route — the per-frame picks and the windows
k_mask_short stages for its unsettled quarters — take such a value from the byte.  A wave of the kernel owns the four 64-sample
strips at 64 w + 256 u of its 1024-sample tile.

Here, on one batch of small notes (n_fft 1024 / hop 256) whose assembled masks are laid out against those tiles and strips,
mask_sparse 1 against 0: mix, smoothed knots, picks and the two mask counters equal bit for bit; the stems through a control
render that keeps them.  The mask array is filled with NaN before every render (and the allocator's blocks before the batch is
prepared), so a value read where nothing was stored ends up as NaN in a pick, a knot and the mix — and what the sparse render
left unwritten can be told: it must be most of the batch, and only waves that are all zeros or all ones.  The fallbacks: a batch
with the f0 jitter, and a render that keeps the stems, write the whole mask; each note rendered alone gives the note's samples
of the batch.

The hop equals the period of the strips, so all picks of a note fall into the same wave index of their tiles: the note with the
lone unvoiced samples has one in another wave of one tile (the picks there come from the byte of a flat wave beside a wave that
is not) and one at a pick of a later tile (that pick comes from the array).
"""
import numpy as np
import pytest

import test_gpu_mask_flags as MF
from goofer_amd import synthetic as syn

SEED = MF.SEED
SA_TILE, HOP = 1024, 256
KW = MF.EDGE_KW                                               # 11025 samples
TINY = MF._TINY


def wave_of(g):
    """Which of the four waves of its tile's workgroup writes sample g of the concatenated axis."""
    return ((g % SA_TILE) & 255) >> 6


def _lone_samples(n, base, sb):
    """Ones but for two samples.  The picks sit at base + 256 t, all in wave w of their tiles.  The first zero: in the first whole
    tile of the note, in wave w + 1, not at a pick.  The second: exactly at the first pick of the third whole tile."""
    m = np.ones(n, dtype=np.float32)
    w = wave_of(base)
    t0 = (base + SA_TILE - 1) // SA_TILE * SA_TILE             # first tile that starts inside the note
    a = t0 + 64 * ((w + 1) % 4) + 7 - base
    picks = base + HOP * np.arange(n // HOP + 1)
    b = int(picks[picks >= t0 + 2 * SA_TILE][0]) - base
    assert 0 < a < b < n and wave_of(base + a) != w and wave_of(base + b) == w and (b % HOP) == 0 and (a % HOP) != 0
    m[a] = 0.0
    m[b] = 0.0
    return m


def _strip_edge(rising):
    def pattern(n, base, sb):
        """An edge exactly where strip 5 of a tile (wave 1, its second strip) begins."""
        at = (SA_TILE - base % SA_TILE) + 3 * SA_TILE + 5 * 64
        assert 0 < at < n and (base + at) % 64 == 0 and wave_of(base + at) == 1
        m = np.zeros(n, dtype=np.float32)
        m[at:] = 1.0
        return m if rising else np.float32(1.0) - m
    return pattern


def _gaps_pattern(n, base, sb):
    """A voiced note with three unvoiced gaps of 50 ms (the neighbour of the all-voiced note in front of it)."""
    m = np.ones(n, dtype=np.float32)
    for a in (700, 4100, 8300):
        m[a:a + 2205] = 0.0
    return m


def _source_gaps(ylen):
    """(the SOURCE mask: synthetic.with_unvoiced_gaps, 30 % of the sample in 50 ms gaps)"""
    src = syn.with_unvoiced_gaps(syn.make_source(3100, seconds=0.45), 0.3, 11)
    assert src["y_len"] == ylen and 0.1 < float(np.mean(src["mask"][:ylen] == 0.0)) < 0.5
    return src["mask"][:ylen].copy()


_source_gaps.raw = True

BATCH = [("t0", TINY(0.03), MF._const(1.0)),                  # 0: 1 sample: every later note starts off the 16-byte grid
         ("t0", TINY(6.81), MF._const(1.0)),                  # 1: 300 samples, less than a tile
         ("t0", TINY(23.23), MF._const(1.0)),                 # 2: 1024 samples
         ("t0", TINY(23.25), MF._const(0.0)),                 # 3: 1025 samples
         ("t0", KW, MF._const(1.0)),                          # 4: voiced, and meets ...
         ("t0", KW, _gaps_pattern),                           # 5: ... a note with gaps inside a tile
         ("t0", KW, _lone_samples),                           # 6
         ("t0", KW, MF._const(0.0)),                          # 7: unvoiced throughout
         ("t0", KW, MF._edge("flag", 0, True)[2]),            # 8: an edge exactly on a tile boundary
         ("t0", KW, MF._edge("flag", 0, False)[2]),           # 9
         ("t0", KW, _strip_edge(True)),                       # 10: ... exactly on a strip boundary
         ("t0", KW, _strip_edge(False)),                      # 11
         ("L1", dict(length_ms=700.0), _source_gaps),         # 12: 50 ms gaps of the source, tiled tail
         ("t0", KW, _source_gaps),                            # 13
         ("t0", KW, MF._const(1.0))]                          # 14: the batch ends inside a tile of ones


@pytest.fixture(scope="module")
def renderer():
    import torch
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    ctx = Context(0)
    # the batch's arrays come from torch's caching allocator: what it hands out is NaN, not fresh zero pages
    junk = [torch.full((1 << 20,), float("nan"), device="cuda") for _ in range(6)]
    del junk
    yield Renderer(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def batch(renderer):
    prep, _, masks = MF._build(renderer, BATCH)
    return prep, masks


def _render(r, prep, sparse, keep_stems=False):
    """One render under option mask_sparse = `sparse` into a mask array of NaN.  mix_only unless keep_stems."""
    ctx = r.ctx
    ctx.set_option("mask_sparse", sparse)
    try:
        prep["mask"].fill_(float("nan"))
        c0 = (ctx.counter("mask_flag_segments"), ctx.counter("mask_staged_segments"))
        out = r.run(prep, seed=SEED, keep_stems=keep_stems)
        ctx.check()
        res = {k: out[k].cpu().numpy().copy() for k in (("harm", "uv", "bre", "mix") if keep_stems else ("mix",))}
        res["knots"] = MF._live_knots(ctx.debug_fetch("mask_short"), prep["sample_off"])
        res["picks"] = ctx.debug_fetch("picks").copy()
        res["counts"] = (ctx.counter("mask_flag_segments") - c0[0], ctx.counter("mask_staged_segments") - c0[1])
        res["mask"] = prep["mask"].cpu().numpy().copy()
    finally:
        ctx.set_option("mask_sparse", 1)
    return res


def _same(a, b, what, keys):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].size > 0, (what, k)
        assert np.all(np.isfinite(a[k])) and np.array_equal(a[k], b[k]) and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
    assert a["counts"] == b["counts"], (what, a["counts"], b["counts"])


@pytest.fixture(scope="module")
def renders(renderer, batch):
    prep, _ = batch
    return _render(renderer, prep, 0), _render(renderer, prep, 1)


@pytest.mark.gpu
def test_batch_layout(batch):
    """The notes are where the cases want them."""
    prep, _ = batch
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    n = np.diff(off)
    assert n[:4].tolist() == [1, 300, 1024, 1025] and np.all(n[4:12] == 11025)
    assert all(int(o) % 4 != 0 for o in off[1:5])             # off the 16-byte grid
    assert off[5] % SA_TILE != 0                               # notes 4 and 5 meet inside a tile
    assert off[-1] % SA_TILE not in (0, SA_TILE - 1)           # a last partial tile


@pytest.mark.gpu
def test_sparse_against_full(renders):
    """mix, knots, picks and counters, mask_sparse 1 against 0 (both mix_only, both into a mask of NaN)."""
    full, sparse = renders
    _same(full, sparse, "mask_sparse 0 against 1", ("mix", "knots", "picks"))
    assert full["counts"][0] > 0 and full["counts"][1] > 0     # segments answered from the flags, and staged windows


@pytest.mark.gpu
def test_what_was_left_unwritten(renderer, renders, batch):
    """mask_sparse 0 writes every value.  mask_sparse 1 writes the same values or nothing; what it leaves out are whole waves
    that are all zeros or all ones, and they are most of the batch; every case of the batch has both kinds."""
    prep, _ = batch
    full, sparse = renders
    m, s = full["mask"], sparse["mask"]
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    assert not np.any(np.isnan(m))
    gone = np.isnan(s)
    assert np.array_equal(m[~gone].view(np.uint32), s[~gone].view(np.uint32))
    print("unwritten share of the mask: %.3f" % gone.mean())
    assert gone.mean() > 0.5
    g = np.arange(m.size)
    wave = (g // SA_TILE) * 4 + wave_of(g)
    for w in np.unique(wave[gone]):
        sel = wave == w
        assert np.all(gone[sel]) and (np.all(m[sel] == 0.0) or np.all(m[sel] == 1.0)) and not np.any(np.signbit(m[sel])), int(w)
    # the lone samples: their waves are written, the other three waves of the first one's tile are not
    k = 6
    zeros = off[k] + np.nonzero(m[off[k]:off[k + 1]] == 0.0)[0]
    assert zeros.size == 2 and not np.any(gone[wave == wave[zeros[0]]]) and not np.any(gone[wave == wave[zeros[1]]])
    tile = (g // SA_TILE) == zeros[0] // SA_TILE
    assert np.count_nonzero(gone[tile]) == 768
    pick_g = off[k] + HOP * np.arange((off[k + 1] - off[k]) // HOP + 1)
    in_tile = pick_g[pick_g // SA_TILE == zeros[0] // SA_TILE]
    assert in_tile.size == 4 and np.all(gone[in_tile])         # picks answered from the byte of a flat wave
    assert zeros[1] in pick_g and not gone[zeros[1]]           # ... and one from the array
    # unvoiced throughout: unwritten tiles of zeros; the tile of two notes is written
    assert np.any(gone[off[7]:off[8]]) and np.all(m[off[7]:off[8]] == 0.0)
    t = off[5] // SA_TILE
    assert not np.any(gone[t * SA_TILE:(t + 1) * SA_TILE])
    # the last partial tile is one of ones, unwritten
    assert np.all(gone[off[-1] // SA_TILE * SA_TILE:])
    # the picks took the values of the full mask
    f_off = np.concatenate([[0], np.cumsum(renderer.ctx.frame_counts(prep["lens"]))]).astype(np.int64)
    got = sparse["picks"].reshape(-1, 2)[:, 1]
    assert got.size == f_off[-1]
    for q in range(off.size - 1):
        n = int(off[q + 1] - off[q])
        at = np.minimum(HOP * np.arange(f_off[q + 1] - f_off[q]), (n - 1) // HOP * HOP)
        assert np.array_equal(got[f_off[q]:f_off[q + 1]], m[off[q] + at]), q


@pytest.mark.gpu
def test_stems_through_a_control_render(renderer, batch, renders):
    """A render that keeps its stems hands the arrays to the caller: the whole mask is written whatever the option says, and the
    stems, knots and picks are those of mask_sparse 0."""
    prep, _ = batch
    a, b = _render(renderer, prep, 0, keep_stems=True), _render(renderer, prep, 1, keep_stems=True)
    _same(a, b, "control renders", ("harm", "uv", "bre", "mix", "knots", "picks"))
    for res in (a, b):
        assert not np.any(np.isnan(res["mask"]))
        assert np.array_equal(res["mask"].view(np.uint32), renders[0]["mask"].view(np.uint32))
        assert np.array_equal(res["knots"], renders[1]["knots"]) and np.array_equal(res["picks"], renders[1]["picks"])
        assert res["counts"] == renders[1]["counts"]


@pytest.mark.gpu
def test_f0_jitter_gets_the_whole_mask(renderer):
    """'sh' on one note: the route multiplies f0 by a jitter under the mask, sample by sample — nothing is left out."""
    spec = [BATCH[4], ("sh50", KW, _gaps_pattern), BATCH[7], BATCH[14]]
    prep, _, _ = MF._build(renderer, spec)
    a, b = _render(renderer, prep, 0), _render(renderer, prep, 1)
    _same(a, b, "sh batch", ("mix", "knots", "picks"))
    assert not np.any(np.isnan(b["mask"])) and np.array_equal(a["mask"].view(np.uint32), b["mask"].view(np.uint32))
    # (the same notes without the flag are left sparse)
    plain, _, _ = MF._build(renderer, [spec[0], ("t0", KW, _gaps_pattern), spec[2], spec[3]])
    assert np.any(np.isnan(_render(renderer, plain, 1)["mask"]))


@pytest.mark.gpu
def test_each_note_alone(renderer, batch, renders):
    """A note rendered as a batch of its own (other tiles, other strips, other neighbours) gives its samples of the batch."""
    prep, masks = batch
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    k_off = np.concatenate([[0], np.cumsum((np.diff(off) + 3) // 4)])
    for k in range(len(BATCH)):
        alone = MF._prepare(renderer, BATCH, masks, keep=[k])
        res = _render(renderer, alone, 1)
        assert np.all(np.isfinite(res["mix"])) and np.array_equal(res["mix"], renders[1]["mix"][off[k]:off[k + 1]]), k
        assert np.array_equal(res["knots"], renders[1]["knots"][k_off[k]:k_off[k + 1]]), k
