"""The f0 / mask kernel with its tile-note table (k_sample_tile_notes, option "sa_table") against itself with the per-workgroup
search and against the per-sample path (option "sa_fast" 0): every word of f0 and mask equal.

One ragged batch of small notes (n_fft 1024 / hop 256): 1, 255, 1024, 1025 and 4097 samples, then notes of 2205 and 300, so that
tiles begin and end inside notes, on their first and last samples, and hold three notes; flat and steep pitch curves and one
whose ticks fall on sample instants (110.25 bpm: 250 samples per tick); reversed, tiled tail, force-voiced; fractional,
all-zero and -0.0 masks; a velocity stretch and a fry note, which take the per-sample path next to the others.  The table is
read back through what it decides: the batch against every note alone, whose table has one note.  The curves are written over
the batch's pitch-bend array on the device.
"""
import numpy as np
import pytest

from goofer_amd import synthetic as syn

SR = 44100
SEED = 29


def _ms(n):
    return (n + 0.3) * 1000.0 / SR


_T = lambda n: dict(length_ms=_ms(n), consonant_ms=0.0)
_S = dict(length_ms=50.0, consonant_ms=0.0)                   # 2205 samples
# (flags, request keywords, mask, curve)
SPEC = [
    ("t0", _T(1), "ones", "flat"),
    ("t0", _T(255), "ones", "steep"),
    ("t0", dict(_T(1024), tempo=110.25), "ones", "steep"),     # ticks on sample instants
    ("t0", _T(1025), "fraction", "own"),
    ("t0", _T(4097), "minus_zero", "steep"),
    ("R1", dict(length_ms=60.0, consonant_ms=40.0), "fraction", "steep"),
    ("L1", dict(length_ms=450.0), "own", "own"),               # tiled tail
    ("FV1", _S, "zeros", "steep"),
    ("t0", _S, "zeros", "own"),
    ("t0", _S, "ones", "flat"),
    ("t0", _S, "fraction", "own"),
    ("t0", dict(length_ms=60.0, velocity=70.0), "own", "own"),  # velocity stretch: sample_assemble_one
    ("vf60", dict(length_ms=60.0), "own", "steep"),            # fry: sample_assemble_one
    ("t0", _T(300), "fraction", "flat"),
]


def _masks(ylen):
    rng = np.random.default_rng(SEED)
    frac = rng.random(ylen).astype(np.float32)
    frac[::7] = 0.0
    frac[3::11] = -0.0
    mz = np.zeros(ylen, dtype=np.float32)
    mz[::3] = -0.0
    mz[ylen // 2:] = 1.0
    return {"ones": np.ones(ylen, dtype=np.float32), "zeros": np.zeros(ylen, dtype=np.float32), "fraction": frac, "minus_zero": mz, "own": None}


def _curve(kind, own, k):
    n = own.size
    if kind == "own":
        return own
    if kind == "flat":
        return np.full(n, 61.25 + k)
    return 60.0 + 12.0 * (-1.0) ** np.arange(n) + 0.01 * np.arange(n)      # steep


def _prepare(r, keep):
    from goofer_amd import _lib
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    import torch
    ylen = syn.make_source(4100, seconds=0.45)["y_len"]
    masks = _masks(ylen)
    jobs = []
    for k in keep:
        flags, kw, mk, _ = SPEC[k]
        src = syn.make_source(4100 + k, seconds=0.45)
        m = src["mask"] if masks[mk] is None else masks[mk]
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], m, src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*syn.request_args(syn.make_request(4100 + k, flags, **kw)))))
    np.random.seed(SEED)
    prep = r.prepare(jobs, note_ids=list(keep))
    plans = prep["keep"]["notes"].cpu().numpy().view(_lib.NOTE_PLAN)
    bend = prep["keep"]["bend"].cpu().numpy().copy()
    for q, k in enumerate(keep):
        lo, n = int(plans["bend_off"][q]), int(plans["n_bend"][q])
        bend[lo:lo + n] = _curve(SPEC[k][3], bend[lo:lo + n], k)
    prep["keep"]["bend"].copy_(torch.from_numpy(bend))
    torch.cuda.synchronize()
    return prep


def _assemble(r, prep, **opts):
    """f0 and mask (uint32 words) of goofer_assemble_batch under the options."""
    import torch
    ctx = r.ctx
    defaults = dict(sa_fast=1, sa_table=1)
    try:
        for k, v in dict(defaults, **opts).items():
            ctx.set_option(k, v)
        prep["f0"].fill_(-7.0)
        prep["mask"].fill_(-7.0)
        r.assemble(prep)
        torch.cuda.synchronize()
    finally:
        for k, v in defaults.items():
            ctx.set_option(k, v)
    return prep["f0"].cpu().numpy().view(np.uint32).copy(), prep["mask"].cpu().numpy().view(np.uint32).copy()


@pytest.fixture(scope="module")
def renderer():
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    ctx = Context(0)
    yield Renderer(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def batch(renderer):
    keep = list(range(len(SPEC)))
    prep = _prepare(renderer, keep)
    ref = _assemble(renderer, prep, sa_fast=0)
    return prep, ref


@pytest.mark.gpu
def test_batch_word_for_word(renderer, batch):
    prep, (f0_ref, mask_ref) = batch
    off = np.asarray(prep["sample_off"], dtype=np.int64)
    lens = np.diff(off)
    assert lens[:5].tolist() == [1, 255, 1024, 1025, 4097] and lens[13] == 300
    assert not np.any(f0_ref == np.float32(-7.0).view(np.uint32)) and not np.any(mask_ref == np.float32(-7.0).view(np.uint32))
    for table in (1, 0):
        f0, mask = _assemble(renderer, prep, sa_table=table)
        for k in range(len(SPEC)):
            a, b = slice(off[k], off[k + 1]), (table, k, SPEC[k])
            assert np.array_equal(mask[a], mask_ref[a]), ("mask", b)
            assert np.array_equal(f0[a], f0_ref[a]), ("f0", b)
    # what the cases are there for arrived
    f0, m = f0_ref.view(np.float32), mask_ref.view(np.float32)
    assert np.any(np.signbit(m[off[4]:off[5]]) & (m[off[4]:off[5]] == 0)) and np.any((m[off[3]:off[4]] > 0) & (m[off[3]:off[4]] < 1))
    assert np.all(m[off[7]:off[8]] == 1.0) and np.all(m[off[8]:off[9]] == 0.0) and np.all(f0[off[8]:off[9]] == 0.0)
    assert np.all(f0[off[9]:off[10]] > 50.0)


@pytest.mark.gpu
def test_every_note_alone(renderer, batch):
    bprep, (f0_ref, mask_ref) = batch
    off = np.asarray(bprep["sample_off"], dtype=np.int64)
    for k in range(len(SPEC)):
        prep = _prepare(renderer, [k])
        slow = _assemble(renderer, prep, sa_fast=0)
        assert np.array_equal(slow[0], f0_ref[off[k]:off[k + 1]]) and np.array_equal(slow[1], mask_ref[off[k]:off[k + 1]]), ("batch", k)
        for opts in (dict(), dict(sa_table=0)):
            f0, mask = _assemble(renderer, prep, **opts)
            assert np.array_equal(f0, slow[0]) and np.array_equal(mask, slow[1]), (k, SPEC[k], opts)


@pytest.mark.gpu
def test_tile_flags_and_stems_equal(renderer):
    """The render path (the kernel with tile flags, on the side stream): stems, mix and k_mask_short's two counters, which only
    agree if the flag words do, with the table and with the search."""
    import torch
    r, ctx = renderer, renderer.ctx
    prep = _prepare(r, list(range(len(SPEC))))
    res = {}
    for v in (1, 0):
        try:
            ctx.set_option("sa_table", v)
            c0 = (ctx.counter("mask_flag_segments"), ctx.counter("mask_staged_segments"))
            out = r.run(prep, seed=SEED, keep_stems=True)
            ctx.check()
            torch.cuda.synchronize()
            res[v] = {k: out[k].cpu().numpy().copy() for k in ("harm", "uv", "bre", "mix")}
            res[v]["f0"], res[v]["mask"] = prep["f0"].cpu().numpy().copy(), prep["mask"].cpu().numpy().copy()
            res[v]["knots"] = ctx.debug_fetch("mask_short").copy()
            res[v]["counts"] = (ctx.counter("mask_flag_segments") - c0[0], ctx.counter("mask_staged_segments") - c0[1])
        finally:
            ctx.set_option("sa_table", 1)
    for k in ("f0", "mask", "knots", "harm", "uv", "bre", "mix"):
        assert res[0][k].shape == res[1][k].shape and np.array_equal(res[0][k].view(np.uint8), res[1][k].view(np.uint8)), k
    print("k_mask_short (flagged, staged):", res[1]["counts"])
    assert res[0]["counts"] == res[1]["counts"] and sum(res[1]["counts"]) > 0
