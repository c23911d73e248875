"""GPU: goofer_legacy_normal_fill (k_legacy_normal_fill, noise.hip) against numpy's own ``np.random.seed(s); np.random.randn(n)``
and the restatement of the stream (tests/mt_ref.py).

The bound.  Everything in the stream but ``log`` is exact integer or correctly rounded float64 arithmetic, and the acceptance of
an attempt does not depend on ``log``: a value can differ from numpy's by what the device's and the host's ``log`` differ in
their last place, carried through one division, one square root and one product (a few ulps of 1.1e-16), while a wrong stream
differs by order 1.  So: attempts counted exactly, every value within relative 1e-14.

Measured on an MI355X (142 738 normals, either kernel): worst relative difference 3.96e-16, worst 2 ulp, 98.886 % of the samples
bit-equal to numpy's."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mt_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENGTHS = [0, 1, 2, 3, 245, 311, 623, 624, 625, 1251, 20001]
PATTERNS = [(0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1)]                       # none, f0 (sh), vol (sr), both
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """every length under every on-pattern (and one note with harmonic volume off, breath on: the third stream behind the
    first), seeds 0 and 2^32 - 1 among them; per note numpy's own draws and the restatement's attempt count"""
    notes = [(n, on) for on, n in itertools.product(PATTERNS, LENGTHS)] + [(311, (1, 0, 1))]
    rng = np.random.default_rng(12)
    seeds = [int(v) for v in rng.integers(0, 2 ** 32, len(notes))]
    big = [i for i, (n, on) in enumerate(notes) if n == 20001 and on == (1, 1, 1)][0]
    odd = [i for i, (n, on) in enumerate(notes) if n == 1251 and on == (1, 1, 1)][0]
    seeds[big], seeds[odd], seeds[3] = 0, 2 ** 32 - 1, 2 ** 32 - 1
    lens = [n for n, _ in notes]
    on = np.array([o for _, o in notes], dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[-1])
    ref = np.full((3, total), np.nan)
    attempts = np.zeros(len(notes), dtype=np.int64)
    state = np.random.get_state()
    try:
        for i, ((n, o), s) in enumerate(zip(notes, seeds)):
            np.random.seed(s)
            for k in range(3):
                if o[k]:
                    ref[k, off[i]:off[i + 1]] = np.random.randn(n)
            attempts[i] = mt_ref.draw(s, n * int(sum(o)))[1]
    finally:
        np.random.set_state(state)
    ref.setflags(write=False)
    return {"notes": notes, "seeds": seeds, "lens": lens, "on": on, "off": off, "total": total, "ref": ref, "attempts": attempts, "odd": odd}


def _guarded(ctx, total):
    raw = [torch.full((total + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.device) for _ in range(3)]
    return raw, tuple(r[GUARD:GUARD + total] for r in raw)


def _ulps(a, b):
    """distance of two float64 arrays in units in the last place (same sign or zero: the values here agree to 1e-14)"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize("wave", [0, 1])
def test_ragged_batch_against_numpy(ctx, batch, wave):
    b = batch
    raw, out = _guarded(ctx, b["total"])
    ctx.set_option("legacy_wave", wave)
    try:
        got, att = ctx.legacy_normal_fill(b["seeds"], b["lens"], b["on"], out=out, attempts=True)
        ctx.check()
    finally:
        ctx.set_option("legacy_wave", 0)
    assert np.array_equal(att.cpu().numpy(), b["attempts"])                  # the acceptances: exactly the restatement's
    host = np.stack([r.cpu().numpy() for r in raw])
    assert np.isnan(host[:, :GUARD]).all() and np.isnan(host[:, -GUARD:]).all()   # nothing in front of or behind an output
    z, ref = host[:, GUARD:-GUARD], b["ref"]
    written = ~np.isnan(ref)
    assert np.array_equal(np.isnan(z), ~written)                             # streams that are off: untouched
    zv, rv = z[written], ref[written]
    rel = np.abs(zv - rv) / np.abs(rv)
    u = _ulps(zv, rv)
    print(f"legacy_wave={wave}: {zv.size} normals, worst relative difference {rel.max():.3e}, worst {int(u.max())} ulp, "
          f"bit-equal {100.0 * float((u == 0).mean()):.3f} %")
    assert float(rel.max()) <= 1e-14
    # the expected ~245 normals per block: no note came near its block bound
    m = np.array([n * int(sum(o)) for n, o in b["notes"]])
    blocks = -(-b["attempts"] // mt_ref.ATTEMPTS)
    assert (blocks <= 2 * -(-m // 245) + 4).all()


def test_one_wave_and_one_workgroup_draw_the_same_bits(ctx, batch):
    b = batch
    res = []
    for wave in (0, 1):
        ctx.set_option("legacy_wave", wave)
        try:
            _, out = _guarded(ctx, b["total"])
            ctx.legacy_normal_fill(b["seeds"], b["lens"], b["on"], out=out)
            ctx.check()
            res.append([torch.nan_to_num(t, nan=7.0) for t in out])
        finally:
            ctx.set_option("legacy_wave", 0)
    assert all(torch.equal(a, c) for a, c in zip(*res))


def test_device_offsets_and_out_fill_the_rows_given(ctx, batch):
    """the Renderer's call: device seeds, device offsets, device switches, two of the three outputs"""
    b = batch
    d_s = ctx.tensor(np.asarray(b["off"], dtype=np.int64))
    d_seed = ctx.tensor(np.asarray(b["seeds"], dtype=np.uint32).view(np.int32))
    d_on = ctx.tensor(b["on"].reshape(-1))
    raw, out = _guarded(ctx, b["total"])
    ret = ctx.legacy_normal_fill(d_seed, d_s, d_on, out=(out[0], None, out[2]))
    ctx.check()
    assert ret[0] is out[0] and ret[1] is None and ret[2] is out[2]
    host = np.stack([r.cpu().numpy() for r in raw])
    assert np.isnan(host[1]).all()                                           # the dropped stream: consumed, not stored
    for k in (0, 2):
        assert np.isnan(host[k, :GUARD]).all() and np.isnan(host[k, -GUARD:]).all()
        z, ref = host[k, GUARD:-GUARD], b["ref"][k]
        w = ~np.isnan(ref)
        assert np.array_equal(np.isnan(z), ~w)
        assert float((np.abs(z[w] - ref[w]) / np.abs(ref[w])).max()) <= 1e-14
    with pytest.raises(ValueError):
        ctx.legacy_normal_fill(d_seed, d_s, d_on)                            # device offsets need out=


def test_a_note_draws_the_same_alone_and_in_the_batch(ctx, batch):
    b = batch
    _, out = _guarded(ctx, b["total"])
    ctx.legacy_normal_fill(b["seeds"], b["lens"], b["on"], out=out)
    for i in (b["odd"], len(b["notes"]) - 1, 1 + len(LENGTHS)):              # all three streams, (1, 0, 1), one sample of f0
        n, on = b["notes"][i]
        alone = ctx.legacy_normal_fill([b["seeds"][i]], [n], [on])
        ctx.check()
        lo, hi = int(b["off"][i]), int(b["off"][i + 1])
        for k in range(3):
            if on[k]:
                assert torch.equal(alone[k], out[k][lo:hi]), (i, k)


def test_bad_arguments_are_refused_before_a_launch(ctx):
    from goofer_amd.device import GooferError, _ptr
    d_seed = ctx.tensor(np.array([5, 1, 2], dtype=np.int32))
    d_s = ctx.tensor(ctx.offsets([3, 4]))
    d_on = ctx.tensor(np.ones(6, dtype=np.uint8))
    raw = torch.full((3 * 8 * 7 + 16,), 0xA5, dtype=torch.uint8, device=ctx.device)
    outs = [raw[56 * k:56 * (k + 1)].view(torch.float64) for k in range(3)]
    d_att = torch.full((2,), -1, dtype=torch.int64, device=ctx.device)
    fill = lambda *a: ctx.lib.goofer_legacy_normal_fill(ctx.h, *a, ctx._stream())   # noqa: E731
    good = (_ptr(d_seed[1:]), _ptr(d_on), _ptr(d_s), 2, 7, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(d_att))
    for k, bad in ((0, None), (1, None), (2, None), (3, -1), (4, -1),
                   (0, C.c_void_p(d_seed.data_ptr() + 2)), (2, C.c_void_p(d_s.data_ptr() + 4)), (5, C.c_void_p(raw.data_ptr() + 4)),
                   (6, C.c_void_p(raw.data_ptr() + 60)), (7, C.c_void_p(raw.data_ptr() + 2)), (8, C.c_void_p(d_att.data_ptr() + 4))):
        args = list(good)
        args[k] = bad
        with pytest.raises(GooferError):
            ctx._check(fill(*args))
    with pytest.raises(GooferError):
        ctx._check(fill(*good[:5], None, None, None, None))                  # no output at all
    ctx.check()
    assert bool((raw == 0xA5).all()) and bool((d_att == -1).all())           # nothing ran
    with pytest.raises(ValueError):
        ctx.legacy_normal_fill([1, 2], [3], [(1, 1, 1)])                     # one seed per note
    for bad in (-1, 2 ** 32, 1.5, True, None):
        with pytest.raises(ValueError):
            ctx.legacy_normal_fill([bad], [3], [(1, 0, 0)])
    with pytest.raises(ValueError):
        ctx.legacy_normal_fill([1], [3], [(1, 1)])                           # three switches per note
    with pytest.raises(ValueError):
        ctx.legacy_normal_fill([1], [-3], [(1, 1, 1)])
    with pytest.raises(ValueError):
        ctx.legacy_normal_fill([1], [3], [(1, 1, 1)], out=(torch.empty(4, dtype=torch.float64, device=ctx.device), None, None))
