"""GPU: the caller-scratch protocol (include/goofer_hip.h) of the eight exports that take scratch from the caller, run with the
arguments the Context methods pass.  A block of exactly the reported size gives the methods' bits and is not written past
its end; a block one byte short is refused before anything is launched; goofer_envelope_knots_batch's query is scratch =
NULL whatever y is."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SR, HOP, LENGTHS = 44100, 256, [9000, 14000]
EXPORTS = ["goofer_track_pitch", "goofer_track_formants", "goofer_track_candidates", "goofer_track_path", "goofer_track_resample",
           "goofer_track_formant_frames", "goofer_per_sample_f0", "goofer_envelope_knots_batch"]


@pytest.fixture(scope="module")
def calls():
    """export name -> (fn, args, output makers, tail, the outputs the method got), recorded from the eight Context methods"""
    from goofer_amd.device import Context
    ctx = Context(0).plan(SR, 1024, HOP)
    rec, helper = {}, ctx._scratch_call

    def spy(fn, args, outs=(), tail=()):
        outs = [lambda make=make: None if (t := make()) is None else t.zero_() for make in outs]   # unwritten parts compare equal
        res, call = helper(fn, args, outs, tail)
        rec[fn.__name__] = (fn, args, outs, tail, [None if r is None else r.clone() for r in res])
        return res, call
    ctx._scratch_call = spy
    t = np.arange(sum(LENGTHS)) / SR
    y = ctx.tensor(np.sin(2 * np.pi * 180 * t) + 0.3 * np.sin(2 * np.pi * 360 * t) + 0.01 * np.random.default_rng(7).standard_normal(t.size))
    y32 = y.float().contiguous()                                                    # the inputs live as long as the records
    f0, p_off, _, _ = ctx.track(y, LENGTHS, SR, HOP)
    cf, cs, cn, c_off = ctx.track_candidates(y, LENGTHS, SR, HOP)
    ctx.track_path(cf, cs, cn, c_off, SR, HOP)
    x11, x_off = ctx.track_resample(y, LENGTHS, SR)
    ctx.track_formant_frames(x11, np.diff(x_off), SR, HOP)
    ctx.per_sample_f0(f0, np.diff(p_off), LENGTHS, SR)
    ctx.envelope_knots(y32, LENGTHS, want_env=True)
    del ctx._scratch_call
    assert sorted(rec) == sorted(EXPORTS)
    yield ctx, rec
    ctx.close()


def _query(ctx, fn, args, n_outs, tail):
    need = C.c_int64(-1)
    ctx._check(fn(ctx.h, *args, *[None] * n_outs, *tail, None, C.byref(need), None))
    assert need.value > 0
    return need.value


@pytest.mark.parametrize("name", EXPORTS)
def test_exact_block_works_and_one_byte_short_is_refused(calls, name):
    from goofer_amd.device import GooferError, _ptr
    ctx, rec = calls
    fn, args, outs, tail, ref = rec[name]
    need = _query(ctx, fn, args, len(outs), tail)
    for short in (1, 0):
        res = [make() for make in outs]
        assert [None if r is None else r.shape for r in res] == [None if w is None else w.shape for w in ref]
        block = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=ctx.device)   # guard bytes behind the reported size
        size = C.c_int64(need - short)
        rc = fn(ctx.h, *args, *map(_ptr, res), *tail, _ptr(block), C.byref(size), ctx._stream())
        torch.cuda.synchronize()
        if short:
            with pytest.raises(GooferError, match=f"scratch of {need - 1} bytes, {need} needed"):
                ctx._check(rc)
            assert not any(bool(r.any()) for r in res if r is not None) and bool((block == 0xA5).all())   # nothing copied or run
        else:
            ctx._check(rc)
            assert bool((block[need:] == 0xA5).all())
            for got, want in zip(res, ref):
                assert (got is None and want is None) or np.array_equal(got.cpu().numpy(), want.cpu().numpy(), equal_nan=True)


def test_envelope_query_is_scratch_null_whatever_y_is(calls):
    ctx, rec = calls
    fn, args, outs, tail, _ = rec["goofer_envelope_knots_batch"]
    f_off = np.full(len(LENGTHS) + 1, -1, dtype=np.int64)
    args = (*args[:-1], f_off.ctypes.data_as(C.c_void_p))
    assert args[0].value                                                            # y: the device signal
    need = _query(ctx, fn, args, len(outs), tail)
    assert f_off.tolist() == [0, *np.cumsum([1 + n // HOP for n in LENGTHS]).tolist()]
    assert _query(ctx, fn, (None, *args[1:]), len(outs), tail) == need
