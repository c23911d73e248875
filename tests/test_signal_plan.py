"""The layout the finishing stages' plans share (goofer_amd/signal_plan.py), pinned on one ragged batch: the tile table of the
limiter, the loudness stage and the compressor, every plan's blob as the bytes of its documented fields in the documented order,
the refusals every ``plan()`` makes before it calls the library, and the empty batch.  Pure host code: no GPU."""
import numpy as np
import pytest

from goofer_amd import compress as CP
from goofer_amd import limit as LM
from goofer_amd import loudness as LD
from goofer_amd import phrase as P
from goofer_amd import rate as RT

SR = 48000
TILE = 4096
LENS = [0, 1, 4095, 4096, 4097, 0, 8193]
SETTINGS = CP.Compressor(-20.0, 4.0)


def _bytes(*arrays):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).ravel() for a in arrays])


def _signal_plans(lens, sr=SR):
    return {"limit": LM.plan(sr, lens), "true_peak": LM.plan(sr, lens, true_peak=True), "loudness": LD.plan(sr, lens),
            "compress": CP.plan(sr, lens, SETTINGS), "rate": RT.plan(44100, sr, lens)}


def test_one_tile_table_for_the_three_tiled_stages():
    assert LM.TILE == LD.TILE == CP.TILE == TILE
    want = np.array([(i, k) for i, n in enumerate(LENS) for k in range(-(-n // TILE))], dtype=np.int32)
    assert want.shape == (1 + 1 + 1 + 2 + 3, 2)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    for name, plan in _signal_plans(LENS).items():
        assert plan.n == len(LENS) and plan.in_off.dtype == np.int64 and np.array_equal(plan.in_off, off), name
        if name == "rate":
            assert plan.total_in == sum(LENS) and plan.total_out == int(plan.out_off[-1])
            continue
        assert plan.total == sum(LENS) and plan.n_tiles == len(want), name
        assert plan.tiles.dtype == np.int32 and plan.tiles.shape == want.shape and np.array_equal(plan.tiles, want), name


def test_every_blob_is_its_documented_fields_back_to_back():
    p = _signal_plans(LENS)
    for name in ("limit", "true_peak"):
        lm = p[name]
        assert lm.true_peak == (name == "true_peak") and lm.tp_taps.size == (0 if name == "limit" else (lm.R - 1) * 2 * lm.Z)
        assert np.array_equal(lm.blob, _bytes(lm.in_off, lm.tiles, lm.taps, lm.tp_taps)), name
        assert lm.blob.dtype == np.uint8 and lm.blob.nbytes == 8 * (len(LENS) + 1) + 8 * lm.n_tiles + 4 * (2 * lm.W + 1) + 4 * lm.tp_taps.size
    ld = p["loudness"]
    assert np.array_equal(ld.blob, _bytes(ld.in_off, ld.seg_off, ld.coef, ld.mats, ld.tiles))
    assert ld.blob.nbytes == 2 * 8 * (len(LENS) + 1) + 8 * 10 + 8 * LD.MATS * 16 + 8 * ld.n_tiles
    cp = p["compress"]
    assert np.array_equal(cp.blob, _bytes(cp.in_off, cp.coef, cp.pows, cp.tiles))
    assert cp.blob.nbytes == 8 * (len(LENS) + 1) + 8 * CP.COEF + 8 * 2 * CP.POWS + 8 * cp.n_tiles
    rt = p["rate"]
    assert rt.taps.shape == (rt.L, 2 * rt.H) and np.array_equal(rt.blob, _bytes(rt.in_off, rt.out_off, rt.taps))
    ph = P.plan_phrase(["0 100 5 35 40 0 100 100 0"] * len(LENS), LENS, SR)
    assert ph.n == len(LENS) and ph.tile_off.dtype == np.int64 and ph.tile_notes.dtype == np.int32
    assert np.array_equal(ph.blob, _bytes(ph.notes, ph.tile_off, ph.tile_notes, np.zeros(1, dtype=np.int32)))     # the pad word
    empty = P.plan_records(np.zeros(0, dtype=ph.notes.dtype), [], 0)
    assert empty.blob.nbytes == 8 + 4 and not empty.blob.any()


def test_every_plan_refuses_a_negative_length_and_a_fractional_rate():
    for lens in ([3, -1], [-5]):
        for make in (lambda l: LM.plan(SR, l), lambda l: LM.plan(SR, l, true_peak=True), lambda l: LD.plan(SR, l),
                     lambda l: CP.plan(SR, l, SETTINGS), lambda l: RT.plan(44100, SR, l)):
            with pytest.raises(ValueError, match="negative length"):
                make(lens)
    for make in (lambda sr: LM.plan(sr, LENS), lambda sr: LM.true_peak_table(sr), lambda sr: LD.plan(sr, LENS),
                 lambda sr: CP.plan(sr, LENS, SETTINGS)):       # (rate.plan takes whole numbers of Hz: it has no such refusal)
        with pytest.raises(ValueError, match="whole number of Hz"):
            make(44100.5)
        make(44100.0)


def test_an_empty_batch():
    for name, plan in _signal_plans([]).items():
        assert plan.n == 0 and plan.in_off.tolist() == [0], name
        if name == "rate":
            assert plan.total_in == 0 and plan.total_out == 0 and plan.out_off.tolist() == [0]
        else:
            assert plan.total == 0 and plan.n_tiles == 0 and plan.tiles.shape == (0, 2), name
