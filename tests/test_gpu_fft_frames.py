"""GPU: the framewise transform entry points on their own (csrc/fft.hip through Context.rfft_frames / Context.irfft_ola), row by
row and frame by frame against float64, one geometry per (owner, form) of with_transform:

  (44100, 1024, 256)   wave, native 512 points: k_rfft_frames (the hot kernel, two bins per store) / k_irfft_frames
  (44100,  768, 192)   wave, native 384 points: the 6-point first pass
  (16000,  130,  40)   wave, Bluestein L = 256, M = 65 odd
  (44100, 2046, 512)   wave, Bluestein L = 2048, M = 1023 odd, 32 points per lane
  (48000, 4096, 1024)  workgroup, native 2048 points
  (48000, 3000, 750)   workgroup, Bluestein L = 4096, tables re-read per frame

One ragged batch per geometry, notes of 1, hop, n_fft / 4 - 1 (frames that reflect more than once: reflect_index's modulo path),
n_fft, 37 hop + 3 and 5 hop samples of fp32 white noise: 52 or 53 frames, so a block boundary (32 frames for a wave-owned size, 16
for the workgroup) falls inside the long note and the last block is partial.

THE RULE is tests/synth_ref.py's, per unit: e_gpu <= 3 E_ref + 2^-23, both errors against a float64 truth and relative to the
unit's own peak; E_ref = the note's worst unit under numpy's fp32 transform and under synth_ref's plain radix-2 / chirp-z fp32
transform, whichever is larger; a unit whose truth is all zero must be all zero.  Forward: a unit is a spectrum row, the truth
np.fft.rfft of the float64 product of the reflect-padded frame and the device's own window (Context.table(0), held to numpy's by
test_plan_tables_match_reference).  Inverse: the device's own spectra go in; at the geometry's hop a unit is a note, at
hop = n_fft (every sample has one covering frame, so a frame shows through) a unit is the stretch of samples one frame covers;
the truth is synth_ref.istft(exact=True).  Everything else here is bit for bit.

MEASURED on the MI355X, worst unit per geometry and direction, E_ref / e_gpu (ratio = (e_gpu - 2^-23) / E_ref, floored at 0):
  geometry           forward                    inverse at the geometry's hop   inverse at hop = n_fft
  44100/1024/256     1.6e-07 / 1.8e-07 (0.38)   1.8e-07 / 1.7e-07 (0.28)        4.2e-06 / 6.3e-06 (1.46)
  44100/768/192      3.1e-07 / 1.7e-07 (0.17)   2.3e-07 / 2.3e-07 (0.48)        1.7e-05 / 2.0e-05 (1.15)
  16000/130/40       2.8e-07 / 2.6e-07 (0.49)   1.7e-07 / 2.4e-07 (0.71)        2.6e-06 / 4.0e-06 (1.50)
  44100/2046/512     3.2e-07 / 2.9e-07 (0.53)   2.2e-07 / 2.2e-07 (0.44)        2.5e-05 / 3.2e-05 (1.28)
  48000/4096/1024    1.9e-07 / 1.9e-07 (0.40)   1.7e-07 / 1.6e-07 (0.26)        6.5e-05 / 1.0e-04 (1.52)
  48000/3000/750     2.4e-07 / 2.9e-07 (0.70)   2.0e-07 / 2.3e-07 (0.54)        4.1e-05 / 5.5e-05 (1.33)
Every ratio is inside the factor 3 with the two yardsticks above; no third yardstick and no raised factor.  (At hop = n_fft the
normalisation divides a frame by its own window, which is as small as 1e-3 next to the frame's ends: the transform's error is
amplified there, for the yardsticks as for the device, so E_ref and e_gpu are both ten to some hundred times what they are at
the geometry's hop.)
"""
import numpy as np
import pytest

import synth_ref as SR
from oracle import goofer_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
GEOMETRIES = [(44100, 1024, 256), (44100, 768, 192), (16000, 130, 40), (44100, 2046, 512), (48000, 4096, 1024), (48000, 3000, 750)]
IDS = ["%d_%d_%d" % g for g in GEOMETRIES]
PATTERN = 0x7FC0DEAD                                               # a quiet NaN with a payload no kernel produces
GUARD_ROWS = 2
LONG, MID = 4, 5                                                   # the notes of 37 hop + 3 and of 5 hop samples

_CPU, _DEV = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def lengths(geo):
    sr, n_fft, hop = geo
    return [1, hop, n_fft // 4 - 1, n_fft, 37 * hop + 3, 5 * hop]


def frame_counts(geo):
    return [1 + n // geo[2] for n in lengths(geo)]


def signals(geo):
    rng = np.random.default_rng(geo[1] * 7 + geo[2])
    return [rng.standard_normal(n).astype(F32) for n in lengths(geo)]


def _off(ctx, counts):
    return ctx.tensor(ctx.offsets(counts))


def _frame_index(n, n_fft, hop):
    """[n_fft, T] indices into the note of every sample of every reflect-padded frame (numpy's own padding)."""
    idx = R.padded_signal(np.arange(n), n_fft).astype(np.int64)
    T = 1 + n // hop
    return idx[np.arange(n_fft)[:, None] + hop * np.arange(T)[None, :]]


def forward(ctx, geo, xs, out=None):
    """Context.rfft_frames over the notes ``xs``: the [F, n_bins] device view of the spectra."""
    ctx.plan(*geo)
    lens = [len(x) for x in xs]
    Ts = ctx.frame_counts(lens)
    S = ctx.rfft_frames(ctx.tensor(np.concatenate(xs)), _off(ctx, lens), _off(ctx, Ts), int(sum(Ts)), out=out)
    ctx.check()
    return S


def inverse(ctx, geo, hop, S, lens):
    """Context.irfft_ola of the rows ``S`` under the plan (sr, n_fft, hop), the notes ``lens`` samples long."""
    ctx.plan(geo[0], geo[1], hop)
    Ts = ctx.frame_counts(lens)
    assert int(sum(Ts)) == S.shape[0]
    y = ctx.irfft_ola(S, _off(ctx, lens), _off(ctx, Ts), int(sum(lens)))
    ctx.check()
    return y.cpu().numpy()


def one_frame_lengths(geo):
    """Note lengths with the batch's frame counts under hop = n_fft."""
    sr, n_fft, hop = geo
    return [(n // hop) * n_fft + n % hop for n in lengths(geo)]


def device(ctx, geo):
    """The clean batch, computed once per geometry and never written to: spectra (device view and host copy), the inverse at the
    geometry's hop and at hop = n_fft, the device's window."""
    if geo not in _DEV:
        xs = signals(geo)
        S = forward(ctx, geo, xs)
        win = ctx.table(0)
        assert win.shape == (geo[1],) and win.dtype == F32
        _DEV[geo] = {"xs": xs, "S": S, "S_host": S.cpu().numpy(), "win": win,
                     "y_hop": inverse(ctx, geo, geo[2], S, lengths(geo)),
                     "y_one": inverse(ctx, geo, geo[1], S, one_frame_lengths(geo))}
    return _DEV[geo]


def forward_refs(geo, win):
    """Per note (truth, numpy fp32, plain fp32) spectra, [T, bins] each: computed once."""
    key = (geo, "fwd")
    if key not in _CPU:
        sr, n_fft, hop = geo
        res = []
        for x in signals(geo):
            fr = x[_frame_index(len(x), n_fft, hop)]
            truth = np.fft.rfft(fr.astype(F64) * win.astype(F64)[:, None], axis=0).T
            fr32 = fr * win[:, None]
            assert fr32.dtype == F32
            res.append((truth, np.fft.rfft(fr32, axis=0).T, SR.rfft_plain(fr32).T))
        _CPU[key] = res
    return _CPU[key]


def _ratio(e, E):
    return max(0.0, (e - SR.EPS32) / E) if E > 0 else (0.0 if e <= SR.EPS32 else np.inf)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_forward_row_by_row(ctx, geo):
    d = device(ctx, geo)
    refs = forward_refs(geo, d["win"])
    Ts = frame_counts(geo)
    assert sum(Ts) > (32 if geo[1] <= 2048 else 16) and sum(Ts) % (32 if geo[1] <= 2048 else 16)
    bad, worst, o = [], (0.0, 0.0, 0.0), 0
    for k, (T, (truth, a, b)) in enumerate(zip(Ts, refs)):
        got = d["S_host"][o:o + T]
        o += T
        assert truth.shape == got.shape == (T, geo[1] // 2 + 1)
        E = max(float(SR.unit_errors(r, truth, "row").max()) for r in (a, b))
        e = SR.unit_errors(got, truth, "row")
        worst = max(worst, (_ratio(float(e.max()), E), E, float(e.max())))
        if not SR.within(e, E):
            t = int(np.argmax(e))
            bad.append(("note %d row %d of %d" % (k, t, T), "e_gpu %.3g  E_ref %.3g  ratio %.2f" % (e[t], E, _ratio(float(e[t]), E))))
    print("MEASURED %s forward  %.1e / %.1e (%.2f)" % ("%d/%d/%d" % geo, worst[1], worst[2], worst[0]))
    assert not bad, bad


def _fill(t):
    t.view(torch.int32).fill_(PATTERN)


def _is_pattern(a):
    return bool(np.all(_bits(a) == PATTERN))


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_row_stride_and_alignment(ctx, geo):
    """16-byte aligned rows with an even stride (k_rfft_frames: two bins per store), an odd stride, and rows that start 8 bytes off
    a 16-byte boundary give the same bits, and nothing outside the n_bins columns of the F rows is written."""
    d = device(ctx, geo)
    nb = geo[1] // 2 + 1
    F = d["S_host"].shape[0]
    from goofer_amd.device import spec_stride
    even = spec_stride(nb) + 16
    odd = nb + 2 if nb % 2 else nb + 3
    assert even % 2 == 0 and odd % 2 == 1 and odd > nb
    for tag, ld, shift in (("even stride, aligned", even, 0), ("odd stride", odd, 0), ("one column in", even, 1)):
        whole = torch.empty((F + GUARD_ROWS, ld), dtype=torch.complex64, device=ctx.device)
        real = torch.view_as_real(whole)
        _fill(real)
        assert whole.data_ptr() % 16 == 0
        out = whole[:F, shift:]
        assert out.stride(0) == ld and out.data_ptr() == whole.data_ptr() + 8 * shift
        S = forward(ctx, geo, d["xs"], out=out)
        host = real.cpu().numpy()                                   # [F + guard, ld, 2] float32
        assert _same_bits(S.cpu().numpy(), d["S_host"]), tag
        assert _is_pattern(host[F:]), (tag, "rows behind the last frame")
        assert _is_pattern(host[:F, shift + nb:]), (tag, "columns behind the bins")
        assert _is_pattern(host[:F, :shift]), (tag, "the column in front of the view")


def _segments(T, n_fft, total):
    """The stretch of a note's samples that frame t alone covers under hop = n_fft."""
    h = n_fft // 2
    return [(max(0, t * n_fft - h), min(total, (t + 1) * n_fft - h)) for t in range(T)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_inverse_note_by_note_and_frame_by_frame(ctx, geo):
    sr, n_fft, hop = geo
    d = device(ctx, geo)
    Ts = frame_counts(geo)
    bad = []
    for tag, hop2, lens, y in (("hop", hop, lengths(geo), d["y_hop"]), ("one", n_fft, one_frame_lengths(geo), d["y_one"])):
        worst, o, f = (0.0, 0.0, 0.0), 0, 0
        for k, (n, T) in enumerate(zip(lens, Ts)):
            St = d["S_host"][f:f + T].T
            got = y[o:o + n]
            o, f = o + n, f + T
            with np.errstate(all="ignore"):
                truth, a, b = (SR.istft(St, d["win"], hop2, n, ex, fft) for ex, fft in ((True, "numpy"), (False, "numpy"), (False, "plain")))
            live = hop2 * (T - 1)
            assert not got[live:].any(), (tag, k, "samples behind the last hop")
            assert not truth[live:].any()
            units = [(0, n)] if tag == "hop" else [s for s in _segments(T, n_fft, live) if s[1] > s[0]]
            if not units:
                continue
            err = lambda v: np.array([SR.unit_errors(v[lo:hi], truth[lo:hi], "note")[0] for lo, hi in units])
            E = max(float(err(a).max()), float(err(b).max()))
            e = err(got)
            worst = max(worst, (_ratio(float(e.max()), E), E, float(e.max())))
            if not SR.within(e, E):
                t = int(np.argmax(e))
                bad.append((tag, "note %d unit %d of %d" % (k, t, len(units)), "e_gpu %.3g  E_ref %.3g  ratio %.2f" % (e[t], E, _ratio(float(e[t]), E))))
        print("MEASURED %s inverse, %s  %.1e / %.1e (%.2f)" % ("%d/%d/%d" % geo, "hop %d" % hop2, worst[1], worst[2], worst[0]))
    assert not bad, bad


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_inverse_ignores_im_of_dc_and_nyquist(ctx, geo):
    """Random values, then NaN, in Im of bins 0 and n_fft / 2 of every row: the same output bits as zeros there (irfft_load drops
    them, like pocketfft's c2r)."""
    d = device(ctx, geo)
    M = geo[1] // 2
    rng = np.random.default_rng(3)
    for tag, fill in (("zeros", lambda F: np.zeros((F, 2), F32)), ("random", lambda F: rng.standard_normal((F, 2)).astype(F32) * 100),
                      ("NaN", lambda F: np.full((F, 2), np.nan, F32))):
        S = d["S"].clone()
        im = ctx.tensor(fill(S.shape[0]))
        torch.view_as_real(S)[:, 0, 1] = im[:, 0]
        torch.view_as_real(S)[:, M, 1] = im[:, 1]
        y = inverse(ctx, geo, geo[2], S, lengths(geo))
        assert _same_bits(y, d["y_hop"]), tag


def _covering_rows(geo, note, sample):
    """Frame indices (in the batch) whose padded frame holds ``sample`` of note ``note``."""
    sr, n_fft, hop = geo
    lens = lengths(geo)
    f0 = sum(1 + n // hop for n in lens[:note])
    idx = _frame_index(lens[note], n_fft, hop)
    return {f0 + int(t) for t in np.nonzero((idx == sample).any(axis=0))[0]}


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_forward_contains_a_nan_and_an_inf(ctx, geo):
    sr, n_fft, hop = geo
    d = device(ctx, geo)
    xs = [x.copy() for x in d["xs"]]
    at_nan, at_inf = 17 * hop + 5, 2 * hop + 1
    xs[LONG][at_nan] = np.nan
    xs[MID][at_inf] = np.inf
    hit = _covering_rows(geo, LONG, at_nan) | _covering_rows(geo, MID, at_inf)
    S = forward(ctx, geo, xs).cpu().numpy()
    clean = d["S_host"]
    assert 0 < len(hit) < S.shape[0]
    for f in range(S.shape[0]):
        if f in hit:                                               # every bin is a sum over every sample of the frame
            assert not np.isfinite(S[f].real).any(), ("row %d covers the sample and has finite bins" % f)
        else:
            assert _same_bits(S[f], clean[f]), ("row %d does not cover the sample and changed" % f)


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_inverse_contains_a_nan(ctx, geo):
    sr, n_fft, hop = geo
    d = device(ctx, geo)
    lens = lengths(geo)
    Ts = frame_counts(geo)
    t = 20
    row = int(sum(Ts[:LONG])) + t
    S = d["S"].clone()
    S[row, 3] = complex(float("nan"), 0.0)
    y = inverse(ctx, geo, hop, S, lens)
    a = int(sum(lens[:LONG]))
    lo, hi = max(0, t * hop - n_fft // 2), min(lens[LONG], t * hop + n_fft // 2)
    outside = np.ones(y.size, bool)
    outside[a + lo:a + hi] = False
    assert np.isnan(y[a + lo:a + hi]).any()
    assert np.array_equal(_bits(y)[outside], _bits(d["y_hop"])[outside])


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_a_note_alone_and_in_company(ctx, geo):
    sr, n_fft, hop = geo
    d = device(ctx, geo)
    lens = lengths(geo)
    Ts = frame_counts(geo)
    o = f = 0
    for k, (n, T) in enumerate(zip(lens, Ts)):
        S = forward(ctx, geo, [d["xs"][k]])
        assert _same_bits(S.cpu().numpy(), d["S_host"][f:f + T]), ("spectra of note %d" % k)
        y = inverse(ctx, geo, hop, S, [n])
        assert _same_bits(y, d["y_hop"][o:o + n]), ("samples of note %d" % k)
        o, f = o + n, f + T
