"""GPU: the seeded phases made on the device (goofer_phase_fill) against numpy itself, exact equality everywhere — the kernel
alone on ragged batches, then through core.synthesize / synthesize_batch (phi_seed= against phi=<the numpy array>) and through
Renderer (phi_seeds= against the same prepared batch fed the host-made matrix, what the renderer did before the kernel)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from goofer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = [0, 1, 6003, 2 ** 32 + 5, 2 ** 64 - 1, 2 ** 127]
# one ragged batch: tiles of 64 frames cross the note boundaries; notes 5 and 6 share a seed and a shape, notes 1 and 7 a seed
BATCH_SEEDS = SEEDS + [2 ** 127, 1]
BATCH_FRAMES = [1, 2, 63, 64, 65, 190, 190, 3]


def numpy_phi(seed, n_bins, T):
    return np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=(n_bins, T)).astype(np.float32)


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n_bins", [33, 513, 1025, 2049])
def test_ragged_batch_equals_numpy(ctx, n_bins):
    rows = ctx.phase_fill(BATCH_SEEDS, BATCH_FRAMES, n_bins=n_bins)
    assert rows.shape == (sum(BATCH_FRAMES), n_bins) and rows.dtype == torch.float32
    got = rows.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(BATCH_FRAMES)])
    for i, (seed, T) in enumerate(zip(BATCH_SEEDS, BATCH_FRAMES)):
        assert np.array_equal(got[off[i]:off[i + 1]].T, numpy_phi(seed, n_bins, T)), (i, seed, T)
    assert np.array_equal(got[off[5]:off[6]], got[off[6]:off[7]])           # the same seed and shape: the same note


def test_one_long_note(ctx):
    """513 bins x 2048 frames: the draw index passes 2^20"""
    got = ctx.phase_fill([6003], [2048], n_bins=513).cpu().numpy()
    assert np.array_equal(got.T, numpy_phi(6003, 513, 2048))


def test_device_offsets_and_records_fill_the_rows_given(ctx):
    """the Renderer's form: staged records and the batch's device frame offsets, into rows made by the caller"""
    from goofer_amd.device import pcg64_words
    frames, seeds = [5, 70, 1], [2 ** 64 - 1, 0, 6003]
    d_w = ctx.tensor(pcg64_words(seeds).view(np.int64))
    d_f = ctx.tensor(ctx.offsets(frames))
    out = ctx.rows(sum(frames), 513)
    assert ctx.phase_fill(d_w, d_f, out=out) is out
    got, off = out.cpu().numpy(), np.concatenate([[0], np.cumsum(frames)])
    for i in range(3):
        assert np.array_equal(got[off[i]:off[i + 1]].T, numpy_phi(seeds[i], 513, frames[i]))


def test_nothing_is_written_outside_the_matrix(ctx):
    """an oversized, byte-filled buffer: the rows behind the last one, the padding columns of every row and the rows of a
    note without a seed keep their bytes"""
    from goofer_amd.device import row_stride
    n_bins, frames, seeds = 513, [65, 7, 64, 1], [1, None, 6003, 2 ** 127]
    ld, total, guard = row_stride(n_bins), sum(frames), 64
    assert ld > n_bins
    raw = torch.full(((total + guard) * ld * 4,), 0xA5, dtype=torch.uint8, device=ctx.device)
    buf = raw.view(torch.float32).view(total + guard, ld)
    ctx.phase_fill(seeds, frames, out=buf[:total, :n_bins])
    host = raw.cpu().numpy().reshape(total + guard, ld * 4)
    assert (host[total:] == 0xA5).all()                                      # behind the matrix's last row
    assert (host[:, 4 * n_bins:] == 0xA5).all()                             # columns n_bins .. ld - 1
    assert (host[65:72] == 0xA5).all()                                       # the note that is not seeded
    got, off = host.view(np.float32), np.concatenate([[0], np.cumsum(frames)])
    for i in (0, 2, 3):
        assert np.array_equal(got[off[i]:off[i + 1], :n_bins].T, numpy_phi(seeds[i], n_bins, frames[i]))


def test_bad_arguments_are_refused_before_a_launch(ctx):
    from goofer_amd.device import GooferError, _ptr, pcg64_words
    d_w = ctx.tensor(np.concatenate([[0], pcg64_words([1, 2]).view(np.int64).ravel()]))   # one spare word in front: [1:] is 8-byte aligned only
    d_f = ctx.tensor(ctx.offsets([3, 4]))
    raw = torch.full((8 * 516 * 4 + 16,), 0xA5, dtype=torch.uint8, device=ctx.device)
    out = raw[:8 * 516 * 4].view(torch.float32)
    fill = lambda w, f, n, total, nb, o, ld: ctx.lib.goofer_phase_fill(ctx.h, w, f, n, total, nb, o, ld, ctx._stream())   # noqa: E731
    good = (_ptr(d_w[1:]), _ptr(d_f), 2, 7, 513, _ptr(out), 516)
    for k, bad in ((0, None), (1, None), (5, None), (2, -1), (3, -1), (4, 0), (6, 512),
                   (0, C.c_void_p(d_w.data_ptr() + 12)), (1, C.c_void_p(d_f.data_ptr() + 4)), (5, C.c_void_p(raw.data_ptr() + 2))):
        args = list(good)
        args[k] = bad
        with pytest.raises(GooferError):
            ctx._check(fill(*args))
    ctx.check()
    assert bool((raw == 0xA5).all())                                         # nothing ran
    with pytest.raises(ValueError):
        ctx.phase_fill([1, 2], [3])                                          # one seed per note
    with pytest.raises(ValueError):
        ctx.phase_fill([-1], [3], n_bins=33)
    with pytest.raises(ValueError):
        ctx.phase_fill([1], [3], out=torch.empty((4, 516), dtype=torch.float32, device=ctx.device)[:, :513])   # four rows for three frames


# ---- core.synthesize / synthesize_batch -------------------------------------------------------------------------------------
def _note(sr, n_fft, hop, seconds=0.25, seed=0):
    rng = np.random.default_rng(seed)
    B, n = n_fft // 2 + 1, int(seconds * sr)
    T = 1 + n // hop
    env = (np.exp(0.3 * rng.standard_normal((B, 1))) * np.linspace(1.0, 0.05, B)[:, None] * (1.0 + 0.2 * rng.random((B, T)))).astype(np.float32)
    t = np.arange(n) / sr
    f0 = (180.0 + 20.0 * np.sin(2 * np.pi * 5.0 * t) + 3.0 * seed).astype(np.float32)
    mask = (t < 0.6 * seconds).astype(np.float32)                            # voiced, then unvoiced: every stem is heard
    return {"env_spec": env, "f0_interp": f0 * mask, "voicing_mask": mask, "y": np.empty(n, bool)}, n


def _same(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.float32 and x.shape == y.shape
        assert np.array_equal(x, y)
    assert float(np.abs(a[2]).max()) > 0.0 and float(np.abs(a[3]).max()) > 0.0   # the aperiodic stems carry the phases


@pytest.mark.parametrize("sr,n_fft,hop", [(44100, 1024, 256), (96000, 2048, 96), (44100, 1000, 250), (96000, 4096, 1024)])
def test_synthesize_phi_seed_equals_the_numpy_array(ctx, sr, n_fft, hop):
    from goofer_amd import core
    note, n = _note(sr, n_fft, hop)
    seed = 2 ** 64 + 6003
    phi = numpy_phi(seed, n_fft // 2 + 1, 1 + n // hop)
    want = core.synthesize(**note, sr=sr, n_fft=n_fft, hop_length=hop, phi=phi, ctx=ctx)
    got = core.synthesize(**note, sr=sr, n_fft=n_fft, hop_length=hop, phi_seed=seed, ctx=ctx)
    _same(got, want)


def test_synthesize_phi_seed_behind_a_time_stretch(ctx):
    """the stretched note's own frame count: 1 + int(1.3 n) // hop"""
    from goofer_amd import core
    sr, n_fft, hop = 44100, 1024, 256
    note, n = _note(sr, n_fft, hop)
    T = 1 + int(n * 1.3) // hop
    assert T != 1 + n // hop
    want = core.synthesize(**note, sr=sr, n_fft=n_fft, hop_length=hop, stretch_factor=1.3, phi=numpy_phi(6003, 513, T), ctx=ctx)
    got = core.synthesize(**note, sr=sr, n_fft=n_fft, hop_length=hop, stretch_factor=1.3, phi_seed=6003, ctx=ctx)
    _same(got, want)


def test_synthesize_batch_mixes_seeds_arrays_and_neither(ctx):
    from goofer_amd import core
    sr, n_fft, hop = 44100, 1024, 256
    made = [_note(sr, n_fft, hop, seconds=0.12 + 0.05 * i, seed=i) for i in range(6)]
    notes = [m[0] for m in made]
    arr = lambda i: numpy_phi(900 + i, 513, 1 + made[i][1] // hop)           # noqa: E731
    phis = [None, arr(1), None, None, arr(4), None]
    phi_seeds = [6003, None, None, 2 ** 127, None, 6003]
    keys = [11, 12, 13, 14, 15, 16]                                           # Philox keys: what the notes without phases draw from
    batch = core.synthesize_batch(notes, sr, n_fft, hop, seeds=keys, phis=phis, phi_seeds=phi_seeds, ctx=ctx)
    for i, note in enumerate(notes):
        assert not isinstance(batch[i], BaseException), batch[i]
        one = core.synthesize(**note, sr=sr, n_fft=n_fft, hop_length=hop, seed=keys[i], phi=phis[i], phi_seed=phi_seeds[i], ctx=ctx)
        _same(batch[i], one)
    # and a seeded note is the note with numpy's array
    _same(batch[3], core.synthesize(**notes[3], sr=sr, n_fft=n_fft, hop_length=hop, phi=numpy_phi(2 ** 127, 513, 1 + made[3][1] // hop), ctx=ctx))


# ---- Renderer ------------------------------------------------------------------------------------------------------------
CASES = [str(n) for n in golden("sampler_index")["names"]]


def _job(name):
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    g = golden("sampler_" + name)
    src = syn.make_source(2000 + CASES.index(name), seconds=0.45)
    source = Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
    return (source, S.decode_request(*[str(a) for a in g["args"]])), int(g["seed"][0])


@pytest.mark.parametrize("names", [["default"], ["L0"], ["su50"], ["default", "sg50", "L0", "su50", "sg50", "formants"]],
                         ids=["default", "L0", "su50", "walker+sg"])
def test_renderer_equals_the_host_made_matrix(ctx, names):
    """render(jobs, phi_seeds=) against the same prepared batch run with the matrix drawn on the host and uploaded"""
    from goofer_amd.render import Renderer
    r = Renderer(ctx)
    jobs, seeds = zip(*[_job(nm) for nm in names])
    got = r.render(list(jobs), seed=3, phi_seeds=list(seeds))
    prep = r.prepare(list(jobs), phi_seeds=list(seeds))
    assert prep["phi_words"] is not None and prep["phi"].shape == (prep["frames"], ctx.n_bins)
    mats = [numpy_phi(sd, ctx.n_bins, 1 + n // r.hop).T for n, sd in zip(prep["lens"], seeds)]
    prep["phi"], prep["phi_words"] = ctx.rows_from(np.concatenate(mats)), None   # the host draw: no fill in run()
    out = r.run(prep, seed=3)
    ctx.check()
    want, off = out["mix"].cpu().numpy(), prep["sample_off"]
    for i, nm in enumerate(names):
        assert np.array_equal(got[i], want[off[i]:off[i + 1]]), nm
        assert float(np.abs(got[i]).max()) > 1e-3


def test_prepare_without_device_calls_launches_nothing(ctx):
    """prepare(device_calls=False) stages the records only; the matrix is filled by run()"""
    from goofer_amd.render import Renderer
    r = Renderer(ctx)
    (job, seed) = _job("default")
    r.render([job], phi_seeds=[seed])                                        # (plans the geometry, makes the samples resident)
    calls = []
    real = ctx.lib.goofer_phase_fill
    try:
        ctx.lib.goofer_phase_fill = lambda *a: calls.append(a) or real(*a)
        prep = r.prepare([job], phi_seeds=[seed], device_calls=False)
        assert calls == []
        ctx.reserve(prep["frames"], prep["samples"], 1)
        torch.cuda.current_stream(ctx.device).synchronize()
        r.run(prep, seed=0)
        assert len(calls) == 1
    finally:
        ctx.lib.goofer_phase_fill = real
    ctx.check()
    assert np.array_equal(prep["phi"].cpu().numpy().T, numpy_phi(seed, ctx.n_bins, prep["frames"]))
    with pytest.raises(ValueError):
        r.prepare([job], phi_seeds=[seed, seed])
    with pytest.raises(ValueError):
        r.prepare([job], phi_seeds=[-1])
