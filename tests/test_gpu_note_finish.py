"""GPU: k_note_finish (csrc/stems.hip) in both of its variants — the one that stores the mix alone (mix_only batches: the timed
step) and the one that also stores the stems and rec — on notes chosen to put every path of the kernel next to every other,
against each note rendered alone and against the stage's own arithmetic.

The seam batch: a note of exactly the kept capacity (12 rows of 4096 samples), notes shorter than one 16-byte group per thread, a
note with rows past the kept ones, odd lengths that misalign the next note's base; a leading note of three samples makes the first
long note's base no multiple of four.  It runs on the walker route with skip_zero 1 (hop bytes present, stems absent over flat
hops; what the allocator hands out for the stems is NaN first, as in tests/test_gpu_noise.py) and with skip_zero 0.

The arithmetic test needs no second run of the kernel.  What the finish pass computes is restated in float32 numpy from the
outputs themselves, GOOFER.py:1121, 1208-1218 and SillySampler.py:1142-1151:
  mix  = ((harm m_h + bre m_b) + uv m_u) vol             exactly (the device forms it from the very values it stores)
  normalize 0: the gain is exactly 1, so rec = (harm + uv) + bre and note_peak = max |rec|, exactly
  otherwise:   gain = float32((1 / float64(peak + 1e-12f)) ^ normalize); the sample that carries the peak gives
               max |rec| = float32(peak gain) (exactly for normalize 1; within 2^-22 where the device's pow and libm's may round
               differently); and rec = ((h + u) + b) g against (h g + u g) + b g differs by the roundings of five float32
               operations on either side: |rec - ((harm + uv) + bre)| <= 3 x 2^-23 (|harm| + |uv| + |bre|)
               (the factor 3 and the 2^-23 of tests/test_gpu_synth_stages.py, here per sample and relative to the operands).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SR, N_FFT, HOP = 44100, 1024, 256
NB = N_FFT // 2 + 1
KEPT = 12 * 4096
# (the leading 3 misaligns the first long note's base)
SEAM_LENS = [3, KEPT, 5, KEPT + 1, 1, 4096, KEPT + 4096 + 1, 300, 257, KEPT - 1]
KEYS = ("harm", "uv", "bre", "rec", "mix")


def _note(n, k):
    """Envelope rows, f0 and a mask with voiced, unvoiced and fractional stretches (so that hops of either noise stem are flat
    zero and left unstored under skip_zero 1) of an n-sample note."""
    T = 1 + n // HOP
    f = np.arange(NB) * (SR / N_FFT)
    env = (np.exp(-f / (2000.0 + 300.0 * k)) * (1.0 + np.exp(-0.5 * ((f - 900.0 - 150.0 * k) / 250.0) ** 2)))
    env = (env[None, :] * (1.0 + 0.3 * np.sin(np.arange(T) * 0.37 + k))[:, None]).astype(F32)
    t = np.arange(n)
    f0 = (180.0 + 20.0 * k + 8.0 * np.sin(t / 900.0)).astype(F32)
    mask = np.ones(n, F32)
    seg = max(1, n // 7)
    mask[seg:2 * seg] = 0.0
    mask[3 * seg:4 * seg] = 0.5
    mask[5 * seg:6 * seg] = 0.0
    return env, f0, mask


def _params(count):
    from goofer_amd.device import default_params
    par = default_params(count)
    for k in range(count):
        par["normalize"][k] = (1.0, 0.0, 0.5)[k % 3]
        par["mix_harm"][k] = 1.0 - 0.05 * (k % 4)
        par["mix_breath"][k] = 0.5 + 0.1 * (k % 3)
        par["mix_unvoiced"][k] = 0.8 + 0.05 * (k % 5)
        par["volume"][k] = 0.6 + 0.07 * (k % 6)
        par["seed"][k, 0] = 100 + k
    return par


class Batch:
    def __init__(self, ctx, lens):
        ctx.plan(SR, N_FFT, HOP)
        self.ctx, self.lens = ctx, list(lens)
        self.notes = [_note(n, k) for k, n in enumerate(self.lens)]
        self.par = _params(len(self.lens))
        self.off = np.concatenate([[0], np.cumsum(self.lens)])

    def run(self, which=None, mix_only=False):
        """The batch (or the notes ``which`` of it, as a batch of their own) through goofer_synth_batch; host arrays."""
        ctx = self.ctx
        which = list(range(len(self.lens))) if which is None else list(which)
        notes = [self.notes[k] for k in which]
        lens = [self.lens[k] for k in which]
        env = ctx.rows_from(np.concatenate([nt[0] for nt in notes]))
        # what the allocator hands out for the stems is NaN, not fresh zero pages: a sample read where nothing was stored shows
        junk = [torch.full((int(sum(lens)) + 4096,), float("nan"), device="cuda") for _ in range(6)]
        del junk
        try:
            out = ctx.synth_batch(env, [nt[0].shape[0] for nt in notes], ctx.tensor(np.concatenate([nt[1] for nt in notes])),
                                  ctx.tensor(np.concatenate([nt[2] for nt in notes])), lens, self.par[which], seed=77,
                                  want_rec=not mix_only, mix_only=mix_only)
            torch.cuda.synchronize()
        except RuntimeError as e:                                 # nothing more is started on this GPU
            pytest.exit("goofer_synth_batch failed on the device: %r" % (e,), returncode=3)
        ctx.check()
        res = {k: out[k].cpu().numpy().copy() for k in (("mix",) if mix_only else KEYS)}
        res["note_peak"] = ctx.debug_fetch("note_peak")[:len(lens)].copy()
        return res


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.set_option("skip_zero", 1)
    c.close()


_seam = {}


def _seam_runs(ctx, skip):
    """The seam batch with stems and rec, with the mix alone, and each note as a batch of its own."""
    if skip not in _seam:
        b = Batch(ctx, SEAM_LENS)
        ctx.set_option("skip_zero", skip)
        try:
            full = b.run()
            lean = b.run(mix_only=True)
            alone = [b.run(which=[k]) for k in range(len(SEAM_LENS))]
        finally:
            ctx.set_option("skip_zero", 1)
        _seam[skip] = (b, full, lean, alone)
    return _seam[skip]


@pytest.mark.parametrize("skip", (1, 0))
def test_the_mix_alone_is_the_mix_beside_the_stems(ctx, skip):
    b, full, lean, alone = _seam_runs(ctx, skip)
    assert np.isfinite(full["mix"]).all() and np.isfinite(full["rec"]).all()
    assert np.array_equal(full["mix"], lean["mix"])
    assert np.array_equal(full["note_peak"], lean["note_peak"])
    if skip:
        assert (full["uv"] == 0).mean() > 0.1 and np.abs(full["uv"]).max() > 0


@pytest.mark.parametrize("skip", (1, 0))
def test_every_seam_note_equals_the_note_rendered_alone(ctx, skip):
    b, full, lean, alone = _seam_runs(ctx, skip)
    for k, one in enumerate(alone):
        a, e = int(b.off[k]), int(b.off[k + 1])
        # (array_equal takes -0 for +0: the sign of a noise stem's zero under a zero gain depends on where the walker's runs
        # begin, tests/test_gpu_synth_stages.py)
        for key in KEYS:
            assert np.array_equal(full[key][a:e], one[key]), (k, key)
        assert np.array_equal(lean["mix"][a:e], one["mix"]), (k, "mix alone")
        assert full["note_peak"][k] == one["note_peak"][0], k


def test_many_short_notes_twice_on_one_handle(ctx):
    rng = np.random.default_rng(20240)
    lens = [int(v) for v in rng.integers(64, 601, size=700)]
    b = Batch(ctx, lens)
    first, second, lean = b.run(), b.run(), b.run(mix_only=True)
    for k in KEYS + ("note_peak",):
        assert np.array_equal(first[k], second[k]), k
    assert np.array_equal(first["mix"], lean["mix"]) and np.isfinite(first["mix"]).all()


def test_finish_arithmetic_restated_in_numpy(ctx):
    b, d, lean, alone = _seam_runs(ctx, 1)
    for k in (1, 6, 9, 3, 7, 5):                                   # normalize 0 (notes 1, 7), 1 (6, 9, 3), 0.5 (5)
        a, e = int(b.off[k]), int(b.off[k + 1])
        p = b.par[k]
        h, u, br, rec, mix = (d[key][a:e] for key in KEYS)
        want = ((h * F32(p["mix_harm"]) + br * F32(p["mix_breath"])) + u * F32(p["mix_unvoiced"])) * F32(p["volume"])
        assert np.array_equal(mix, want), (k, "mix")
        peak = F32(d["note_peak"][k])
        assert peak > 0
        amt = float(min(max(F32(p["normalize"]), F32(0.0)), F32(1.0)))
        if amt == 0.0:
            assert np.array_equal(rec, (h + u) + br), (k, "rec")
            assert peak == np.max(np.abs(rec)), (k, "note_peak")
        else:
            x = 1.0 / float(F32(peak + F32(1e-12)))
            gain = F32(x) if amt == 1.0 else F32(x ** amt)
            got_peak = np.max(np.abs(rec))
            if amt == 1.0:
                assert got_peak == F32(peak * gain), (k, "peak of rec", got_peak, peak, gain)
            else:
                assert abs(float(got_peak) - float(peak) * float(gain)) <= 2.0 ** -22 * float(got_peak), (k, "peak of rec")
            bound = 3.0 * 2.0 ** -23 * (np.abs(h).astype(np.float64) + np.abs(u) + np.abs(br))
            err = np.abs(rec.astype(np.float64) - ((h + u) + br).astype(np.float64))
            assert np.all(err <= bound), (k, "rec", float(np.max(err - bound)))
