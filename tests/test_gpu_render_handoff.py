"""GPU: what goofer_render_batch hands from its assembly half to its synthesis half (the early fork of the pulse chain, the f0
kernel on the side stream, the fused warp of the harmonic rows) belongs to that one call.  Fused renders, plain
goofer_assemble_batch / goofer_synth_batch calls and a render whose synthesis half refuses, interleaved on one handle: every
result equals, bit for bit, what a fresh handle gives."""
import numpy as np
import pytest

from goofer_amd import synthetic as syn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 11
# three notes of 150 .. 300 ms at 44.1 kHz / 1024 / 256, one with a formant shift (the fused warp has work to do); no 'sg' / 'sr':
# the stem walkers, forked early
NOTES_A = [("t0", 150.0), ("g30fa20fb-10", 220.0), ("V80", 300.0)]
NOTES_B = NOTES_A + [("sr50", 200.0)]                         # + one 'sr' note: assembly + one plain synthesis per pipeline


def _jobs(notes):
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    jobs = []
    for i, (flags, ms) in enumerate(notes):
        src = syn.make_source(2100 + i, seconds=0.45)
        req = syn.make_request(2100 + i, flags, length_ms=ms)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*syn.request_args(req))))
    return jobs


def _prepare(r, notes):
    np.random.seed(SEED)                                      # the 'sr' note's host draws
    return r.prepare(_jobs(notes), note_ids=list(range(len(notes))))


def _mix(r, prep, **kw):
    out = r.run(prep, seed=SEED, **kw)["mix"].clone()
    r.ctx.check()
    return out


def _plain_synth(r, prep):
    """goofer_synth_batch alone on the arrays the assembly wrote: Renderer.run's call without the assembly descriptor."""
    out = r.ctx.synth_batch(prep["env"], prep["env_lens"], prep["f0"], prep["mask"], prep["lens"], prep["params"],
                            formants=prep["formants"], phi=prep["phi"], seed=SEED, want_rec=False, want_mix=True,
                            offsets=prep["offsets"], mix_only=True)["mix"].clone()
    r.ctx.check()
    return out


@pytest.fixture(scope="module")
def fresh():
    """Each render on a handle of its own: batch A fused and split, batch B."""
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    ref = {}
    for key, notes, kw in (("A", NOTES_A, {}), ("A_split", NOTES_A, {"split": True}), ("B", NOTES_B, {})):
        ctx = Context(0)
        try:
            r = Renderer(ctx)
            ref[key] = _mix(r, _prepare(r, notes), **kw)
        finally:
            ctx.close()
    assert float(ref["A"].abs().max()) > 0 and float(ref["B"].abs().max()) > 0
    return ref


@pytest.fixture()
def renderer():
    from goofer_amd.device import Context
    from goofer_amd.render import Renderer
    ctx = Context(0)
    yield Renderer(ctx)
    ctx.close()


def test_interleaved_calls_on_one_handle(fresh, renderer):
    """Fused A, mixed B (goofer_assemble_batch + two plain goofer_synth_batch), split A, fused A again on one handle."""
    r = renderer
    a, b = _prepare(r, NOTES_A), _prepare(r, NOTES_B)
    assert torch.equal(fresh["A"], fresh["A_split"])
    assert torch.equal(_mix(r, a), fresh["A"])
    assert torch.equal(_mix(r, b), fresh["B"])
    assert torch.equal(_mix(r, a, split=True), fresh["A_split"])
    assert torch.equal(_mix(r, a), fresh["A"])


def test_refused_synthesis_inside_a_render_leaves_nothing_behind(fresh, renderer, monkeypatch):
    """goofer_render_batch whose synthesis half refuses its batch (n_bins off by one: GOOFER_EINVAL, an argument refusal) after
    the assembly ran with the warp request and the early fork armed."""
    from goofer_amd.device import GooferError
    r = renderer
    ctx = r.ctx
    a = _prepare(r, NOTES_A)
    real = ctx.lib.goofer_render_batch

    def off_by_one(h, asmb, batch, stream):
        b = batch._obj
        b.n_bins += 1
        try:
            return real(h, asmb, batch, stream)
        finally:
            b.n_bins -= 1
    with monkeypatch.context() as m:
        m.setattr(ctx.lib, "goofer_render_batch", off_by_one)
        with pytest.raises(GooferError, match="batch geometry does not match the plan"):
            r.run(a, seed=SEED)
    ctx.check()
    assert torch.equal(_plain_synth(r, a), fresh["A_split"])
    assert torch.equal(_mix(r, a), fresh["A"])
