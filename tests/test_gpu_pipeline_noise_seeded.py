"""GPU: ``PipelinedRenderer.render_iter(noise_seeds=)`` hands each batch's legacy seeds to the ``Renderer.render(noise_seeds=)`` path:
the same bits as rendering the batches one by one, whatever the depth and however the batches are coalesced."""
import numpy as np
import pytest

from goofer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FLAGS = ["sh50", "sr50", "sh30sr70", "g0", "sh50sr50", "sh40sr40"]
LENGTH_MS = [300, 350, 420, 250, 333, 380]
LEGACY = [50, 2 ** 32 - 1, 0, 53, 4027, 55]
CUTS = [(0, 2), (2, 3), (3, 6)]                                # three batches of 2, 1 and 3 notes


def _batches():
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    srcs, reqs = [], []
    for k, (flags, ms) in enumerate(zip(FLAGS, LENGTH_MS)):
        src = syn.make_source(7100 + k, seconds=0.4)
        srcs.append(Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]))
        reqs.append(S.decode_request("C4", "100", flags, "10", str(ms), "30", "30", "100", "0", "!120", "AA"))
    return [(srcs[a:b], reqs[a:b]) for a, b in CUTS], [LEGACY[a:b] for a, b in CUTS]


def test_render_iter_forwards_each_batchs_seeds():
    from goofer_amd.device import Context
    from goofer_amd.render import PipelinedRenderer, Renderer
    batches, seeds = _batches()
    ctx = Context(0)
    try:
        r = Renderer(ctx)
        want = [r.render(list(zip(*b)), seed=11, noise_seeds=s) for b, s in zip(batches, seeds)]
        other = r.render(list(zip(*batches[0])), seed=11, noise_seeds=[s ^ 1 for s in seeds[0]])
    finally:
        ctx.close()
    assert not np.array_equal(other[0], want[0][0])            # (the seeds are heard)
    before = np.random.get_state()
    for depth, coalesce in ((2, 1), (1, 3)):
        p = PipelinedRenderer(0, depth=depth, workers=2, coalesce=coalesce)
        try:
            got = [[mix[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)] for mix, off in
                   p.render_iter(batches, seed=11, noise_seeds=seeds)]
            assert len(got) == len(want)
            for b, (g, w) in enumerate(zip(got, want)):
                assert len(g) == len(w)
                for i, (a, c) in enumerate(zip(g, w)):
                    assert np.array_equal(a, c), (depth, coalesce, b, i)
            with pytest.raises(ValueError):                    # a list of the wrong length: raised when its batch is reached
                list(p.render_iter(batches[:1], seed=11, noise_seeds=[seeds[0][:1]]))
            with pytest.raises(ValueError):
                list(p.render_iter(batches[:1], seed=11, noise_seeds=[[2 ** 32, 1]]))
            with pytest.raises(ValueError):                    # a batch without an entry
                list(p.render_iter(batches[:1], seed=11, noise_seeds=[]))
            if coalesce > 1:                                   # one device batch seeds all of its notes or none
                with pytest.raises(ValueError):
                    list(p.render_iter(batches, seed=11, noise_seeds=[seeds[0], None, seeds[2]]))
        finally:
            p.close()
    after = np.random.get_state()
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])
