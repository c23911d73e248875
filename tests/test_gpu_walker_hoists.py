"""GPU: the harmonic walker reduces a note's spectrum maximum once per note, not once per frame — the same values as before.

k_harm_stem folds a frame's |S|^2 into a per-lane running maximum and reduces it over the lanes, roots it and sends the atomic
where its wave leaves a note and behind its frame loop.  The maximum, the harmonic stem it divides and the mix must not change,
for every way a 32-frame run can meet a note (tiny batches: run_length gives its minimum, so run boundaries fall inside notes and
several notes share a run):

* against the one-kernel-per-step route (option "stems" 0), whose k_harm_shape still sends a maximum per frame;
* against each note rendered alone.

n_fft 1024 / hop 256, the only geometry the walkers take.
"""
import numpy as np
import pytest

import synth_ref as SR
from test_gpu_ragged_tiles import _same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GEO = (44100, 1024, 256)
HOP = GEO[2]
RUN = 32                                                      # run_length's minimum: frames per walker wave
OUTPUTS = ("harm", "uv", "bre", "rec", "mix")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    c.plan(*GEO)
    yield c
    c.close()


def render(ctx, cases, **options):
    """One goofer_synth_batch over ``cases`` under ``options``: {output: host array}, plus the notes' spectrum maxima."""
    from goofer_amd.core import note_params_from_kwargs
    par = np.concatenate([note_params_from_kwargs(1, **c["kw"]) for c in cases])
    par["seed"][:, 0] = [c["note_id"] for c in cases]         # keys the Philox phases: the same alone and in the batch
    for name, v in options.items():
        ctx.set_option(name, v)
    try:
        out = ctx.synth_batch(ctx.rows_from(np.concatenate([c["env"].T for c in cases])), [c["env"].shape[1] for c in cases],
                              ctx.tensor(np.concatenate([c["f0"] for c in cases])), ctx.tensor(np.concatenate([c["mask"] for c in cases])),
                              [c["n"] for c in cases], par, phi=ctx.rows_from(np.concatenate([c["phi"].T for c in cases])), seed=5)
        ctx.check()
        res = {k: out[k].cpu().numpy() for k in OUTPUTS}
        res["note_mag"] = ctx.debug_fetch("note_mag")[:len(cases)].copy()
    finally:
        for name in options:
            ctx.set_option(name, {"stems": 1, "td_blur": 1}[name])
    return res


def offsets(cases):
    return np.concatenate([[0], np.cumsum([c["n"] for c in cases])])


def same_outputs(what, got, want, names=OUTPUTS):
    """The harmonic stem by its words.  The other outputs by value, as tests/test_gpu_synth.py and tests/test_gpu_noise.py compare
    them (np.array_equal): a noise stem over a hop whose mask gain is exactly zero is the product x * 0.0f = +-0.0f, with the sign
    of x, where its frames were transformed, and +0.0f where they were skipped — and which frames of a note are skipped goes by
    the option and by where the runs start (the first three frames of a run count no hop as flat).  Every sample that is not zero
    has the same bits."""
    for name in names:
        if name == "harm":
            _same_bits("%s: %s" % (what, name), got[name], want[name])
            continue
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        assert np.isfinite(got[name]).all() and np.isfinite(want[name]).all(), (what, name)
        bad = np.nonzero(got[name] != want[name])[0]
        assert bad.size == 0, "%s: %s: %d of %d samples differ, first at %d (%r, %r)" % (
            what, name, bad.size, got[name].size, bad[0], got[name][bad[0]], want[name][bad[0]])


FRAMES = [1, 2, 3, 4, 5, 31, 32, 33, 40, 70]
MEETINGS = {
    # the ten frame counts and the same reversed: 442 frames in fourteen runs; notes 7 (33 frames, across a run boundary) and 17 (3
    # frames, inside a run) are silent between loud neighbours
    "every_count": (FRAMES + FRAMES[::-1], (7, 17)),
    # 65 frames: the last run is the single frame of the last note, alone
    "single_frame_run": ([31, 33, 1], ()),
}


def meeting_cases(tag):
    frames, silent = MEETINGS[tag]
    cases = []
    for k, T in enumerate(frames):
        n = (T - 1) * HOP + 57 + 13 * (k % 7)
        # loud notes: another pitch per note, so that their spectrum maxima differ and one leaking into a neighbour shows; a period
        # of under 57 samples, so that the shortest note holds a pulse
        c = SR.make_case(GEO, 9100 + k, n, "T%d" % T, mask="blocks", f0=0.0)
        if k not in silent:
            c["mask"][:] = 1.0                                # voiced throughout: a pulse train in every frame
            c["f0"][:] = 900.0 + 137.0 * (k % 5)
        c["note_id"] = 40 + k
        assert c["env"].shape[1] == T
        cases.append(c)
    return cases


_walked = {}


def walked(ctx, tag):
    """The batch through the walkers, rendered once per module."""
    if tag not in _walked:
        cases = meeting_cases(tag)
        _walked[tag] = (cases, render(ctx, cases))
        for v in _walked[tag][1].values():
            v.setflags(write=False)
    return _walked[tag]


def test_the_batches_meet_runs_in_every_way():
    frames, silent = MEETINGS["every_count"]
    f_off = np.concatenate([[0], np.cumsum(frames)])
    assert f_off[-1] == 442 and -(-f_off[-1] // RUN) == 14
    inside = [k for k in range(len(frames)) if f_off[k] // RUN == (f_off[k + 1] - 1) // RUN]
    across = [k for k in range(len(frames)) if (f_off[k + 1] - 1) // RUN - f_off[k] // RUN >= 2]
    starts = [k for k in range(len(frames)) if f_off[k] % RUN == 0]
    assert len(inside) >= 8 and across and starts               # several notes in one run, a note over three runs, a note that opens a run
    assert any(sum(1 for k in inside if f_off[k] // RUN == r) >= 3 for r in range(14))
    for k in silent:
        assert 0 < k < len(frames) - 1 and k - 1 not in silent and k + 1 not in silent
    assert f_off[7] // RUN != (f_off[8] - 1) // RUN and 17 in inside
    frames, _ = MEETINGS["single_frame_run"]
    assert sum(frames) % RUN == 1 and frames[-1] == 1


@pytest.mark.parametrize("tag", list(MEETINGS))
def test_note_maximum_per_note_equals_the_per_frame_route(ctx, tag):
    """Option "stems" 1 against 0 (k_harm_shape: one atomic per frame), the 5-tap bin blur as a pass over the bins on both sides
    as in tests/test_gpu_noise.py: the maxima themselves, the harmonic stem (harm / max|S| * gain) and the mix, note by note."""
    cases = meeting_cases(tag)
    a = render(ctx, cases, stems=1, td_blur=0)
    b = render(ctx, cases, stems=0, td_blur=0)
    off = offsets(cases)
    _same_bits("note_mag", a["note_mag"], b["note_mag"])
    for k in MEETINGS[tag][1]:
        assert a["note_mag"][k] == np.float32(1e-8) and not np.any(a["harm"][off[k]:off[k + 1]])
    loud = [k for k in range(len(cases)) if k not in MEETINGS[tag][1]]
    assert all(a["note_mag"][k] > 1e-6 for k in loud) and len(set(a["note_mag"][loud].tolist())) >= 3, a["note_mag"]
    for k, c in enumerate(cases):
        sl = slice(int(off[k]), int(off[k + 1]))
        same_outputs("note %d (%s)" % (k, c["name"]), {n: a[n][sl] for n in OUTPUTS}, {n: b[n][sl] for n in OUTPUTS})
    assert np.isfinite(a["mix"]).all() and np.any(a["harm"])


@pytest.mark.parametrize("tag", list(MEETINGS))
def test_notes_alone_and_in_the_batch(ctx, tag):
    """Each note alone in its own call (one run, one wave, the maximum sent behind the loop) against the batch."""
    cases, batch = walked(ctx, tag)
    off = offsets(cases)
    for k, c in enumerate(cases):
        alone = render(ctx, [c])
        sl = slice(int(off[k]), int(off[k + 1]))
        _same_bits("note_mag of note %d" % k, alone["note_mag"], batch["note_mag"][k:k + 1])
        same_outputs("note %d (%s)" % (k, c["name"]), alone, {n: batch[n][sl] for n in OUTPUTS})
