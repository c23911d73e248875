"""CPU: the seeded phase stream (goofer_phase_fill) as tests/pcg_ref.py restates it against numpy itself, the names the feature
adds at every layer, and the input checks that happen before any device is touched."""
import inspect
import os
import re

import numpy as np
import pytest

import pcg_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 6003, 2 ** 32 + 5, 2 ** 64 - 1, 2 ** 127]


@pytest.fixture(scope="module")
def numpy_phases():
    """default_rng(s).uniform(0, 2 pi, (B, T)).astype(float32), made once per (seed, shape)"""
    return {(s, B, T): P.numpy_phases(s, B, T) for s in SEEDS for B, T in ((33, 5), (513, 190))}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", [(33, 5), (513, 190)])
def test_restatement_reproduces_numpy(numpy_phases, seed, shape):
    """seed -> words, step, output, value: draw by draw, and bin by bin behind a jump (the kernel's order)."""
    ref = numpy_phases[(seed, *shape)]
    assert ref.dtype == np.float32
    assert np.array_equal(P.phases(seed, *shape), ref)
    assert np.array_equal(P.phases_by_jump(seed, *shape), ref)


def test_a_tile_in_the_middle_of_a_note(numpy_phases):
    """frames [64, 128) of a 190-frame note: each bin jumps to b * T + 64"""
    ref = numpy_phases[(6003, 513, 190)]
    assert np.array_equal(P.phases_by_jump(6003, 513, 190, frames=(64, 128)), ref[:, 64:128])


@pytest.mark.parametrize("k", [0, 1, 2, 300 * 190 + 17, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 63 + 11, 2 ** 64 - 1, (1 << 70) - 12345])
def test_jump_matches_advance(k):
    """the table's jump against numpy's own PCG64.advance, k >= 2^32 and a 70-bit k included"""
    for seed in (7, 2 ** 127):
        state, inc = P.seed_words(seed)
        bg = np.random.PCG64(seed)
        bg.advance(k)
        assert P.jump(state, inc, k) == int(bg.state["state"]["state"])
        assert int(bg.state["state"]["inc"]) == inc


def test_jump_matches_stepping():
    state, inc = P.seed_words(6003)
    s = state
    for k in range(0, 300):
        assert P.jump(state, inc, k) == s
        s = P.step(s, inc)


def test_jump_table_entries_compose():
    tab = P.jump_table()
    assert tab[0] == (P.MULT, 1) and len(tab) == 64
    for j in range(63):                                         # 2^j steps twice are 2^(j+1) steps
        A, G = tab[j]
        assert tab[j + 1] == ((A * A) & P.M128, (G * A + G) & P.M128)


def test_seed_records():
    """device.pcg64_words: four 64-bit words per note, numpy's own state; None is the zero record"""
    from goofer_amd.device import pcg64_words
    w = pcg64_words([6003, None, 2 ** 127, np.int64(6003)])
    assert w.dtype == np.uint64 and w.shape == (4, 4)
    for row, seed in ((0, 6003), (2, 2 ** 127), (3, 6003)):
        state, inc = P.seed_words(seed)
        assert [int(v) for v in w[row]] == [state & P.M64, state >> 64, inc & P.M64, inc >> 64]
        assert int(w[row, 2]) & 1                               # an increment is odd: the zero record cannot be a seed's
    assert not w[1].any()
    for bad in (-1, 1.5, "7", True):
        with pytest.raises(ValueError):
            pcg64_words([bad])


def test_the_new_names_exist():
    from goofer_amd import _lib, cli, core
    from goofer_amd.device import Context
    from goofer_amd.render import GooferResampler, Renderer
    assert "goofer_phase_fill" in _lib.EXPORTS
    header = open(os.path.join(REPO, "include", "goofer_hip.h")).read()
    assert re.search(r"\bint goofer_phase_fill\(goofer_ctx \*ctx,", header)
    assert "launch_phase_fill" in open(os.path.join(REPO, "goofer_amd", "csrc", "launchers.h")).read()
    assert callable(getattr(Context, "phase_fill"))
    kwonly = lambda f, name: inspect.signature(f).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY   # noqa: E731
    assert kwonly(core.synthesize, "phi_seed")
    assert kwonly(core.synthesize_batch, "phi_seeds") and kwonly(core.resynthesize_batch, "phi_seeds")
    assert kwonly(GooferResampler.__init__, "phi_seed")
    assert kwonly(cli.BatchCollector.__init__, "phi_seed")
    assert "phi_seeds" in inspect.signature(Renderer.prepare).parameters
    assert "phi_seed" not in core._synth_defaults()             # a call argument, not a gf.synthesize keyword of the notes


@pytest.mark.parametrize("value", ["-3", "1.5", "abc", "0x10", "1e3", "+-1"])
def test_cli_refuses_a_bad_phase_seed_before_anything_is_rendered(monkeypatch, caplog, value):
    from goofer_amd import cli, device, render

    def boom(*a, **k):
        raise AssertionError("a device context was made")
    monkeypatch.setattr(device.Context, "__init__", boom)
    monkeypatch.setattr(render, "GooferResampler", boom)
    monkeypatch.setattr(cli, "serve", boom)
    monkeypatch.setenv("GOOFER_PHI_SEED", value)
    args = ["a.wav", "b.wav", "C4", "100", "g0", "0", "1000", "0", "0", "100", "0", "!120", "AA"]
    assert cli.main(args) == 1                                  # the 13-argument call
    assert "GOOFER_PHI_SEED" in caplog.text
    assert cli.main([]) == 1                                    # the server


def test_cli_passes_the_phase_seed_on(monkeypatch):
    from goofer_amd import cli, render
    seen = []
    monkeypatch.setattr(render, "GooferResampler", lambda *a, **k: seen.append((a, k)))
    args = ["a.wav", "b.wav", "C4", "100", "g0", "0", "1000", "0", "0", "100", "0", "!120", "AA"]
    monkeypatch.setenv("GOOFER_PHI_SEED", str(2 ** 70 + 1))
    assert cli.main(args) == 0
    monkeypatch.delenv("GOOFER_PHI_SEED")
    assert cli.main(args) == 0
    assert seen == [(tuple(args), {"phi_seed": 2 ** 70 + 1}), (tuple(args), {})]   # unset: the call as it always was


def test_collector_call_shapes(tmp_path):
    """without a seed the collector calls render(jobs, seed=<fresh>) as before; with one, every note of the batch gets it"""
    from goofer_amd import cli, core
    from goofer_amd import synthetic as syn
    calls = []

    class Spy:
        hop = 256

        def render(self, jobs, **kw):
            calls.append((len(jobs), kw))
            return [np.zeros(100, dtype=np.float32) for _ in jobs]

    src = syn.make_source(100, seconds=0.4)
    wav = tmp_path / "s.wav"
    core.save_features(wav.with_name("s_features.goofy"), src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"])
    args = [str(wav), str(tmp_path / "o.wav")] + syn.request_args(syn.make_request(100, "t0g0", length_ms=200))
    for seed in (None, 2 ** 64 + 6003):
        col = cli.BatchCollector(renderer=Spy(), window_s=0.0, phi_seed=seed)
        try:
            batch = [cli._Pending(args), cli._Pending(args)]
            col._render(batch)
            assert all(p.error is None and p.done.is_set() for p in batch)
        finally:
            col.close()
    (n0, kw0), (n1, kw1) = calls
    assert n0 == n1 == 2
    assert list(kw0) == ["seed"] and isinstance(kw0["seed"], int)
    assert kw1 == {"seed": 6003, "phi_seeds": [2 ** 64 + 6003] * 2}
    with pytest.raises(ValueError):
        cli.BatchCollector(renderer=Spy(), phi_seed=-1)


def test_synthesize_refuses_bad_phase_arguments_before_a_context_is_made(monkeypatch):
    from goofer_amd import core, device

    def boom(*a, **k):
        raise AssertionError("a device context was made")
    monkeypatch.setattr(device.Context, "__init__", boom)
    monkeypatch.setattr(core, "_ctx", boom)
    env, x = np.ones((513, 5), dtype=np.float32), np.zeros(1024, dtype=np.float32)
    with pytest.raises(ValueError, match="exclusive"):
        core.synthesize(env, x, x, x, 44100, phi=np.zeros((513, 5), dtype=np.float32), phi_seed=3)
    for bad in (-1, -2 ** 70, 2.5):
        with pytest.raises(ValueError, match="non-negative integer"):
            core.synthesize(env, x, x, x, 44100, phi_seed=bad)
    note = {"env_spec": env, "f0_interp": x, "voicing_mask": x, "y": x}
    with pytest.raises(ValueError):
        core.synthesize_batch([note, note], 44100, phi_seeds=[1])                    # the wrong length
    with pytest.raises(ValueError):
        core.synthesize_batch([note], 44100, phi_seeds=[-5])
    with pytest.raises(ValueError):
        core.synthesize_batch([note], 44100, phis=[np.zeros((513, 5), dtype=np.float32)], phi_seeds=[5])   # both for one note
    with pytest.raises(ValueError):
        core.resynthesize_batch([x], 44100, variants=[{}, {}], phi_seeds=[1])
