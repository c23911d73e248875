"""CPU: numpy's legacy normal stream (goofer_legacy_normal_fill) as tests/mt_ref.py restates it against numpy itself, the names
the feature adds at every layer, and the input checks that happen before any device is touched."""
import inspect
import os
import re

import numpy as np
import pytest

import mt_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 4027, 2 ** 32 - 1]
COUNTS = [1, 2, 3, 245, 624, 1001]


@pytest.fixture()
def global_state():
    """the tests below seed numpy's global generator: put it back"""
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", COUNTS)
def test_restatement_reproduces_numpy(global_state, seed, n):
    """the values bit for bit, and the generator afterwards: key, position, cached-normal flag and value"""
    np.random.seed(seed)
    ref = np.random.randn(n)
    name, key, pos, has_gauss, cached = np.random.get_state()
    z, attempts, (mt, p, hg, c) = M.draw(seed, n)
    assert z.dtype == np.float64 and np.array_equal(z, ref)
    assert name == "MT19937" and np.array_equal(key, mt)
    assert (pos, has_gauss) == (p, hg)
    if has_gauss:
        assert cached == c
    assert p == 4 * attempts - M.WORDS * ((4 * attempts - 1) // M.WORDS)      # the attempts count is the stream position


@pytest.mark.parametrize("seed", SEEDS)
def test_sequential_twist_draws_the_same(seed):
    a = M.draw(seed, 1001, twist=M.twist_sequential)
    b = M.draw(seed, 1001)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2][0], b[2][0])


def test_two_odd_calls_are_one_call_of_the_summed_length(global_state):
    """the second normal of a pair waits for the next call: a note's randn calls are consecutive slices of one stream"""
    for seed, (n1, n2) in ((4027, (3, 5)), (0, (245, 311)), (2 ** 32 - 1, (1, 1))):
        np.random.seed(seed)
        two = np.concatenate([np.random.randn(n1), np.random.randn(n2)])
        np.random.seed(seed)
        one = np.random.randn(n1 + n2)
        assert np.array_equal(two, one)
        assert np.array_equal(M.draw(seed, n1 + n2)[0], two)


def test_parallel_twist_equals_the_sequential_one():
    """the kernel's three wide steps against k = 0..623 in order, over 5 blocks"""
    for seed in (5, 2 ** 32 - 1):
        a = b = M.seed_words(seed)
        for _ in range(5):
            a, b = M.twist_sequential(a), M.twist_parallel(b)
            assert np.array_equal(a, b)


def test_seed_words_are_numpys(global_state):
    for seed in SEEDS:
        np.random.seed(seed)
        _, key, pos, has_gauss, _ = np.random.get_state()
        assert np.array_equal(M.seed_words(seed), key) and pos == M.WORDS and has_gauss == 0


def test_a_block_is_156_attempts_and_their_count_is_the_stream_position(global_state):
    assert M.WORDS == 4 * M.ATTEMPTS
    acc, a, b = M.block_attempts(M.twist_parallel(M.seed_words(1)))
    assert acc.shape == a.shape == b.shape == (M.ATTEMPTS,)
    for seed, n in ((1, 2 * int(acc.sum())), (1, 2 * int(acc.sum()) + 1), (4027, 20001)):
        z, attempts, (mt, pos, _, _) = M.draw(seed, n)
        np.random.seed(seed)
        np.random.randn(n)
        st = np.random.get_state()
        blocks = -(-attempts // M.ATTEMPTS)
        assert st[2] == pos == 4 * attempts - M.WORDS * (blocks - 1)
        assert blocks <= 2 * M.expected_blocks(n) + 4                         # the kernel's bound on its block loop
    # exactly the accepted attempts of the first block: all 156 attempts of it are not needed unless the last one is accepted
    assert M.draw(1, 2 * int(acc.sum()))[1] == int(np.nonzero(acc)[0][-1]) + 1
    assert M.draw(1, 2 * int(acc.sum()) + 1)[1] > M.ATTEMPTS


def test_seed_checks():
    from goofer_amd import sampler as S
    assert S.check_noise_seed(None) is None
    assert S.check_noise_seed(0) == 0 and S.check_noise_seed(2 ** 32 - 1) == 2 ** 32 - 1
    assert S.check_noise_seed(np.uint32(4027)) == 4027 and type(S.check_noise_seed(np.int64(7))) is int
    for bad in (True, False, np.True_, 1.0, 2.5, "7", -1, 2 ** 32, 2 ** 70):
        with pytest.raises(ValueError, match=r"integer in \[0, 2\*\*32\)"):
            S.check_noise_seed(bad)


def test_env_noise_seed(monkeypatch):
    from goofer_amd import sampler as S
    monkeypatch.delenv("GOOFER_NOISE_SEED", raising=False)
    assert S.env_noise_seed() is None
    for text, value in (("", None), ("  ", None), ("0", 0), (" 4027 ", 4027), (str(2 ** 32 - 1), 2 ** 32 - 1)):
        monkeypatch.setenv("GOOFER_NOISE_SEED", text)
        assert S.env_noise_seed() == value
    for text in ("-3", "1.5", "abc", "0x10", "1e3", "+-1", str(2 ** 32), str(2 ** 70)):
        monkeypatch.setenv("GOOFER_NOISE_SEED", text)
        with pytest.raises(ValueError, match="GOOFER_NOISE_SEED"):
            S.env_noise_seed()


def test_the_new_names_exist():
    from goofer_amd import _lib, cli
    from goofer_amd.device import Context
    from goofer_amd.render import GooferResampler, Renderer
    assert "goofer_legacy_normal_fill" in _lib.EXPORTS
    header = open(os.path.join(REPO, "include", "goofer_hip.h")).read()
    assert re.search(r"\bint goofer_legacy_normal_fill\(goofer_ctx \*ctx,", header)
    assert "1812433253" in header and "0x9908b0df" in header                  # the documentation carries the stream's definition
    assert "launch_legacy_normal_fill" in open(os.path.join(REPO, "goofer_amd", "csrc", "launchers.h")).read()
    assert "k_legacy_normal_fill" in open(os.path.join(REPO, "goofer_amd", "csrc", "noise.hip")).read()
    assert callable(getattr(Context, "legacy_normal_fill"))
    kwonly = lambda f, name: inspect.signature(f).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY   # noqa: E731
    assert kwonly(GooferResampler.__init__, "noise_seed")
    assert kwonly(cli.BatchCollector.__init__, "noise_seed")
    assert "noise_seeds" in inspect.signature(Renderer.prepare).parameters
    assert "noise_seeds" in inspect.signature(Renderer.render).parameters


@pytest.mark.parametrize("value", ["-3", "1.5", "abc", "0x10", "1e3", str(2 ** 32)])
def test_cli_refuses_a_bad_noise_seed_before_anything_is_rendered(monkeypatch, caplog, value):
    from goofer_amd import cli, device, render

    def boom(*a, **k):
        raise AssertionError("a device context was made")
    monkeypatch.setattr(device.Context, "__init__", boom)
    monkeypatch.setattr(render, "GooferResampler", boom)
    monkeypatch.setattr(render, "Renderer", boom)
    monkeypatch.setattr(cli, "serve", boom)
    monkeypatch.delenv("GOOFER_PHI_SEED", raising=False)
    monkeypatch.setenv("GOOFER_NOISE_SEED", value)
    args = ["a.wav", "b.wav", "C4", "100", "sh50", "0", "1000", "0", "0", "100", "0", "!120", "AA"]
    assert cli.main(args) == 1                                                # the 13-argument call
    assert "GOOFER_NOISE_SEED" in caplog.text
    assert cli.main([]) == 1                                                  # the server


def test_cli_passes_the_noise_seed_on(monkeypatch):
    from goofer_amd import cli, render
    seen = []
    monkeypatch.setattr(render, "GooferResampler", lambda *a, **k: seen.append((a, k)))
    args = ["a.wav", "b.wav", "C4", "100", "sh50sr50", "0", "1000", "0", "0", "100", "0", "!120", "AA"]
    monkeypatch.delenv("GOOFER_PHI_SEED", raising=False)
    monkeypatch.setenv("GOOFER_NOISE_SEED", "4027")
    assert cli.main(args) == 0
    monkeypatch.setenv("GOOFER_PHI_SEED", "6027")
    assert cli.main(args) == 0
    monkeypatch.delenv("GOOFER_NOISE_SEED")
    monkeypatch.delenv("GOOFER_PHI_SEED")
    assert cli.main(args) == 0
    assert seen == [(tuple(args), {"noise_seed": 4027}), (tuple(args), {"phi_seed": 6027, "noise_seed": 4027}), (tuple(args), {})]


def test_collector_call_shapes(tmp_path):
    """with a noise seed every request of a batch gets it (each request is one reference process); without one the call is
    the call it always was"""
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
    for kw in ({}, {"noise_seed": 4027}, {"phi_seed": 6027, "noise_seed": 4027}):
        col = cli.BatchCollector(renderer=Spy(), window_s=0.0, **kw)
        try:
            batch = [cli._Pending(args), cli._Pending(args)]
            col._render(batch)
            assert all(p.error is None and p.done.is_set() for p in batch)
        finally:
            col.close()
    (n0, kw0), (n1, kw1), (n2, kw2) = calls
    assert n0 == n1 == n2 == 2
    assert list(kw0) == ["seed"]
    assert sorted(kw1) == ["noise_seeds", "seed"] and kw1["noise_seeds"] == [4027, 4027]
    assert kw2 == {"seed": 6027, "phi_seeds": [6027, 6027], "noise_seeds": [4027, 4027]}
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError):
            cli.BatchCollector(renderer=Spy(), noise_seed=bad)


def test_resampler_refuses_a_bad_noise_seed_before_anything_is_read(monkeypatch):
    from goofer_amd import device, render

    def boom(*a, **k):
        raise AssertionError("a device context was made")
    monkeypatch.setattr(device.Context, "__init__", boom)
    for bad in (-1, 2 ** 32, 2.0, True):
        with pytest.raises(ValueError, match="noise_seed"):
            render.GooferResampler("missing.wav", "out.wav", "C4", "100", noise_seed=bad)
