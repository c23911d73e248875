"""CPU: the job rule of goofer_legacy_normal_jobs (tests/legacy_jobs_ref.py over tests/mt_ref.py) against numpy's own
``np.random.seed(s)`` followed by one ``randn(n)`` per destination, the names the seeded ``synthesize`` adds at every layer, and
the seed checks that happen before any device is touched.

mt_ref.draw reproduces numpy bit for bit on the host (tests/test_legacy_stream.py asserts equality), so the layouts here are
compared for equality too."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import legacy_jobs_ref as J

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 4027, 2 ** 32 - 1]
COUNTS = [1, 2, 61, 123, 1501]                                 # 4 x 61 = 244 and 123 = 245 / 2 straddle the 245-normal average block
SUBSETS = [s for r in range(5) for s in itertools.combinations(range(4), r)]


@pytest.fixture()
def global_state():
    """the tests below seed numpy's global generator: put it back"""
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", COUNTS)
def test_job_layout_is_one_randn_per_enabled_stream(global_state, seed, n):
    """every subset of the four streams (f0, sub-harmonic f0, harmonic volume, breath volume): the enabled ones are the job's
    destinations in order; an odd n carries the cached second normal into the next stream"""
    for subset in SUBSETS:
        np.random.seed(seed)
        ref = [np.random.randn(n) for _ in subset]
        z, attempts = J.job(seed, n, len(subset))
        assert z.shape == (len(subset), n) and z.dtype == np.float64
        for k in range(len(subset)):
            assert np.array_equal(z[k], ref[k]), (subset, k)
        if not subset:
            assert attempts == 0
        else:                                                  # the attempts are the stream position numpy reports
            pos = np.random.get_state()[2]
            assert pos == 4 * attempts - 624 * ((4 * attempts - 1) // 624), subset


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_roughness_job_is_the_float32_draw_of_its_own_seeding(global_state, idx):
    for n in COUNTS:
        np.random.seed(99)
        np.random.randn(3)                                     # a cached normal from before: the re-seeding clears it
        np.random.seed(1337 + idx)
        ref = np.random.randn(n).astype(np.float32).astype(np.float64)
        z, _ = J.job(1337 + idx, n, 1, f32=True)
        assert np.array_equal(z[0], ref)
        assert np.array_equal(z[0], z[0].astype(np.float32).astype(np.float64))
        if n > 2:
            assert not np.array_equal(J.job(1337 + idx, n, 1)[0][0], ref)      # (the rounding is not a no-op)


def test_run_fills_slices_drops_null_destinations_and_skips_empty_jobs(global_state):
    a, b = np.full(40, np.nan), np.full(40, np.nan)
    table = [(7, 5, [("a", 3), None, ("b", 10)], False),       # the middle stream is consumed and dropped
             (8, 0, [("a", 20)], False), (9, 4, [], False),    # nothing drawn
             (1337, 6, [("b", 30)], True)]
    att = J.run(table, {"a": a, "b": b})
    np.random.seed(7)
    r = [np.random.randn(5) for _ in range(3)]
    assert np.array_equal(a[3:8], r[0]) and np.array_equal(b[10:15], r[2])
    np.random.seed(1337)
    assert np.array_equal(b[30:36], np.random.randn(6).astype(np.float32).astype(np.float64))
    written = np.zeros(40, dtype=bool)
    written[3:8] = True
    assert np.array_equal(~np.isnan(a), written)
    assert att[1] == att[2] == 0 and att[0] > 0 and att[3] > 0


def test_the_new_names_exist():
    from goofer_amd import _lib, core, resynth
    from goofer_amd.device import Context
    from goofer_amd.render import PipelinedRenderer
    assert "goofer_legacy_normal_jobs" in _lib.EXPORTS and _lib.LEGACY_JOB.itemsize == 88
    header = open(os.path.join(REPO, "include", "goofer_hip.h")).read()
    assert re.search(r"\bint goofer_legacy_normal_jobs\(goofer_ctx \*ctx, const goofer_legacy_job \*jobs,", header)
    assert "launch_legacy_normal_jobs" in open(os.path.join(REPO, "goofer_amd", "csrc", "launchers.h")).read()
    kernels = open(os.path.join(REPO, "goofer_amd", "csrc", "noise.hip")).read()
    assert "k_legacy_normal_jobs" in kernels
    assert kernels.count("1812433253u") == 1 and kernels.count("0x9908b0dfu") == 1      # the recurrence and the twist: once
    assert callable(getattr(Context, "legacy_normal_jobs"))
    kwonly = lambda f, name: inspect.signature(f).parameters[name]                      # noqa: E731
    for f, name in ((core.synthesize, "noise_seed"), (core.synthesize_batch, "noise_seeds"), (core.resynthesize_batch, "noise_seeds"),
                    (core.resynthesize, "noise_seed")):
        p = kwonly(f, name)
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert inspect.signature(PipelinedRenderer.render_iter).parameters["noise_seeds"].default is None
    assert "noise_seed" not in core._synth_defaults()                                   # a call argument, not a note setting
    assert resynth.build_parser().parse_args(["--noise-seed", "4027", "a.wav"]).noise_seed == 4027
    assert resynth.build_parser().parse_args(["a.wav"]).noise_seed is None


def test_bad_seeds_are_refused_before_a_device_context_exists(monkeypatch):
    from goofer_amd import core, device

    def boom(*a, **k):
        raise AssertionError("a device context was made")
    monkeypatch.setattr(device.Context, "__init__", boom)
    monkeypatch.setattr(core, "_ctx", boom)
    note = {"env_spec": np.ones((513, 4), dtype=np.float32), "f0_interp": np.zeros(800), "voicing_mask": np.zeros(800), "y": np.zeros(800)}
    before = np.random.get_state()
    for bad in (-1, 2 ** 32, 1.5, True, "7"):
        with pytest.raises(ValueError, match="noise_seed"):
            core.synthesize(note["env_spec"], note["f0_interp"], note["voicing_mask"], note["y"], 44100, f0_jitter=True, noise_seed=bad)
        with pytest.raises(ValueError, match="noise_seeds"):
            core.synthesize_batch([note, note], 44100, noise_seeds=[3, bad], f0_jitter=True)
        with pytest.raises(ValueError, match="noise_seeds"):
            core.resynthesize_batch([note["y"]], 44100, noise_seeds=[bad], f0_jitter=True)
        with pytest.raises(ValueError, match="noise_seeds"):
            core.resynthesize(note["y"], 44100, noise_seed=bad, f0_jitter=True)
    for wrong in ([], [1], [1, 2, 3]):
        with pytest.raises(ValueError, match="noise seeds"):
            core.synthesize_batch([note, note], 44100, noise_seeds=wrong)
    with pytest.raises(ValueError, match="noise seeds"):
        core.resynthesize_batch([note["y"]], 44100, variants=[{}, {}], noise_seeds=[1, 2])   # per signal, not per variant
    after = np.random.get_state()
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])                  # nothing was drawn


@pytest.mark.parametrize("value", ["-1", str(2 ** 32), "1.5", "abc"])
def test_resynth_cli_refuses_a_bad_noise_seed_before_anything_is_read(monkeypatch, value):
    from goofer_amd import core, resynth

    def boom(*a, **k):
        raise AssertionError("something was rendered")
    monkeypatch.setattr(core, "resynthesize_batch", boom)
    with pytest.raises(SystemExit) as e:
        resynth.main(["--noise-seed", value, "missing.wav"])
    assert e.value.code == 2
