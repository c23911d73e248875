"""GPU: a seeded reference run of an sh / sr note reproduced from the seeds alone — ``noise_seeds`` / ``noise_seed`` /
``$GOOFER_NOISE_SEED`` beside the phase seed — through Renderer.render, GooferResampler, the 13-argument command line and the
HTTP server.  The legacy normals are drawn on the device (goofer_legacy_normal_fill); no test here seeds numpy's global
generator for the code under test.

Bounds: the fixture's note at ``e < 2e-5`` (tests/test_gpu_sampler.py's jitter test) and its wav within 1 LSB
(tests/test_gpu_frontend_seeded.check_wav's arithmetic); oracle renders at test_gpu_sampler's ``TOL``."""
import http.client
import threading
import wave

import numpy as np
import pytest

from conftest import golden, rms_err
from goofer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = [str(n) for n in golden("sampler_index")["names"]]
NAME = "sh50sr50"
TOL = 1e-4                                                                      # tests/test_gpu_sampler.py's oracle bound

# six notes: sh only, sr only, both, neither, both (an even length), both with 'sd30'; four of the lengths are odd
FLAGS = ["sh50", "sr50", "sh30sr70", "g0", "sh50sr50", "sh40sr40sd30"]
LENGTH_MS = [300, 350, 420, 250, 333, 380]
PHI = [900 + k for k in range(6)]
LEGACY = [50, 2 ** 32 - 1, 0, 53, 4027, 55]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bank(tmp_path_factory):
    """(fixture, wav path with its .goofy written beside it, the 11 request strings) of sampler_sh50sr50.npz"""
    from goofer_amd import core
    root = tmp_path_factory.mktemp("bank")
    g = golden("sampler_" + NAME)
    src = syn.make_source(2000 + CASES.index(NAME), seconds=0.45)                # test_gpu_sampler._job's source
    wav = root / f"{NAME}.wav"
    core.save_features(wav.with_name(f"{NAME}_features.goofy"), src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"],
                       src["y_len"])
    return g, wav, [str(a) for a in g["args"]]


@pytest.fixture(scope="module")
def six():
    """the six jobs and, per note, the oracle's render alone after np.random.seed(its legacy seed)"""
    from goofer_amd import sampler as S
    from goofer_amd.render import Source
    from oracle import sampler_ref as SR
    jobs, refs = [], []
    state = np.random.get_state()
    try:
        for k, (flags, ms) in enumerate(zip(FLAGS, LENGTH_MS)):
            src = syn.make_source(7100 + k, seconds=0.4)
            args = ("C4", "100", flags, "10", str(ms), "30", "30", "100", "0", "!120", "AA")
            feats = (src["env_pack"], src["f0"].copy(), src["mask"].copy(), {a: b.copy() for a, b in src["formants"].items()}, src["sr"],
                     src["y_len"])
            np.random.seed(LEGACY[k])
            refs.append(SR.render(feats, SR.decode_request(*args), seed=PHI[k]))
            jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                         S.decode_request(*args)))
    finally:
        np.random.set_state(state)
    assert any(len(r) % 2 for r in refs) and any(len(r) % 2 == 0 for r in refs)
    return jobs, refs


def pcm16(x):
    """render.write_wav's own int16 arithmetic"""
    return np.round(np.clip(np.asarray(x).astype(np.float64), -1.0, 1.0 - 1.0 / 32768) * 32768.0).astype("<i2")


def check_wav(path, ref, sr=44100):
    """PCM16 of the reference's length, every sample within 1 LSB of the reference through write_wav's arithmetic; the bytes"""
    with wave.open(str(path), "rb") as w:
        assert w.getframerate() == sr and w.getnchannels() == 1 and w.getsampwidth() == 2
        assert w.getnframes() == len(ref)
        raw = w.readframes(w.getnframes())
    got = np.frombuffer(raw, dtype="<i2").astype(np.int64)
    worst = int(np.abs(got - pcm16(ref).astype(np.int64)).max())
    print(path.name, "worst int16 difference", worst, "samples that differ", int((got != pcm16(ref)).sum()), "of", len(ref))
    assert worst <= 1, (path.name, worst)
    assert int(np.abs(got).max()) > 1000                                        # (audio, not silence)
    return raw


def _seeds(g):
    return int(g["seed"][0]), int(g["seed"][1])


def test_resampler_matches_the_reference(ctx, bank, tmp_path):
    from goofer_amd.render import GooferResampler, Renderer
    g, wav, args = bank
    phi, legacy = _seeds(g)
    out = tmp_path / "out.wav"
    before = np.random.get_state()
    r = GooferResampler(str(wav), str(out), *args, renderer=Renderer(ctx), phi_seed=phi, noise_seed=legacy)
    after = np.random.get_state()
    ref = g["out"]
    assert r.out.shape == ref.shape
    e = rms_err(r.out, ref) / max(1.0, float(np.max(np.abs(ref))))
    print(NAME, "rms_err / max(1, peak)", e)
    assert e < 2e-5, e                                                          # test_jitter_flags_sh_sr_match_reference's bound
    check_wav(out, ref)
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])      # the global generator was not touched


def test_command_line_matches_the_reference(bank, tmp_path, monkeypatch):
    from goofer_amd import cli
    g, wav, args = bank
    phi, legacy = _seeds(g)
    out = tmp_path / "cli.wav"
    monkeypatch.setenv("GOOFER_PHI_SEED", str(phi))
    monkeypatch.setenv("GOOFER_NOISE_SEED", str(legacy))
    assert cli.main([str(wav), str(out)] + args) == 0
    check_wav(out, g["out"])


def _post(port, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", "/", body=body.encode("utf-8"))
    r = c.getresponse()
    res = r.status, r.read().decode()
    c.close()
    return res


def test_server_matches_the_reference(ctx, bank, tmp_path):
    from goofer_amd import cli
    from goofer_amd.render import Renderer
    g, wav, args = bank
    phi, legacy = _seeds(g)
    collector = cli.BatchCollector(Renderer(ctx), phi_seed=phi, noise_seed=legacy, window_s=0.0)
    httpd, _ = cli.serve(0, collector, host="127.0.0.1")
    port = httpd.server_address[1]
    th = threading.Thread(target=httpd.serve_forever, daemon=True)
    th.start()
    try:
        raws = []
        for k in range(2):                                                       # a request and the same request again: the same bytes
            out = tmp_path / f"srv{k}.wav"
            assert _post(port, " ".join([str(wav), str(out)] + args)) == (200, "")
            raws.append(check_wav(out, g["out"]))
        assert raws[0] == raws[1]
    finally:
        httpd.shutdown()
        httpd.server_close()
        collector.close()


def test_six_note_batch_against_the_oracle_and_against_single_renders(ctx, six):
    from goofer_amd.render import Renderer
    jobs, refs = six
    r = Renderer(ctx)
    before = np.random.get_state()
    batch = r.render(jobs, phi_seeds=PHI, noise_seeds=LEGACY)
    after = np.random.get_state()
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])      # np.random.get_state() is unchanged
    for k, (out, ref) in enumerate(zip(batch, refs)):
        assert out.shape == ref.shape, k
        e = rms_err(out, ref) / max(1.0, float(np.max(np.abs(ref))))
        print(FLAGS[k], len(ref), "rms_err / max(1, peak)", e)
        assert e < TOL, (FLAGS[k], e)
    for k, job in enumerate(jobs):
        (one,) = r.render([job], phi_seeds=[PHI[k]], noise_seeds=[LEGACY[k]])
        assert np.array_equal(one, batch[k]), (FLAGS[k], float(np.max(np.abs(one - batch[k]))))


def test_device_growl_with_legacy_jitter(ctx, six):
    """noise="device" with noise_seeds: sh / sr from the legacy stream (the notes without 'sj' render as under noise="host"),
    'sj' from the device's own stream"""
    from goofer_amd.render import Renderer
    jobs, _ = six
    host = Renderer(ctx).render(jobs[:3], seed=5, phi_seeds=PHI[:3], noise_seeds=LEGACY[:3])
    dev = Renderer(ctx, noise="device").render(jobs[:3], seed=5, phi_seeds=PHI[:3], noise_seeds=LEGACY[:3])
    for a, b in zip(host, dev):
        assert np.array_equal(a, b)


def test_without_a_noise_seed_two_renders_of_an_sh_request_still_differ(ctx, bank, tmp_path):
    from goofer_amd import cli
    from goofer_amd.render import Renderer
    g, wav, args = bank
    collector = cli.BatchCollector(Renderer(ctx), phi_seed=_seeds(g)[0], window_s=0.0)
    try:
        assert collector.noise_seed is None
        raws = []
        for k in range(2):
            out = tmp_path / f"u{k}.wav"
            collector.submit([str(wav), str(out)] + args)
            with wave.open(str(out), "rb") as w:
                assert w.getnframes() == len(g["out"])
                raws.append(w.readframes(w.getnframes()))
        assert raws[0] != raws[1]
    finally:
        collector.close()


def test_prepare_without_device_calls_launches_nothing(ctx, six, monkeypatch):
    from goofer_amd.render import Renderer
    jobs, _ = six
    r = Renderer(ctx)
    r.render(jobs[:1], phi_seeds=PHI[:1], noise_seeds=LEGACY[:1])               # (plans the geometry, makes the sources resident)
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("goofer_"):
                return fn

            def wrapped(*a):
                called.append(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(ctx, "lib", Spy(ctx.lib))
    before = np.random.get_state()
    prep = r.prepare(jobs, phi_seeds=PHI, noise_seeds=LEGACY, device_calls=False)
    after = np.random.get_state()
    launches = [c for c in called if c not in ("goofer_host_plan_into", "goofer_last_error")]
    assert launches == [], launches                                             # no library call that touches the device
    assert prep["noise_f0"] is None and prep["noise_vol"] is None               # nothing drawn, nothing uploaded per sample
    assert prep["legacy_noise"]["seeds"].numel() == 6 and prep["legacy_noise"]["on"].numel() == 18
    assert before[2:] == after[2:] and np.array_equal(before[1], after[1])
    monkeypatch.undo()
    with pytest.raises(ValueError):
        r.prepare(jobs, noise_seeds=LEGACY[:5])
    with pytest.raises(ValueError):
        r.prepare(jobs, noise_seeds=[None] + LEGACY[1:])
    with pytest.raises(ValueError):
        r.prepare(jobs, noise_seeds=[2 ** 32] + LEGACY[1:])
