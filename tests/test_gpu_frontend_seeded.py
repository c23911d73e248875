"""GPU: the audio a host receives — out.wav of GooferResampler, of the 13-argument command line and of the HTTP server —
against the reference's own renders (tests/golden/sampler_*.npz, or the oracle where the server's one seed is not the
fixture's), with the reference's phases injected by seed (phi_seed / $GOOFER_PHI_SEED).  The fixtures' flags draw nothing
but phases."""
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
NAMES = ["default", "L0", "formants", "br_es_neg", "R1", "vol_mix"]


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bank(tmp_path_factory):
    """name -> (fixture, wav path with its .goofy written beside it, the 11 request strings, the oracle's feature tuple)"""
    from goofer_amd import core
    root = tmp_path_factory.mktemp("bank")
    out = {}
    for name in NAMES:
        g = golden("sampler_" + name)
        src = syn.make_source(2000 + CASES.index(name), seconds=0.45)             # test_gpu_sampler._job's source
        wav = root / f"{name}.wav"
        core.save_features(wav.with_name(f"{name}_features.goofy"), src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"],
                           src["y_len"])
        feats = (src["env_pack"], src["f0"].copy(), src["mask"].copy(), {k: v.copy() for k, v in src["formants"].items()}, src["sr"],
                 src["y_len"])
        out[name] = (g, wav, [str(a) for a in g["args"]], feats)
    return out


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


@pytest.mark.parametrize("name", NAMES)
def test_resampler_matches_the_reference(ctx, bank, tmp_path, name):
    from goofer_amd.render import GooferResampler, Renderer
    g, wav, args, _ = bank[name]
    out = tmp_path / "out.wav"
    r = GooferResampler(str(wav), str(out), *args, renderer=Renderer(ctx), phi_seed=int(g["seed"][0]))
    ref = g["out"]
    assert r.out.shape == ref.shape
    e = rms_err(r.out, ref) / max(1.0, float(np.max(np.abs(ref))))
    print(name, "rms_err / max(1, peak)", e)
    assert e < 2e-5, (name, e)                                                  # test_note_matches_reference's bound
    check_wav(out, ref)


@pytest.mark.parametrize("name", ["default", "formants"])
def test_command_line_matches_the_reference(bank, tmp_path, monkeypatch, name):
    from goofer_amd import cli
    g, wav, args, _ = bank[name]
    out = tmp_path / "cli.wav"
    monkeypatch.setenv("GOOFER_PHI_SEED", str(int(g["seed"][0])))
    assert cli.main([str(wav), str(out)] + args) == 0
    check_wav(out, g["out"])


def _post(port, body):
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", "/", body=body.encode("utf-8"))
    r = c.getresponse()
    res = r.status, r.read().decode()
    c.close()
    return res


def test_server_matches_the_reference_and_repeats_itself(ctx, bank, tmp_path):
    """six concurrent requests under one seed (the `default` fixture's: its reference is the fixture, the others' the oracle's
    render with that seed), then one of them again in a batch of its own: the same bytes"""
    from goofer_amd import cli
    from goofer_amd.render import Renderer
    from oracle import sampler_ref as SR
    seed = int(bank["default"][0]["seed"][0])
    refs = {}
    for name in NAMES:
        g, _, args, feats = bank[name]
        refs[name] = g["out"] if int(g["seed"][0]) == seed else SR.render(feats, SR.decode_request(*args), seed=seed)
    collector = cli.BatchCollector(Renderer(ctx), phi_seed=seed, window_s=0.25)
    httpd, _ = cli.serve(0, collector, host="127.0.0.1")
    port = httpd.server_address[1]
    th = threading.Thread(target=httpd.serve_forever, daemon=True)
    th.start()
    try:
        bodies = {name: " ".join([str(bank[name][1]), str(tmp_path / f"{name}.wav")] + bank[name][2]) for name in NAMES}
        answers = {}
        ts = [threading.Thread(target=lambda nm=nm: answers.__setitem__(nm, _post(port, bodies[nm]))) for nm in NAMES]
        for t in ts:
            t.start()
        for t in ts:
            t.join(180)
        assert answers == {nm: (200, "") for nm in NAMES}
        assert max(collector.batches) >= 2                                       # requests shared a device batch
        raw = {nm: check_wav(tmp_path / f"{nm}.wav", refs[nm]) for nm in NAMES}
        for nm in ("L0", "default"):                                             # again, each alone in its batch
            n_batches = len(collector.batches)
            again = tmp_path / f"{nm}_again.wav"
            assert _post(port, " ".join([str(bank[nm][1]), str(again)] + bank[nm][2])) == (200, "")
            assert collector.batches[n_batches:] == [1]
            with wave.open(str(again), "rb") as w:
                assert w.readframes(w.getnframes()) == raw[nm], nm
    finally:
        httpd.shutdown()
        httpd.server_close()
        collector.close()


def test_without_a_seed_two_renders_of_a_request_still_differ(ctx, bank, tmp_path):
    from goofer_amd import cli
    from goofer_amd.render import Renderer
    _, wav, args, _ = bank["default"]
    collector = cli.BatchCollector(Renderer(ctx), window_s=0.0)
    try:
        assert collector.phi_seed is None
        raws = []
        for k in range(2):
            out = tmp_path / f"u{k}.wav"
            collector.submit([str(wav), str(out)] + args)
            with wave.open(str(out), "rb") as w:
                assert w.getnframes() == len(bank["default"][0]["out"])
                raws.append(w.readframes(w.getnframes()))
        assert raws[0] != raws[1]
    finally:
        collector.close()
