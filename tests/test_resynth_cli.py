"""python -m goofer_amd.resynth without a GPU: argument parsing, keyword checks (exit status 2 before anything is read) and
output naming."""
import wave
from pathlib import Path

import numpy as np
import pytest

from goofer_amd import resynth


def _settings(argv):
    ap = resynth.build_parser()
    args = ap.parse_args(argv)
    return args, resynth.settings(args, ap.error)


def test_shortcuts_set_and_variants_parse():
    args, (kw, variants) = _settings(["x.wav", "--pitch", "1.5", "--F2", "0.9", "--stretch", "1.25", "--set", "f0_jitter=True",
                                      "--set", "subharm_semitones=[-12, 7]", "--variant", "formant_shift=0.8,add_subharm=True",
                                      "--variant", "subharm_semitones=[-12, -24],pitch_shift=2"])
    assert kw == {"pitch_shift": 1.5, "F2_shift": 0.9, "stretch_factor": 1.25, "f0_jitter": True, "subharm_semitones": [-12, 7]}
    assert variants == [{"formant_shift": 0.8, "add_subharm": True}, {"subharm_semitones": [-12, -24], "pitch_shift": 2}]
    assert args.n_fft == 1024 and args.hop is None and not args.stems and args.seed is None and args.out is None


def test_no_variant_is_none_and_bare_words_are_strings():
    _, (kw, variants) = _settings(["x.wav", "--set", "normalize=0.5"])
    assert variants is None and kw == {"normalize": 0.5}
    assert resynth.parse_assignment("key=hello") == ("key", "hello")
    assert resynth.parse_variant("a=word,b='q,r',c=(1, 2)") == {"a": "word", "b": "q,r", "c": (1, 2)}


@pytest.mark.parametrize("argv", [["x.wav", "--set", "no_such_keyword=1"], ["x.wav", "--variant", "pitch_shift=1,bogus=2"],
                                  ["x.wav", "--set", "novalue"], ["x.wav", "--variant", "1,2"]])
def test_unknown_or_malformed_keyword_exits_2_before_reading(argv, monkeypatch):
    from goofer_amd import trackers
    monkeypatch.setattr(trackers, "read_audio", lambda p: pytest.fail("read before the keywords were checked"))
    with pytest.raises(SystemExit) as e:
        resynth.main(argv)
    assert e.value.code == 2


def test_hop_defaults_to_a_quarter_of_n_fft(monkeypatch, tmp_path):
    seen = {}

    def fake(signals, sr, n_fft, hop, **kw):
        seen.update(n_fft=n_fft, hop=hop)
        return [(np.zeros(4, np.float32),) * 4 for _ in signals]
    from goofer_amd import core
    monkeypatch.setattr(core, "resynthesize_batch", fake)
    f = tmp_path / "a.wav"
    with wave.open(str(f), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(22050)
        w.writeframes(np.zeros(200, "<i2").tobytes())
    assert resynth.main([str(f), "--n-fft", "2048"]) == 0
    assert seen == {"n_fft": 2048, "hop": 512}
    assert (tmp_path / "a_reconstruct.wav").exists() and not (tmp_path / "a_harmonic.wav").exists()


def test_output_names():
    src = Path("/data/bank/sub/la.wav")
    assert resynth.output_paths(src) == [{"reconstruct": Path("/data/bank/sub/la_reconstruct.wav")}]
    stems = resynth.output_paths(src, stems=True)[0]
    assert stems == {n: Path(f"/data/bank/sub/la_{n}.wav") for n in ("reconstruct", "harmonic", "breathiness", "unvoiced")}
    two = resynth.output_paths(src, Path("/data/bank"), "/out", 2, False)
    assert two == [{"reconstruct": Path("/out/sub/la_v0_reconstruct.wav")}, {"reconstruct": Path("/out/sub/la_v1_reconstruct.wav")}]
    assert resynth.output_paths(src, None, "/out", 1, True)[0]["unvoiced"] == Path("/out/la_v0_unvoiced.wav")
    assert dict(resynth.STEM_NAMES) == {"reconstruct": 0, "harmonic": 1, "breathiness": 3, "unvoiced": 2}


def test_folder_scan_skips_own_outputs(tmp_path):
    for name in ("a.wav", "a_reconstruct.wav", "a_v1_harmonic.wav", "b.WAV", "notes.txt", "sub/c.flac", "sub/c_unvoiced.wav"):
        p = tmp_path / name
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    found = resynth.collect_inputs([str(tmp_path), str(tmp_path / "a.wav")])
    assert [(f.relative_to(tmp_path).as_posix(), r) for f, r in found] == [("a.wav", tmp_path), ("b.WAV", tmp_path), ("sub/c.flac", tmp_path)]
