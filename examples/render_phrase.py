"""The four notes of render_batch.py as ONE phrase: rendered as a batch, then trimmed, enveloped, cross-faded and mixed into one
track on the device — the step UTAU leaves to a `wavtool` — and downloaded once (needs an MI355X).

    python examples/render_phrase.py out.wav

Each note carries, beside its resampler arguments, what UTAU would hand the wavtool: ``stp length p1 p2 p3 v1 v2 v3 v4 [ovr [p4
[p5 v5]]]`` (length in ms or ticks@tempo, envelope positions in ms, values in percent, ``ovr`` the overlap with the note
before).  ``R <length>`` is a rest."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from goofer_amd import sampler as S
from goofer_amd import synthetic as syn
from goofer_amd.render import Renderer, Source, write_wav


def main(out_wav):
    renderer = Renderer()
    notes = [
        (("C4", "100", "g-10", "30", "600", "80", "50", "100", "0", "!120", "AA"), "0 480@120 5 35 40 0 80 80 0"),
        (("E4", "100", "t30fa20fb-10B30", "30", "900", "80", "50", "90", "0", "!120", "AA#20#AP"), "0 720@120+30 5 35 40 0 80 80 0 30"),
        (None, "R 240@120"),
        (("G4", "80", "L1sg40st-30", "30", "1200", "80", "50", "100", "0", "!120", "AA"), "0 960@120 5 35 40 0 70 60 0 0 10 100 85"),
        (("A3", "120", "vf30sa20pd40", "30", "700", "80", "50", "100", "0", "!120", "AA#10#BA#10#AA"), "20 480@120+40 5 35 60 0 80 80 0 40"),
    ]
    jobs, entries = [], []
    for args, wavtool in notes:
        entries.append(wavtool)
        if args is None:
            continue
        src = syn.make_source(100 + len(jobs), seconds=0.5)            # stands in for core.load_features(<stem>_features.goofy)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
    track = renderer.render_phrase(jobs, entries, seed=1, pcm16=True)   # int16, converted on the device: what the wav holds
    write_wav(out_wav, track, jobs[0][0].sr)
    print(f"{out_wav}: {len(track)} samples, {len(track) / jobs[0][0].sr:.2f} s, peak {abs(track.astype(int)).max() / 32768:.3f}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "phrase.wav")
