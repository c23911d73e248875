"""The four notes of render_phrase.py as TWO tracks of a song: each rendered and assembled into its own track on the device,
panned left and right, mixed onto a stereo bus, brought to -16 LUFS and under -1 dBTP as a pair, and downloaded once as
interleaved int16 (needs an MI355X).

    python examples/render_song.py out.wav

A track is ``(jobs, entries, bus.Track)``: what ``render_phrase`` takes, and the fader — volume in dB, pan in [-1, 1], the
track's position on the bus in ms, and what runs over the track alone in front of the bus (eq, compress, reverb)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from goofer_amd import bus
from goofer_amd import limit as LM
from goofer_amd import sampler as S
from goofer_amd import synthetic as syn
from goofer_amd.render import Renderer, Source, write_wav


def main(out_wav):
    renderer = Renderer()
    notes = [
        (("C4", "100", "g-10", "30", "600", "80", "50", "100", "0", "!120", "AA"), "0 480@120 5 35 40 0 80 80 0"),
        (("E4", "100", "t30fa20fb-10B30", "30", "900", "80", "50", "90", "0", "!120", "AA#20#AP"), "0 720@120+30 5 35 40 0 80 80 0 30"),
        (("G4", "80", "L1sg40st-30", "30", "1200", "80", "50", "100", "0", "!120", "AA"), "0 960@120 5 35 40 0 70 60 0 0 10 100 85"),
        (("A3", "120", "vf30sa20pd40", "30", "700", "80", "50", "100", "0", "!120", "AA#10#BA#10#AA"), "20 480@120+40 5 35 60 0 80 80 0 40"),
    ]
    jobs, entries = [], []
    for k, (args, wavtool) in enumerate(notes):
        src = syn.make_source(100 + k, seconds=0.5)                      # stands in for core.load_features(<stem>_features.goofy)
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*args)))
        entries.append(wavtool)
    tracks = [(jobs[:2], entries[:2], bus.Track(gain_db=-3.0, pan=-0.5)),
              (jobs[2:], entries[2:], bus.Track(gain_db=0.0, pan=0.5, start_ms=250.0, eq="hp:120"))]
    frames, stats = renderer.render_song(tracks, seed=1, pcm16=True, out_sr=48000, loudness=-16.0,
                                         limit=LM.Limiter(10.0 ** (-1.0 / 20.0), true_peak=True), return_stats=True)
    write_wav(out_wav, frames, 48000)                                    # [N, 2] int16: a two-channel wav
    print(f"{out_wav}: {len(frames)} frames, {len(frames) / 48000:.2f} s, {stats['lufs_in']:.2f} LUFS in, gain {stats['gain']:.3f}, "
          f"true peak {LM.dbtp(stats['true_peak_in']):.2f} -> {LM.dbtp(stats['true_peak_out']):.2f} dBTP")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "song.wav")
