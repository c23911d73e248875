"""The stereo bus: finished tracks panned and mixed on the device, then brought to a loudness and under a ceiling as a pair.

What follows a ``wavtool`` in every host is the mixer: a song is a lead, harmonies and a choir, each a track with a volume and a
pan fader, summed onto a stereo bus that is delivered at, say, -16 LUFS and -1 dBTP.  The reference project has no counterpart;
the definition is this project's own (``include/goofer_hip.h``, "stereo bus").  The bus is planar, L then R, a ragged
batch of two signals of equal length, so rate conversion, equaliser and reverb run on it as they are; the limiter and the
loudness gate have channel-linked forms (``goofer_limit_linked``, ``goofer_loudness_link``) and the int16 conversion an
interleaving one (``goofer_pcm16_planar``).  Here: the pan law (host, float64), the track records checked and the cover table
made by the library's planner (``goofer_host_bus_plan``), the song file, and a command line,

    python -m goofer_amd.bus [--rate HZ] [--loudness LUFS] [--limit [DB] [--true-peak]] song.txt out.wav

``song.txt`` holds one line per track, ``job.txt [gain_db [pan [start_ms]]] [eq=SPEC] [compress=SPEC] [reverb=SPEC] [mute]``::

    lead.txt 0 0
    harmony.txt -6 -0.5 0 eq=hp:120
    choir.txt -9 0.6 250 reverb=room:1.2:-10 mute

``job.txt`` is a phrase job file (``goofer_amd.phrase``), relative to the song file; ``gain_db`` in [-144, 24], ``pan`` in
[-1, 1] (-1 left, 1 right, constant power), ``start_ms`` >= 0 the track's position on the bus; the SPECs are those of
``python -m goofer_amd.phrase`` and run on the track alone, in front of the bus.  Empty lines and lines that start with ``#`` are
skipped.  ``--rate``, ``--loudness`` and ``--limit [DB] [--true-peak]`` are ``goofer_amd.phrase``'s, for the bus: the loudness
is the stereo programme's and the limiter gives both channels one gain.  The stage statistics go to stderr.
``Renderer.render_song`` is the same for (jobs, entries, Track) triples, ``core.bus_mix`` for host arrays.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

TILE = _lib.BUS_TILE
MIN_GAIN_DB, MAX_GAIN_DB = -144.0, 24.0


@dataclass(frozen=True)
class Track:
    """One fader of the bus: volume in dB, pan in [-1, 1], the track's position on the bus in ms, whether it is muted (a muted
    track is rendered by nobody and is not in the plan), and what ``render_song`` runs over the track alone in front of the bus:
    ``eq``, ``compress``, ``reverb`` as ``render_phrase`` takes them, and ``seed`` (None: the song's seed plus the track's
    index)."""
    gain_db: float = 0.0
    pan: float = 0.0
    start_ms: float = 0.0
    mute: bool = False
    eq: object = None
    compress: object = None
    reverb: object = None
    seed: object = None


def gains(gain_db, pan):
    """The pan law: (gl, gr), fp32.  g = 10^(gain_db / 20), theta = (pan + 1) pi / 4, gl = fp32(g cos theta), gr = fp32(g sin
    theta), in float64; exact at the ends (the far channel is +0) and in the middle (both fp32(g sqrt(0.5))).  Raises ValueError
    for a gain_db that is not finite or outside [-144, 24] and a pan outside [-1, 1]."""
    gain_db, pan = float(gain_db), float(pan)
    if not math.isfinite(gain_db) or not MIN_GAIN_DB <= gain_db <= MAX_GAIN_DB:
        raise ValueError("bus: gain_db is finite and lies in [%g, %g]" % (MIN_GAIN_DB, MAX_GAIN_DB))
    if not -1.0 <= pan <= 1.0:                                 # (a NaN fails both)
        raise ValueError("bus: pan lies in [-1, 1]")
    g = 10.0 ** (gain_db / 20.0)
    if pan == -1.0:
        return np.float32(g), np.float32(0.0)
    if pan == 1.0:
        return np.float32(0.0), np.float32(g)
    if pan == 0.0:
        m = np.float32(g * math.sqrt(0.5))
        return m, m
    th = (pan + 1.0) * math.pi / 4.0
    return np.float32(g * math.cos(th)), np.float32(g * math.sin(th))


def samples(ms, sr) -> int:
    """floor(ms * sr / 1000 + 0.5)"""
    return int(math.floor(float(ms) * float(sr) / 1000.0 + 0.5))


@dataclass
class BusPlan(SP.CoverPlan):
    """What goofer_bus_mix takes for one song: ``tracks`` (_lib.BUS_TRACK [n], the tracks that are not muted, with the device
    pointers they were planned for), the cover table ``tile_off`` (int64 [tiles + 1]) / ``tile_tracks`` (int32), ``total_out``,
    the samples of one channel; ``index``: which of the caller's tracks each record is; ``blob`` holds the three arrays back to
    back for one upload."""
    tracks: np.ndarray
    index: np.ndarray
    tile_off: np.ndarray
    tile_tracks: np.ndarray
    BLOB = ("tracks", "tile_off", "tile_tracks")

    @property
    def in_off(self):
        """the bus as a ragged batch of two signals: [0, N, 2N]"""
        return np.array([0, self.total_out, 2 * self.total_out], dtype=np.int64)


def cover(records: np.ndarray, total_out: int):
    """goofer_host_bus_plan: the records checked and the cover table of the bus's tiles, (tile_off, tile_tracks).  Raises
    ValueError for a record the library refuses."""
    records = np.ascontiguousarray(records, dtype=_lib.BUS_TRACK)
    if int(total_out) < 0:
        raise ValueError("bus: total_out >= 0")
    if (int(total_out) + TILE - 1) // TILE >= 1 << 31:
        raise ValueError("bus: a bus of 2^31 tiles or more")
    return SP.cover(_lib.load().goofer_host_bus_plan, records, (), total_out, TILE,
                    lambda rc: "goofer_host_bus_plan refused the tracks (%d): lengths, starts and total_out >= 0, finite gains, "
                               "4-byte aligned pointers" % rc)


def plan(ptrs_or_tensors, lengths, tracks, sr, total_out=None) -> BusPlan:
    """The records, the cover table and the bus length of a song, ready for one upload.  ``ptrs_or_tensors``: per track a device
    tensor (its ``data_ptr()`` is taken; the caller keeps it alive) or the device address as an int; ``lengths``: the tracks'
    sample counts; ``tracks``: one ``Track`` each (its eq / compress / reverb / seed are the renderer's business, not the
    bus's); ``sr``: the rate the tracks are at.  Muted tracks get no record.  ``total_out`` defaults to the largest start + length
    of a track that sounds (0 without one)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    tracks = list(tracks)
    if not (len(ptrs_or_tensors) == len(lengths) == len(tracks)):
        raise ValueError("bus.plan: one pointer, one length and one Track per track")
    if int(sr) != sr or int(sr) < 1:
        raise ValueError("bus.plan: the sample rate is a whole number of Hz")
    if lengths.size and lengths.min() < 0:
        raise ValueError("bus.plan: a negative length")
    keep = [k for k, t in enumerate(tracks) if not t.mute]
    rec = np.zeros(len(keep), dtype=_lib.BUS_TRACK)
    for j, k in enumerate(keep):
        t, p = tracks[k], ptrs_or_tensors[k]
        if not (float(t.start_ms) >= 0.0) or not math.isfinite(float(t.start_ms)):
            raise ValueError("bus.plan: start_ms is finite and >= 0")
        gl, gr = gains(t.gain_db, t.pan)
        rec[j] = (int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p), lengths[k], samples(t.start_ms, sr), gl, gr)
    if total_out is None:
        total_out = int((rec["start"] + rec["len"]).max()) if len(rec) else 0
    tile_off, tile_tracks = cover(rec, int(total_out))
    return BusPlan(len(rec), int(total_out), int(sr), rec, np.asarray(keep, dtype=np.int64), tile_off, tile_tracks)


# ---- the song file -----------------------------------------------------------------------------------------------------------

def parse_line(text):
    """One line of a song file: (job file as written, Track).  ``job.txt [gain_db [pan [start_ms]]] [eq=SPEC] [compress=SPEC]
    [reverb=SPEC] [mute]``; the numbers come first, in this order."""
    toks = text.split()
    if not toks:
        raise ValueError("a track is `job.txt [gain_db [pan [start_ms]]] [eq=SPEC] [compress=SPEC] [reverb=SPEC] [mute]`")
    nums, kw, mute, named = [], {}, False, False
    for tok in toks[1:]:
        if tok == "mute":
            mute = named = True
        elif "=" in tok and tok.split("=", 1)[0] in ("eq", "compress", "reverb"):
            k, v = tok.split("=", 1)
            if k in kw or not v:
                raise ValueError(f"`{k}=` is given once, with a value")
            kw[k], named = v, True
        else:
            if named or len(nums) == 3:
                raise ValueError(f"`{tok}`: gain_db, pan and start_ms come first, then eq= compress= reverb= mute")
            nums.append(float(tok))
    if "eq" in kw:
        from . import eq as EQ
        kw["eq"] = EQ.parse(kw["eq"])
    if "compress" in kw:
        from . import compress as CP
        kw["compress"] = CP.parse(kw["compress"])
    if "reverb" in kw:
        from . import reverb as RV
        kw["reverb"] = RV.parse(kw["reverb"])
    t = Track(*nums, mute=mute, **kw)
    gains(t.gain_db, t.pan)
    if not (t.start_ms >= 0.0) or not math.isfinite(t.start_ms):
        raise ValueError("start_ms is finite and >= 0")
    return toks[0], t


def read_song(path):
    """The lines of a song file: [(job file, resolved against the song file's folder, Track)]."""
    out, here = [], os.path.dirname(os.path.abspath(str(path)))
    with open(path, encoding="utf-8") as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                job, t = parse_line(line)
            except ValueError as err:
                raise ValueError(f"{path}:{ln}: {err}") from None
            out.append((job if os.path.isabs(job) else os.path.join(here, job), t))
    return out


def render_file(path, out_wav, renderer=None, seed=None, tracker=None, pcm16=True, out_sr=None, loudness=None, limit=None, stats=None):
    """``python -m goofer_amd.bus``: the job files of a song rendered track by track on the device, mixed and finished as
    ``Renderer.render_song`` does, and written as one two-channel wav.  The samples of the job files are found like
    ``phrase.render_job`` finds them.  ``stats``, a dict, receives ``render_song``'s statistics where ``loudness`` or ``limit``
    asks for a stage that has some."""
    from . import phrase as P
    from .render import Renderer, write_wav
    song = read_song(path)
    renderer = renderer or Renderer()
    if seed is None:
        seed = P.draw_seed(np.uint32)
    tracks = []
    for job, t in song:
        if t.mute:
            tracks.append(([], [], t))
            continue
        jobs, entries = P.load_job(job, renderer, tracker)
        tracks.append((jobs, entries, t))
    live = [jobs for jobs, _, t in tracks if not t.mute]
    if not live:
        raise ValueError(f"{path}: no track that sounds")
    sr = live[0][0][0].sr if out_sr is None else int(out_sr)
    bus = P.rendered(renderer.render_song, stats, loudness is not None or limit is not None, tracks=tracks, seed=seed, pcm16=pcm16,
                     out_sr=out_sr, loudness=loudness, limit=limit)
    write_wav(out_wav, bus, sr)
    return bus


def main(argv=None) -> int:
    import logging
    from . import limit as LM
    from . import phrase as P
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    opts, argv = P.parse_options(list(sys.argv[1:] if argv is None else argv), ("--rate", "--limit", "--loudness", "--true-peak"))
    out_sr, limit, loudness, true_peak = opts.get("--rate"), opts.get("--limit"), opts.get("--loudness"), "--true-peak" in opts
    if len(argv) != 2 or (true_peak and limit is None):
        logging.error("Usage:\n  python -m goofer_amd.bus [--rate HZ] [--loudness LUFS] [--limit [DB] [--true-peak]] song.txt out.wav")
        return 1
    stats = {}
    try:
        bus = render_file(argv[0], argv[1], out_sr=out_sr, limit=LM.Limiter(limit, true_peak=True) if true_peak else limit, stats=stats,
                          loudness=loudness)
    except Exception:                   # noqa: BLE001
        logging.exception("Failed to render")
        return 1
    P.report_levels(stats, loudness, limit, true_peak)
    logging.info(f"Writing {argv[1]}: {len(bus)} frames, 2 channels")
    return 0


if __name__ == "__main__":
    sys.exit(main())
