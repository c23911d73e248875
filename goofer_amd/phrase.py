"""Phrase assembly: the rendered notes of a batch enveloped, cross-faded and mixed into one track on the device.

UTAU hands this step to a separate ``wavtool``: each note is trimmed (``stp``, ``length``), shaped by a seven-knot volume
envelope, overlapped with its neighbour and summed onto the song's time line.  The reference project has no counterpart; the
definition is this project's own (``include/goofer_hip.h``, goofer_phrase_note) and the kernel is
``goofer_phrase_mix``.  Here: wavtool's arguments turned into note records (host, float64), the records checked and the
cover table made by the library's planner (``goofer_host_phrase_plan``), and a command line,

    python -m goofer_amd.phrase [--rate HZ] [--eq SPEC] [--compress T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]] [--reverb SPEC] [--loudness LUFS] [--limit [DBFS] [--true-peak]] job.txt out.wav

``job.txt`` holds one line per note, the 13 resampler arguments, ``|``, then wavtool's ``stp length p1 p2 p3 v1 v2 v3 v4 [ovr
[p4 [p5 v5]]]``::

    voice/a.wav a.wav C4 100 g-5 30 600 80 50 100 0 !120 AA | 0 480@120+20 5 35 40 0 100 100 0 20
    R 240@120

(the second argument, the resampler's out file, is not written: the notes stay on the device).  ``R <length>`` is a rest; empty
lines and lines that start with ``#`` are skipped.  ``--rate HZ`` converts the mixed track from the voicebank's rate to HZ on
the device (goofer_amd.rate) before it becomes int16; the wav's header carries HZ.  ``--limit [DBFS]`` runs the look-ahead peak
limiter (goofer_amd.limit) over the track at the rate of the wav, with the ceiling DBFS decibels relative to full scale (bare:
32767/32768), and reports the track's peak in front of it and its greatest gain reduction on stderr; with ``--true-peak`` (a
flag without a value, only together with ``--limit``) the ceiling is read as dBTP and holds for the signal reconstructed between
the samples too, and stderr reports the track's true peak in front of and behind the limiter.  ``--loudness LUFS``
measures the track's integrated loudness after BS.1770 (goofer_amd.loudness) and scales the track to LUFS, in front of the
limiter, the gain capped at 20 dB; the measured loudness and the gain go to stderr too.  ``--compress
T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]`` runs the dynamic range compressor (goofer_amd.compress) over the track behind the rate
conversion and in front of the loudness stage: threshold T in dB re full scale, ratio R (``inf`` allowed), attack and release in
ms (5 and 100), knee width in dB (6), make-up gain in dB (0); its greatest gain reduction goes to stderr.  ``--eq SPEC`` runs
the parametric equaliser (goofer_amd.eq) over the track behind the rate conversion and in front of the compressor: SPEC is up
to eight bands joined by commas, each ``kind:f0[:gain_db[:q]]`` with the kinds ``hp lp ls hs peak notch``, f0 in Hz between
1/600 and 0.45 of the wav's rate, gain_db in [-9, 9] for ``ls hs peak`` and q in [0.1, 8] (``ls hs``: [0.1, 2]; default sqrt(1/2)), as in
``--eq hp:80,peak:3000:3:1,hs:10000:4``.
``--reverb SPEC`` runs the convolution reverb (goofer_amd.reverb) over the track behind the compressor and in front of the
loudness stage: ``room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]]`` for a synthetic room, ``ir:PATH[:WET_DB[:PREDELAY_MS]]`` for a mono
wav at the output's rate; the impulse response's length and the tail it adds go to stderr, e.g. ``--reverb room:1.2:-10:20``.
``Renderer.render_phrase`` is the same for (Source, Request) jobs.
"""
from __future__ import annotations

import math
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import signal_plan as SP

TILE = _lib.PHRASE_TILE
MAX_TAKE = 1 << 24


def parse_length(text) -> float:
    """wavtool's length in ms: plain milliseconds, or ``ticks@tempo[+-ms]`` = ticks / 480 * 60000 / tempo +- ms."""
    if isinstance(text, (int, float)):
        return float(text)
    s = str(text).strip()
    if "@" not in s:
        return float(s)
    ticks, rest = s.split("@", 1)
    cut = max(rest.rfind("+"), rest.rfind("-"))
    if cut > 0 and rest[cut - 1] not in "eE":
        tempo, extra = rest[:cut], float(rest[cut:])
    else:
        tempo, extra = rest, 0.0
    return float(ticks) / 480.0 * 60000.0 / float(tempo) + extra


def samples(ms: float, sr) -> int:
    """floor(ms * sr / 1000 + 0.5)"""
    return int(math.floor(float(ms) * float(sr) / 1000.0 + 0.5))


def envelope_overlap(args) -> float:
    """``ovr`` of wavtool's envelope arguments ``p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]]`` in ms (missing: 0)."""
    return float(args[7]) if len(args) > 7 else 0.0


def envelope_knots(args, length_ms: float, sr):
    """The seven knots of a note's record from wavtool's envelope arguments ``p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]]`` (ms
    positions, percent values): (pos float32 [7] in samples, val float32 [7] linear).  In ms the knots are [0, p1, p1 + p2,
    p1 + p2 + p5, L - p4 - p3, L - p4, L] with the values [0, v1, v2, v5, v3, v4, 0] / 100; a missing p4 is 0, a missing
    p5 / v5 repeats knot 2.  Positions are clamped to [0, L], made non-decreasing by a running maximum, converted to samples
    (* sr / 1000, not rounded), rounded to float32 and held at or below ``(float)take``, which the last one is set to
    (take = floor(L * sr / 1000 + 0.5) may lie below L * sr / 1000)."""
    a = [float(v) for v in args]
    if len(a) < 7 or len(a) == 10 or len(a) > 11:
        raise ValueError(f"envelope: p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]] expected, got {len(a)} values")
    L = float(length_ms)
    if not (L >= 0.0) or not all(math.isfinite(v) for v in a):
        raise ValueError("envelope: the length must be >= 0 ms and every argument finite")
    p1, p2, p3, v1, v2, v3, v4 = a[:7]
    p4 = a[8] if len(a) > 8 else 0.0
    p5, v5 = (a[9], a[10]) if len(a) > 10 else (0.0, v2)
    pos_ms = np.array([0.0, p1, p1 + p2, p1 + p2 + p5, L - p4 - p3, L - p4, L], dtype=np.float64)
    pos_ms = np.maximum.accumulate(np.clip(pos_ms, 0.0, L))
    take = samples(L, sr)
    pos = np.minimum((pos_ms * float(sr) / 1000.0).astype(np.float32), np.float32(take))
    pos[0], pos[6] = 0.0, np.float32(take)
    val = (np.array([0.0, v1, v2, v5, v3, v4, 0.0], dtype=np.float64) / 100.0).astype(np.float32)
    return pos, val


def place(lengths_ms, overlaps_ms, sr) -> np.ndarray:
    """Track positions of the entries of a phrase laid end to end: b_0 = -ovr_0, b_i = b_(i-1) + L_(i-1) - ovr_i in ms and
    float64; start_i = floor(b_i * sr / 1000 + 0.5), int64 (a first overlap puts start_0 below 0: those samples are dropped)."""
    starts = np.zeros(len(lengths_ms), dtype=np.int64)
    b = 0.0
    for i, (L, ovr) in enumerate(zip(lengths_ms, overlaps_ms)):
        b = b - float(ovr) if i == 0 else b + float(lengths_ms[i - 1]) - float(ovr)
        starts[i] = samples(b, sr)
    return starts


@dataclass
class Entry:
    """One line of a phrase: a note (wavtool's arguments) or a rest (``rest=True``: only ``length`` counts)."""
    length: float                                  # ms
    envelope: tuple = ()                           # p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]]
    stp: float = 0.0                               # ms dropped from the note's head
    rest: bool = False

    @classmethod
    def parse(cls, text):
        """``stp length p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]]`` (a string or its tokens), or ``R length``."""
        toks = text.split() if isinstance(text, str) else list(text)
        if toks and str(toks[0]) in ("R", "r"):
            if len(toks) != 2:
                raise ValueError("a rest is `R <length>`")
            return cls(parse_length(toks[1]), rest=True)
        if len(toks) < 9:
            raise ValueError(f"wavtool arguments: stp length p1 p2 p3 v1 v2 v3 v4 [ovr [p4 [p5 v5]]] expected, got {len(toks)} values")
        return cls(parse_length(toks[1]), tuple(float(v) for v in toks[2:]), float(toks[0]))

    @property
    def overlap(self) -> float:
        return 0.0 if self.rest else envelope_overlap(self.envelope)


@dataclass
class PhrasePlan(SP.CoverPlan):
    """What goofer_phrase_mix takes for one phrase: ``notes`` (_lib.PHRASE_NOTE [n]), the cover table ``tile_off`` (int64
    [tiles + 1]) / ``tile_notes`` (int32), ``total_out``; ``blob`` holds the three back to back for one upload."""
    notes: np.ndarray
    note_len: np.ndarray
    tile_off: np.ndarray
    tile_notes: np.ndarray
    BLOB = ("notes", "tile_off", "tile_notes")                 # device_tables: these three (the records as bytes), in this order


def cover(notes: np.ndarray, note_len, total_out: int):
    """goofer_host_phrase_plan: the records checked and the cover table of the track's tiles, (tile_off, tile_notes).  Raises
    ValueError for a record the library refuses."""
    notes = np.ascontiguousarray(notes, dtype=_lib.PHRASE_NOTE)
    note_len = np.ascontiguousarray(note_len, dtype=np.int64)
    if note_len.shape != notes.shape:
        raise ValueError("one length per note")
    return SP.cover(_lib.load().goofer_host_phrase_plan, notes, (note_len.ctypes.data,), total_out, TILE,
                    lambda rc: "goofer_host_phrase_plan refused the phrase (%d): knots must be finite and non-decreasing from 0 to "
                               "take, 0 <= take <= 2^24, skip >= 0, lengths and total_out >= 0" % rc)


def plan_records(notes, note_len, total_out: int, sr: int = 0) -> PhrasePlan:
    """A PhrasePlan from finished records (any starts): checked, covered and packed."""
    notes = np.ascontiguousarray(notes, dtype=_lib.PHRASE_NOTE)
    note_len = np.ascontiguousarray(note_len, dtype=np.int64)
    total_out = int(total_out)
    tile_off, tile_notes = cover(notes, note_len, total_out)
    return PhrasePlan(len(notes), total_out, int(sr), notes, note_len, tile_off, tile_notes)


def plan_phrase(entries, note_lens, sr, starts=None, total_out=None) -> PhrasePlan:
    """The records, the cover table and the track length of a phrase, ready for one upload.  ``entries``: ``Entry`` objects
    (or what ``Entry.parse`` takes), rests included; ``note_lens``: the rendered sample counts of the notes (the entries that
    are not rests), in order; ``sr``: the batch's rate.  Notes are placed end to end with their overlaps (``place``) unless
    ``starts`` gives each note's track position in samples; ``total_out`` defaults to the largest end of any note or rest."""
    entries = [e if isinstance(e, Entry) else Entry.parse(e) for e in entries]
    idx = [i for i, e in enumerate(entries) if not e.rest]
    note_lens = np.asarray(note_lens, dtype=np.int64)
    if len(idx) != len(note_lens):
        raise ValueError(f"{len(idx)} notes among the entries, {len(note_lens)} rendered lengths")
    takes = np.array([samples(e.length, sr) for e in entries], dtype=np.int64)
    if takes.size and takes.max() > MAX_TAKE:
        raise ValueError("an entry longer than 2^24 samples")
    placed = place([e.length for e in entries], [e.overlap for e in entries], sr)
    if starts is None:
        note_starts = placed[idx]
    else:
        note_starts = np.asarray(starts, dtype=np.int64)
        if note_starts.shape != (len(idx),):
            raise ValueError("starts: one track position per note")
    if total_out is None:
        ends = placed + takes
        if starts is not None and idx:
            ends = np.concatenate([ends, note_starts + takes[idx]])
        total_out = max(0, int(ends.max())) if ends.size else 0
    notes = np.zeros(len(idx), dtype=_lib.PHRASE_NOTE)
    for k, i in enumerate(idx):
        e = entries[i]
        pos, val = envelope_knots(e.envelope, e.length, sr)
        skip = samples(e.stp, sr)
        if skip < 0:
            raise ValueError("stp must be >= 0")
        notes[k] = (note_starts[k], skip, takes[i], pos, val)
    return plan_records(notes, note_lens, total_out, sr)


def read_job(path):
    """The lines of a job file: [(resampler arguments or None for a rest, Entry)]."""
    from . import sampler as S
    out = []
    with open(path, encoding="utf-8") as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                if "|" not in line:
                    e = Entry.parse(line)
                    if not e.rest:
                        raise ValueError("a note is `<13 resampler arguments> | <wavtool arguments>`")
                    out.append((None, e))
                else:
                    left, right = line.rsplit("|", 1)
                    out.append((S.split_arguments(left.strip()), Entry.parse(right)))
            except ValueError as err:
                raise ValueError(f"{path}:{ln}: {err}") from None
    return out


def load_job(path, renderer, tracker=None):
    """The notes of a job file as ``Renderer.render_phrase`` takes them: (jobs, entries).  ``in_file`` is resolved like the
    resampler front end does: ``<stem>_features.goofy`` beside the wav, analysed and cached first when it is missing
    (``trackers.ensure_features_batch``; the tracker: the argument, else ``$GOOFER_TRACKER``)."""
    from pathlib import Path
    from . import core, trackers
    from . import sampler as S
    from .render import Source
    lines = read_job(path)
    wavs = [Path(a[0]) for a, _ in lines if a is not None]
    feats = trackers.ensure_features_batch(wavs, hop_length=renderer.hop, tracker=tracker, ctx=renderer.ctx) if wavs else {}
    sources, jobs = {}, []
    for a, _ in lines:
        if a is None:
            continue
        feat = feats[Path(a[0])]
        if isinstance(feat, BaseException):
            raise feat
        if feat not in sources:
            sources[feat] = Source.from_pack(*core.load_features(feat))
        jobs.append((sources[feat], S.decode_request(*a[2:13])))
    if not jobs:
        raise ValueError(f"{path}: no note")
    return jobs, [e for _, e in lines]


def render_job(path, out_wav, renderer=None, seed=None, tracker=None, pcm16=True, out_sr=None, limit=None, stats=None, loudness=None,
               compress=None, eq=None, reverb=None):
    """``python -m goofer_amd.phrase``: the notes of a job file rendered as one batch and written as one wav.  ``in_file`` is
    resolved like the resampler front end does: ``<stem>_features.goofy`` beside the wav, analysed and cached first when it is
    missing (``trackers.ensure_features_batch``; the tracker: the argument, else ``$GOOFER_TRACKER``).  ``out_sr``: the rate of
    the wav (``render_phrase``'s; None: the voicebank's).  ``limit``: ``render_phrase``'s (None: no limiter); with it ``stats``,
    a dict, receives the limiter's ``peak_in`` and ``min_gain`` (a true-peak limiter's ``true_peak_in`` and ``true_peak_out`` too).  ``loudness``: ``render_phrase``'s (None: the track's level is
    left as it is); with it ``stats`` receives ``lufs_in``, ``momentary_max`` and ``gain``.  ``compress``: ``render_phrase``'s (None:
    no compressor); with it ``stats`` receives ``max_reduction_db``.  ``eq``: ``render_phrase``'s (None: no equaliser); it has no
    statistic.  ``reverb``: ``render_phrase``'s (None: no reverb); with it ``stats`` receives ``reverb_taps``, the impulse
    response's length, and ``reverb_tail``, the samples it adds to the track."""
    from .render import Renderer, write_wav
    renderer = renderer or Renderer()
    jobs, entries = load_job(path, renderer, tracker)
    if seed is None:
        seed = draw_seed(np.uint64)
    if reverb is not None:
        from . import reverb as RV
        reverb = RV.parse(reverb)
        rv_plan = RV.plan(jobs[0][0].sr if out_sr is None else int(out_sr), [], reverb)
        if stats is not None:
            stats.update({"reverb_taps": rv_plan.L, "reverb_tail": rv_plan.added})
    track = rendered(renderer.render_phrase, stats, limit is not None or loudness is not None or compress is not None, jobs=jobs,
                     entries=entries, seed=seed, pcm16=pcm16, out_sr=out_sr, limit=limit, loudness=loudness, compress=compress, eq=eq,
                     reverb=reverb)
    write_wav(out_wav, track, jobs[0][0].sr if out_sr is None else int(out_sr))
    return track


# ---- what the two command lines share (this one and goofer_amd.bus) -----------------------------------------------------------

def draw_seed(dtype) -> int:
    """A seed for a render that was given none, from the system's entropy.  The width is the caller's: a phrase draws 64 bits,
    a song 32 (its tracks get seed + index)."""
    return int(np.random.SeedSequence().generate_state(1, dtype=dtype)[0])


def rendered(render, stats, with_stats, **kw):
    """``render(**kw)``: ``Renderer.render_phrase`` or ``render_song``, asked for its statistics only where a stage that has some
    is on (``with_stats``; they refuse ``return_stats`` otherwise); the statistics go into ``stats``, a dict or None."""
    if not with_stats:
        return render(**kw)
    out, st = render(return_stats=True, **kw)
    if stats is not None:
        stats.update(st)
    return out


def parse_options(argv, accepted):
    """The options in front of the two file names of a command line: ({option: value}, what is left of ``argv``).  ``accepted``:
    the options this command line takes, of ``--rate HZ``, ``--loudness LUFS``, ``--eq SPEC``, ``--compress SPEC``, ``--reverb
    SPEC``, ``--limit [DB]`` (a linear ceiling; bare: the default one) and the flag ``--true-peak``.  An option is read only
    while more than two arguments are left, and a value that does not parse ends the loop, so that more than two are left
    then: the caller's usage line."""
    import importlib
    from . import limit as LM
    stages = {"--eq": "eq", "--compress": "compress", "--reverb": "reverb"}       # parsed by their modules, loaded when asked for
    values = {"--rate": int, "--loudness": float}
    opts = {}
    while len(argv) > 2 and argv[0] in accepted:
        name = argv[0]
        if name == "--true-peak":
            opts[name], argv = True, argv[1:]
        elif name == "--limit":
            try:                        # --limit DB, or bare: the default ceiling
                opts[name] = 10.0 ** (float(argv[1]) / 20.0)
                argv = argv[2:]
            except ValueError:
                opts[name], argv = LM.CEILING, argv[1:]
        else:
            parse = values.get(name) or importlib.import_module("." + stages[name], __package__).parse
            try:
                opts[name] = parse(argv[1])
            except ValueError:
                break
            argv = argv[2:]
    return opts, argv


def report_levels(stats, loudness, limit, true_peak):
    """The lines of the loudness stage and the limiter on stderr, from a render's statistics.  (A peak of 0 prints as -inf
    dBFS: ``limit.dbtp``, which is what both command lines spelt out.)"""
    from . import limit as LM
    if loudness is not None:
        print("Loudness: measured %.2f LUFS (momentary max %.2f), gain %.2f dB (target %.2f LUFS)"
              % (stats["lufs_in"], stats["momentary_max"], LM.dbtp(stats["gain"]), loudness), file=sys.stderr)
    if true_peak:
        print("Limiter: input true peak %.2f dBTP, output true peak %.2f dBTP, greatest reduction %.2f dB (ceiling %.2f dBTP)"
              % (LM.dbtp(stats["true_peak_in"]), LM.dbtp(stats["true_peak_out"]), LM.reduction_db(stats["min_gain"]), LM.dbtp(limit)),
              file=sys.stderr)
    elif limit is not None:
        print("Limiter: input peak %.2f dBFS, greatest reduction %.2f dB (ceiling %.2f dBFS)"
              % (LM.dbtp(stats["peak_in"]), LM.reduction_db(stats["min_gain"]), LM.dbtp(limit)), file=sys.stderr)


def main(argv=None) -> int:
    import logging
    from . import eq as EQ
    from . import limit as LM
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    opts, argv = parse_options(list(sys.argv[1:] if argv is None else argv),
                               ("--rate", "--limit", "--loudness", "--compress", "--true-peak", "--eq", "--reverb"))
    out_sr, limit, loudness, compress, eq, reverb = (opts.get(k) for k in ("--rate", "--limit", "--loudness", "--compress", "--eq", "--reverb"))
    true_peak = "--true-peak" in opts
    if len(argv) != 2 or (true_peak and limit is None):
        logging.error("Usage:\n  python -m goofer_amd.phrase [--rate HZ] [--eq KIND:F0[:GAIN_DB[:Q]],...] [--compress T:R[:ATTACK:RELEASE[:KNEE[:MAKEUP]]]] "
                      "[--reverb room:RT60_S[:WET_DB[:PREDELAY_MS[:SEED]]] | ir:PATH[:WET_DB[:PREDELAY_MS]]] [--loudness LUFS] "
                      "[--limit [DBFS] [--true-peak]] job.txt out.wav")
        return 1
    stats = {}
    try:
        track = render_job(argv[0], argv[1], out_sr=out_sr, limit=LM.Limiter(limit, true_peak=True) if true_peak else limit, stats=stats,
                           loudness=loudness, compress=compress, eq=eq, reverb=reverb)
    except Exception:                   # noqa: BLE001
        logging.exception("Failed to render")
        return 1
    if eq is not None:
        print("Equaliser: %s" % ", ".join("%s %g Hz%s q %.3g" % (b.kind, b.f0_hz, " %+g dB" % b.gain_db if b.kind in EQ.GAINED else "", b.q)
                                          for b in eq), file=sys.stderr)
    if compress is not None:
        print("Compressor: greatest reduction %.2f dB (threshold %.2f dBFS, ratio %g, attack %g ms, release %g ms, knee %g dB, make-up %g dB)"
              % (stats["max_reduction_db"], compress.threshold_db, compress.ratio, compress.attack_ms, compress.release_ms, compress.knee_db,
                 compress.makeup_db), file=sys.stderr)
    if reverb is not None:
        print("Reverb: impulse response of %d taps, wet %g dB, dry %g dB, pre-delay %g ms; the tail adds %d samples"
              % (stats["reverb_taps"], reverb.wet_db, reverb.dry_db, reverb.predelay_ms, stats["reverb_tail"]), file=sys.stderr)
    report_levels(stats, loudness, limit, true_peak)
    logging.info(f"Writing {argv[1]}: {len(track)} samples")
    return 0


if __name__ == "__main__":
    sys.exit(main())
