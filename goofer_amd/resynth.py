"""Wav-to-wav resynthesis from the command line: GOOFER.py's script mode (GOOFER.py:1222-1330) batched over many files.

    python -m goofer_amd.resynth [--out DIR] [--n-fft 1024] [--hop N] [--tracker native|native:key=value,...|praat|module:fn]
           [--pitch R] [--formant R] [--stretch R] [--F1 R ... --F4 R] [--set key=value ...]
           [--variant "key=value,key=value" ...] [--stems] [--seed S] [--noise-seed N] INPUT...

Each INPUT is an audio file or a folder, scanned like folder mode (every audio file below it; files this command wrote
itself, ``*_reconstruct.wav`` and the stems, are left out).  Files are read with ``trackers.read_audio`` (channels averaged),
grouped by sample rate and rendered by ``core.resynthesize_batch``: analysis and every variant's synthesis in batched device
passes.  For ``<stem>.wav`` it writes ``<stem>_reconstruct.wav`` and with ``--stems`` also ``_harmonic.wav``,
``_breathiness.wav`` (aper_bre) and ``_unvoiced.wav`` (aper_uv), the reference's names, as PCM16 (``render.write_wav``);
with several variants ``_v<k>`` (k from 0) goes before the suffix.  Outputs go next to each input, or under ``--out`` (a
folder input's layout below it is kept).

``--set key=value`` takes any ``synthesize`` keyword, the value a Python literal (a bare word is a string); ``--variant``
takes a comma-separated list of them, one synthesis per ``--variant`` from one analysis.  An unknown keyword exits with
status 2 before anything is read.  ``--seed S`` seeds the legacy ``np.random`` stream (the jitter draws) and gives
variant v of the k-th file (in input order) the Philox key S + k * variants + v.  ``--noise-seed N`` (an integer in
[0, 2**32)) renders every variant of every file as a reference process does that calls ``np.random.seed(N)`` just before its
``synthesize``: the jitter and roughness draws are then made on the device (``resynthesize_batch(noise_seeds=)``) and the
``np.random`` stream is not used for them.  A file that fails is logged and skipped;
the exit status is 1 if any file failed, else 0.
"""
from __future__ import annotations

import argparse
import ast
import logging
import re
import sys
from pathlib import Path

STEM_NAMES = (("reconstruct", 0), ("harmonic", 1), ("breathiness", 3), ("unvoiced", 2))   # suffix, index in the 4-tuple
_OWN_OUTPUT = re.compile(r"_(?:v\d+_)?(?:reconstruct|harmonic|breathiness|unvoiced)$")
_SHORTCUTS = (("pitch", "pitch_shift"), ("formant", "formant_shift"), ("stretch", "stretch_factor"), ("F1", "F1_shift"),
              ("F2", "F2_shift"), ("F3", "F3_shift"), ("F4", "F4_shift"))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m goofer_amd.resynth", description="Analyse wavs and resynthesise them on the GPU "
                                 "(the reference's extract_features -> synthesize flow, batched).")
    ap.add_argument("inputs", nargs="+", metavar="INPUT", help="audio files or folders")
    ap.add_argument("--out", default=None, help="output folder (default: next to each input)")
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=None, help="hop length (default n_fft // 4)")
    ap.add_argument("--tracker", default=None, help="native, native:key=value,... (trackers.TrackerSettings, e.g. native:pitch_floor=40,max_formant=5000), praat or "
                                                    "module:function (default: $GOOFER_TRACKER, else Praat)")
    for flag, key in _SHORTCUTS:
        ap.add_argument(f"--{flag}", type=float, default=None, dest=key, help=f"synthesize's {key}")
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="any synthesize keyword (repeatable)")
    ap.add_argument("--variant", action="append", default=[], metavar="K=V,K=V", help="one synthesis per --variant")
    ap.add_argument("--stems", action="store_true", help="also write the harmonic, breathiness and unvoiced stems")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--noise-seed", type=int, default=None, metavar="N",
                    help="np.random.seed(N) before every synthesize: its jitter and roughness draws, made on the device")
    return ap


def _literal(text: str):
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        return text


def parse_assignment(text: str) -> tuple:
    key, sep, value = text.partition("=")
    if not sep or not key.strip():
        raise ValueError(f"expected key=value, got {text!r}")
    return key.strip(), _literal(value.strip())


def parse_variant(text: str) -> dict:
    """``"a=1,b=[1, 2],c=x"`` -> {"a": 1, "b": [1, 2], "c": "x"}: commas inside brackets or quotes do not split."""
    try:
        call = ast.parse(f"f({text})", mode="eval").body
    except SyntaxError as e:
        raise ValueError(f"cannot parse variant {text!r}") from e
    if not isinstance(call, ast.Call) or call.args:
        raise ValueError(f"a variant is key=value pairs, got {text!r}")
    out = {}
    for kw in call.keywords:
        if kw.arg is None:
            raise ValueError(f"a variant is key=value pairs, got {text!r}")
        try:
            out[kw.arg] = ast.literal_eval(kw.value)
        except ValueError:
            out[kw.arg] = ast.get_source_segment(f"f({text})", kw.value)
    return out


def settings(args, error) -> tuple:
    """(synthesize keywords, variants or None) of parsed ``args``; ``error(message)`` for anything that is not a synthesize
    keyword (argparse's: exits with status 2)."""
    from .core import _synth_defaults
    known = _synth_defaults()
    kw = {key: getattr(args, key) for _, key in _SHORTCUTS if getattr(args, key) is not None}
    try:
        kw.update(parse_assignment(s) for s in args.set)
        variants = [parse_variant(v) for v in args.variant] or None
    except ValueError as e:
        error(str(e))
    for name in list(kw) + [k for v in variants or () for k in v]:
        if name not in known:
            error(f"unknown synthesize keyword {name!r}")
    return kw, variants


def collect_inputs(inputs) -> list:
    """[(audio file, folder it was found under or None)] in input order, each file once."""
    from .trackers import AUDIO_SUFFIXES
    out, seen = [], set()
    for item in inputs:
        p = Path(item)
        if p.is_dir():
            found = [(f, p) for f in sorted(p.rglob("*")) if f.is_file() and f.suffix.lower() in AUDIO_SUFFIXES
                     and not _OWN_OUTPUT.search(f.stem)]
        else:
            found = [(p, None)]
        for f, root in found:
            if f not in seen:
                seen.add(f)
                out.append((f, root))
    return out


def output_paths(src, root=None, out_dir=None, n_variants=None, stems=False) -> list:
    """Per variant (one entry when ``n_variants`` is None) {suffix: output path} for the input ``src`` found under ``root``."""
    src = Path(src)
    folder = src.parent if out_dir is None else Path(out_dir) / (src.parent.relative_to(root) if root is not None else Path())
    names = [n for n, _ in STEM_NAMES] if stems else ["reconstruct"]
    tags = [""] if n_variants is None else [f"_v{k}" for k in range(n_variants)]
    return [{n: folder / f"{src.stem}{tag}_{n}.wav" for n in names} for tag in tags]


def main(argv=None) -> int:
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    ap = build_parser()
    args = ap.parse_args(argv)
    kw, variants = settings(args, ap.error)
    hop = args.hop if args.hop is not None else args.n_fft // 4
    if args.n_fft < 2 or hop < 1:
        ap.error(f"n_fft {args.n_fft} and hop {hop} must be positive")
    if args.noise_seed is not None and not 0 <= args.noise_seed < 2 ** 32:
        ap.error(f"--noise-seed must be an integer in [0, 2**32), got {args.noise_seed}")

    import numpy as np
    from . import core, trackers
    from .render import write_wav
    files = collect_inputs(args.inputs)
    if not files:
        logging.error("no audio files found")
        return 1
    if args.seed is not None:
        np.random.seed(args.seed)
    n_var = 1 if variants is None else len(variants)
    failed = 0
    groups = {}
    for k, (f, root) in enumerate(files):
        try:
            y, sr = trackers.read_audio(f)
        except Exception as e:                                    # noqa: BLE001 - reported per file
            logging.error(f"[ERROR] {f}: {e}")
            failed += 1
            continue
        groups.setdefault(sr, []).append((k, f, root, y))
    for sr, members in groups.items():
        seeds = None
        if args.seed is not None:
            seeds = [args.seed + k * n_var + v for k, *_ in members for v in range(n_var)]
        try:
            res = core.resynthesize_batch([m[3] for m in members], sr, args.n_fft, hop, pitch_tracker=args.tracker, variants=variants,
                                          seeds=seeds, noise_seeds=None if args.noise_seed is None else [args.noise_seed] * len(members),
                                          **kw)
        except Exception as e:                                    # noqa: BLE001 - the group could not run: each of its files failed
            res = [e] * len(members)
        for (k, f, root, _), r in zip(members, res):
            outs = r if isinstance(r, BaseException) or variants is not None else [r]
            err = outs if isinstance(outs, BaseException) else next((o for o in outs if isinstance(o, BaseException)), None)
            if err is not None:
                logging.error(f"[ERROR] {f}: {err}")
                failed += 1
                continue
            try:
                for stems, paths in zip(outs, output_paths(f, root, args.out, None if variants is None else n_var, args.stems)):
                    for name, idx in STEM_NAMES:
                        if name in paths:
                            paths[name].parent.mkdir(parents=True, exist_ok=True)
                            write_wav(paths[name], stems[idx], sr)
                logging.info(f"[DONE] {f}")
            except Exception as e:                                # noqa: BLE001
                logging.error(f"[ERROR] {f}: {e}")
                failed += 1
    logging.info(f"[DONE] {len(files) - failed} of {len(files)} files resynthesised")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
