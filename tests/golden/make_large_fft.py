"""Fixture for n_fft above 2048 (large_fft.npz): gf.stft / gf.istft at the workgroup-transform sizes and a few short
gf.synthesize renders, from the reference itself under make_golden.py's stubs (imported, not edited).

    python tests/golden/make_large_fft.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stubs, imports the reference as mg.gf)

gf, syn = mg.gf, mg.syn

# (tag, samples, n_fft, hop): 4096 natively, the other sizes through Bluestein at L = 4096 (2052: the smallest, 2050 stays
# refused); "e" is shorter than one frame
# (small enough to keep the file under 1 MiB: the spectra do not compress)
STFT_CASES = [("a", 5000, 4096, 1024), ("b", 700, 4096, 96), ("c", 8000, 3000, 750), ("d", 5000, 2052, 512),
              ("e", 1500, 4094, 1023)]

# (name, keywords, sr, n_fft, hop, seconds)
SYNTH_CASES = [("sr96_4096", dict(), 96000, 4096, 1024, 0.08),
               ("sr96_4096_fshift", dict(formant_shift=0.8, F1_shift=1.2, F2_shift=0.9), 96000, 4096, 1024, 0.06),
               ("sr44_3000", dict(), 44100, 3000, 750, 0.12)]


def gen_stft_istft(out):
    r = np.random.default_rng(4096)
    for tag, n, n_fft, hop in STFT_CASES:
        x = r.standard_normal(n).astype(np.float32)
        win = gf.get_cached_window(44100, n_fft)
        S = gf.stft(x, n_fft=n_fft, hop_length=hop, window=win)
        y = gf.istft(S, hop_length=hop, window=win, length=n)
        out.update({f"x_{tag}": x, f"S_{tag}": S.astype(np.complex64), f"y_{tag}": y, f"geo_{tag}": np.array([n_fft, hop])})
    out["cases"] = np.array([c[0] for c in STFT_CASES])


def gen_synthesize(out):
    """make_golden.gen_synthesize's pattern: the reference's random phases come from default_rng(seed), which the tests
    reproduce as the injected phi."""
    out["names"] = np.array([c[0] for c in SYNTH_CASES])
    for idx, (name, kw, sr, n_fft, hop, secs) in enumerate(SYNTH_CASES):
        src = syn.make_source(900 + idx, sr, n_fft, hop, seconds=secs)
        env = gf.decode_env_from_knots(src["env_pack"])
        n = src["y_len"]
        t = np.arange(n) / sr
        mask = src["mask"].copy()
        f0 = ((196.0 * 2 ** (0.3 * np.sin(2 * np.pi * 3.1 * t))) * mask).astype(np.float32)   # (stored as given: fp32 values)
        seed = 9000 + idx
        mg._RNG_SEED[0] = seed
        rec, harm, uv, bre = gf.synthesize(env, f0.astype(np.float64), mask, np.empty(n, bool), sr,
                                           n_fft=n_fft, hop_length=hop, formants=src["formants"], **kw)
        mg._RNG_SEED[0] = None
        out[f"{name}_env"] = env
        out[f"{name}_f0"] = f0
        out[f"{name}_mask"] = mask
        out[f"{name}_formants"] = np.stack([src["formants"][i] for i in (1, 2, 3, 4)], 0)
        out[f"{name}_geo"] = np.array([sr, n_fft, hop, seed])
        out[f"{name}_kw_keys"] = np.array(list(kw.keys()) or ["_"])
        out[f"{name}_kw_vals"] = np.array([float(v) for v in kw.values()] or [0.0])
        out[f"{name}_rec"], out[f"{name}_harm"], out[f"{name}_uv"], out[f"{name}_bre"] = rec, harm, uv, bre


if __name__ == "__main__":
    out = {}
    gen_stft_istft(out)
    gen_synthesize(out)
    mg.save("large_fft", **out)
