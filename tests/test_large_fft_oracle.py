"""The oracle at n_fft above 2048 against the reference's own stft / istft / synthesize (golden/large_fft.npz, written by
golden/make_large_fft.py): the CPU side of tests/test_gpu_large_fft.py."""
import numpy as np
import pytest

from conftest import golden, rel_rms, rms_err
from oracle import goofer_ref as R


def _synth_case(g, name):
    sr, n_fft, hop, seed = (int(v) for v in g[f"{name}_geo"])
    kw = {k: float(v) for k, v in zip(g[f"{name}_kw_keys"], g[f"{name}_kw_vals"]) if k != "_"}
    env = g[f"{name}_env"]
    f0 = g[f"{name}_f0"].astype(np.float64)
    n = len(f0)
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=(env.shape[0], 1 + n // hop)).astype(np.float32)
    F = g[f"{name}_formants"]
    return dict(env=env, f0=f0, mask=g[f"{name}_mask"], n=n, sr=sr, n_fft=n_fft, hop=hop, phi=phi,
                formants={i + 1: F[i] for i in range(4)}, kw=kw)


def test_fixture_covers_the_new_sizes():
    g = golden("large_fft")
    sizes = {int(g[f"geo_{t}"][0]) for t in g["cases"]}
    assert {4096, 3000, 2052, 4094} <= sizes
    assert any(len(g[f"x_{t}"]) < int(g[f"geo_{t}"][0]) for t in g["cases"])       # a signal shorter than one frame
    assert {int(g[f"{nm}_geo"][1]) for nm in g["names"]} == {4096, 3000}


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e"])
def test_oracle_stft_istft_at_large_n_fft(tag):
    g = golden("large_fft")
    n_fft, hop = (int(v) for v in g[f"geo_{tag}"])
    x = g[f"x_{tag}"]
    win = R.sqrt_hann(n_fft)
    S = R.stft(x, n_fft, hop, win)
    assert S.shape == g[f"S_{tag}"].shape == (n_fft // 2 + 1, 1 + len(x) // hop)
    assert rel_rms(S, g[f"S_{tag}"]) < 1e-7, (tag, rel_rms(S, g[f"S_{tag}"]))
    y = R.istft(g[f"S_{tag}"], hop, win, len(x))
    assert rms_err(y, g[f"y_{tag}"]) < 1e-7 * max(1.0, float(np.abs(g[f"y_{tag}"]).max())), tag


def test_oracle_synthesize_at_large_n_fft():
    g = golden("large_fft")
    for name in g["names"]:
        c = _synth_case(g, name)
        outs = R.synthesize(c["env"], c["f0"], c["mask"], np.empty(c["n"], bool), c["sr"], n_fft=c["n_fft"], hop_length=c["hop"],
                            formants=c["formants"], phi=c["phi"], **c["kw"])
        for got, key in zip(outs, ("rec", "harm", "uv", "bre")):
            ref = g[f"{name}_{key}"]
            assert got.shape == ref.shape, (name, key)
            e = rms_err(got, ref) / max(1.0, float(np.max(np.abs(ref))))
            assert e < 1e-5, (name, key, e)
