"""CPU: the analysis restatement (analysis_ref.py) against the oracle and the reference's golden data, the candidate knot tables
the batched kernel scores, and the oracle margins of the signals test_gpu_analysis_oracle.py builds to sit on the K search's
edges: so that a failure there names the kernel, not the test's assumptions."""
import numpy as np
import pytest

import analysis_ref as A
from conftest import golden
from oracle import goofer_ref as R

from goofer_amd import core

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000)
SIZES = (64, 512, 768, 1000, 1024, 2048)
SKIP_T = (295, 310, 343)              # frame counts where numpy's floor skips a frame an exact integer linspace probes
LONG = ((16000, 64, 16), 65575)       # one signal above 65 536 frames


def _oracle_K(env, sr, n_fft):
    return len(R.compress_env_to_knots(env, sr=sr, n_fft=n_fft)["hz_knots"])


def test_candidate_errors_reproduce_golden_choices():
    """The reference chose K = len(hz_knots) for these envelopes; candidate_errors and the oracle agree with it."""
    g, cc = golden("knots"), golden("cold_cache")
    for env, hz in ((g["an_env"], g["an_hz_knots"]), (g["sm_env"], g["sm_hz_knots"]), (cc["env_spec"], cc["hz_knots"])):
        errs = A.candidate_errors(env, 44100, 1024)
        assert errs.shape == (len(A.CANDIDATES),) and np.all(np.isfinite(errs))
        assert A.decide(errs)[0] == len(hz) == _oracle_K(env, 44100, 1024)
        assert np.array_equal(A.candidate_bins(44100, 1024, len(hz))[0], hz)


@pytest.mark.parametrize("geom", A.GEOMETRIES[:4] + A.GEOMETRIES[6:7], ids=lambda g: "%d-%d-%d" % g)
def test_candidate_errors_pick_the_oracles_K(geom):
    sr, n_fft, hop = geom
    for kind, y in A.signal_set(sr, n_fft, hop)[::3]:
        env, pack = R.envelope_of(y, sr, n_fft, hop)
        assert A.decide(A.candidate_errors(env, sr, n_fft))[0] == len(pack["hz_knots"]), (kind, len(y))


@pytest.mark.parametrize("n_fft", SIZES)
def test_knot_candidate_tables_are_the_oracles(n_fft):
    """core.knot_candidate_tables (what goofer_envelope_knots_batch scores) = mel_knots + nearest-bin rounding, back to back."""
    for sr in RATES:
        hz, bins = core.knot_candidate_tables(sr, n_fft)
        assert hz.dtype == np.float32 and bins.dtype == np.int32
        assert hz.size == bins.size == sum(A.CANDIDATES) == 1232
        o = 0
        for K in A.CANDIDATES:
            want_hz, want_bins = A.candidate_bins(sr, n_fft, K)
            assert np.array_equal(hz[o:o + K], want_hz), (sr, n_fft, K)
            assert np.array_equal(bins[o:o + K], want_bins), (sr, n_fft, K)
            assert bins[o:o + K].min() >= 0 and bins[o:o + K].max() <= n_fft // 2
            o += K


def test_probe_rows_floor_skips():
    for T in (1, 2, 3, 255, 256, 257, 513, 65575):
        p = A.probe_rows(T)
        assert p.size == min(256, T) and p[0] == 0 and p[-1] == T - 1 and np.all(np.diff(p) >= 1)
        assert np.array_equal(p, np.linspace(0, T - 1, min(256, T), dtype=int))
    p = set(A.probe_rows(295).tolist())
    assert 97 in p and 99 in p and 98 not in p and A.skipped_probes(295) == [98, 196]
    for T in SKIP_T + (LONG[1],):
        assert A.skipped_probes(T), T
    assert A.skipped_probes(256) == [] and A.skipped_probes(257) == []


@pytest.mark.parametrize("c", (0, 1, 2))
def test_boundary_signals_sit_on_eps(c):
    """The resonator clicks of test_gpu_analysis_oracle (d): the deciding candidate's oracle error is eps (1 -+ 1e-2) and
    the oracle's K steps from candidate c to c + 1 across it, with every other deciding error well clear of eps."""
    sr, n_fft, hop = A.BOUNDARY_GEOM
    for cc, side, y, errs in A.boundary_signals((c,)):
        assert abs(errs[c] / (A.EPS * (1 + side * 1e-2)) - 1) < 1e-4, errs
        env, pack = R.envelope_of(y, sr, n_fft, hop)
        assert np.array_equal(errs, A.candidate_errors(env, sr, n_fft))
        want = A.CANDIDATES[c] if side < 0 else A.CANDIDATES[c + 1]
        assert A.decide(errs)[0] == len(pack["hz_knots"]) == want
        assert 0.99e-2 < A.margin(errs) < 1.01e-2
        others = np.delete(A.deciding(errs), c)
        assert np.all(np.abs(others / A.EPS - 1) > 5e-2), errs


@pytest.mark.parametrize("case", [((44100, 512, 512), T) for T in SKIP_T] + [LONG], ids=lambda c: "T%d" % c[1])
def test_probe_skip_signals(case):
    """A burst seen only by frames the probe set skips leaves the oracle at K = 32; in the probed neighbour it raises K."""
    (sr, n_fft, hop), T = case
    f = A.skipped_probes(T)[0]
    probes = set(A.probe_rows(T).tolist())
    n = (T - 1) * hop
    for frame, rises in ((f, False), (f - 1, True)):
        start, m = A.own_samples(frame, n_fft, hop)
        seen = {t for t in range(T) if t * hop - n_fft // 2 < start + m and start < t * hop + n_fft // 2}
        assert (frame in probes) == rises and bool(seen & probes) == rises, (frame, sorted(seen))
        env, pack = R.envelope_of(A.with_burst(n, start, m, sr, seed=frame), sr, n_fft, hop)
        assert env.shape[1] == T
        K = len(pack["hz_knots"])
        assert (K > 32) == rises and A.decide(A.candidate_errors(env, sr, n_fft))[0] == K


def test_nan_sample_makes_the_oracle_fall_back():
    """What test_gpu_analysis_oracle (f) expects of the kernels: numpy's max and maximum propagate NaN, so one NaN sample in
    silence rejects every candidate (K = 192) and leaves NaN knots in the frames that see it."""
    sr, n_fft, hop = 44100, 1024, 256
    y = np.zeros(4000, dtype=np.float32)
    y[2000] = np.nan
    with np.errstate(invalid="ignore"):
        env, pack = R.envelope_of(y, sr, n_fft, hop)
    errs = A.candidate_errors(env, sr, n_fft)
    assert np.all(np.isnan(errs)) and len(pack["hz_knots"]) == 192
    bad = ~np.isfinite(pack["knot_vals_log"].astype(np.float32))
    frames = np.flatnonzero(bad.any(axis=0))
    assert np.array_equal(frames, np.flatnonzero(np.isnan(env).any(axis=0))) and 0 < frames.size < env.shape[1]
    assert np.all(bad[:, frames]) and np.all(np.isnan(pack["knot_vals_log"][:, frames]))


def test_truth_envelope_bounds_the_oracle():
    """The fp64 yardstick agrees with the oracle's fp32 STFT to fp32 rounding, frame by frame."""
    for sr, n_fft, hop in A.GEOMETRIES[1::2]:
        for kind, y in A.signal_set(sr, n_fft, hop)[-6:]:
            env, _ = R.envelope_of(y, sr, n_fft, hop)
            truth = A.truth_envelope(y, sr, n_fft, hop)
            assert truth.shape == env.shape
            assert A.frame_error(env, truth).max() < 1e-5, (sr, n_fft, kind)


def test_dip_kinds_defeat_the_element_bound():
    """Why test_gpu_analysis_oracle (a) bounds DIP_KINDS per frame: numpy's own envelope is further than the golden
    per-element bound (rtol 2e-6, atol 1e-9) from the fp64 truth in their dips; silence and dither stay well inside it."""
    sr, n_fft, hop = 22050, 512, 128
    worst = {}
    for kind, y in A.signal_set(sr, n_fft, hop):
        env, _ = R.envelope_of(y, sr, n_fft, hop)
        truth = A.truth_envelope(y, sr, n_fft, hop)
        worst[kind] = max(worst.get(kind, 0.0), np.max(np.abs(env - truth) / (1e-9 + 2e-6 * np.abs(truth))))
    for kind, w in worst.items():
        assert (w > 1.0 if kind in A.DIP_KINDS else w < 0.25), (kind, w)
