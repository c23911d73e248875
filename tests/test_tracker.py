"""CPU: the native f0 / formant tracker's registration, frame layout and input checks, and its algorithm (the numpy
restatement in tracker_ref.py) against ground-truth signals (tracker_truth.py)."""
import numpy as np
import pytest

import tracker_ref as R
import tracker_truth as T

from goofer_amd import trackers

RATES = (22050, 44100, 48000, 96000)
HOP = 256


def test_native_is_registered_and_selectable(monkeypatch):
    assert trackers.get("native") is trackers.native_tracker
    monkeypatch.setenv("GOOFER_TRACKER", "native")
    assert trackers.get() is trackers.native_tracker


def test_native_is_not_the_default(monkeypatch):
    monkeypatch.delenv("GOOFER_TRACKER", raising=False)
    try:
        import parselmouth  # noqa: F401
    except ImportError:
        with pytest.raises(trackers.TrackerUnavailable):
            trackers.get()


@pytest.mark.parametrize("sr", RATES)
def test_frame_layout(sr):
    """floor((dur - 40 ms) / dt) + 1 pitch frames and floor((dur' - 50 ms) / dt) + 1 formant frames, from the library's own
    geometry, the restatement's and the plain float formula."""
    from goofer_amd.device import track_frame_offsets
    win = R.min_length(sr)
    lengths = [win, win + 1, win + HOP - 1, win + HOP, sr, 3 * sr + 17, 6000 * sr // 11000, 6000 * sr // 11000 - 1]
    p_off, f_off = track_frame_offsets(lengths, sr, HOP)
    dt = HOP / sr
    for k, n in enumerate(lengths):
        np_ = int(np.floor((n / sr - 0.04) / dt + 1e-9)) + 1
        assert p_off[k + 1] - p_off[k] == R.pitch_frames(n, sr, HOP) == np_, (n, np_)
        m = n * 11000 // sr
        nf = 0 if m < 550 else int(np.floor((m / 11000 - 0.05) / dt + 1e-9)) + 1
        assert f_off[k + 1] - f_off[k] == R.formant_frames(n, sr, HOP) == nf, (n, nf)
    starts = R.pitch_starts(sr, sr, HOP)                       # centred: equal margins to within a sample
    head, tail = starts[0], sr - (starts[-1] + R.pitch_window(sr))
    assert abs(head - tail) <= 1


def test_short_signal_is_refused_with_the_minimum_length():
    sr = 44100
    n = R.min_length(sr)
    with pytest.raises(ValueError, match=str(n)):
        trackers.native_tracker(np.zeros(n - 1), sr, HOP, 10)
    with pytest.raises(ValueError, match=str(n)):
        R.track_pitch(np.zeros(n - 1), sr, HOP)
    from goofer_amd.device import GooferError, track_frame_offsets
    with pytest.raises(GooferError):
        track_frame_offsets([n - 1], sr, HOP)
    assert track_frame_offsets([n], sr, HOP)[0][-1] == 1


@pytest.mark.parametrize("sr", RATES)
def test_restatement_meets_ground_truth(sr):
    y, f0, kind = T.synth(sr)
    s = T.score(R.track_pitch(y, sr, HOP), R.track_formants(y, sr, HOP), f0, kind, sr, HOP)
    T.assert_meets_bars(s)


def test_restatement_edge_cases():
    sr = 22050
    n = R.min_length(sr)
    t = np.arange(sr // 2) / sr
    cases = {
        "zeros": np.zeros(sr // 2),
        "dc": np.full(sr // 2, 0.3),
        "square": np.clip(4.0 * np.sign(np.sin(2 * np.pi * 150 * t)), -1, 1),
        "one_window": T.synth(sr)[0][sr // 4:sr // 4 + n],
    }
    for name, y in cases.items():
        f0, forms = R.track(y, sr, HOP)
        assert np.isfinite(f0).all() and np.isfinite(forms).all(), name
        if name in ("zeros", "dc"):
            assert not f0.any(), name
    assert not R.track_formants(cases["zeros"], sr, HOP).any()
    f0, _ = R.track(cases["square"], sr, HOP)
    assert np.all(np.abs(f0[2:-2] / 150.0 - 1.0) < 0.01)


# -- the restatement's diagnostics (tracker_ref.*_diag), which the GPU oracle tests rely on ---------------------------
def test_candidate_flags_near_thresholds_and_not_far_from_them():
    sr, hop = 22050, 256
    y, _, _ = T.synth(sr)
    cands, fragile, peaks = R.pitch_candidates(y, sr, hop)
    assert not fragile.any() and all(np.array_equal(c[0], d[0]) for c, d in zip(cands, [R.frame_candidates(
        y[s:s + R.pitch_window(sr)], R.hann(R.pitch_window(sr)), _rw(sr), sr, np.abs(y - y.mean()).max()) for s in
        R.pitch_starts(len(y), sr, hop)]))
    W = R.pitch_window(sr)
    w, rw = R.hann(W), _rw(sr)
    x = y[sr // 8:sr // 8 + W]
    gp = np.abs(y - y.mean()).max()
    assert not R.frame_candidates_diag(x, w, rw, sr, gp)[2]
    # a constant frame: rounding residue after the mean is removed
    assert R.frame_candidates_diag(np.full(W, 0.3), w, rw, sr, 0.3)[2]
    assert not R.frame_candidates_diag(np.zeros(W), w, rw, sr, 0.0)[2]
    # the signal's peak at the silence level
    assert R.frame_candidates_diag(x, w, rw, sr, R.SILENT_PEAK * (1 + 1e-12))[2]
    # a peak's frequency against the floor or the ceiling: flagged once eps reaches the distance
    fq, _, fr, _ = R.frame_candidates_diag(np.sin(2 * np.pi * 400.0 * np.arange(W) / sr), w, rw, sr, 1.0)
    reach = min(abs(fq[1] / R.FLOOR - 1.0), abs(fq[1] / R.CEILING - 1.0))
    assert not fr and 0.0 < reach < 1.0
    assert R.frame_candidates_diag(np.sin(2 * np.pi * 400.0 * np.arange(W) / sr), w, rw, sr, 1.0, eps=reach * 1.01)[2]


def _rw(sr):
    W = R.pitch_window(sr)
    w = R.hann(W)
    return np.correlate(w, w, mode="full")[W - 1:] / np.dot(w, w)


def test_candidate_pruning_runs_and_flags_a_tie_at_the_14th():
    sr = 22050
    W = R.pitch_window(sr)
    x = np.sin(2 * np.pi * 2000.0 * np.arange(W) / sr)
    f, s, fragile, peaks = R.frame_candidates_diag(x, R.hann(W), _rw(sr), sr, 1.0)
    assert peaks > R.MAX_CAND - 1 and len(f) == R.MAX_CAND and not fragile
    # the 14th against the 15th strongest: flagged once eps reaches their gap
    assert R.frame_candidates_diag(x, R.hann(W), _rw(sr), sr, 1.0, eps=1.0)[2]


def test_viterbi_flags_exact_and_near_ties_only():
    tsc = 0.01 * 22050 / 256
    a = lambda *v: np.array(v, np.float64)                                     # noqa: E731
    tie = [(a(0.0, 100.0, 400.0), a(0.1, 0.9, 0.9)), (a(0.0, 200.0), a(0.1, 0.9)), (a(0.0, 200.0), a(0.1, 0.9))]
    f0, gap, fragile = R.viterbi_diag(tie, tsc)
    assert np.array_equal(f0, [100.0, 200.0, 200.0]) and np.array_equal(f0, R.viterbi(tie, tsc))
    assert gap[1] == 0.0 and fragile[0] and not fragile[1:].any()
    near = [(a(0.0, 100.0, 400.0), a(0.1, 0.9, 0.9 + 1e-12)), (a(0.0, 200.0), a(0.1, 0.9))]
    f0, gap, fragile = R.viterbi_diag(near, tsc)
    assert np.array_equal(f0, [400.0, 200.0]) and 0 < gap[1] < 1e-11 and fragile[0] and not fragile[1]
    final = [(a(0.0, 300.0), a(0.1, 0.9)), (a(0.0, 150.0, 600.0), a(0.1, 0.9, 0.9))]
    f0, gap, fragile = R.viterbi_diag(final, tsc)
    assert np.array_equal(f0, [300.0, 150.0]) and gap[0] == 0.0 and fragile.all()
    far = [(a(0.0, 100.0, 400.0), a(0.1, 0.9, 0.5)), (a(0.0, 200.0), a(0.1, 0.9))]
    assert not R.viterbi_diag(far, tsc)[2].any()
    sr, hop = 44100, 256
    y, _, _ = T.synth(sr)
    cands, _, _ = R.pitch_candidates(y, sr, hop)
    f0, gap, fragile = R.viterbi_diag(cands, 0.01 * sr / hop)
    assert np.array_equal(f0, R.track_pitch(y, sr, hop)) and not fragile.any()


def _ar_frame(poles, n=R.FORMANT_WIN, seed=0):
    rng = np.random.default_rng(seed)
    a = np.array([1.0])
    for f, r in poles:
        a = np.convolve(a, [1.0, -2 * r * np.cos(2 * np.pi * f / R.FORMANT_SR), r * r])
    e = rng.standard_normal(n + 400)
    yv = np.zeros(len(e))
    for t in range(len(e)):
        yv[t] = e[t] - sum(a[k] * yv[t - k] for k in range(1, len(a)) if t - k >= 0)
    return yv[400:] * R.gauss_window(n)


def test_formant_flags_boundary_roots_and_not_clear_frames():
    clear = _ar_frame([(700.0, 0.97), (1220.0, 0.96), (2600.0, 0.95), (3500.0, 0.94), (4500.0, 0.93)])
    f, fragile = R.frame_formants_diag(clear)
    assert not fragile and np.array_equal(f, R.frame_formants(clear))
    assert np.all(np.abs(f[:3] / np.array([700.0, 1220.0, 2600.0]) - 1.0) < 0.05)
    # the root nearest a cut-off, with an eps that just reaches it, and a tiny one that does not
    z = R.poly_roots(R.burg(clear, R.ORDER))
    fr = np.abs(np.arctan2(z.imag, z.real) * R.FORMANT_SR / (2 * np.pi))
    reach = np.min(np.minimum(np.abs(fr - 50.0) / 50.0, np.abs(fr - 5450.0) / 5450.0))
    assert R.frame_formants_diag(clear, root_eps=reach * 1.001)[1]
    assert not R.frame_formants_diag(clear, root_eps=reach * 0.5)[1]
    # Burg stopping below order 10 (a frame of one sample), Aberth running out (z^10), roots closer than the threshold
    short = np.array([0.5, 0.0])
    assert len(R.burg(short, R.ORDER)) - 1 < R.ORDER and R.frame_formants_diag(short)[1]
    assert R.poly_roots_diag(np.r_[1.0, np.zeros(10)])[1] == R.ABERTH_ITERS
    assert R.frame_formants_diag(clear, close=10.0)[1]
    assert not R.frame_formants_diag(np.zeros(R.FORMANT_WIN))[1]


@pytest.mark.parametrize("sr", (8000, 11000, 11025, 16000, 32000, 88200))
def test_restatement_is_finite_at_every_rate(sr):
    y, _, _ = T.synth(sr, segments=(("glide", 0.3), ("silence", 0.05), ("steady", 0.25)))
    for hop in (100, 441):
        f0, forms = R.track(y, sr, hop)
        assert np.isfinite(f0).all() and np.isfinite(forms).all()
        assert len(f0) == R.pitch_frames(len(y), sr, hop) and len(forms) == R.formant_frames(len(y), sr, hop)
        assert (f0 > 0).mean() > 0.5
    assert len(R.resample(y, sr)) == R.resampled_length(len(y), sr)
    if sr == 11000:                                                           # ratio 1: interpolation at the samples
        np.testing.assert_allclose(R.resample(y, sr)[30:-30], y[30:-30], atol=2e-3)


def test_restatement_non_finite_behaviour():
    """What the GPU is held to: a NaN or inf sample makes the signal's peak NaN, so every frame's unvoiced strength is
    0.45 and only the frames holding the sample lose their voiced candidates; an all-NaN signal is unvoiced, no formants."""
    sr, hop = 22050, 256
    y, _, _ = T.synth(sr)
    clean_f0 = R.track_pitch(y, sr, hop)
    W = R.pitch_window(sr)
    starts = R.pitch_starts(len(y), sr, hop)
    mid = len(y) // 2 + 1000
    for val in (np.nan, np.inf, -np.inf):
        b = y.copy()
        b[mid] = val
        cands, _, _ = R.pitch_candidates(b, sr, hop)
        assert all(c[1][0] == R.VOICING for c in cands)
        holds = (starts <= mid) & (mid < starts + W)
        assert all(len(c[0]) == 1 for c, h in zip(cands, holds) if h)
        f0, forms = R.track(b, sr, hop)
        assert np.isfinite(f0).all() and np.isfinite(forms).all()
        assert not f0[holds].any() and (f0 > 0).sum() >= 0.9 * (clean_f0 > 0).sum()
    f0, forms = R.track(np.full(sr // 2, np.nan), sr, hop)
    assert not f0.any() and not forms.any()


def test_sample_rate_and_hop_refusals_at_the_boundaries():
    from goofer_amd.device import GooferError, track_frame_offsets
    for sr in (8000, 96000):
        assert trackers.native_refusal(R.min_length(sr), sr) is None
        assert track_frame_offsets([R.min_length(sr)], sr, HOP)[0][-1] == 1
    for sr in (7999, 96001):
        assert isinstance(trackers.native_refusal(sr, sr), ValueError)
        with pytest.raises(GooferError):
            track_frame_offsets([sr], sr, HOP)
    for hop in (0, -1):
        with pytest.raises(GooferError):
            track_frame_offsets([44100], 44100, hop)


def test_stage_entry_points_refuse_in_their_query_form():
    """The single-stage calls check rate, hop and offsets before anything else, with no context and no device."""
    import ctypes as C
    from goofer_amd import _lib
    lib = _lib.load()
    off = np.array([0, 4000], np.int64)
    out = np.zeros(2, np.int64)
    need = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731

    def rcs(sr, hop, o=off):
        return (lib.goofer_track_candidates(None, None, p(o), 1, sr, hop, p(out), None, None, None, None, C.byref(need), None),
                lib.goofer_track_path(None, None, None, None, p(o), 1, sr, hop, None, None, C.byref(need), None),
                lib.goofer_track_resample(None, None, p(o), 1, sr, p(out), None, None, C.byref(need), None),
                lib.goofer_track_formant_frames(None, None, p(o), 1, sr, hop, p(out), None, None, C.byref(need), None))
    assert rcs(8000, 256) == (0, 0, 0, 0) and rcs(96000, 1) == (0,) * 4
    for sr, hop in ((7999, 256), (96001, 256)):
        assert all(rc != 0 for rc in rcs(sr, hop))
    assert all(rc != 0 for k, rc in enumerate(rcs(8000, 0)) if k != 2)        # the resampler takes no hop
    assert all(rc != 0 for rc in rcs(8000, 256, np.array([1, 4000], np.int64)))
    assert lib.goofer_track_path(None, None, None, None, p(np.array([0, 5, 3], np.int64)), 2, 8000, 256, None, None,
                                 C.byref(need), None) != 0
