"""GPU: the native tracker (csrc/tracker.hip) against its numpy restatement (tracker_ref.py) stage by stage — candidates,
Viterbi path, 11 kHz resampling, formant frames — over a matrix of rates, hops and signals (tracker_cases.py), then end to
end, in mixed batches, on non-finite samples and on crafted inputs.  Frames the restatement flags as within reach of a
flipped decision (the *_diag helpers) are left out of the tight checks; the share left in is asserted.

Measured worst on the MI355X (bound in brackets): candidate frequencies 6.6e-11 relative (1e-9); candidate and unvoiced
strengths 9.5e-13 absolute (1e-9); f0 of unflagged signals 1.4e-13 relative (1e-9); the 11 kHz signal 2.4e-15 x the
signal's peak (1e-12); formants 2.3e-8 relative (1e-6).  Unflagged: 30083 of 30346 pitch frames, 22691 of 22719 formant
frames, 207 of 221 signals; 3059 frames had more than 14 peaks.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

import tracker_cases as C
import tracker_ref as R

pytestmark = pytest.mark.gpu

F_REL, S_ABS, F0_REL, X11_REL, FORM_REL = 1e-9, 1e-9, 1e-9, 1e-12, 1e-6
WORST = {}


def _worst(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.close()
    print("\ntracker oracle worst:", {k: f"{v:.2e}" for k, v in sorted(WORST.items())})


@pytest.fixture(scope="module")
def ref():
    """The matrix and the restatement's answers, computed in worker processes (numpy only; they never open the GPU)."""
    cases = C.matrix()
    workers = max(1, min(8, len(os.sched_getaffinity(0))))
    with mp.get_context("spawn").Pool(workers) as pool:
        refs = pool.map(C.restate, cases, chunksize=1)
    return cases, refs


def _dev(ctx, a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype or np.float64)).to(ctx.device)


def _groups(cases):
    g = {}
    for k, (sr, hop, _, _) in enumerate(cases):
        g.setdefault((sr, hop), []).append(k)
    return g


@pytest.fixture(scope="module")
def gpu(ctx, ref):
    """Per case: the GPU's candidates, path on them, 11 kHz signal, formant frames on it, and Context.track's tracks, each
    (sr, hop) group as one ragged batch."""
    cases, _ = ref
    out = [None] * len(cases)
    for (sr, hop), idx in _groups(cases).items():
        ys = [cases[k][3] for k in idx]
        lengths = [len(y) for y in ys]
        y = _dev(ctx, np.concatenate(ys))
        cf, cs, cn, p_off = ctx.track_candidates(y, lengths, sr, hop)
        f0_path = ctx.track_path(cf, cs, cn, p_off, sr, hop).cpu().numpy()
        x11, x_off = ctx.track_resample(y, lengths, sr)
        forms, m_off = ctx.track_formant_frames(x11, np.diff(x_off), sr, hop)
        f0, p_off2, forms2, m_off2 = ctx.track(y, lengths, sr, hop)
        cf, cs, cn, x11, forms = cf.cpu().numpy(), cs.cpu().numpy(), cn.cpu().numpy(), x11.cpu().numpy(), forms.cpu().numpy()
        f0, forms2 = f0.cpu().numpy(), forms2.cpu().numpy()
        assert np.array_equal(p_off, p_off2) and np.array_equal(m_off, m_off2)
        for j, k in enumerate(idx):
            a, b = p_off[j], p_off[j + 1]
            out[k] = {"cf": cf[a:b], "cs": cs[a:b], "cn": cn[a:b], "f0_path": f0_path[a:b], "f0": f0[a:b],
                      "x11": x11[x_off[j]:x_off[j + 1]], "forms_stage": forms[m_off[j]:m_off[j + 1]],
                      "forms": forms2[m_off[j]:m_off[j + 1]]}
    return out


def _gpu_cands(g):
    return [(g["cf"][i, :g["cn"][i]].copy(), g["cs"][i, :g["cn"][i]].copy()) for i in range(len(g["cn"]))]


def _signal_flagged(r):
    return bool(r["cand_fragile"].any() or r["path_fragile"].any() or r.get("formant_fragile", np.zeros(0, bool)).any())


def test_compositions_equal_their_stages(gpu):
    for g in gpu:
        assert np.array_equal(g["f0"], g["f0_path"])
        assert np.array_equal(g["forms"], g["forms_stage"])


def test_candidates_match_restatement(ref, gpu):
    cases, refs = ref
    n_frames = n_unflagged = 0
    for (sr, hop, name, _), r, g in zip(cases, refs, gpu):
        assert len(g["cn"]) == len(r["cands"]), (sr, hop, name)
        for i, (f, s) in enumerate(r["cands"]):
            n_frames += 1
            if r["cand_fragile"][i]:
                continue
            n_unflagged += 1
            n = g["cn"][i]
            assert n == len(f), (sr, hop, name, i, n, len(f))
            gf, gs = g["cf"][i, :n], g["cs"][i, :n]
            assert gf[0] == 0.0
            if n > 1:
                _worst("cand_f_rel", np.max(np.abs(gf[1:] / f[1:] - 1.0)))
            _worst("cand_s_abs", np.max(np.abs(gs - s)))
            assert np.all(np.abs(gf[1:] - f[1:]) <= F_REL * f[1:]), (sr, hop, name, i)
            assert np.all(np.abs(gs - s) <= S_ABS), (sr, hop, name, i)
    assert n_unflagged >= 0.95 * n_frames, (n_unflagged, n_frames)
    print(f"\ncandidates: {n_unflagged} of {n_frames} frames unflagged; "
          f"{sum(int((r['peaks'] > R.MAX_CAND - 1).sum()) for r in refs)} frames with more than 14 peaks")
    for (sr, hop, name, _), r in zip(cases, refs):       # the pruning of 15+ peaks really runs on the sines
        if name in ("sine2k", "pair"):
            assert (r["peaks"] > R.MAX_CAND - 1).mean() > 0.5, (sr, name)


def test_path_on_gpu_candidates_matches_restatement(ref, gpu):
    cases, _ = ref
    for (sr, hop, name, _), g in zip(cases, gpu):
        f0, _, fragile = R.viterbi_diag(_gpu_cands(g), 0.01 * sr / hop)
        ok = ~fragile
        assert np.array_equal(g["f0_path"][ok], f0[ok]), (sr, hop, name)


def test_resample_matches_restatement(ref, gpu):
    cases, refs = ref
    for (sr, hop, name, y), r, g in zip(cases, refs, gpu):
        if "x11" not in r:
            continue
        assert g["x11"].shape == r["x11"].shape, (sr, name)
        peak = np.abs(y).max()
        if len(r["x11"]):
            _worst("x11_rel_peak", np.max(np.abs(g["x11"] - r["x11"])) / peak if peak > 0 else 0.0)
            assert np.all(np.abs(g["x11"] - r["x11"]) <= X11_REL * peak), (sr, hop, name)


def _close_formants(got, want, tol=FORM_REL):
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    on = want != 0
    if on.any():
        err = np.max(np.abs(got[on] / want[on] - 1.0))
        _worst("formant_rel", err)
        assert err <= tol, err


def test_formant_frames_on_gpu_resample_match_restatement(ref, gpu):
    cases, _ = ref
    n_frames = n_unflagged = 0
    for (sr, hop, name, _), g in zip(cases, gpu):
        if name == "long":
            continue
        forms, fragile = R.formants_of_11k(g["x11"], sr, hop)
        assert g["forms_stage"].shape == forms.shape, (sr, hop, name)
        n_frames += len(fragile)
        n_unflagged += int((~fragile).sum())
        _close_formants(g["forms_stage"][~fragile], forms[~fragile])
    assert n_unflagged >= 0.95 * n_frames, (n_unflagged, n_frames)
    print(f"\nformant frames: {n_unflagged} of {n_frames} unflagged")


def test_end_to_end_matches_restatement(ctx, ref, gpu):
    from goofer_amd import trackers
    cases, refs = ref
    unflagged = 0
    for (sr, hop, name, y), r, g in zip(cases, refs, gpu):
        f0, _ = trackers.native_tracker(y, sr, hop, 10, ctx=ctx)
        assert np.array_equal(f0, g["f0"]), (sr, hop, name)
        rf0 = r["f0"]
        if _signal_flagged(r):
            if "formants" in r:
                _compare_loose((g["f0"], g["forms"]), (rf0, r["formants"]))
            continue
        unflagged += 1
        assert np.array_equal(g["f0"] > 0, rf0 > 0), (sr, hop, name)
        v = rf0 > 0
        if v.any():
            _worst("f0_rel", np.max(np.abs(g["f0"][v] / rf0[v] - 1.0)))
        assert np.all(np.abs(g["f0"][v] - rf0[v]) <= F0_REL * rf0[v]), (sr, hop, name)
        if "formants" in r:
            _close_formants(g["forms"], r["formants"])
    assert unflagged >= 0.9 * len(cases), (unflagged, len(cases))
    print(f"\nend to end: {unflagged} of {len(cases)} signals unflagged")


def _compare_loose(gpu, ref):
    """test_gpu_tracker's bars, for signals the restatement flags."""
    (gf0, gfm), (rf0, rfm) = gpu, ref
    assert gf0.shape == rf0.shape and gfm.shape == rfm.shape
    assert np.isfinite(gf0).all() and np.isfinite(gfm).all()
    assert np.mean((gf0 > 0) == (rf0 > 0)) >= 0.995
    both = (gf0 > 0) & (rf0 > 0)
    assert np.all(np.abs(gf0[both] / rf0[both] - 1.0) <= 1e-4)
    defined = (gfm > 0) & (rfm > 0)
    assert np.all(np.abs(gfm[defined] - rfm[defined]) <= 0.5)
    assert np.mean((gfm > 0) == (rfm > 0)) >= 0.995


# -- crafted inputs ------------------------------------------------------------------------------------------------
def _path(ctx, cand_lists, sr, hop):
    """The GPU path of per-signal candidate lists [[(freqs, strengths) per frame]]."""
    import torch
    frames = [c for sig in cand_lists for c in sig]
    F = len(frames)
    cf, cs = np.zeros((F, 15)), np.zeros((F, 15))
    cn = np.zeros(F, np.int32)
    for i, (f, s) in enumerate(frames):
        cf[i, :len(f)], cs[i, :len(s)], cn[i] = f, s, len(f)
    off = np.concatenate([[0], np.cumsum([len(sig) for sig in cand_lists])]).astype(np.int64)
    f0 = ctx.track_path(_dev(ctx, cf), _dev(ctx, cs), torch.as_tensor(cn).to(ctx.device), off, sr, hop).cpu().numpy()
    return [f0[off[k]:off[k + 1]] for k in range(len(cand_lists))]


def test_path_on_crafted_candidates(ctx):
    sr, hop = 22050, 256
    tsc = 0.01 * sr / hop
    a = lambda *v: np.array(v, np.float64)                                     # noqa: E731
    tie = [(a(0.0, 100.0, 400.0), a(0.1, 0.9, 0.9)), (a(0.0, 200.0), a(0.1, 0.9))]   # |log2(100/200)| = |log2(400/200)| = 1
    final_tie = [(a(0.0, 300.0), a(0.1, 0.9)), (a(0.0, 150.0, 600.0), a(0.1, 0.9, 0.9))]
    one_frame = [(a(0.0, 220.0, 440.0), a(0.5, 0.8, 0.8))]
    rng = np.random.default_rng(11)
    rand = []
    for n_frames in (1, 2, 40, 300):
        sig = []
        for _ in range(n_frames):
            n = int(rng.choice([1, 15, *range(1, 16)]))
            f = np.concatenate([[0.0], np.sort(rng.uniform(75.0, 950.0, n - 1))])
            sig.append((f, rng.uniform(0.0, 1.5, n)))
        rand.append(sig)
    lists = [tie, final_tie, one_frame, *rand]
    got = _path(ctx, lists, sr, hop)
    assert np.array_equal(got[0], [100.0, 200.0])                           # the first best predecessor wins
    assert np.array_equal(got[1], [300.0, 150.0])                           # the first best final candidate wins
    assert np.array_equal(got[2], [220.0])
    for k, (g, sig) in enumerate(zip(got, lists)):
        f0, _, fragile = R.viterbi_diag(sig, tsc)
        assert np.array_equal(g[~fragile], f0[~fragile])
        if k >= 3:                                                            # the random lists have no near-tie
            assert not fragile.any()
    assert np.array_equal(R.viterbi(tie, tsc), got[0]) and np.array_equal(R.viterbi(final_tie, tsc), got[1])


def _ar(poles_hz_r, n, seed, amp=1.0):
    """An AR process at 11 kHz with pole pairs (Hz, radius); a pole at 0 Hz is one real pole."""
    rng = np.random.default_rng(seed)
    a = np.array([1.0])
    for f, r in poles_hz_r:
        if f == 0.0:
            a = np.convolve(a, [1.0, -r])
        else:
            a = np.convolve(a, [1.0, -2 * r * np.cos(2 * np.pi * f / 11000.0), r * r])
    e = rng.standard_normal(n + 500)
    y = np.zeros(n + 500)
    for t in range(len(y)):
        k = min(t, len(a) - 1)
        y[t] = e[t] - np.dot(a[1:k + 1], y[t - 1::-1][:k]) if k else e[t]
    y = y[500:]
    return amp * y / np.abs(y).max()


def test_formant_frames_on_crafted_frames(ctx):
    n = R.FORMANT_WIN + 300
    base = [(700.0, 0.97), (1220.0, 0.96), (2600.0, 0.95), (3500.0, 0.94)]
    frames = {
        "near_50": _ar([(50.5, 0.98)] + base, n, 1),
        "near_5450": _ar(base + [(5449.0, 0.95)], n, 2),
        "real_pole": _ar(base + [(0.0, 0.9), (0.0, -0.8)], n, 3),
        "sinusoid": np.sin(2 * np.pi * 1000.0 * np.arange(n) / 11000.0),
        "zeros": np.zeros(n),
        "one_sample": np.where(np.arange(n) == n // 2, 0.7, 0.0),
        "amp1e-150": _ar(base, n, 4, 1e-150),
        "amp1e150": _ar(base, n, 4, 1e150),
    }
    xs = list(frames.values())
    for hop in (64, 256):
        forms, f_off = ctx.track_formant_frames(_dev(ctx, np.concatenate(xs)), [len(x) for x in xs], 11000, hop)
        forms = forms.cpu().numpy()
        for k, (name, x) in enumerate(frames.items()):
            want, fragile = R.formants_of_11k(x, 11000, hop)
            got = forms[f_off[k]:f_off[k + 1]]
            assert got.shape == want.shape and np.isfinite(got).all(), name
            _close_formants(got[~fragile], want[~fragile])
            if name == "zeros":
                assert not got.any() and not fragile.any()
            if name in ("amp1e-150", "amp1e150", "real_pole"):
                assert not fragile.any(), name
        big, small = forms[f_off[7]:f_off[8]], forms[f_off[6]:f_off[7]]
        np.testing.assert_allclose(big, small, rtol=1e-9)                  # Burg is scale-free


# -- batches, non-finite samples, refusals ---------------------------------------------------------------------------
def _tracks(ctx, ys, sr, hop):
    y = _dev(ctx, np.concatenate(ys))
    f0, p_off, forms, f_off = ctx.track(y, [len(s) for s in ys], sr, hop)
    f0, forms = f0.cpu().numpy(), forms.cpu().numpy()
    return [(f0[p_off[k]:p_off[k + 1]], forms[f_off[k]:f_off[k + 1]]) for k in range(len(ys))]


def _nonfinite(sr):
    v = C.voice(sr, 0.4, 5)
    mid = len(v) // 2
    nan1, inf1, run = v.copy(), v.copy(), v.copy()
    nan1[mid] = np.nan
    inf1[mid] = np.inf
    run[:len(v) // 5] = np.nan
    return {"nan": nan1, "inf": inf1, "nan_run": run, "all_nan": np.full(len(v), np.nan)}


def test_batches_equal_single_calls_bit_for_bit(ctx):
    for sr in C.RATES:
        hop = C.HOPS[sr][0]
        sig = C.signals(sr, hop, True)
        short = C.voice(sr, 0.4, 6)[:int(0.045 * sr)]                          # 40-50 ms: pitch frames, no formant frame
        assert R.formant_frames(len(short), sr, hop) == 0 < R.pitch_frames(len(short), sr, hop)
        ys = [short, sig["synth"], sig["click"], short, _nonfinite(sr)["nan"], sig["glide"], sig["len_min"], short]
        batch = _tracks(ctx, ys, sr, hop)
        for k, y in enumerate(ys):
            (one,) = _tracks(ctx, [y], sr, hop)
            assert np.array_equal(one[0], batch[k][0]) and np.array_equal(one[1], batch[k][1]), (sr, k)


@pytest.mark.parametrize("sr", (8000, 22050, 96000))
def test_non_finite_samples_match_restatement(ctx, sr):
    hop = 256
    clean = C.voice(sr, 0.4, 7)
    bad = _nonfinite(sr)
    ys = [clean]
    for y in bad.values():
        ys += [y, clean]
    got = _tracks(ctx, ys, sr, hop)
    (alone,) = _tracks(ctx, [clean], sr, hop)
    for k in range(0, len(ys), 2):                                            # the clean neighbours are unaffected
        assert np.array_equal(got[k][0], alone[0]) and np.array_equal(got[k][1], alone[1])
    for k, (name, y) in enumerate(bad.items()):
        f0, forms = got[2 * k + 1]
        rf0, rforms = R.track(y, sr, hop)
        assert np.array_equal(f0 > 0, rf0 > 0), (name, int((f0 > 0).sum()), int((rf0 > 0).sum()))
        v = rf0 > 0
        assert np.all(np.abs(f0[v] - rf0[v]) <= F0_REL * rf0[v]), name
        assert np.isfinite(forms).all() and np.array_equal(forms == 0, rforms == 0), name
        on = rforms != 0
        assert np.all(np.abs(forms[on] - rforms[on]) <= FORM_REL * rforms[on]), name
        if name in ("nan", "inf"):                                            # only the frames holding the sample turn unvoiced
            assert v.sum() >= 0.8 * (alone[0] > 0).sum(), name


def test_refusals_on_the_device(ctx):
    from goofer_amd import trackers
    from goofer_amd.device import GooferError
    for sr in (8000, 96000):
        y = C.voice(sr, 0.3, 8)
        assert trackers.native_refusal(len(y), sr) is None
        assert len(trackers.native_tracker(y, sr, 256, 10, ctx=ctx)[0]) == R.pitch_frames(len(y), sr, 256)
    y = _dev(ctx, np.zeros(8000))
    calls = (lambda sr, hop: ctx.track(y, [8000], sr, hop), lambda sr, hop: ctx.track_candidates(y, [8000], sr, hop),
             lambda sr, hop: ctx.track_formant_frames(y, [8000], sr, hop))
    for sr, hop in ((7999, 256), (96001, 256), (22050, 0), (22050, -4)):
        for call in calls:
            with pytest.raises(GooferError):
                call(sr, hop)
    for sr in (7999, 96001):
        with pytest.raises(GooferError):
            ctx.track_resample(y, [8000], sr)
    cf, cs, cn, off = ctx.track_candidates(y, [8000], 8000, 256)
    for sr, hop in ((7999, 256), (96001, 256), (8000, 0)):
        with pytest.raises(GooferError):
            ctx.track_path(cf, cs, cn, off, sr, hop)
