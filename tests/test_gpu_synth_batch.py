"""core.synthesize_batch on the MI355X: bit for bit the sequential core.synthesize calls, its launch counts, and the three ragged
entries it is built from (goofer_ingest_rows, goofer_warp_bins_ragged, goofer_stretch_ragged)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    return Context(0).plan(44100, 1024, 256)


def _source(i, seconds):
    from goofer_amd import core, synthetic as syn
    s = syn.make_source(500 + i, seconds=seconds)
    env = core.decode_env_from_knots(s["env_pack"]).astype(np.float64)
    env *= 1.0 + 1e-3 * np.sin(np.arange(env.size)).reshape(env.shape)          # fp64 values that do not sit on the fp32 grid
    return s, env


def _note_kwargs(rng, n):
    pick = lambda p: rng.random() < p                            # noqa: E731
    kw = {}
    if pick(0.5): kw["pitch_shift"] = float(np.round(rng.uniform(0.6, 1.7), 3))
    if pick(0.5): kw["formant_shift"] = float(np.round(rng.uniform(0.7, 1.4), 3))
    for k in ("F1_shift", "F3_shift"):
        if pick(0.3): kw[k] = float(np.round(rng.uniform(0.7, 1.4), 2))
    if pick(0.4): kw["normalize"] = float(np.round(rng.uniform(0.0, 1.0), 2))
    if pick(0.4): kw.update(f0_jitter=True, f0_jitter_strength=float(np.round(rng.uniform(0.05, 1.5), 3)))
    if pick(0.2): kw.update(volume_jitter=True, volume_jitter_strength_harm=0.5, volume_jitter_strength_breath=1.0)
    if pick(0.2): kw.update(add_subharm=True, subharm_weight=0.7, subharm_semitones=[-12, 7] if pick(0.5) else -12)
    if pick(0.25):
        kw.update(roughness_on=True, rough_alpha=float(np.round(rng.uniform(0.2, 1.0), 2)))
        if pick(0.5): kw["rough_k_list"] = (2, 5)
    if pick(0.35):
        kw["stretch_factor"] = float(np.round(rng.uniform(0.6, 1.5), 2))
        if pick(0.5):                                            # regions at the edges: from the start, to the end, past it
            dur = n / 44100.0
            a = 0.0 if pick(0.5) else float(np.round(rng.uniform(0.0, dur), 3))
            kw.update(start_sec=a, end_sec=float(a + (dur + 0.5 if pick(0.5) else rng.uniform(0.01, 0.2))))
    return kw


def _same(a, b):
    if isinstance(b, BaseException):
        return isinstance(a, type(b)) and str(a) == str(b)
    return len(a) == len(b) == 4 and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _sequential(notes, seeds, phis, ctx, **kw):
    from goofer_amd import core
    out = []
    for note, seed, phi in zip(notes, seeds, phis):
        try:
            out.append(core.synthesize(**{**kw, **note}, sr=44100, seed=seed, phi=phi, ctx=ctx))
        except Exception as e:
            out.append(e)
    return out


def _both(notes, seeds, phis, ctx, **kw):
    from goofer_amd import core
    np.random.seed(77)
    seq = _sequential(notes, seeds, phis, ctx, **kw)
    st_seq = np.random.get_state()
    np.random.seed(77)
    bat = core.synthesize_batch(notes, 44100, seeds=seeds, phis=phis, ctx=ctx, **kw)
    st_bat = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(st_seq, st_bat)), "legacy RNG state differs"
    return seq, bat


def test_random_notes_equal_sequential_calls(ctx):
    rng = np.random.default_rng(2024)
    notes = []
    for i in range(48):
        seconds = 0.0 if i == 5 else float(rng.uniform(0.05, 3.0))
        s, env = _source(i, seconds)
        note = {"env_spec": env if i % 3 else env.astype(np.float32), "f0_interp": s["f0"] * np.float32(rng.uniform(0.7, 1.6)),
                "voicing_mask": s["mask"], "y": np.zeros(s["y_len"]), "formants": s["formants"]}
        note.update(_note_kwargs(rng, s["y_len"]))
        notes.append(note)
    notes[7].update(stretch_factor=1.2, start_sec=0.4, end_sec=0.4)            # an empty region: that slot raises
    seeds = [int(v) for v in rng.integers(0, 2 ** 63, 48)]
    seq, bat = _both(notes, seeds, [None] * 48, ctx, breath_strength=0.15)
    assert isinstance(bat[7], ValueError)
    for i, (a, b) in enumerate(zip(bat, seq)):
        assert _same(a, b), f"note {i} ({sorted(k for k in notes[i] if k not in ('env_spec', 'f0_interp', 'voicing_mask', 'y'))})"


def test_injected_phases_and_knot_envelopes(ctx):
    from goofer_amd import synthetic as syn
    notes, phis = [], []
    for i in range(6):
        s, env = _source(40 + i, 0.3 + 0.2 * i)
        frames = 1 + s["y_len"] // 256
        notes.append({"env_spec": s["env_pack"] if i % 2 else env, "f0_interp": s["f0"], "voicing_mask": s["mask"],
                      "y": np.zeros(s["y_len"]), "formants": s["formants"], "pitch_shift": 1.0 + 0.1 * i,
                      "stretch_factor": 1.3 if i >= 4 else 1.0})
        phis.append(syn.phase_matrix(60 + i, 513, frames if i < 4 else 1 + int(s["y_len"] * 1.3) // 256))
    seq, bat = _both(notes, [None] * 6, phis, ctx)
    assert all(_same(a, b) for a, b in zip(bat, seq))
    # knots dict against its decoded fp32 array
    s, _ = _source(50, 0.5)
    from goofer_amd import core
    dec = core.decode_env_from_knots(s["env_pack"], ctx=ctx)
    ctx.plan(44100, 1024, 256)
    base = {"f0_interp": s["f0"], "voicing_mask": s["mask"], "y": np.zeros(s["y_len"])}
    a, b = core.synthesize_batch([{**base, "env_spec": s["env_pack"]}, {**base, "env_spec": dec}], 44100, seeds=[3, 3], ctx=ctx)
    assert _same(a, b)


def test_fp64_envelope_rounds_like_numpy(ctx):
    from goofer_amd import core
    s, env = _source(70, 0.8)
    base = {"f0_interp": s["f0"], "voicing_mask": s["mask"], "y": np.zeros(s["y_len"]), "formant_shift": 1.1}
    a, b = core.synthesize_batch([{**base, "env_spec": env}, {**base, "env_spec": env.astype(np.float32)}], 44100, seeds=[9, 9], ctx=ctx)
    assert _same(a, b)


class _Counting:
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


@pytest.mark.parametrize("stretched", [False, True])
def test_launch_count_does_not_grow_with_notes(ctx, stretched):
    from goofer_amd import core
    rng = np.random.default_rng(5)
    counts = []
    for n in (8, 64):
        notes = []
        for i in range(n):
            s, env = _source(i % 16, float(rng.uniform(0.2, 0.6)))
            notes.append({"env_spec": env, "f0_interp": s["f0"], "voicing_mask": s["mask"], "y": np.zeros(s["y_len"]),
                          "formants": s["formants"], "pitch_shift": float(rng.uniform(0.8, 1.2)), "formant_shift": float(rng.uniform(0.9, 1.1)),
                          "F2_shift": 1.1 if i % 2 else 1.0, "uv_strength": float(rng.uniform(0.2, 1.0))})
        lib = ctx.lib
        ctx.lib = _Counting(lib)
        try:
            core.synthesize_batch(notes, 44100, seeds=list(range(n)), ctx=ctx, stretch_factor=1.3 if stretched else 1.0)
            counts.append(ctx.lib.calls)
        finally:
            ctx.lib = lib
    assert counts[0] == counts[1]
    assert counts[0]["goofer_synth_batch"] == 1
    assert counts[0]["goofer_ingest_rows"] == 1
    if stretched:
        assert counts[0]["goofer_stretch_ragged"] == 1 and counts[0]["goofer_warp_bins_ragged"] == 1


def _interp_np(x, a, b, m):
    """concat(x[:a], np.interp stretch of x[a:b] to m rows, x[b:]) along axis 0, in fp64 rounded to fp32 (GOOFER.py:597-616)."""
    seg = x[a:b].astype(np.float64)
    xo, xi = np.linspace(0, 1, m), np.linspace(0, 1, b - a)
    mid = np.stack([np.interp(xo, xi, seg[:, c]) for c in range(x.shape[1])], axis=1) if x.ndim == 2 else np.interp(xo, xi, seg)
    return np.concatenate([x[:a], mid.astype(np.float32), x[b:]])


def test_ragged_stretch_beyond_the_single_call_row_limit(ctx):
    rng = np.random.default_rng(11)
    rows = [40000, 300, 5]
    cuts = [(100, 39000), (0, 300), (2, 3)]
    outs = [100 + 2 * 38900 + 1000, 450, 4 + 7]
    envs = [rng.random((r, 8), dtype=np.float32) for r in rows]
    s_lens, s_cuts, s_outs = [70000, 9, 1], [(5, 69000), (0, 9), (0, 1)], [5 + 80000 + 1000, 4, 3]
    f0s = [rng.random(n, dtype=np.float32) for n in s_lens]
    h = ctx.rows(sum(rows), 8)
    h.copy_(torch.as_tensor(np.concatenate(envs)))
    nz = ctx.rows_like(h)
    nz.copy_(h * 2)
    f0 = ctx.tensor(np.concatenate(f0s))
    h2, n2, f2, m2 = ctx.stretch_ragged(h, nz, rows, cuts, outs, f0, f0 * 3, s_lens, s_cuts, s_outs)
    assert outs[0] > 65535
    ro, so = np.cumsum([0] + outs), np.cumsum([0] + s_outs)
    H, N, F, M = h2.cpu().numpy(), n2.cpu().numpy(), f2.cpu().numpy(), m2.cpu().numpy()
    for i in range(3):
        (a, b), m = cuts[i], outs[i] - cuts[i][0] - (rows[i] - cuts[i][1])
        assert np.array_equal(H[ro[i]:ro[i + 1]], _interp_np(envs[i], a, b, m))
        assert np.array_equal(N[ro[i]:ro[i + 1]], _interp_np(envs[i] * 2, a, b, m))
        (a, b), m = s_cuts[i], s_outs[i] - s_cuts[i][0] - (s_lens[i] - s_cuts[i][1])
        assert np.array_equal(F[so[i]:so[i + 1]], _interp_np(f0s[i], a, b, m))
        assert np.array_equal(M[so[i]:so[i + 1]], _interp_np(f0s[i] * np.float32(3), a, b, m))


def test_ingest_and_ragged_warp_equal_the_single_entries(ctx):
    from goofer_amd import core
    rng = np.random.default_rng(3)
    Ts = [1, 70, 0, 129, 64]
    envs = [rng.random((513, T)) + 0.01 for T in Ts]
    rows = ctx.ingest_rows(ctx.tensor(np.concatenate([e.ravel() for e in envs])), Ts, 513)
    rows32 = ctx.ingest_rows(ctx.tensor(np.concatenate([e.astype(np.float32).ravel() for e in envs])), Ts, 513)
    off = np.cumsum([0] + Ts)
    F = np.concatenate([np.stack([core._fit(700.0 * (k + 1) + 50 * rng.standard_normal(T), T) for k in range(4)], axis=1) for T in Ts])
    fs = [[1.2, 1.0, 0.8, 1.0], [1.0, 1.0, 1.0, 1.0], [1.1, 1.1, 1.1, 1.1], [0.9, 1.3, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]]
    ratio, anchor = [1.0, 1.15, 0.9, 1.0, 1.0], [True, True, False, True, False]
    warped = ctx.warp_bins_ragged(rows, Ts, ctx.tensor(F), fs, ratio, anchor)
    for i, e in enumerate(envs):
        single = ctx.rows_from(e.astype(np.float32).T)
        sl = slice(int(off[i]), int(off[i + 1]))
        assert torch.equal(rows[sl], single) and torch.equal(rows32[sl], single)
        if Ts[i]:
            w = ctx.warp_bins(single, ctx.tensor(F[sl]), fs[i] if anchor[i] else None, ratio[i])
            assert torch.equal(warped[sl], w), i
