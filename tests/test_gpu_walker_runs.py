"""GPU: the four frame walkers (k_noise_stems, k_harm_stem: csrc/stems.hip; k_irfft_ola3, k_irfft_ola1: csrc/samples.hip) at the
run lengths of a full-size batch, on a batch of under 2 000 frames, against the float64 truth of tests/synth_ref.py.

The launchers choose the frames per wave from the waves the device holds (walk_run_choice, csrc/launchers.h): a batch leaves the
floor of 32 frames (8 halos where the halo is above 4) only with tens of thousands of frames, and the 1024-note workload runs
at 64 to 95.  Option "walk_run" N puts N — clamped to what the automatic choice can return for the kernel — in its place, and
goofer_counter "walk_run_*" reads back what the last launch got; every test asserts that read-back.  The batch is
synth_ref.long_batch (LONG_FRAMES: notes of 1..5 frames, forty one-frame notes in a row, notes of 61 .. 67, 127 .. 130, 257 and
about 300 frames), and before anything is judged synth_ref.run_coverage must hold on the batch's frame_off at the run that ran:
runs that start at frames 0, 1, 2, 3 and beyond the halo of a note, runs that end on a note's last frame and on its last but
one, a run of three whole notes, a note of three runs and, for the two stem walkers, a record refill (frame_block, 64 frames)
inside a note and on a note's first frame, and a last record block that reaches past the batch.

  truth        every stage, unit by unit, e_gpu <= FACTOR * E_ref + 2^-23 with the judge of tests/test_gpu_synth_stages.py
               (judge_notes: E_ref from the CPU restatements only, the project's factor 3, zero tails exactly zero, frame_skip)
  bits         every forced run against walk_run 0: the five outputs, note_mag and note_peak bit for bit — the overlap-add runs
               in ascending frame order however the frames are cut into runs.  The one allowance is that of
               test_gpu_synth_stages.py and holds on the walker routes' uv / bre only: the sign of a zero under an fp32 gain
               that is exactly zero
  philox       the same without injected phases (the production noise path: a refill redoes load_nyquist)
  render       Renderer.render (goofer_render_batch: a refill redoes mark_plain) on six sources of 104 .. 293 frames, warping
               and plain flags interleaved: bits between the runs, and the oracle within the 1e-4 of tests/test_gpu_hard.py
  clamp        walk_run 1 and 100000 give the floor and the cap, and the bits of walk_run 0

MEASURED on the MI355X: worst note per route, forced run and stage on the long batch, E_ref / e_gpu (ratio = (e_gpu - 2^-23) / E_ref,
floored at 0; vacuous notes left out of the figures as in tests/test_gpu_synth_stages.py).  The runs of a route share one line:
their outputs are the same bits, so their figures are the same.  Every stage holds the project's factor 3 — the largest ratio
is 1.58 — and no factor was raised.  Zero-sign differences under a zero fp32 gain, forced runs against walk_run 0: 3 420 samples
over the six runs on the walkers and td_blur 0 routes, 0 with skip_zero 0 and on every other route, 1 122 with Philox phases
(65 and 128), 0 on the render path.  Render at walk_run 128 against the oracle: 7.3e-09 .. 2.9e-08 sample-RMS over the six notes.
  walkers, walk_run 62, 65, 95, 128
      env_harm  8.1e-08 / 1.0e-07 (0.00)   note_mag  2.5e-07 / 2.2e-07 (0.42)   harm      2.4e-07 / 3.4e-07 (0.93)
      uv        2.6e-07 / 3.4e-07 (0.83)   bre       2.5e-07 / 3.2e-07 (0.80)   rec       2.2e-07 / 3.9e-07 (1.22)
      mix       2.2e-07 / 3.3e-07 (0.95)   note_peak 2.4e-07 / 2.0e-07 (0.34)
  ola3, walk_run 62, 65, 95, 128
      S_harm    3.0e-07 / 3.2e-07 (0.67)   S_uv      6.8e-08 / 2.3e-07 (1.58)   S_breath  1.1e-07 / 2.9e-07 (1.47)
      note_mag  2.5e-07 / 2.2e-07 (0.42)   harm      7.8e-07 / 1.2e-06 (1.34)   bre       2.4e-07 / 3.3e-07 (0.85)
      rec       3.1e-07 / 4.0e-07 (0.93)   mix       3.1e-07 / 3.4e-07 (0.73)   note_peak 2.4e-07 / 1.4e-07 (0.07)
      uv        2.5e-07 / 3.2e-07 (0.79)
  ola3_256, walk_run 62, 65, 95, 128
      S_harm    2.9e-07 / 3.6e-07 (0.84)   S_uv      9.0e-08 / 2.5e-07 (1.44)   S_breath  1.2e-07 / 2.9e-07 (1.36)
      note_mag  3.4e-07 / 3.3e-07 (0.63)   harm      2.6e-06 / 3.3e-06 (1.23)   bre       1.9e-07 / 3.0e-07 (0.98)
      rec       1.3e-07 / 2.6e-07 (1.03)   mix       2.0e-07 / 2.9e-07 (0.88)   note_peak 2.5e-07 / 2.0e-07 (0.31)
      uv        2.0e-07 / 3.1e-07 (0.93)
  ola1_skip, walk_run 95, 256
      S_harm    2.2e-07 / 2.8e-07 (0.75)   S_uv      7.3e-08 / 2.2e-07 (1.46)   S_breath  1.3e-07 / 3.1e-07 (1.46)
      note_mag  2.1e-07 / 2.2e-07 (0.50)   harm      1.4e-07 / 2.5e-07 (0.91)   bre       2.0e-07 / 3.2e-07 (1.03)
      rec       1.8e-07 / 2.9e-07 (0.92)   mix       1.9e-07 / 2.9e-07 (0.89)   note_peak 2.7e-07 / 2.3e-07 (0.43)
      uv        2.2e-07 / 2.9e-07 (0.75)
  ola1_hop96, walk_run 256
      S_harm    1.7e-07 / 2.4e-07 (0.67)   S_uv      9.9e-08 / 2.7e-07 (1.55)   S_breath  9.8e-08 / 2.4e-07 (1.24)
      note_mag  1.7e-07 / 1.6e-07 (0.24)   harm      2.0e-07 / 3.1e-07 (0.93)   bre       3.5e-07 / 5.4e-07 (1.18)
      rec       2.5e-07 / 3.9e-07 (1.09)   mix       2.5e-07 / 4.5e-07 (1.32)   note_peak 2.5e-07 / 3.2e-07 (0.78)
      uv        3.1e-07 / 4.2e-07 (0.96)
  ola3_2048 (k_irfft_ola3<1024>), walk_run 62, 65, 95, 128
      S_harm    2.2e-07 / 2.8e-07 (0.75)   S_uv      7.3e-08 / 2.2e-07 (1.46)   S_breath  1.3e-07 / 3.1e-07 (1.46)
      note_mag  2.1e-07 / 2.2e-07 (0.50)   harm      1.4e-07 / 2.5e-07 (0.91)   bre       2.0e-07 / 3.2e-07 (1.03)
      rec       1.8e-07 / 2.9e-07 (0.92)   mix       1.9e-07 / 2.9e-07 (0.89)   note_peak 2.7e-07 / 2.3e-07 (0.43)
      uv        2.2e-07 / 2.9e-07 (0.75)
  ola3_wide (hop 512 at n_fft 1024: wider than the kernel's slots), walk_run 62, 65, 95, 128
      S_harm    2.3e-07 / 3.2e-07 (0.88)   S_uv      1.0e-07 / 2.6e-07 (1.43)   S_breath  1.4e-07 / 3.1e-07 (1.41)
      note_mag  2.4e-07 / 2.1e-07 (0.38)   harm      2.3e-07 / 3.1e-07 (0.85)   bre       2.8e-07 / 4.0e-07 (1.04)
      rec       1.6e-07 / 2.6e-07 (0.88)   mix       2.4e-07 / 3.6e-07 (1.00)   note_peak 3.3e-07 / 1.6e-07 (0.12)
      uv        2.2e-07 / 3.2e-07 (0.92)
  ola1_wide (hop 1024 at n_fft 2048: knots from global memory, no frame_skip), walk_run 95, 256
      S_harm    1.8e-07 / 2.6e-07 (0.75)   S_uv      7.1e-08 / 2.2e-07 (1.45)   S_breath  1.1e-07 / 2.9e-07 (1.53)
      note_mag  1.1e-07 / 2.0e-07 (0.71)   harm      1.9e-07 / 3.0e-07 (0.99)   bre       1.7e-07 / 3.2e-07 (1.17)
      rec       2.2e-07 / 2.9e-07 (0.76)   mix       1.9e-07 / 2.9e-07 (0.90)   note_peak 2.2e-07 / 1.6e-07 (0.20)
      uv        2.1e-07 / 3.6e-07 (1.17)
Zero-sign differences on the three, forced runs against walk_run 0: 0.
"""
import numpy as np
import pytest

import synth_ref as SR
from test_gpu_synth_stages import (ROUTES, Tally, _bit_mismatches, _pulse_runs, _restore, _run, _set, _three, _zero_gain,   # noqa: F401
                                   judge_notes)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIGMA = 100.0
OUTS = ("harm", "uv", "bre", "rec", "mix")
# route: (the counters of the walkers it launches, their cap)
WALKERS = {"walkers": (("walk_run_noise", "walk_run_harm"), 128), "walkers_td_blur0": (("walk_run_noise", "walk_run_harm"), 128),
           "walkers_skip_zero0": (("walk_run_noise", "walk_run_harm"), 128), "ola3": (("walk_run_ola3",), 128),
           "ola3_256": (("walk_run_ola3",), 128), "ola1_skip": (("walk_run_ola1",), 256), "ola1_hop96": (("walk_run_ola1",), 256),
           "ola3_2048": (("walk_run_ola3",), 128), "ola3_wide": (("walk_run_ola3",), 128), "ola1_wide": (("walk_run_ola1",), 256)}
TRUTH_RUNS = {"walkers": (62, 65, 95, 128), "ola3": (62, 65, 95, 128), "ola3_256": (62, 65, 95, 128), "ola1_skip": (95, 256),
              "ola1_hop96": (256,), "ola3_2048": (62, 65, 95, 128), "ola3_wide": (62, 65, 95, 128), "ola1_wide": (95, 256)}
BIT_RUNS = dict({r: (61, 62, 64, 65, 95, 128) for r in ("walkers", "walkers_td_blur0", "walkers_skip_zero0", "ola3", "ola3_256")},
                ola1_skip=(95, 256), ola1_hop96=(256,), ola3_2048=(62, 65, 95, 128), ola3_wide=(62, 65, 95, 128), ola1_wide=(95, 256))

_long = {}


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    c.set_option("walk_run", 0)
    _restore(c)
    c.close()


def _notes(geo):
    if geo not in _long:
        _long[geo] = SR.long_batch(geo)
    return _long[geo]


def _halo(geo):
    return (geo[1] + geo[2] - 1) // geo[2] - 1


def _floor(geo):
    return 32 if _halo(geo) <= 4 else 8 * _halo(geo)


def _walk(ctx, route, run, views=False, seed=None, profile=False):
    """One batch of the route at option walk_run ``run``, with note_mag / note_peak; asserts the run every walker of the route
    was launched with (``run`` clamped to [floor, cap]; 0: the floor, which is what the device chooses for a batch this small)."""
    geo, opts, names, kind, has_skip = ROUTES[route]
    counters, cap = WALKERS[route]
    ctx.set_option("walk_run", run)
    d = _run(ctx, geo, _notes(geo), SIGMA, views=views, seed=seed, profile=profile)
    want = _floor(geo) if run == 0 else min(max(run, _floor(geo)), max(cap, _floor(geo)))
    for name in counters:
        assert ctx.counter(name) == want, (route, run, name, ctx.counter(name), want)
    if not views:
        for name in ("note_mag", "note_peak"):
            d[name] = ctx.debug_fetch(name)
    d["run"] = want
    return d


def _covered(route, d):
    geo, kind = ROUTES[route][0], ROUTES[route][3]
    cov = SR.run_coverage(d["f_off"], d["run"], _halo(geo), blocks=kind == "walkers")
    assert all(cov.values()), (route, d["run"], [k for k, v in cov.items() if not v])


def _same_bits(route, a, b, zero, tag, bad):
    signs = 0
    for st in OUTS:
        m, sg = _bit_mismatches(a[st], b[st], zero.get(st))
        signs += sg
        if m:
            bad.append((tag, st, m))
    for st in ("note_mag", "note_peak"):
        m, _ = _bit_mismatches(a[st], b[st])
        if m:
            bad.append((tag, st, m))
    return signs


@pytest.mark.parametrize("route,run", [(r, n) for r, runs in TRUTH_RUNS.items() for n in runs])
def test_long_runs_against_the_float64_truth(ctx, route, run):
    geo, opts, names, kind, has_skip = ROUTES[route]
    try:
        _set(ctx, opts)
        d = _walk(ctx, route, run, views=True, profile=True)
    finally:
        ctx.set_option("walk_run", 0)
        _restore(ctx)
    assert d["names"] == names
    assert (d["frame_skip"] is not None and d["frame_skip"].size > 0) == has_skip
    assert d["run"] == run
    _covered(route, d)
    tally = Tally("%s/run%d" % (route, run))
    skipped = judge_notes(d, _notes(geo), geo, SIGMA, "long", kind, has_skip, tally)
    tally.report()
    if has_skip:
        print("frame_skip: unvoiced %d  breath %d  neither %d of %d" % (skipped[1], skipped[2], skipped[0], int(d["f_off"][-1])))
        assert skipped[1] > 0 and skipped[2] > 0 and skipped[0] > 0
    assert not tally.bad, tally.bad[:12]


@pytest.mark.parametrize("route", list(BIT_RUNS))
def test_the_run_changes_no_bit(ctx, route):
    geo, opts, names, kind, has_skip = ROUTES[route]
    zero = _zero_gain(_notes(geo), SIGMA) if kind == "walkers" else {}
    bad, signs = [], 0
    try:
        _set(ctx, opts)
        base = _walk(ctx, route, 0)
        for run in BIT_RUNS[route]:
            d = _walk(ctx, route, run)
            assert d["run"] == run
            _covered(route, d)
            signs += _same_bits(route, base, d, zero, run, bad)
    finally:
        ctx.set_option("walk_run", 0)
        _restore(ctx)
    print("%s: %d zero-sign differences under a zero fp32 gain" % (route, signs))
    assert not bad, (route, bad)


def test_philox_phases_at_long_runs(ctx):
    """The production noise path: no injected phases, the walker draws them, and the Nyquist bin's word with the frame records."""
    geo = ROUTES["walkers"][0]
    zero = _zero_gain(_notes(geo), SIGMA)
    bad, signs = [], 0
    try:
        _set(ctx, {})
        base = _walk(ctx, "walkers", 0, seed=20240611)
        assert np.any(base["uv"]) and np.any(base["bre"])
        for run in (65, 128):
            d = _walk(ctx, "walkers", run, seed=20240611)
            _covered("walkers", d)
            signs += _same_bits("walkers", base, d, zero, run, bad)
    finally:
        ctx.set_option("walk_run", 0)
        _restore(ctx)
    print("philox: %d zero-sign differences under a zero fp32 gain" % signs)
    assert not bad, bad


RENDER_FLAGS = ["fa30fb-20fc10fd-10V80B20U-30", "t0g0", "g20fb30", "V80B20U-30br20", "fa-25fc20B40", "t-7fst40"]   # warping, plain, ...
RENDER_MS = [500, 800, 1100, 1300, 1500, 1600]                # 104, 156, 207, 242, 276 and 293 frames at 44100 / 256
TOL = 1e-4                                                    # tests/test_gpu_hard.py


def test_render_path_at_long_runs(ctx):
    """goofer_render_batch: the harmonic walker reads warped copies of the warping notes' rows and the assembled rows of the
    others (frame_block::mark_plain), so warping and plain notes alternate across the record refills."""
    from conftest import rms_err
    from goofer_amd import sampler as S
    from goofer_amd import synthetic as syn
    from goofer_amd.render import Renderer, Source
    from oracle import sampler_ref as OR
    jobs, feats, reqs, seeds = [], [], [], []
    for i, (flags, ms) in enumerate(zip(RENDER_FLAGS, RENDER_MS)):
        src = syn.make_hard_source(7100 + i, seconds=0.6)
        req = syn.make_request(7100 + i, flags, length_ms=float(ms))
        jobs.append((Source.from_pack(src["env_pack"], src["f0"], src["mask"], src["formants"], src["sr"], src["y_len"]),
                     S.decode_request(*syn.request_args(req))))
        feats.append((src["env_pack"], src["f0"].copy(), src["mask"].copy(), {k: v.copy() for k, v in src["formants"].items()},
                      src["sr"], src["y_len"]))
        reqs.append(req)
        seeds.append(7700 + i)
    r = Renderer(ctx)
    res = {}
    try:
        _set(ctx, {})
        for run in (0, 65, 128):
            ctx.set_option("walk_run", run)
            try:
                outs, parts = r.render(jobs, phi_seeds=seeds, return_parts=True)
                torch.cuda.synchronize()
            except RuntimeError as e:                         # nothing more is started on this GPU
                pytest.exit("goofer_render_batch failed on the device: %r" % (e,), returncode=3)
            want = 32 if run == 0 else run
            assert ctx.counter("walk_run_noise") == want and ctx.counter("walk_run_harm") == want
            stems = {k: parts["stems"][k].cpu().numpy() for k in ("harm", "uv", "bre", "mix")}
            res[run] = (outs, stems, np.asarray(parts["sample_off"]))
    finally:
        ctx.set_option("walk_run", 0)
        _restore(ctx)
    s_off = res[0][2]
    frames = [1 + int(n) // 256 for n in np.diff(s_off)]
    assert all(100 <= t <= 300 for t in frames), frames
    f_off = np.concatenate([[0], np.cumsum(frames)])
    for run in (65, 128):                                     # a refill inside a note and the clamped last block, at least
        cov = SR.run_coverage(f_off, run, 3, blocks=True)
        assert cov["refill_inside"] and cov["final_block"] and cov["3_runs"] and cov["t0>halo"], (run, cov)
    bad, signs = [], 0
    for run in (65, 128):
        for k in ("harm", "uv", "bre", "mix"):
            # (the zero-sign allowance: wherever both are zero on the two noise stems — the gain there is not restated on the host)
            zero_ok = np.ones(res[0][1][k].shape, bool) if k in ("uv", "bre") else None
            m, sg = _bit_mismatches(res[0][1][k], res[run][1][k], zero_ok)
            signs += sg
            if m:
                bad.append((run, k, m))
        for i, (a, b) in enumerate(zip(res[0][0], res[run][0])):
            if _bit_mismatches(a, b)[0]:
                bad.append((run, "out", i))
    print("render: %d zero-sign differences" % signs)
    assert not bad, bad
    errs = []
    for i, (o, f, req) in enumerate(zip(res[128][0], feats, reqs)):
        ref = OR.render(f, OR.decode_request(*syn.request_args(req)), seed=seeds[i], n_fft=1024, hop=256)
        assert o.shape == ref.shape and np.isfinite(o).all(), i
        errs.append(rms_err(o, ref) / max(1.0, float(np.max(np.abs(ref)))))
    print("render at walk_run 128 vs oracle: %s" % ["%.2e" % e for e in errs])
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("route", ["walkers", "ola1_hop96"])
def test_walk_run_is_clamped_to_the_automatic_range(ctx, route):
    geo, opts, names, kind, has_skip = ROUTES[route]
    counters, cap = WALKERS[route]
    zero = _zero_gain(_notes(geo), SIGMA) if kind == "walkers" else {}
    bad = []
    try:
        _set(ctx, opts)
        base = _walk(ctx, route, 0)
        lo = _walk(ctx, route, 1)
        hi = _walk(ctx, route, 100000)
        assert lo["run"] == _floor(geo) and hi["run"] == cap and base["run"] == _floor(geo)
        assert _floor(geo) == {"walkers": 32, "ola1_hop96": 168}[route]
        _same_bits(route, base, lo, zero, "floor", bad)
        _same_bits(route, base, hi, zero, "cap", bad)
    finally:
        ctx.set_option("walk_run", 0)
        _restore(ctx)
    assert not bad, (route, bad)
