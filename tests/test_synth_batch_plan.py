"""core.synthesize_batch without a device: pass planning, call-level errors and per-note refusals."""
import numpy as np
import pytest

from goofer_amd import core


def _keys(kws):
    return [core.synth_pass_key({**core._synth_defaults(), **kw}) for kw in kws]


def test_common_case_is_one_pass():
    rng = np.random.default_rng(0)
    kws = [{"pitch_shift": float(rng.uniform(0.5, 2.0)), "formant_shift": float(rng.uniform(0.8, 1.2)),
            "F1_shift": float(rng.uniform(0.8, 1.2)), "uv_strength": float(rng.uniform(0, 1)), "breath_strength": 0.2,
            "normalize": float(rng.uniform(0, 1)), "apply_brightness": bool(i % 2), "cut_subharm_below_f0": bool(i % 3),
            "f0_jitter": bool(i % 2), "f0_jitter_strength": float(rng.uniform(0.1, 2.0))} for i in range(64)]
    assert core.plan_synth_passes(_keys(kws), [200] * 64) == [list(range(64))]


def test_call_settings_split_passes():
    kws = [{}, {"noise_transition_smoothness": 50}, {}, {"add_subharm": True}, {"add_subharm": True, "subharm_semitones": -24},
           {"add_subharm": True}, {"volume_jitter": True}, {"volume_jitter": True, "volume_vibrato": True}]
    assert core.plan_synth_passes(_keys(kws), [10] * len(kws)) == [[0, 2], [1], [3, 5], [4], [6], [7]]


def test_unused_jitter_speeds_do_not_split():
    kws = [{"f0_jitter_speed": 30}, {"volume_jitter_speed": 12}, {"f0_jitter": True, "f0_jitter_speed": 70}, {},
           {"f0_jitter": True, "f0_jitter_speed": 70}, {"f0_jitter": True, "f0_jitter_speed": 20}]
    assert core.plan_synth_passes(_keys(kws), [10] * len(kws)) == [[0, 1, 2, 3, 4], [5]]


def test_stretched_notes_get_their_own_passes_and_phases_split():
    keys = _keys([{}, {"stretch_factor": 1.3}, {}, {"stretch_factor": 0.7, "pitch_shift": 1.5}])
    keys.append(core.synth_pass_key(core._synth_defaults(), has_phi=True))
    assert core.plan_synth_passes(keys, [10] * 5) == [[0, 2], [1, 3], [4]]


def test_frame_budget_cuts_and_skipped_notes():
    keys = _keys([{}] * 6)
    keys[2] = None                                            # a refused note renders nothing
    assert core.plan_synth_passes(keys, [40, 40, 999, 40, 100, 10], frame_budget=100) == [[0, 1], [3], [4], [5]]


def _note(n=1000, T=None, **kw):
    T = 1 + n // 256 if T is None else T
    return {"env_spec": np.ones((513, T), np.float32), "f0_interp": np.full(n, 200, np.float32),
            "voicing_mask": np.ones(n, np.float32), "y": np.zeros(n), **kw}


@pytest.mark.parametrize("call", [
    lambda: core.synthesize_batch([_note()], 44100, bogus=1),
    lambda: core.synthesize_batch([_note(pitchshift=2.0)], 44100),
    lambda: core.synthesize_batch([_note(), _note()], 44100, seeds=[1]),
    lambda: core.synthesize_batch([_note()], 44100, phis=[None, None]),
    lambda: core.synthesize_batch([{"env_spec": None, "f0_interp": None, "y": []}], 44100),
])
def test_call_level_errors_raise_before_any_draw(call):
    np.random.seed(5)
    before = np.random.get_state()
    with pytest.raises((TypeError, ValueError)):
        call()
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_unknown_keyword_message_matches_synthesize():
    with pytest.raises(TypeError, match=r"synthesize\(\) got an unexpected keyword argument 'bogus'"):
        core.synthesize_batch([_note()], 44100, bogus=1)


class _HostOnly:
    """A context stand-in: planning only.  Every note below is refused (or empty) before any device work."""
    n_bins = 513

    def plan(self, *a):
        return self


def test_per_note_refusals_land_in_their_slots():
    notes = [_note(stretch_factor=1.3, start_sec=0.5, end_sec=0.5),                          # empty stretch region
             _note(add_subharm=True, subharm_semitones=list(range(-20, -3))),               # 17 ratios
             {**_note(), "f0_interp": np.ones((2, 1000), np.float32)},                      # 2-D f0
             _note(n=0),                                                                    # nothing to render
             _note(stretch_factor=1.3, start_sec=0.0, end_sec=0.001, T=3)]                  # empty envelope region
    np.random.seed(9)
    before = np.random.get_state()
    res = core.synthesize_batch(notes, 44100, ctx=_HostOnly())
    assert isinstance(res[0], ValueError) and str(res[0]) == "x cannot be empty"
    assert isinstance(res[1], NotImplementedError)
    assert isinstance(res[2], ValueError)
    assert len(res[3]) == 4 and all(a.dtype == np.float32 and a.size == 0 for a in res[3])
    assert isinstance(res[4], ValueError) and str(res[4]) == "x cannot be empty"
    assert all(np.array_equal(a, b) for a, b in zip(before, np.random.get_state()))      # refused notes draw nothing
