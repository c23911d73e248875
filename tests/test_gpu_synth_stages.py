"""GPU: goofer_synth_batch stage by stage, unit by unit, on every route, against the float64 restatement of tests/synth_ref.py.

One ragged batch per geometry and transition sigma (synth_ref.batches: about sixty notes of at most 36 frames, two batches of
their own for the sigmas 4 and 2000, seventy notes of one to nine samples followed by a long one), injected phases, then
goofer_debug_fetch.  The device's own pulse train — first held to R.pulse_train within the 5e-6 of tests/test_gpu_kernels.py — is
the input of the truth and of both yardsticks, and every stage behind the spectra is fed the DEVICE's spectra, note_mag and mask
knots, so it is judged on its own error:

  e_gpu <= FACTOR * E_ref + 2^-23   per unit (envelope row, spectrum row, time frame, note of samples)

peak = the largest |truth| of the unit; E_ref = the note's worst unit, the larger of the oracle's arithmetic and of the same with
a plain radix-2 fp32 transform (synth_ref.fft_plain), both from the CPU restatement, never from a device run.  No RMS; no bin,
frame or sample left out; a unit whose truth is all zero must be all zero.  f0 is bit-equal.  mask_short has its derived bound
(2 r + 1) 2^-53 truth + 2^-1074 against a long-double truth.  note_mag / note_peak inherit the bound of what they reduce, relative
to themselves.

Routes (asserted through profile_stage_names; the names tell the walkers, the fused option and its absence apart, the debug views
the rest: frame_skip exists only on the k_irfft_ola1 + k_frame_skip route, and `frames` is only written — and here judged — where
the separate kernels run):
  walkers / td_blur 0 / skip_zero 0   (44100, 1024, 256)   final stems, note_mag, note_peak, rec, mix; env_harm (k_warp_bins)
  stems 0: k_irfft_ola3               (44100, 1024, 256)   + S_harm, S_uv, S_breath, mask_short
  fused_ola 0: separate kernels       (44100, 1024, 256)   + frames
  k_irfft_ola3<256>                   (22050, 512, 128)
  k_irfft_ola1 + k_frame_skip         (44100, 2048, 512), (96000, 2048, 96: hop != n_fft / 4)
  separate kernels: factor three      (44100, 768, 192); Bluestein (44100, 1000, 250); workgroup transform (48000, 4096, 1024)
  ... and the other forms of with_transform (csrc/fft.hip), each through the separate kernels with `frames` judged:
      bluestein_256    (16000, 130, 40)     wave, Bluestein L = 256 (66 bins: an even count)
      bluestein_512    (22050, 320, 80)     wave, Bluestein L = 512
      bluestein_2048   (44100, 2046, 512)   wave, Bluestein L = 2048, 32 points per lane (1024 bins: an even count)
      bluestein_wg     (48000, 3000, 750)   workgroup, Bluestein L = 4096, tables re-read per frame
      radix3_1536      (44100, 1536, 384)   wave, native 768 points (12-point first pass)
  Every geometry above that is not (.., 1024, 256) or n_fft 2048 reports the stage names of the one-kernel overlap-add (OLA:
  the names follow the option, fused_ola 1) and runs the separate transforms + k_ola3_gains: the `frames` view is written.
The views env_harm (spectra routes) and env_noise (every route) are carved but never written: the warp and the sigma-1.75 blur are
folded into k_harm_shape / k_noise_spectra, so those two are judged through S_harm and S_uv (|S_uv| = env_noise bin by bin).

The frame_skip check: a frame marked skipped must have, over every sample it reaches, a truth gain whose fp32 value is exactly
zero — F32(ms) for breath, 1.0f - F32(ms) for unvoiced (the reference takes 1 - ms on the fp32 mask; in float64 an all-ones mask
smooths to 1 - 1e-16, never to 1).

What these small batches reach of the walkers (csrc/stems.hip) and what they leave to tests/test_gpu_fullsize.py: a batch here has
about 1 100 frames (main), 150-250 (the others), so frame_block splits it into many runs that START and END inside notes (halo
replay, the flush of a note's last hops by the wave that owns its last frame, runs that hold several whole notes: the seventy
tiny ones).  run_length stays at its floor of 32 frames per wave (no batch here fills the device's wave slots), so with notes of
up to 36 frames a run ends inside a note and the next one replays its halo; frame_block::load runs once per wave and its refill
after 64 frames is NOT reached.  tests/test_gpu_walker_runs.py forces the runs of a full-size batch (option "walk_run": 61 to 128
frames per wave, 256 for k_irfft_ola1) on a batch of under 2 000 frames with notes of up to 303 frames and judges them with this
file's judge_notes(): the 64-frame record refill with its load_nyquist / mark_plain, the clamp of a block that reaches past the
last frame, runs of several long notes and notes longer than a run.  What remains with tests/test_gpu_fullsize.py: the grid that
fills the device a whole number of times (the automatic run above its floor) and offsets at the 2^31 scale.

MEASURED on the MI355X: worst note per route and stage over the four batches, E_ref / e_gpu (ratio = (e_gpu - 2^-23) / E_ref, floored
at 0).  Every stage holds the project's factor 3 — the largest ratio is 2.00 — so no factor was raised.  Left out of the figures, not
of the assertion: the unvoiced stem of an all-voiced note, whose truth is the transform times 1 - ms = 1e-16 and which every fp32
arithmetic (the oracle's too) makes exactly zero, E_ref = e_gpu = 1.
  walkers
      env_harm  6.0e-08 / 9.6e-08 (0.00)   note_mag  1.7e-07 / 1.3e-07 (0.06)   harm      2.0e-07 / 3.2e-07 (1.02)
      uv        1.9e-07 / 3.8e-07 (1.38)   bre       2.1e-07 / 4.0e-07 (1.30)   rec       2.3e-07 / 3.5e-07 (1.03)
      mix       1.8e-07 / 4.1e-07 (1.62)   note_peak 2.3e-07 / 3.0e-07 (0.79)
  walkers, td_blur 0
      env_harm  6.0e-08 / 9.6e-08 (0.00)   note_mag  1.7e-07 / 1.3e-07 (0.06)   harm      2.0e-07 / 3.2e-07 (1.01)
      uv        1.9e-07 / 3.8e-07 (1.38)   bre       2.1e-07 / 4.0e-07 (1.30)   rec       2.3e-07 / 3.5e-07 (1.03)
      mix       1.6e-07 / 2.9e-07 (1.08)   note_peak 2.3e-07 / 3.0e-07 (0.79)
  walkers, skip_zero 0
      env_harm  6.0e-08 / 9.6e-08 (0.00)   note_mag  1.7e-07 / 1.3e-07 (0.06)   harm      2.0e-07 / 3.2e-07 (1.02)
      uv        1.9e-07 / 3.8e-07 (1.38)   bre       2.1e-07 / 4.0e-07 (1.30)   rec       2.3e-07 / 3.5e-07 (1.03)
      mix       1.8e-07 / 4.1e-07 (1.62)   note_peak 2.3e-07 / 3.0e-07 (0.79)
  stems 0: k_irfft_ola3
      S_harm    2.2e-07 / 3.2e-07 (0.90)   S_uv      9.5e-08 / 2.8e-07 (1.70)   S_breath  6.3e-08 / 2.2e-07 (1.67)
      note_mag  1.7e-07 / 1.3e-07 (0.06)   harm      1.3e-07 / 2.8e-07 (1.25)   uv        2.9e-07 / 4.2e-07 (1.05)
      bre       1.5e-07 / 3.2e-07 (1.31)   rec       1.7e-07 / 2.9e-07 (1.04)   mix       1.5e-07 / 2.7e-07 (1.03)
      note_peak 1.5e-07 / 2.2e-07 (0.69)
  fused_ola 0: separate kernels
      S_harm    2.2e-07 / 3.2e-07 (0.90)   S_uv      9.5e-08 / 2.8e-07 (1.70)   S_breath  6.3e-08 / 2.2e-07 (1.67)
      note_mag  1.7e-07 / 1.3e-07 (0.06)   frames    1.7e-07 / 2.9e-07 (1.02)   harm      1.3e-07 / 2.8e-07 (1.25)
      uv        2.9e-07 / 4.2e-07 (1.05)   bre       1.5e-07 / 3.2e-07 (1.31)   rec       1.7e-07 / 2.9e-07 (1.04)
      mix       1.5e-07 / 2.7e-07 (1.03)   note_peak 1.5e-07 / 2.2e-07 (0.69)
  22050/512/128: k_irfft_ola3<256>
      S_harm    3.6e-07 / 7.2e-07 (1.66)   S_uv      9.7e-08 / 2.9e-07 (1.71)   S_breath  5.4e-08 / 1.9e-07 (1.31)
      note_mag  3.4e-07 / 2.4e-07 (0.35)   harm      1.7e-07 / 2.8e-07 (0.96)   uv        1.8e-07 / 2.7e-07 (0.82)
      bre       2.2e-07 / 3.0e-07 (0.82)   rec       1.7e-07 / 2.4e-07 (0.73)   mix       1.9e-07 / 2.9e-07 (0.95)
      note_peak 1.4e-07 / 1.6e-07 (0.30)
  44100/2048/512: k_irfft_ola1 + k_frame_skip
      S_harm    3.7e-07 / 4.0e-07 (0.74)   S_uv      8.5e-08 / 2.8e-07 (1.90)   S_breath  9.3e-08 / 3.1e-07 (2.00)
      note_mag  1.4e-07 / 2.3e-07 (0.82)   harm      1.8e-07 / 3.1e-07 (1.06)   uv        2.2e-07 / 3.2e-07 (0.91)
      bre       2.7e-07 / 3.5e-07 (0.87)   rec       1.4e-07 / 2.7e-07 (1.11)   mix       2.4e-07 / 3.8e-07 (1.10)
      note_peak 2.0e-07 / 1.8e-07 (0.29)
  96000/2048/96: k_irfft_ola1
      S_harm    1.7e-07 / 2.8e-07 (0.98)   S_uv      6.7e-08 / 2.3e-07 (1.60)   S_breath  1.2e-07 / 3.1e-07 (1.54)
      note_mag  1.5e-07 / 1.9e-07 (0.44)   harm      2.7e-07 / 3.9e-07 (1.03)   uv        2.5e-07 / 4.5e-07 (1.29)
      bre       2.3e-07 / 3.5e-07 (1.03)   rec       2.3e-07 / 4.6e-07 (1.45)   mix       3.3e-07 / 4.6e-07 (1.05)
      note_peak 2.8e-07 / 2.5e-07 (0.48)
  44100/768/192: separate, factor three
      S_harm    3.2e-07 / 3.5e-07 (0.73)   S_uv      9.3e-08 / 2.5e-07 (1.43)   S_breath  1.1e-07 / 2.9e-07 (1.58)
      note_mag  3.2e-07 / 2.0e-07 (0.27)   frames    2.7e-06 / 5.4e-06 (1.93)   harm      1.4e-07 / 3.6e-07 (1.70)
      uv        2.7e-07 / 3.5e-07 (0.85)   bre       2.6e-07 / 3.9e-07 (1.04)   rec       1.8e-07 / 3.8e-07 (1.46)
      mix       1.9e-07 / 3.8e-07 (1.39)   note_peak 2.3e-07 / 2.0e-07 (0.36)
  44100/1000/250: Bluestein
      S_harm    3.3e-07 / 3.9e-07 (0.82)   S_uv      6.7e-08 / 2.4e-07 (1.85)   S_breath  5.6e-08 / 2.1e-07 (1.63)
      note_mag  3.4e-07 / 1.9e-07 (0.20)   frames    3.2e-07 / 6.5e-07 (1.64)   harm      2.1e-07 / 2.9e-07 (0.85)
      uv        2.5e-07 / 5.1e-07 (1.57)   bre       2.1e-07 / 3.2e-07 (0.95)   rec       2.3e-07 / 3.1e-07 (0.86)
      mix       2.2e-07 / 3.1e-07 (0.86)   note_peak 2.7e-07 / 1.7e-07 (0.19)
  48000/4096/1024: workgroup transform
      S_harm    2.0e-07 / 3.0e-07 (0.93)   S_uv      9.2e-08 / 2.7e-07 (1.68)   S_breath  8.7e-08 / 2.6e-07 (1.64)
      note_mag  2.1e-07 / 2.1e-07 (0.42)   frames    1.6e-07 / 2.4e-07 (0.73)   harm      1.5e-07 / 2.7e-07 (0.97)
      uv        1.5e-07 / 2.7e-07 (0.97)   bre       2.2e-07 / 3.8e-07 (1.15)   rec       1.7e-07 / 3.1e-07 (1.16)
      mix       2.0e-07 / 3.3e-07 (1.02)   note_peak 1.5e-07 / 1.9e-07 (0.47)
The five transform forms added later (the largest ratio is 2.32, still inside the factor 3 with both yardsticks of synth_ref:
no third yardstick was needed for the Bluestein stages and no factor was raised):
  16000/130/40: Bluestein L = 256
      S_harm    5.5e-07 / 8.8e-07 (1.39)   S_uv      8.9e-08 / 3.3e-07 (2.32)   S_breath  6.3e-08 / 2.5e-07 (2.12)
      note_mag  2.6e-07 / 2.2e-07 (0.36)   frames    2.6e-07 / 4.4e-07 (1.24)   harm      1.2e-07 / 3.1e-07 (1.62)
      uv        2.1e-07 / 3.5e-07 (1.12)   bre       1.8e-07 / 3.4e-07 (1.23)   rec       1.2e-07 / 2.7e-07 (1.23)
      mix       1.4e-07 / 3.3e-07 (1.53)   note_peak 2.1e-07 / 3.1e-07 (0.89)
  22050/320/80: Bluestein L = 512
      S_harm    3.3e-07 / 3.4e-07 (0.65)   S_uv      5.4e-08 / 2.3e-07 (2.11)   S_breath  5.4e-08 / 2.3e-07 (2.11)
      note_mag  2.8e-07 / 1.9e-07 (0.27)   frames    5.7e-07 / 9.8e-07 (1.50)   harm      1.8e-07 / 2.9e-07 (0.96)
      uv        1.7e-07 / 3.4e-07 (1.34)   bre       1.4e-07 / 2.9e-07 (1.15)   rec       1.4e-07 / 2.7e-07 (1.13)
      mix       1.4e-07 / 2.5e-07 (0.94)   note_peak 1.5e-07 / 2.2e-07 (0.71)
  44100/2046/512: Bluestein L = 2048
      S_harm    2.6e-07 / 3.3e-07 (0.81)   S_uv      8.6e-08 / 2.5e-07 (1.54)   S_breath  1.2e-07 / 3.2e-07 (1.66)
      note_mag  1.8e-07 / 1.7e-07 (0.30)   frames    5.4e-07 / 8.9e-07 (1.42)   harm      2.0e-07 / 3.4e-07 (1.13)
      uv        2.1e-07 / 3.9e-07 (1.27)   bre       2.1e-07 / 3.3e-07 (1.02)   rec       1.4e-07 / 3.4e-07 (1.62)
      mix       1.8e-07 / 3.4e-07 (1.19)   note_peak 1.7e-07 / 2.7e-07 (0.88)
  48000/3000/750: workgroup, Bluestein L = 4096
      S_harm    1.9e-07 / 3.5e-07 (1.23)   S_uv      9.8e-08 / 2.8e-07 (1.58)   S_breath  1.1e-07 / 2.7e-07 (1.38)
      note_mag  1.9e-07 / 2.4e-07 (0.64)   frames    2.3e-07 / 3.4e-07 (0.95)   harm      1.7e-07 / 2.9e-07 (1.07)
      uv        2.6e-07 / 3.8e-07 (1.01)   bre       2.2e-07 / 3.4e-07 (1.01)   rec       2.0e-07 / 3.4e-07 (1.06)
      mix       1.5e-07 / 3.0e-07 (1.21)   note_peak 2.2e-07 / 2.9e-07 (0.78)
  44100/1536/384: native 768 points
      S_harm    3.8e-07 / 5.1e-07 (1.02)   S_uv      9.8e-08 / 2.6e-07 (1.45)   S_breath  1.2e-07 / 2.7e-07 (1.31)
      note_mag  3.3e-07 / 2.1e-07 (0.27)   frames    6.2e-07 / 5.9e-07 (0.76)   harm      2.0e-07 / 2.8e-07 (0.82)
      uv        2.7e-07 / 3.6e-07 (0.89)   bre       2.1e-07 / 3.0e-07 (0.86)   rec       1.5e-07 / 2.6e-07 (0.98)
      mix       2.0e-07 / 3.0e-07 (0.90)   note_peak 2.7e-07 / 2.0e-07 (0.31)
The three inputs of the LDS-ring walkers that no table reached (the largest ratio is 2.00; the same figures under the build
before the walkers moved onto csrc/ola_walk.h and after, whose bits are the same):
  44100/2048/512, stems 0: k_irfft_ola3<1024>, eight register slots per hop
      S_harm    3.7e-07 / 4.0e-07 (0.74)   S_uv      8.5e-08 / 2.8e-07 (1.90)   S_breath  9.3e-08 / 3.1e-07 (2.00)
      note_mag  1.4e-07 / 2.3e-07 (0.82)   harm      1.8e-07 / 3.1e-07 (1.06)   uv        2.2e-07 / 3.2e-07 (0.91)
      bre       2.7e-07 / 3.5e-07 (0.87)   rec       1.4e-07 / 2.7e-07 (1.11)   mix       2.4e-07 / 3.8e-07 (1.10)
      note_peak 2.0e-07 / 1.8e-07 (0.29)
  44100/1024/512: k_irfft_ola3<512>, a hop wider than its slots (halo 1)
      S_harm    2.3e-07 / 2.9e-07 (0.74)   S_uv      9.2e-08 / 2.6e-07 (1.56)   S_breath  7.3e-08 / 2.3e-07 (1.55)
      note_mag  1.9e-07 / 1.7e-07 (0.29)   harm      2.3e-07 / 4.3e-07 (1.35)   uv        2.7e-07 / 3.7e-07 (0.91)
      bre       2.1e-07 / 3.6e-07 (1.16)   rec       2.0e-07 / 3.9e-07 (1.37)   mix       1.8e-07 / 3.9e-07 (1.50)
      note_peak 2.0e-07 / 2.8e-07 (0.81)
  44100/2048/1024: k_irfft_ola1, knots from global memory, no frame_skip (halo 1)
      S_harm    1.7e-07 / 3.2e-07 (1.18)   S_uv      9.8e-08 / 2.7e-07 (1.49)   S_breath  1.0e-07 / 2.8e-07 (1.55)
      note_mag  1.6e-07 / 2.1e-07 (0.56)   harm      1.0e-07 / 2.1e-07 (0.87)   uv        2.0e-07 / 3.0e-07 (0.91)
      bre       1.9e-07 / 3.0e-07 (0.97)   rec       2.5e-07 / 3.2e-07 (0.80)   mix       1.9e-07 / 2.8e-07 (0.85)
      note_peak 2.5e-07 / 1.9e-07 (0.30)
"""
import numpy as np
import pytest

import synth_ref as SR
from oracle import goofer_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32, F64 = np.float32, np.float64
G0 = (44100, 1024, 256)

_HEAD = ["setup_maps", "", "", "phase_inc", "pulse_onsets", "pulse_place"]
_TAIL = ["env_edit", "env_rows", "sample_assemble"]
STEMS = _HEAD + ["mask_short", "noise_stems", "", "harm_stem", "", "", "", "note_finish", ""] + _TAIL
OLA = _HEAD + ["rfft_frames", "harm_shape", "", "noise_spectra", "", "", "mask_short", "irfft_ola3", "apply_gain"] + _TAIL
SEPARATE = _HEAD + ["rfft_frames", "harm_shape", "irfft_harm", "noise_spectra", "irfft_breath", "irfft_unvoiced", "mask_short",
                    "ola3_gains", "apply_gain"] + _TAIL

# route: (geometry, options, stage names, kind, frame_skip view)
ROUTES = {
    "walkers": (G0, {}, STEMS, "walkers", False),
    "walkers_td_blur0": (G0, {"td_blur": 0}, STEMS, "walkers", False),
    "walkers_skip_zero0": (G0, {"skip_zero": 0}, STEMS, "walkers", False),
    "ola3": (G0, {"stems": 0}, OLA, "fused", False),
    "separate": (G0, {"fused_ola": 0}, SEPARATE, "separate", False),
    "ola3_256": ((22050, 512, 128), {}, OLA, "fused", False),
    "ola1_skip": ((44100, 2048, 512), {}, OLA, "fused", True),
    "ola1_hop96": ((96000, 2048, 96), {}, OLA, "fused", True),
    "ola3_2048": ((44100, 2048, 512), {"stems": 0}, OLA, "fused", False),      # k_irfft_ola3<1024>: eight register slots per hop
    "ola3_wide": ((44100, 1024, 512), {}, OLA, "fused", False),               # a hop wider than k_irfft_ola3's slots (halo 1)
    "ola1_wide": ((44100, 2048, 1024), {}, OLA, "fused", False),              # k_irfft_ola1, knots from global memory, no frame_skip
    "radix3": ((44100, 768, 192), {}, OLA, "separate", False),
    "bluestein": ((44100, 1000, 250), {}, OLA, "separate", False),
    "workgroup": ((48000, 4096, 1024), {}, OLA, "separate", False),
    "bluestein_256": ((16000, 130, 40), {}, OLA, "separate", False),
    "bluestein_512": ((22050, 320, 80), {}, OLA, "separate", False),
    "bluestein_2048": ((44100, 2046, 512), {}, OLA, "separate", False),
    "bluestein_wg": ((48000, 3000, 750), {}, OLA, "separate", False),
    "radix3_1536": ((44100, 1536, 384), {}, OLA, "separate", False),
}
DEFAULTS = {"td_blur": 1, "skip_zero": 1, "stems": 1, "fused_ola": 1}
BATCHES = ("main", "sigma4", "sigma2000", "tiny")

# The factor of every stage is the project's 3.  (A stage that needs another one gets it here, with its cause beside it.)
FACTOR = {}

_matrix, _from_pulse = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from goofer_amd.device import Context
    c = Context(0)
    yield c
    for k, v in DEFAULTS.items():
        c.set_option(k, v)
    c.close()


def _batches(geo):
    if geo not in _matrix:
        _matrix[geo] = SR.batches(geo)
    return _matrix[geo]


def _params(notes):
    from goofer_amd.core import note_params_from_kwargs
    par = np.concatenate([note_params_from_kwargs(1, **c["kw"]) for c in notes])
    for k, c in enumerate(notes):
        for name, v in dict(SR.MIX_DEFAULT, **c["mix"]).items():
            par[name][k] = v
    return par


def _run(ctx, geo, notes, sigma, views=True, profile=False, seed=None, device=False):
    """One goofer_synth_batch over ``notes``; the outputs and (views) the debug views as host arrays.  ``seed``: no phases are
    injected, the noise walker draws its own (Philox) under this seed.  ``device``: the five outputs stay device tensors (a
    caller that compares them there: tests/test_gpu_repeat.py)."""
    from goofer_amd.device import GooferError
    sr, n_fft, hop = geo
    nb = n_fft // 2 + 1
    ctx.plan(*geo)
    lens = [c["n"] for c in notes]
    env_len = [c["env"].shape[1] for c in notes]
    env = ctx.rows_from(np.concatenate([c["env"].T for c in notes]))
    forms = ctx.tensor(np.concatenate([SR.formant_rows(c).T for c in notes]).astype(F64))
    phi = ctx.rows_from(np.concatenate([c["phi"].T for c in notes])) if seed is None else None
    if profile:
        ctx.profile_begin(1)
    try:
        out = ctx.synth_batch(env, env_len, ctx.tensor(np.concatenate([c["f0"] for c in notes])),
                              ctx.tensor(np.concatenate([c["mask"] for c in notes])), lens, _params(notes), formants=forms, phi=phi,
                              seed=seed or 0, transition_sigma=sigma)
        torch.cuda.synchronize()
    except RuntimeError as e:                                 # GooferError or torch's device error: nothing more is started on this GPU
        pytest.exit("goofer_synth_batch failed on the device: %r" % (e,), returncode=3)
    res = {k: out[k] if device else out[k].cpu().numpy() for k in ("harm", "uv", "bre", "rec", "mix")}
    if profile:
        ctx.profile_end()
        res["names"] = ctx.profile_stage_names()
    ctx.check()
    res["s_off"], res["f_off"] = out["sample_off"], out["frame_off"]
    if views:
        F = int(out["frame_off"][-1])
        ld = env.stride(0)
        for name in ("f0", "pulse", "mask_short", "note_mag", "note_peak"):
            res[name] = ctx.debug_fetch(name)
        res["env_harm"] = ctx.debug_fetch("env_harm").reshape(F, ld)[:, :nb]
        for name in ("S_harm", "S_uv", "S_breath"):
            v = ctx.debug_fetch(name)
            res[name] = v.reshape(F, SR_STRIDE(nb))[:, :nb] if v.size else None
        v = ctx.debug_fetch("frames")
        res["frames"] = v.reshape(F, n_fft) if v.size else None
        try:
            res["frame_skip"] = ctx.debug_fetch("frame_skip")
        except GooferError:                                   # EINVAL: the route carves no such view
            res["frame_skip"] = None
    return res


def SR_STRIDE(nb):
    from goofer_amd.device import spec_stride
    return spec_stride(nb)


def _set(ctx, opts):
    for k, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(k, v)


def _restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.plan(*G0)


def _three(case, geo, sigma, pulse, given=None):
    """(truth, oracle arithmetic, the same with the plain fp32 transform) of one note."""
    with np.errstate(all="ignore"):
        return tuple(SR.synth_note(case, geo, exact=ex, fft=fft, pulse=pulse, given=given, sigma=sigma)
                     for ex, fft in ((True, "numpy"), (False, "numpy"), (False, "plain")))


def _pulse_runs(geo, batch, k, case, sigma, pulse):
    key = (geo, batch, k)
    hit = _from_pulse.get(key)
    if hit is None or not np.array_equal(hit[0], pulse):
        hit = _from_pulse[key] = (pulse.copy(), _three(case, geo, sigma, pulse))
    return hit[1]


class Tally:
    def __init__(self, tag):
        self.tag, self.worst, self.bad, self.vacuous = tag, {}, [], {}

    def add(self, stage, note, e, E):
        f = FACTOR.get(stage, 3.0)
        ratio = max(0.0, (e - SR.EPS32) / E) if E > 0 else (0.0 if e <= SR.EPS32 else np.inf)
        if E >= 0.5:                                          # a stem under a gain of 1e-16 that fp32 takes for zero: see report()
            self.vacuous[stage] = self.vacuous.get(stage, 0) + 1
        elif stage not in self.worst or (ratio, e) > self.worst[stage][:2]:
            self.worst[stage] = (ratio, e, E, note)
        if not e <= f * E + SR.EPS32:
            self.bad.append((stage, note, "e_gpu %.3g  E_ref %.3g  ratio %.2f" % (e, E, ratio)))

    def judge(self, stage, note, got, truth, refs):
        ok, e, E = SR.judge(stage, got, truth, *refs, factor=FACTOR.get(stage, 3.0))
        self.add(stage, note, e, E)

    def scalar(self, stage, note, got, truth, refs, E_stage):
        """note_mag / note_peak: relative to themselves, with the bound of the stage they reduce."""
        t = truth[stage]
        if t == 0.0:
            self.add(stage, note, 0.0 if got == 0.0 else np.inf, 0.0)
            return
        E = max([abs(r[stage] - t) / t for r in refs] + [E_stage])
        self.add(stage, note, abs(float(got) - t) / t, E)

    def report(self):
        """The worst note of every stage.  Left out of the figures (not of the assertion): notes whose truth stem is the
        transform times a gain of 1e-16 — 1 - ms under an all-ones mask, whose float64 knots sum to 1 - 1e-16 — which every fp32
        arithmetic, the oracle's included, makes exactly zero: E_ref = e_gpu = 1 there."""
        for stage, (ratio, e, E, note) in self.worst.items():
            print("MEASURED %-28s %-10s %.2e / %.2e (%.2f)  %s%s" % (self.tag, stage, E, e, ratio, note,
                                                                     "  [+%d vacuous]" % self.vacuous[stage] if stage in self.vacuous else ""))


def _frame_reach(t, n, n_fft, hop):
    return max(0, t * hop - n_fft // 2), min(n, t * hop + n_fft // 2)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_stages_against_the_float64_truth(ctx, route, batch):
    geo, opts, names, kind, has_skip = ROUTES[route]
    sr, n_fft, hop = geo
    sigma, notes = _batches(geo)[batch]
    radius = int(4.0 * max(1.0, sigma / SR.MASK_DS) + 0.5)
    if batch == "sigma2000":
        assert radius == 2000 and 2 * radius + 1024 > 4608      # k_mask_short's per-sample fallback loop
    try:
        _set(ctx, opts)
        d = _run(ctx, geo, notes, sigma, profile=True)
    finally:
        _restore(ctx)
    assert d["names"] == names
    assert (d["frame_skip"] is not None and d["frame_skip"].size > 0) == has_skip
    assert int(d["f_off"][-1]) > 32 or batch != "main"
    tally = Tally("%s/%s" % (route, batch))
    skipped = judge_notes(d, notes, geo, sigma, batch, kind, has_skip, tally)
    tally.report()
    if has_skip and batch == "main":
        print("frame_skip: unvoiced %d  breath %d  neither %d of %d" % (skipped[1], skipped[2], skipped[0], int(d["f_off"][-1])))
        assert skipped[1] > 0 and skipped[2] > 0 and skipped[0] > 0
    assert not tally.bad, tally.bad[:12]


def judge_notes(d, notes, geo, sigma, batch, kind, has_skip, tally):
    """Every stage of every note of one _run() against the float64 truth, unit by unit, into ``tally``; asserts what has no
    tolerance (f0, the pulse's and mask_short's own bounds, zero gains, zero tails, the frame_skip check).  ``batch`` names the
    notes in the cache of the CPU runs.  Returns the frame_skip counts {1: unvoiced, 2: breath, 0: neither}.  Shared with
    tests/test_gpu_walker_runs.py."""
    sr, n_fft, hop = geo
    radius = int(4.0 * max(1.0, sigma / SR.MASK_DS) + 0.5)
    s_off, f_off = d["s_off"], d["f_off"]
    skipped = {1: 0, 2: 0, 0: 0}
    for k, c in enumerate(notes):
        a, b, fa, fb = int(s_off[k]), int(s_off[k + 1]), int(f_off[k]), int(f_off[k + 1])
        n, name = c["n"], c["name"]
        pulse = d["pulse"][a:b]
        f0s = (np.array(c["f0"], dtype=F32) * F32(SR.KW_DEFAULT["pitch_shift"] if "pitch_shift" not in c["kw"] else c["kw"]["pitch_shift"]))
        assert np.array_equal(d["f0"][a:b], f0s), (name, "f0")
        ref_pulse = R.pulse_train(f0s, sr)
        assert np.max(np.abs(pulse - ref_pulse)) < 5e-6, (name, "pulse")
        truth, ra, rb = _pulse_runs(geo, batch, k, c, sigma, pulse)
        assert truth["T"] == fb - fa
        # mask_short: the derived bound
        ns = (n + SR.MASK_DS - 1) // SR.MASK_DS
        kb = a // SR.MASK_DS + k
        knots = d["mask_short"][kb:kb + ns]
        tk = truth["mask_short"]
        assert np.all(np.abs(knots - tk) <= (2 * radius + 1) * 2.0 ** -53 * np.abs(tk) + 2.0 ** -1074), (name, "mask_short")
        if kind == "walkers":
            tally.judge("env_harm", name, d["env_harm"][fa:fb], truth, (ra, rb))
            gt, ga, gb = truth, ra, rb
        else:
            for st in ("S_harm", "S_uv", "S_breath"):
                got = d[st][fa:fb]
                if st != "S_harm" and has_skip:                 # a skipped frame's row is not written: it is judged below
                    bit = 1 if st == "S_uv" else 2
                    keep = (d["frame_skip"][fa:fb] & bit) == 0
                    got = np.where(keep[:, None], got, truth[st].astype(np.complex64))
                tally.judge(st, name, got, truth, (ra, rb))
            E_S = SR.e_ref("S_harm", truth, ra, rb)
            tally.scalar("note_mag", name, d["note_mag"][k], truth, (ra, rb), E_S)
            given = {"S_harm": d["S_harm"][fa:fb], "S_uv": d["S_uv"][fa:fb], "S_breath": d["S_breath"][fa:fb],
                     "note_mag": float(d["note_mag"][k]), "mask_short": knots}
            if has_skip:                                        # (unwritten rows: the truth's, which the skip check holds to zero gain)
                sk = d["frame_skip"][fa:fb]
                given["S_uv"] = np.where((sk & 1)[:, None] == 0, given["S_uv"], truth["S_uv"].astype(np.complex64))
                given["S_breath"] = np.where((sk & 2)[:, None] == 0, given["S_breath"], truth["S_breath"].astype(np.complex64))
            gt, ga, gb = _three(c, geo, sigma, pulse, given)
            if kind == "separate":
                tally.judge("frames", name, d["frames"][fa:fb], gt, (ga, gb))
        if kind == "walkers":
            tally.scalar("note_mag", name, d["note_mag"][k], truth, (ra, rb), SR.e_ref("S_harm", truth, ra, rb))
        for st in ("harm", "uv", "bre", "rec", "mix"):
            tally.judge(st, name, d[st][a:b], gt, (ga, gb))
        tally.scalar("note_peak", name, d["note_peak"][k], gt, (ga, gb), SR.e_ref("rec", gt, ga, gb))
        # an exactly-zero truth gain: the device's samples are +-0, and the zero tail is zero
        assert not np.any(d["uv"][a:b][gt["gain_uv"] == 0.0]), (name, "uv under a zero gain")
        assert not np.any(d["bre"][a:b][gt["gain_bre"] == 0.0]), (name, "bre under a zero gain")
        # ... and so where the gain is zero as fp32 takes it (1.0f - F32(ms): an all-ones mask smooths to 1 - 1e-16 in float64)
        ms32 = gt["mask_smooth"].astype(F32)
        assert not np.any(d["uv"][a:b][(F32(1.0) - ms32) == 0]), (name, "uv under a zero fp32 gain")
        assert not np.any(d["bre"][a:b][ms32 == 0]), (name, "bre under a zero fp32 gain")
        tail = hop * (fb - fa - 1)
        for st in ("harm", "uv", "bre", "rec", "mix"):
            assert not np.any(d[st][a + tail:b]), (name, st, "zero tail")
        if has_skip:
            ms32 = truth["mask_smooth"].astype(F32)
            for t, sk in enumerate(d["frame_skip"][fa:fb]):
                lo, hi = _frame_reach(t, n, n_fft, hop)
                if sk & 1:
                    assert not np.any(F32(1.0) - ms32[lo:hi]), (name, t, "unvoiced frame skipped under a non-zero gain")
                if sk & 2:
                    assert not np.any(ms32[lo:hi]), (name, t, "breath frame skipped under a non-zero gain")
                skipped[1] += int(sk & 1 != 0)
                skipped[2] += int(sk & 2 != 0)
                skipped[0] += int(sk == 0)
    return skipped


def _zero_gain(notes, sigma):
    """Per sample of the concatenated batch: is the fp32 gain of the unvoiced / breath stem exactly zero — 1.0f - F32(ms) or the
    uv strength, F32(ms) or the breath strength, ms the truth's smoothed mask."""
    zu, zb = [], []
    for c in notes:
        kw = dict(SR.KW_DEFAULT, **c["kw"])
        ms32 = SR.mask_upsample(SR.mask_knots(c["mask"], sigma, exact=True), c["n"], True).astype(F32)
        zu.append(((F32(1.0) - ms32) == 0) | (kw["uv_strength"] == 0))
        zb.append((ms32 == 0) | (kw["breath_strength"] == 0))
    return {"uv": np.concatenate(zu), "bre": np.concatenate(zb)}


def _bit_mismatches(x, y, zero_ok=None):
    """Samples whose 32 bits differ.  ``zero_ok``: where one zero may be -0 and the other +0 (both must be zeros there).
    Returns (mismatches, sign-of-zero differences inside zero_ok)."""
    diff = x.view(np.uint32) != y.view(np.uint32)
    if zero_ok is None:
        return int(diff.sum()), 0
    signs = diff & zero_ok & (x == 0) & (y == 0)
    return int((diff & ~signs).sum()), int(signs.sum())


# On the walker routes the two noise stems carry one bit that is not a function of the note alone: the SIGN of a sample that is
# exactly zero because its fp32 gain is.  k_noise_stems stores such a hop as the product x * 0, which keeps the sign of x, unless
# it finds the hop flat (skip_zero 1), stores nothing and leaves a flag for k_note_finish, which takes +0; a hop is tested for
# flatness only where the run's staged knots cover it, and where a run begins depends on the batch.  So uv and bre of the walker
# routes are compared bit for bit EXCEPT that at a sample whose fp32 gain is exactly zero -0 and +0 count as the same; harm, rec
# and mix of the walker routes, and all five outputs of every other route, are compared bit for bit with no exception.
@pytest.mark.parametrize("route", list(ROUTES))
def test_sub_batches_reproduce_the_full_batch_bits(ctx, route):
    geo, opts, names, kind, has_skip = ROUTES[route]
    sigma, notes = _batches(geo)["main"]
    zero = _zero_gain(notes, sigma) if kind == "walkers" else {}
    bad, signs = [], 0
    try:
        _set(ctx, opts)
        full = _run(ctx, geo, notes, sigma, views=False)
        for first, count in ((0, 1), (10, 3), (14, 4), (21, 5), (30, 13), (len(notes) - 1, 1)):
            sub = _run(ctx, geo, notes[first:first + count], sigma, views=False)
            a, b = int(full["s_off"][first]), int(full["s_off"][first + count])
            for st in ("harm", "uv", "bre", "rec", "mix"):
                m, sg = _bit_mismatches(full[st][a:b], sub[st], zero[st][a:b] if st in zero else None)
                signs += sg
                if m:
                    bad.append((first, count, st, m))
    finally:
        _restore(ctx)
    print("%s: %d zero-sign differences under a zero fp32 gain" % (route, signs))
    assert not bad, (route, bad)


@pytest.mark.parametrize("batch", BATCHES)
def test_walkers_skip_zero_changes_no_bit(ctx, batch):
    """skip_zero 1 against skip_zero 0 on the walker route, bit for bit — with the one allowance described above, which is this
    very option's doing: with skip_zero 0 every hop is stored as x * 0, with 1 a flat hop is finished as +0."""
    sigma, notes = _batches(G0)[batch]
    zero = _zero_gain(notes, sigma)
    try:
        res = []
        for skip in (1, 0):
            _set(ctx, {"skip_zero": skip})
            res.append(_run(ctx, G0, notes, sigma, views=False, profile=True))
    finally:
        _restore(ctx)
    assert res[0]["names"] == STEMS and res[1]["names"] == STEMS
    bad, signs = [], 0
    for st in ("harm", "uv", "bre", "rec", "mix"):
        m, sg = _bit_mismatches(res[0][st], res[1][st], zero.get(st))
        signs += sg
        if m:
            bad.append((st, m))
    print("skip_zero 1 / 0, %s: %d zero-sign differences under a zero fp32 gain" % (batch, signs))
    assert not bad, bad
