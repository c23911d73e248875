"""GPU: what a plain `bench.py` line holds and what `--full` adds to it, on a small default workload.  Child processes, like
the driver's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("stage_ms", "stage_ms_from", "roofline", "roofline_noise", "roofline_harm", "roofline_fft", "roofline_step", "variants",
             "value_skip_zero_off", "value_unvoiced_30pct", "value_two_in_flight", "pcie_inclusive", "host_inclusive", "cpu_baseline",
             "config4", "config5")


def _bench(*args):
    cmd = [sys.executable, os.path.join(HERE, "bench.py"), "--gpus", "1", "--notes", "64", "--steps", "2", "--warmup", "1", *args]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=HERE)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _headline(line):
    assert line["metric"] == "resynth_frames_per_sec" and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0.0
    frames = line["config"]["frames_per_gpu"]
    assert abs(line["value"] - frames / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]


def test_a_plain_run_prints_the_headline_and_its_dump_only(tmp_path):
    dump = tmp_path / "dump"
    line = _bench("--dump-outputs", str(dump))
    _headline(line)
    assert not [k for k in FULL_ONLY if k in line]
    assert line["config"]["notes_per_gpu"] == 64 and line["dump_outputs"]["notes"] == 64
    assert sorted(os.listdir(dump)) == ["mix.npy", "note_ids.npy", "note_samples.npy"]


def test_full_adds_the_stage_times_rooflines_and_variants():
    line = _bench("--full", "--no-cpu-baseline", "--no-host-inclusive", "--no-legs")
    _headline(line)
    assert line["stage_ms"] and line["roofline"]["kernel"] and line["roofline"]["frac"] > 0.0
    assert line["roofline_fft"]["ms_per_launch"] > 0.0 and line["stage_ms"]["rfft_frames_standalone"] > 0.0
    assert line["value_skip_zero_off"] > 0.0 and line["value_unvoiced_30pct"] > 0.0 and line["value_two_in_flight"] > 0.0
    assert line["pcie_inclusive"]["h2d_bytes"] > 0
    assert not [k for k in ("host_inclusive", "cpu_baseline", "config4", "config5") if k in line]
