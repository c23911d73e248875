"""GPU: the fixed-job path of bench.py end to end on ONE GPU — what the driver runs at 1, 2, 4 and 8 GPUs for BASELINE
configs 4 / 5 (`--job-notes`): LPT assignment, sub-batches ordered by length, the per-rank frame counts, the imbalance and the
optional ragged gather in the printed line.  A child process, like the driver's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_bench_job_mode_line_on_one_gpu():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(here, "bench.py"), "--gpus", "1", "--full", "--job-notes", "2048", "--config", "4", "--gather",
           "--no-cpu-baseline", "--no-variants", "--no-host-inclusive", "--steps", "2", "--warmup", "1", "--sub-batch", "1024"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=here,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    from goofer_amd import synthetic as syn
    frames = sum(syn.config_note_frames(4, i) for i in range(2048))
    assert line["scaling"] == "strong" and line["n_gpus"] == 1
    assert line["per_rank_frames"] == [frames] and line["imbalance"] == 1.0
    assert line["config"]["notes_per_gpu"] == 2048 and line["config"]["sub_batches_per_gpu"] == 2
    assert line["config"]["frames_per_gpu"] == frames
    g = line["gather_to_rank0"]
    assert g["bytes"] == 0 and g["ms"] >= 0.0                      # one rank: nothing crosses a link, the call still runs
    assert line["value"] > 1e6 and abs(line["value"] - frames * line["steps"] / (line["ms_per_step"] * 1e-3 * line["steps"])) < 1e-6 * line["value"]
    assert line["roofline"]["kernel"] and line["roofline"]["frac"] > 0.0


def test_bench_dump_outputs_of_a_job_in_two_sub_batches(tmp_path):
    """--dump-outputs of a fixed job rendered in two sub-batches: a seeded sample of whole notes under 64 MB, in note-id order,
    drawn from both sub-batches of the last timed step, every dumped note the bits that note renders to on its own."""
    import numpy as np
    import torch
    from goofer_amd import synthetic as syn
    from goofer_amd.device import Context
    from goofer_amd.workload import SamplerWorkload
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(here, "bench.py"), "--gpus", "1", "--job-notes", "2048", "--config", "4",
           "--no-cpu-baseline", "--no-variants", "--no-host-inclusive", "--steps", "3", "--warmup", "1", "--sub-batch", "1024",
           "--dump-outputs", str(dump)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=here,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0.0
    files = ["mix.npy", "note_ids.npy", "note_samples.npy"]
    assert sorted(os.listdir(dump)) == files and line["dump_outputs"]["files"] == files
    assert sum(os.path.getsize(dump / f) for f in files) <= 64_000_000
    mix, ids, lens = (np.load(dump / f) for f in files)
    assert mix.dtype == np.float32 and ids.dtype == np.float64 and lens.dtype == np.float64
    ids, lens = ids.astype(np.int64), lens.astype(np.int64)
    assert 0 < ids.size < 2048 and line["dump_outputs"]["notes"] == ids.size and mix.size == lens.sum()
    assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < 2048 and bool(np.isfinite(mix).all())
    hop = syn.config_geometry(4)["hop"]
    est = [syn.config_note_frames(4, i) for i in range(2048)]
    assert all(1 + n // hop == est[i] for i, n in zip(ids, lens))
    first = set(sorted(range(2048), key=lambda i: (-est[i], i))[:1024])           # the longest notes: bench.py's first sub-batch
    assert any(int(i) in first for i in ids) and any(int(i) not in first for i in ids)
    off = np.concatenate([[0], np.cumsum(lens)])
    ctx = Context(0)
    try:
        for j in (0, ids.size // 2, ids.size - 1):
            got = SamplerWorkload(ctx, 4, [int(ids[j])]).step()["mix"]
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), mix[off[j]:off[j + 1]]), int(ids[j])
    finally:
        ctx.close()
