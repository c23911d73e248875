"""bench.py --dump-outputs without a GPU: which notes the dump holds, and the arguments bench.py refuses before it starts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_note_is_dumped_when_they_fit():
    lens = [44100, 3000, 96000]
    assert bench.dump_selection(lens, sum(lens)).tolist() == [0, 1, 2]


def test_a_larger_step_is_sampled_in_whole_notes_within_the_budget():
    lens = np.random.default_rng(7).integers(4000, 130000, size=2048)
    budget = int(lens.sum() // 5)
    pick = bench.dump_selection(lens, budget)
    assert 0 < pick.size < lens.size and np.all(np.diff(pick) > 0)
    total = int(lens[pick].sum())
    assert total <= budget
    rest = np.setdiff1d(np.arange(lens.size), pick)
    assert total + int(lens[rest].min()) > budget                  # no note left out would still have fitted
    assert np.array_equal(pick, bench.dump_selection(lens, budget))
    assert not np.array_equal(pick, bench.dump_selection(lens, budget, seed=bench.DUMP_SEED + 1))


def test_the_dump_budget_stays_under_64_mb():
    assert bench.DUMP_BYTES <= 64_000_000


@pytest.mark.parametrize("args", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_bench_refuses_a_run_without_timed_steps(args):
    res = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                         timeout=120, cwd=REPO)
    assert res.returncode == 2 and "--steps must be at least 1" in res.stderr, res.stderr[-2000:]
