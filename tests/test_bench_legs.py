"""What a plain bench.py run does and what --full adds.

A plain run sets up, warms up, times its steps, writes --dump-outputs and prints the headline line; the legs
that take runs of their own after the timed steps (end to end, small batches, CPU baselines, parity sample)
come only with --full, and must not change what the timed steps computed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FIELDS = ("seq_idx", "profile_idx", "null_loglik", "alt_loglik")


def test_e2e_steps_without_full_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "1", "--e2e-steps", "2"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr


def _bench(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "DCP_BENCH_FORCE_DIST")}
    r = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
@pytest.mark.timeout(700)
def test_plain_run_is_the_headline_alone_and_full_adds_the_legs(tmp_path):
    # --planted: query 350 of the last timed step carries a real hit, so the dumps are not empty
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--nprof", "300", "--qstep", "128", "--planted"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(common + ["--full", "--no-cpu-baseline", "--e2e-steps", "1", "--dump-outputs", str(tmp_path / "full")])
    for out in (plain, full):
        assert all(k in out for k in HEADLINE) and out["steps"] == 2 and out["warmup"] == 1
        assert out["unit"] == "Gcell/s" and out["value"] > 0 and out["roofline"]["kernel_ms_per_step"] > 0
    assert plain["e2e"] is None and plain["small_batches"] is None
    assert not {"cpu_baseline", "cpu_baseline_optimised", "parity_check"} & set(plain)
    assert full["e2e"]["steps"] == 1 and set(full["small_batches"]) == {"1", "8", "64", "what"}
    # the legs run after the timed steps and the dump: both runs hand back the same hit records
    assert len(np.load(tmp_path / "plain" / "seq_idx.npy")) > 0
    for f in FIELDS:
        assert np.array_equal(np.load(tmp_path / "plain" / (f + ".npy")), np.load(tmp_path / "full" / (f + ".npy")))
