"""bench.py's line on the device, at a small size: a plain run carries the headline and nothing that needs runs of its own; --full adds
the sub-records (here without the PPO update, the live counter passes and the CPU baseline, which take minutes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--envs", "4096", "--steps", "32", "--warmup", "4", "--preroll", "64"]
FULL_ONLY = ("lockstep", "step_api", "roofline", "ppo_update", "roofline_learner", "cpu_baseline", "gpu_over_cpu_all_cores")


def _bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["status"] == "ok", line
    return line


def test_plain_run_prints_the_headline_only(hip_lib, tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["metric"] == "Catan env-steps/sec at 65k parallel games" and line["unit"] == "env-steps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8/u32 (integer bitboards)"
    assert line["steps"] == 32 and line["timed_passes"] == 32 and line["invalid_actions"] == 0
    assert line["value"] > 0 and line["ms_per_step"] == pytest.approx(line["timed_s"] / 32 * 1e3)
    assert line["value"] == pytest.approx(line["env_steps_executed"] / line["timed_s"])
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    counters = np.load(tmp_path / "policy_counters.npy")
    assert counters.shape == (4096,)
    for name in ("state", "state_games", "masks", "mask_games"):
        assert (tmp_path / f"{name}.npy").exists()


def test_full_run_adds_the_sub_records(hip_lib):
    line = _bench("--full", "--ppo-steps", "0", "--no-cpu-baseline", "--no-live-pmc")
    assert line["lockstep"]["steps"] == 32 and line["lockstep"]["value"] > 0
    assert line["step_api"]["catan_step_deferred_us_per_call"] > 0
    assert line["roofline"]["avg_launch_us"] > 0 and line["roofline"]["kernel"].startswith("k_step")
    assert "ppo_update" not in line and "cpu_baseline" not in line
