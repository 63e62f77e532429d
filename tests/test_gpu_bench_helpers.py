"""GPU: the two timed loops of tools/parent_compare.py run, call what they are given in the order they promise and return figures of
the promised shape.  No timing value is asserted: what a step costs is the tools' to measure, not the suite's."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import parent_compare as pc  # noqa: E402

pytestmark = pytest.mark.gpu


def test_step_call_times_and_event_call_times(hip_lib):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(256, seed=1)
    seen = []
    out = pc.step_call_times(env, 8, 2, between=lambda name, phase: seen.append((name, phase)))
    assert sorted(out) == ["catan_step_deferred_us", "catan_step_us"]
    assert all(math.isfinite(v) and v > 0 for v in out.values()), out
    assert seen == [("catan_step", "warmed"), ("catan_step", "timed"), ("catan_step_deferred", "warmed"), ("catan_step_deferred", "timed")]
    assert env.invalid_action_count() == 0
    assert sorted(pc.step_call_times(env, 8, 2)) == sorted(out)          # `between` is optional

    buf = torch.empty((256, 18), dtype=torch.int32, device=env.device)
    counts = {"scripted": 0, "random": 0}

    def call(name, fn):
        def run():
            counts[name] += 1
            fn()
        return run
    t = pc.event_call_times({"scripted": call("scripted", lambda: env.sample_scripted_actions(out=buf)),
                             "random": call("random", lambda: env.sample_random_actions(7, out=buf))}, reps=4, rounds=2)
    assert counts == {"scripted": 10 + 4 * 2, "random": 10 + 4 * 2}       # the warm-up, then reps x rounds
    assert sorted(t) == ["random", "scripted"]
    for per_call in t.values():
        assert sorted(per_call) == ["device_us", "host_issue_us"]
        for lo, mid, hi in per_call.values():
            assert all(math.isfinite(v) and v >= 0 for v in (lo, mid, hi)) and lo <= mid <= hi
    print(out, t)
    assert env.invalid_action_count() == 0
