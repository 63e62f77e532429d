"""The offline evaluator's device tallies on the HIP env with the fixture net (sampled, bf16 autocast)."""
import os
import random

import numpy as np
import pytest
import torch

import policy_fixture as pf
from settlers_of_catan_rl_amd import evaluation as ev
from settlers_of_catan_rl_amd.env import VecCatanEnv
from settlers_of_catan_rl_amd.policy import CatanPolicy

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_sampled_games_tallies_are_consistent():
    g = np.load(os.path.join(GOLD, "policy_small.npz"))
    net, _ = pf.load_fixture_policy(g, "ff", "cuda")
    torch.manual_seed(7)
    opp = CatanPolicy().cuda().eval()
    n = 1024
    orders = ev.sample_orders(n, random.Random(3))
    res = ev.run_evaluation_episodes(VecCatanEnv(n, seed=5, auto_reset=False, device="cuda"), [net, opp, opp, opp], orders, max_steps=2500,
                                     autocast_dtype=torch.bfloat16, generator=torch.Generator(device="cuda").manual_seed(9), stats=True)
    dec = res["policy_decisions"]
    assert (dec > 0).all()
    assert np.array_equal(res["action_types"].sum(1), dec)
    assert [len(t) for t in res["type_log_probs"]] == dec.tolist()
    assert np.isfinite(res["entropy"]).all() and (res["entropy"] >= 0).all()
    assert np.isfinite(res["value"]).all()
    lps = np.concatenate([[lp for _, lp in tl] for tl in res["type_log_probs"]])
    assert np.isfinite(lps).all() and (lps <= 1e-6).all()
    counts = np.zeros(13, dtype=np.int64)
    for tl in res["type_log_probs"]:
        for t, _ in tl:
            counts[t] += 1
    assert np.array_equal(counts, res["action_types"].sum(0))
