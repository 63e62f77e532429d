"""Evaluation protocol (reference RL/ppo/evaluation_manager.py) on CPU: the batched episode runner against the reference's
EvaluationManager.run_evaluation_game with identical nets (arg-max actions), seat orders and game streams."""
import random

import numpy as np
import torch

import golden_util
from settlers_of_catan_rl_amd import evaluation as ev
from oracle_vec_env import OracleVecEnv


def test_sample_orders_is_the_reference_shuffle():
    random.seed(5)
    want = []
    for _ in range(6):
        o = [2, 4, 3, 1]
        random.shuffle(o)
        want.append(o)
    assert np.array_equal(ev.sample_orders(6, random.Random(5)), np.array(want))


def _scripted_action(L, env_ptr, seed, env_id, step, masks_flat):
    import ctypes as C
    m = np.ascontiguousarray(masks_flat, dtype=np.float32)
    out = np.zeros(18, dtype=np.int32)
    L.orc_sample_action(env_ptr, seed + 99, env_id, int(step), m.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def test_episodes_match_reference_evaluation_manager():
    """Full games: the reference EvaluationManager.run_evaluation_game (its env routed to the game's philox stream, its four
    policies replaced by a scripted uniform-random legal policy keyed by (game, decision number); tests/golden/ref_checks.npz,
    tools/gen_golden.py gen_ref_checks) against the batched runner on the oracle-backed env with the same scripted policy:
    winner index, policy-0 victory points, game length and policy-0 decisions per game, for random seat orders."""
    fx = golden_util.load("ref_checks.npz")
    seed, orders, want = int(fx["eval_seed"]), fx["eval_orders"], fx["eval_want"]
    n = len(orders)
    env = OracleVecEnv(n, seed, auto_reset=False)

    def act_fn(net, idx, f, lists, lens, masks):
        return torch.tensor(np.stack([_scripted_action(env.L, env.b.env_ptr(int(i)), seed, int(i), env.steps_taken[int(i)], masks[j].numpy())
                                      for j, i in enumerate(idx)]), dtype=torch.int64)

    class Tag(object):
        pass
    central, opp = Tag(), Tag()
    got = ev.run_evaluation_episodes(env, [central, opp, opp, opp], np.array(orders), act_fn=act_fn)
    for g in range(n):
        winner, vps, steps, decisions = (int(x) for x in want[g])
        assert (got["winner"][g], got["victory_points"][g], got["game_steps"][g], got["policy_decisions"][g]) == \
               (winner, vps, steps, decisions), (g, want[g], {k: v[g] for k, v in got.items()})
    assert len({tuple(o) for o in orders}) > 1


def test_episodes_with_lstm_policy_keep_state_per_seat():
    """An LSTM central policy against a feed-forward opponent: every seat of the central policy carries its own (h, c)
    (evaluation_manager.py:20-26,50-59).  Checked by replaying game 0 alone with the same sampled actions forced."""
    import torch
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(0)
    central = CatanPolicy(include_lstm=True).eval()
    opp = CatanPolicy().eval()
    seen = []
    orig = central.act

    def spy(*a, **kw):
        out = orig(*a, **kw)
        seen.append((kw["hidden"][0].clone(), out[3][0].clone()))
        return out
    central.act = spy
    n = 3
    env = OracleVecEnv(n, 5, auto_reset=False)
    orders = np.array([[1, 2, 3, 4], [2, 1, 4, 3], [3, 4, 1, 2]])
    res = ev.run_evaluation_episodes(env, [central, opp, opp, opp], orders, max_steps=24, deterministic=True)
    assert (res["winner"] == -1).all() and (res["game_steps"] == 25).all()
    assert sum(h.shape[0] for h, _ in seen) == int(res["policy_decisions"].sum())
    # the first decision of a seat starts from zero, later ones from that seat's previous output
    assert float(seen[0][0].abs().max()) == 0.0
    assert any(float(h.abs().max()) > 0 for h, _ in seen[1:])
