"""Replay of tests/golden/fs_eval_small.npz (tools/gen_golden_fs_eval.py: the reference's evaluation/evaluation_manager.py
run_evaluation_game with a scripted planner as policies[0]) through `evaluation.run_evaluation_episodes(searchers={0: stub})`;
shared by the CPU test (oracle-backed env) and the `-m gpu` test (HIP env)."""
import numpy as np
import torch

import golden_util as gu
from rollout_fixture import CountingEnv, ReplayPolicy, scripted_log_prob
from settlers_of_catan_rl_amd import evaluation, spec


class StubSearcher(object):
    """plays the recorded action of every game it is asked to decide and records the call"""
    policy = None

    def __init__(self, cenv, table):
        self.cenv, self.table, self.calls = cenv, table, {}

    def act(self, env, games=None, initial_settlement=None, deterministic=False, **kw):
        assert env is self.cenv and not kw, kw
        g = games.cpu()
        k = self.cenv.steps_taken[g]
        for gi, ki, fl in zip(g.tolist(), k.tolist(), np.asarray(initial_settlement).tolist()):
            self.calls.setdefault(gi, []).append((ki, int(bool(fl))))
        return self.table.table[g, k].numpy(), {"next_hidden": None}


def check_fs_eval_fixture(make_env):
    """make_env(n, seed) -> freshly created env WITHOUT auto-reset whose game i draws from the Philox stream (seed, i)"""
    g = gu.load("fs_eval_small.npz")
    n, seed = int(g["n_games"]), int(g["seed"])
    env = make_env(n, seed)
    cenv = CountingEnv(env)
    table = ReplayPolicy(cenv, [g[f"g{i}_trace"] for i in range(n)])
    stub = StubSearcher(cenv, table)

    def act_fn(net, idx, f, lists, lens, masks):                      # the three scripted nets, as the generator's: value 1.5, entropy 0.75
        k = torch.minimum(cenv.steps_taken, table.lens)
        a = table.table[torch.arange(n), k][idx.cpu()].to(f.device)
        return {"actions": a, "logp": scripted_log_prob(a), "value": torch.full((len(idx),), 1.5), "entropy": torch.full((len(idx),), 0.75)}
    orders = np.stack([g[f"g{i}_order"].astype(np.int64) for i in range(n)])
    assert len(set(orders[:, 0].tolist())) == n                       # the planner plays a different PlayerId in each game
    res = evaluation.run_evaluation_episodes(cenv, [object(), object(), object(), object()], orders, act_fn=act_fn, max_steps=2500, stats=True,
                                             searchers={0: stub})
    blobs = env.export_state().cpu().numpy()
    for i in range(n):
        w, vp, steps, dec = [int(x) for x in g[f"g{i}_result"]]
        assert (int(res["winner"][i]), int(res["victory_points"][i]), int(res["game_steps"][i]), int(res["policy_decisions"][i])) == (w, vp, steps, dec), i
        flags = g[f"g{i}_flags"]
        assert stub.calls[i] == [(int(a), int(b)) for a, b, _ in flags], i       # the rows it was asked to decide, and the flag of every call
        assert len(flags) == dec and flags[:, 1].sum() >= 2, i
        assert np.array_equal(res["action_types"][i], g[f"g{i}_action_types"]), i
        assert res["entropy"][i] == float(g[f"g{i}_entropy"]) == 0.0 and res["value"][i] == float(g[f"g{i}_value"]) == 0.0, i
        want = [(int(t), float(lp)) for t, lp in g[f"g{i}_type_log_probs"]]
        assert [(int(t), float(lp)) for t, lp in res["type_log_probs"][i]] == want and all(lp == 0.0 for _, lp in want), i
        assert np.array_equal(blobs[i], g[f"g{i}_final_blob"]), spec.describe_state_diff(g[f"g{i}_final_blob"], blobs[i])
    return n
