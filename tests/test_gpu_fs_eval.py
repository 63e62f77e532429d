"""GPU: the forward search on a device-side state fork, a sub-list of games, and search players in evaluation games."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sim_env(n):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=4, env_id0=1 << 20, dense_reward=True, auto_reset=False)


def test_fork_and_blob_broadcast_give_identical_searches(hip_lib):
    """64 roots, 16 simulations per root, depth 4, arg-max heads, fixture weights: identical chosen actions and bit-identical
    mean values under both `state_broadcast` settings; the same for a sub-list of the games"""
    import forward_search_fixture as ff
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd import forward_search as fs
    net = ff.fixture_net("cuda")
    R = 64
    root = VecCatanEnv(R, seed=3)
    root.random_rollout(0, 600)
    before = root.export_state().clone()
    games = torch.tensor([41, 3, 17, 60, 5, 22, 9, 33, 2, 50], device="cuda")
    out = {}
    for mode in ("fork", "blob"):
        s = fs.ForwardSearch(net, _sim_env, R, max_depth=4, sims_per_root=16, sims_per_round=8, state_broadcast=mode, seed=2)
        out[mode] = s.act(root, deterministic=True)
        s2 = fs.ForwardSearch(net, _sim_env, R, max_depth=4, sims_per_root=16, sims_per_round=8, state_broadcast=mode, seed=2)
        out[mode + "_sub"] = s2.act(root, deterministic=True, games=games)
        assert s.sim_env.invalid_action_count() == 0 and s2.sim_env.invalid_action_count() == 0
    assert torch.equal(root.export_state(), before)
    for a, b in (("fork", "blob"), ("fork_sub", "blob_sub")):
        assert np.array_equal(out[a][0], out[b][0])
        for k in ("n_proposed", "best", "finished_each", "mean_value"):
            assert np.array_equal(out[a][1][k], out[b][1][k]), (a, k)
    assert out["fork_sub"][0].shape[0] == games.numel()
    assert int((out["fork"][1]["n_proposed"] > 1).sum()) > 8        # searches did run


def test_fs_eval_fixture_on_device(hip_lib):
    import fs_eval_fixture as fx
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    assert fx.check_fs_eval_fixture(lambda n, seed: VecCatanEnv(n, seed=seed, auto_reset=False)) == 3


def test_search_player_in_evaluation_games_end_to_end(hip_lib):
    """16 games, policy 0 a real ForwardSearch (8 simulations per decision, depth 3), three copies of one net, 80 steps"""
    from settlers_of_catan_rl_amd import evaluation, reference_api as ra
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    import random
    torch.manual_seed(0)
    net = CatanPolicy().cuda().eval()
    runs = []
    for _ in range(2):
        planner = ra.ForwardSearchPolicy(net, None, max_init_actions=6, max_depth=3, sims_per_root=8, sims_per_round=4, device="cuda", seed=11,
                                         autocast_dtype=None)
        assert planner.policy_type == "forward_search"
        env = VecCatanEnv(16, seed=21, auto_reset=False)
        searcher = planner.make_searcher(16, _sim_env)
        res = evaluation.run_evaluation_episodes(env, [net, net, net, net], evaluation.sample_orders(16, random.Random(5)), max_steps=80,
                                                 deterministic=True, stats=True, searchers={0: searcher})
        assert (res["policy_decisions"] > 0).all()
        assert env.invalid_action_count() == 0 and searcher.sim_env.invalid_action_count() == 0
        assert (res["entropy"] == 0.0).all() and (res["value"] == 0.0).all()
        runs.append(res)
    for k in ("winner", "victory_points", "game_steps", "policy_decisions", "action_types"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
