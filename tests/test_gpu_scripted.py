"""GPU: the rule-based "builder" player - k_sample_scripted against the numpy restatement of the rule
(tests/scripted_reference.py), game lists and streams, stepping its actions, its strength against uniform-random players, and its
place in the evaluation protocol and the rollout collector."""
import random

import numpy as np
import pytest
import torch

import scripted_reference as sr
from guarded import ptr as P, stream

pytestmark = pytest.mark.gpu

N, SEED = 96, 7          # 96 games: a partial wave and a partial workgroup.  Seed 7: its coverage was checked with the numpy rule on the CPU oracle


def _env(n, seed, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=seed, **kw)


def test_kernel_equals_the_numpy_rule_over_600_steps(hip_lib):
    """Lock-step, auto-reset on.  At every step the kernel decides all 96 games and so does the numpy rule from export_state() +
    get_action_masks(): all 18 words equal.  Two games in three step the bot's action, the third a uniform-random legal one (which games
    rotates with the step), so that states a pure builder never reaches - open trades, hands above seven cards - are decided too.
    Every row 1..12 of the table and every playable card must have been compared at least once, and the fall-back row never."""
    env = _env(N, SEED)
    rows, cards = np.zeros(14, dtype=np.int64), np.zeros(5, dtype=np.int64)
    g = torch.arange(N, device="cuda")
    for step in range(600):
        got = env.sample_scripted_actions()
        want, row = sr.decide_all(env.export_state().cpu().numpy(), env.get_action_masks().cpu().numpy())
        got_h = got.cpu().numpy()
        bad = np.flatnonzero((got_h != want).any(1))
        assert bad.size == 0, (step, int(bad[0]), int(row[bad[0]]), got_h[bad[0]].tolist(), want[bad[0]].tolist())
        np.add.at(rows, row, 1)
        np.add.at(cards, want[row == 8, 4], 1)
        rnd = env.sample_random_actions(step)
        env.step(torch.where((((g + step) % 3) == 0)[:, None], rnd, got))
    print("decisions per row of the table:", rows[1:].tolist(), "per card:", cards.tolist())
    assert env.invalid_action_count() == 0
    assert (rows[1:13] > 0).all(), rows.tolist()
    assert all(cards[c] > 0 for c in (sr.KNIGHT, sr.ROAD_BUILDING, sr.YEAR_OF_PLENTY, sr.MONOPOLY)) and cards[sr.VICTORY_POINT] == 0, cards.tolist()
    assert rows[13] == 0 and env.scripted_fallback_count() == 0


def test_game_lists_and_streams(hip_lib):
    env = _env(N, SEED)
    env.random_rollout(0, 200)
    full = env.sample_scripted_actions()
    sub = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:37].to("cuda")
    assert torch.equal(env.sample_scripted_actions(games=sub.to(torch.int32)), full[sub])
    assert torch.equal(env.sample_scripted_actions(games=sub), full[sub])                      # (an int64 list is converted)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = env.sample_scripted_actions(games=sub.to(torch.int32))
        all_side = env.sample_scripted_actions()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(on_side, full[sub]) and torch.equal(all_side, full)
    out = torch.full((37, 18), -5, dtype=torch.int32, device="cuda")
    assert env.sample_scripted_actions(games=sub, out=out) is out and torch.equal(out, full[sub])
    # ids outside the handle get the placeholder answer (EndTurn), as catan_masks_of gives them the placeholder masks
    odd = torch.tensor([3, -1, N, 5], dtype=torch.int32, device="cuda")
    a = env.sample_scripted_actions(games=odd)
    assert torch.equal(a[[0, 3]], full[[3, 5]]) and a[1].tolist() == [10] + [0] * 17 and a[2].tolist() == [10] + [0] * 17


def test_stepping_the_bots_actions_is_always_legal(hip_lib):
    for deferred in (False, True):
        env = _env(N, SEED + 1)
        for _ in range(300):
            a = env.sample_scripted_actions()
            if deferred:
                env.step_deferred(a, window=4)
            else:
                env.step(a)
        if deferred:
            env.step_flush()
        assert env.invalid_action_count() == 0 and env.scripted_fallback_count() == 0, deferred


class UniformRandom(object):
    """the env's uniform-random legal sampler as a policy keyed by game (the draw index is the pass number)"""
    wants_games, include_lstm = True, False

    def __init__(self, env):
        self.env, self.passes = env, 0

    def act(self, f, lists, lens, masks, games=None, **_kw):
        a = self.env.sample_random_actions(self.passes).long()
        self.passes += 1
        a = a if games is None else a[games.long()]
        z = torch.zeros((a.shape[0], 1), device=a.device)
        return z, a, z


def test_the_bot_beats_three_uniform_random_players(hip_lib):
    """512 evaluation games, policy 0 the bot, the others uniform-random, fresh seat orders.  A player no better than the others wins a
    quarter of the games; the bot's share must lie more than five binomial standard errors above that:
    0.25 + 5 * sqrt(0.25 * 0.75 / 512) = 0.3457.  Draws (2 500 steps without a winner) are at most 5 % of the games."""
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    n = 512
    env = _env(n, 21, auto_reset=False)
    rnd = UniformRandom(env)
    res = ev.run_evaluation_episodes(env, [ScriptedPolicy(env), rnd, rnd, rnd], ev.sample_orders(n, random.Random(3)), max_steps=2500)
    share, draws = float(np.mean(res["winner"] == 0)), float(np.mean(res["winner"] == -1))
    print(f"scripted against three uniform-random players: win share {share:.4f}, draws {draws:.4f}, mean game steps {res['game_steps'].mean():.1f}")
    assert env.invalid_action_count() == 0 and env.scripted_fallback_count() == 0
    assert draws <= 0.05, draws
    assert share > 0.25 + 5.0 * (0.25 * 0.75 / n) ** 0.5, share


def test_protocol_with_the_scripted_baseline(hip_lib):
    """32 games, 100 steps at most: log["random"] is what a call without baselines gives under the same rng, log["scripted"] has its
    four keys.  The nets are CatanPolicy as it is - it takes no size, and the test helpers hold no smaller policy; the games are kept
    short instead."""
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    torch.manual_seed(0)
    central, opp = CatanPolicy().cuda().eval(), CatanPolicy().cuda().eval()
    envs = []

    def make_env(n):
        envs.append(_env(n, 8, auto_reset=False))
        return envs[-1]

    def run(**kw):
        torch.manual_seed(5)
        return ev.run_evaluation_protocol(make_env, central, opp, 32, update_num=2, rng=random.Random(1), max_steps=100, stats=True, **kw)
    plain, plain_summary = run()
    log, summary = run(baselines={"scripted": ScriptedPolicy})
    assert list(log) == ["update", "random", "scripted"] and log["random"] == plain["random"] and summary.startswith(plain_summary)
    assert set(log["scripted"]) == set(log["random"]) and "32 games against scripted." in summary
    assert len(envs) == 3 and all(e.invalid_action_count() == 0 for e in envs) and envs[2].scripted_fallback_count() == 0
    assert 0 < log["scripted"]["avg_policy_decisions"] < log["scripted"]["avg_game_length"]


def test_scripted_policy_as_policy_zero_has_zero_statistics(hip_lib):
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = _env(16, 4, auto_reset=False)
    bot = ScriptedPolicy(env)
    res = ev.run_evaluation_episodes(env, [bot, bot, bot, bot], ev.sample_orders(16, random.Random(2)), max_steps=200, stats=True, detailed=True)
    assert (res["policy_decisions"] > 0).all() and float(np.abs(res["entropy"]).max()) == 0.0 and float(np.abs(res["value"]).max()) == 0.0
    assert res["action_types"].sum() == res["policy_decisions"].sum() and all(lp == 0.0 for game in res["type_log_probs"] for _, lp in game)


def _collect(n, T, seed, gathers, fused, **ckw):
    import rollout_fixture as rf
    from test_gpu_collector import SamplerPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = _env(n, seed)
    env.random_rollout(0, 150)
    cenv = rf.CountingEnv(env)
    col = RolloutCollector(cenv, SamplerPolicy(cenv), T, opponents=[ScriptedPolicy(env)], seed=seed, **ckw)
    col.fused_bookkeeping = fused
    out = []
    for _ in range(gathers):
        st = col.gather_rollouts()
        snap = {k: getattr(st, k).clone().cpu() for k in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks")}
        snap["games_complete"] = st.games_complete
        snap["state"] = env.export_state().cpu()
        snap["n_obs"] = col.n_obs.clone().cpu(); snap["iters"] = col.iters
        out.append(snap)
        col.after_rollouts()
    assert env.invalid_action_count() == 0 and env.scripted_fallback_count() == 0
    return out


def test_collector_with_a_scripted_opponent(hip_lib):
    """T = 8, N = 64, the three opponent slots of every game played by the bot: the device loop (_gather_device) and the tensor-operation
    loop (_gather_tensor) store identical rollouts, and so does the device loop under the default deferred window."""
    from test_gpu_collector import _same
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    base = _collect(64, 8, 5, 2, False, deferred_window=0)
    assert any(int((s["actions"][:, :, 0] != 0).sum()) > 0 for s in base)
    _same(base, _collect(64, 8, 5, 2, True, deferred_window=0), "device loop")
    assert RolloutCollector.DEFAULT_DEFERRED_WINDOW > 0
    _same(base, _collect(64, 8, 5, 2, True), "device loop, default deferred window")


def test_bad_arguments_name_the_entry_point(hip_lib):
    from settlers_of_catan_rl_amd import _lib
    L = _lib.lib()
    env = _env(64, 0)
    st = stream()
    out = torch.zeros((128, 18), dtype=torch.int32, device="cuda")

    def err(rc):
        assert rc == -1                                  # CATAN_EINVAL (include/catan_hip.h)
        return L.catan_last_error().decode()
    assert "catan_sample_scripted_actions" in err(L.catan_sample_scripted_actions(None, None, 64, P(out), st))
    assert "catan_sample_scripted_actions" in err(L.catan_sample_scripted_actions(env.h, None, 64, None, st))
    assert "catan_sample_scripted_actions" in err(L.catan_sample_scripted_actions(env.h, None, 0, P(out), st))
    assert "catan_sample_scripted_actions" in err(L.catan_sample_scripted_actions(env.h, None, 65, P(out), st))
    assert L.catan_scripted_fallback_count(None, st) == -1
    assert L.catan_sample_scripted_actions(env.h, None, 64, P(out), st) == 0 and L.catan_scripted_fallback_count(env.h, st) == 0
