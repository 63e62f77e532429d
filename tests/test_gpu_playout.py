"""GPU: the playout player (csrc/catan_players.hip) - catan_playout_actions against the restatement of its decision over
the CPU oracle (tests/playout_reference.py), integer for integer, on the roots of tests/test_playout_reference_cpu.py (initial
placements, turns, answers to offers, a discard, a planted win in one); the root handle untouched; determinism; the forms of `games`;
every refusal; legal and teacher-forceable rows; the player in evaluation games and as a collector's teacher."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import playout_reference as pr
import scripted_reference as sr
from guarded import ptr as P, stream as _stream
from settlers_of_catan_rl_amd import _lib, spec

pytestmark = pytest.mark.gpu

SIM_GAMES = 300                 # 7 x 5 x 3 = 105 and 3 x 8 x 12 = 288 slots in use: a tail of untouched slots either way
ROWS7 = [0, 3, 5, 7, 9, 11, 16]  # initial, initial, respond, turn, turn, discard, the planted position
ROWS3 = [2, 16, 10]
F = pr.FIELDS


def _env(n, seed, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def _roots():
    return np.concatenate([pr.fixture_roots(), pr.near_win_root()[None]])


def _root_env(**kw):
    env = _env(17, 3, **kw)
    env.import_state(torch.from_numpy(_roots()))
    return env


def _sim_env(n=SIM_GAMES, **kw):
    return _env(n, pr.SIM_SEED, env_id0=pr.SIM_ENV_ID0, auto_reset=False, **kw)


def _cfg(builder=1, trader=1, randoms=3, playouts=3, depth=2, playout_style="trader", determinise=1, step_idx=3):
    return dict(builder=builder, trader=trader, randoms=randoms, playouts=playouts, depth=depth, playout_style=playout_style,
                determinise=determinise, step_idx=step_idx)


@functools.lru_cache(maxsize=None)
def _reference(games, items):
    """computed once per (games, cfg), shared by the tests that need it, never edited"""
    return pr.decide(_roots(), None if games is None else list(games), dict(items), pr.SIM_SEED, pr.SIM_ENV_ID0)


def _ref(games, cfg):
    return _reference(None if games is None else tuple(games), tuple(sorted(cfg.items())))


def _call(root, sim, games, cfg):
    g = None if games is None else torch.tensor(games, dtype=torch.int32, device="cuda")
    a, chosen, stats = root.playout_actions(sim, g, candidates=(cfg["builder"], cfg["trader"], cfg["randoms"]), playouts=cfg["playouts"],
                                            depth=cfg["depth"], playout_style=cfg["playout_style"], determinise=cfg["determinise"],
                                            step_idx=cfg["step_idx"], return_stats=True)
    return a.cpu().numpy(), chosen.cpu().numpy(), stats.cpu().numpy()


PARITY = [("7x5x3 depth 40 trader determinised", ROWS7, _cfg(depth=40)),
          ("7x5x3 depth 2 trader open", ROWS7, _cfg(determinise=0)),
          ("7x5x3 depth 2 builder determinised", ROWS7, _cfg(playout_style="builder")),
          ("7x5x3 depth 2 builder open", ROWS7, _cfg(playout_style="builder", determinise=0)),
          ("7x5x3 depth 1", ROWS7, _cfg(depth=1)),
          ("3x8x12 depth 2", ROWS3, _cfg(randoms=6, playouts=12)),
          ("3x8x12 depth 40 builder", ROWS3, _cfg(randoms=6, playouts=12, depth=40, playout_style="builder")),
          ("17x1x1 depth 1", None, _cfg(trader=0, randoms=0, playouts=1, depth=1)),
          ("17x1x1 depth 40 random only", None, _cfg(builder=0, trader=0, randoms=1, playouts=1, depth=40)),
          ("17x4x2 depth 2 all roots", None, _cfg(randoms=2, playouts=2))]


@pytest.mark.parametrize("name,games,cfg", PARITY, ids=[p[0] for p in PARITY])
def test_parity_with_the_reference(hip_lib, name, games, cfg):
    """actions, chosen and every stats field equal the reference's; the playouts took no illegal action; one sim handle serves a second,
    different call (its games are scratch)"""
    root, sim = _root_env(), _sim_env()
    want = _ref(games, cfg)
    a, chosen, stats = _call(root, sim, games, cfg)
    print(name, "chosen", chosen.tolist(), "score sums", stats[:, :, F["score_sum"]].tolist(), "steps", stats[:, :, F["steps_sum"]].tolist())
    assert want.invalid == 0
    assert np.array_equal(stats, want.stats), (stats.tolist(), want.stats.tolist())
    assert np.array_equal(chosen, want.chosen) and np.array_equal(a, want.actions)
    assert sim.invalid_action_count() == 0
    other = _cfg(randoms=2, playouts=2, depth=1, determinise=0)
    a2, chosen2, stats2 = _call(root, sim, [16, 4], other)
    want2 = _ref([16, 4], other)
    assert np.array_equal(stats2, want2.stats) and np.array_equal(chosen2, want2.chosen) and np.array_equal(a2, want2.actions)


def test_planted_win_in_one(hip_lib):
    K = 4
    cfg = _cfg(playouts=K, depth=1)
    a, chosen, stats = _call(_root_env(), _sim_env(), [16], cfg)
    assert a[0].tolist() == [sr.CITY, 0] + [0] * 16 and chosen[0] == 0
    assert stats[0, 0].tolist() == [1, K, K, K, K * (1000 + 10 * (10 - 2)), K * 10, K] and not stats[0, 1].any()


def _snapshot(env):
    cnt = env.scripted_trade_counts()
    return dict(state=env.export_state().cpu(), masks=env.get_action_masks_packed().clone().cpu(), trade=cnt, fallback=env.scripted_fallback_count(),
                invalid=env.invalid_action_count(), counters=env.policy_counters().cpu())


def test_the_root_is_untouched(hip_lib):
    root, twin, sim = _root_env(), _root_env(), _sim_env()
    for e in (root, twin):                          # both styles have sampled on the root before: its counter blocks exist and hold something
        e.sample_scripted_actions()
        e.sample_scripted_actions(style="trader")
    before = _snapshot(root)
    _call(root, sim, ROWS7, _cfg(depth=6))
    _call(root, sim, None, _cfg(randoms=2, playouts=2, depth=3))
    after = _snapshot(root)
    for k in ("state", "masks", "counters"):
        assert torch.equal(before[k], after[k]), k
    assert before["trade"] == after["trade"] and before["trade"]["decisions"] == 17
    assert before["fallback"] == after["fallback"] and before["invalid"] == after["invalid"] == 0
    acts = twin.sample_scripted_actions(style="trader")
    assert torch.equal(acts, root.sample_scripted_actions(style="trader"))
    (r1, d1), (r2, d2) = root.step(acts), twin.step(acts)
    assert torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(root.export_state(), twin.export_state())
    assert torch.equal(root.get_action_masks_packed(), twin.get_action_masks_packed())


def test_determinism_and_step_idx(hip_lib):
    root = _root_env()
    cfg = _cfg(depth=12)
    first, again = _call(root, _sim_env(), ROWS7, cfg), _call(root, _sim_env(), ROWS7, cfg)
    sim = _sim_env()
    _call(root, sim, ROWS3, _cfg(randoms=6, playouts=12, depth=5))          # a used sim handle gives the same as a fresh one
    third = _call(root, sim, ROWS7, cfg)
    for x, y, z in zip(first, again, third):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # another step index: other random candidates, the builder's and the trader's as before
    want3, want4 = _ref(ROWS7, cfg), _ref(ROWS7, dict(cfg, step_idx=4))
    assert np.array_equal(want3.cand[:, :2], want4.cand[:, :2]) and not np.array_equal(want3.cand[:, 2:], want4.cand[:, 2:])
    a4, chosen4, stats4 = _call(root, _sim_env(), ROWS7, dict(cfg, step_idx=4))
    assert np.array_equal(stats4, want4.stats) and np.array_equal(chosen4, want4.chosen) and np.array_equal(a4, want4.actions)
    assert np.array_equal(stats4[:, :2, F["valid"]], first[2][:, :2, F["valid"]])


def test_the_forms_of_games(hip_lib):
    root = _root_env()
    cfg = _cfg(randoms=2, playouts=2)
    implicit, explicit = _call(root, _sim_env(), None, cfg), _call(root, _sim_env(), list(range(17)), cfg)
    for x, y in zip(implicit, explicit):
        assert np.array_equal(x, y)
    # a game listed twice: two rows in different slots - equal candidates, independently played; bad ids between them
    games = [10, -1, 10, 17, 16, 1 << 20]
    cfg = _cfg(depth=40, randoms=0)
    a, chosen, stats = _call(root, _sim_env(), games, cfg)
    want = _ref(games, cfg)
    assert np.array_equal(stats, want.stats) and np.array_equal(chosen, want.chosen) and np.array_equal(a, want.actions)
    # (game 10 is chosen so that the two rows' dice - the slots' own streams - lead to different sums: the rows are played independently)
    assert np.array_equal(want.cand[0], want.cand[2]) and not np.array_equal(want.stats[0], want.stats[2])
    for j in (1, 3, 5):
        assert a[j].tolist() == [sr.ENDTURN] + [0] * 17 and chosen[j] == -1 and not stats[j].any()


def test_every_refusal(hip_lib):
    L = hip_lib
    root, sim = _root_env(), _sim_env()
    _call(root, sim, ROWS3, _cfg())
    sim_before = sim.export_state().cpu()
    out = torch.full((17, 18), -9, dtype=torch.int32, device="cuda")
    chosen = torch.full((17,), -9, dtype=torch.int32, device="cuda")
    stats = torch.full((17, 8, 7), -9, dtype=torch.int64, device="cuda")
    games = torch.arange(17, dtype=torch.int32, device="cuda")
    good = dict(builder=1, trader=1, randoms=2, playouts=2, depth=2, playout_style=1, determinise=1, step_idx=0)

    def refused(r=root, s=sim, g=games, rows=4, use_cfg=True, actions=out, **edit):
        cfg = _lib.CatanPlayoutCfg(**dict(good, **edit))
        rc = L.catan_playout_actions(r.h if r is not None else None, s.h if s is not None else None, P(g), rows, C.byref(cfg) if use_cfg else None,
                                     P(actions), P(chosen), P(stats), _stream())
        assert rc == -1, (rc, edit)                                  # CATAN_EINVAL (include/catan_hip.h)
        msg = L.catan_last_error().decode()
        assert "catan_playout_actions" in msg, msg
        return msg
    assert "null handle" in refused(r=None) and "null handle" in refused(s=None)
    assert "null cfg" in refused(use_cfg=False)
    assert "null actions" in refused(actions=None)
    assert "same handle" in refused(s=root)
    auto = _env(64, 1)                                               # auto_reset = 1
    assert "auto_reset" in refused(s=auto)
    for kw in (dict(max_proposed_trades_per_turn=2), dict(max_actions_per_turn=50)):
        assert "differ" in refused(s=_sim_env(64, **kw))
    assert "n_rows" in refused(rows=0) and "n_rows" in refused(rows=-3)
    assert "root handle's games" in refused(g=None, rows=18)
    assert "exceeds the sim handle" in refused(rows=17, randoms=6, playouts=3)       # 17 x 8 x 3 = 408 > 300
    assert "exceeds the sim handle" in refused(rows=1 << 40)
    for edit in (dict(builder=0, trader=0, randoms=0), dict(randoms=7), dict(randoms=-1), dict(builder=2), dict(trader=-1)):
        refused(**edit)
    for edit in (dict(playouts=0), dict(playouts=65), dict(depth=0), dict(depth=-1), dict(playout_style=2), dict(playout_style=-1)):
        refused(**edit)
    mt_root, mt_sim = _env(1, 0), _env(1, 0, auto_reset=False)
    mt_root.seed_mt19937(1, 2); mt_sim.seed_mt19937(1, 2)
    assert "MT19937" in refused(r=mt_root, g=None, rows=1, randoms=0, trader=0, playouts=1)
    assert "MT19937" in refused(s=mt_sim, g=None, rows=1, randoms=0, trader=0, playouts=1)
    for which in ("root", "sim"):                                    # an open catan_step_deferred sequence on either handle
        r2, s2 = _root_env(), _sim_env()
        e = r2 if which == "root" else s2
        e.step_deferred(e.sample_random_actions(0), window=4)
        assert "deferred" in refused(r=r2, s=s2)
        e.step_flush()
    torch.cuda.synchronize()
    assert bool((out == -9).all()) and bool((chosen == -9).all()) and bool((stats == -9).all())     # nothing was launched
    assert torch.equal(sim.export_state().cpu(), sim_before)
    with pytest.raises(ValueError, match="playout_style"):
        root.playout_actions(sim, candidates=(1, 1, 2), playouts=2, depth=2, playout_style="banker", determinise=True, step_idx=0)
    assert L.catan_playout_actions(root.h, sim.h, P(games), 4, C.byref(_lib.CatanPlayoutCfg(**good)), P(out), None, None, _stream()) == 0      # chosen, stats: optional
    torch.cuda.synchronize()
    assert bool((out[:4, 0] >= 0).all()) and bool((out[4:] == -9).all())


def test_chosen_rows_are_legal_and_teacher_forceable(hip_lib):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy
    root = _root_env()
    pol = PlayoutPolicy(root, randoms=2, playouts=2, depth=6, sim_games=5 * 8, seed=pr.SIM_SEED)       # 5 rows a call: 4 chunks for 17 games
    f, lists, lens = root.get_obs()
    masks = root.get_action_masks()
    _, a, _ = pol.act(f, lists, lens, masks)
    assert pol.last_stats.shape == (17, 4, 7) and pol.last_chosen.shape == (17,) and pol.step_idx == 4        # a step index per chunk
    roots = _roots()
    import oracle_lib
    for g in range(17):
        env = oracle_lib.OracleEnv(0, g)
        env.import_(roots[g])
        assert env.is_legal(a[g].cpu().numpy().astype(np.int32)), (g, a[g].tolist())
    twin = _root_env()
    twin.step(a.to(torch.int32))
    assert twin.invalid_action_count() == 0
    pol.step_idx = 0
    labels = pol.label()
    assert torch.equal(labels[:, 0].long(), a[:, 0]) and labels.dtype == torch.int32
    torch.manual_seed(3)
    net = CatanPolicy().cuda().eval()
    with torch.no_grad():
        _, acts, _ = net.act(f, lists, lens.long(), masks)
        out = net.evaluate_actions(f, lists, lens.long(), masks, acts, teacher_actions=labels.long())
    assert len(out) == 4 and out[3].shape == (17, 1) and bool(torch.isfinite(out[3]).all())
    assert pol.sim.invalid_action_count() == 0


def test_evaluation_games_with_the_playout_player(hip_lib):
    """8 games, PlayoutPolicy in seat 0 against three builders, at most 60 steps: they run and return winners (no strength is claimed)"""
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, ScriptedPolicy
    env = _env(8, 21, auto_reset=False)
    pol, bot = PlayoutPolicy(env, randoms=1, playouts=2, depth=4), ScriptedPolicy(env)
    res = ev.run_evaluation_episodes(env, [pol, bot, bot, bot], ev.sample_orders(8, random.Random(3)), max_steps=60)
    assert res["winner"].shape == (8,) and set(res["winner"].tolist()) <= {-1, 0, 1, 2, 3} and (res["game_steps"] > 0).all()
    assert pol.step_idx > 0 and pol.sim.n == 3 * 2 * 8 and env.invalid_action_count() == 0 and pol.sim.invalid_action_count() == 0


def _collector(n, T, **ckw):
    """a collector at its DEFAULT arguments (no deferred_window given) over an env some way into its games"""
    import rollout_fixture as rf
    from test_gpu_collector import SamplerPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    env = _env(n, 5)
    env.random_rollout(0, 60)
    cenv = rf.CountingEnv(env)
    return env, cenv, SamplerPolicy(cenv), RolloutCollector


def test_collector_with_a_playout_teacher(hip_lib):
    """T = 4, N = 8, the collector's default arguments: RolloutCollector(teacher=PlayoutPolicy(env)) steps lock-step on its own account
    (the player forks the env's games, which an open catan_step_deferred sequence forbids) and fills storage.teacher_actions with
    completed rows of legal types, two rollouts in a row; a deferred window asked for explicitly is refused with the reason"""
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, TraderPolicy
    env, cenv, sampler, RolloutCollector = _collector(8, 4)
    pol = PlayoutPolicy(env, randoms=1, playouts=2, depth=3)
    col = RolloutCollector(cenv, sampler, 4, seed=5, teacher=pol)
    assert col.deferred_window == 0
    for _ in range(2):
        st = col.gather_rollouts()
        labels, n_act = st.teacher_actions.cpu().numpy(), col.n_act.cpu().numpy()
        assert labels.shape == (4, 8, 18) and n_act.sum() > 0 and pol.step_idx > 0
        for g in range(8):
            k = min(int(n_act[g]), 4)
            assert ((labels[:k, g, 0] >= 0) & (labels[:k, g, 0] <= 12)).all()
        col.after_rollouts()
    assert env.invalid_action_count() == 0 and pol.sim.invalid_action_count() == 0
    with pytest.raises(ValueError, match="lock-step"):
        RolloutCollector(cenv, sampler, 4, seed=5, teacher=PlayoutPolicy(env), deferred_window=4)
    RolloutCollector(cenv, sampler, 4, seed=5, teacher=PlayoutPolicy(env), deferred_window=0)
    assert RolloutCollector(cenv, sampler, 4, seed=5, teacher=TraderPolicy(env)).deferred_window == RolloutCollector.DEFAULT_DEFERRED_WINDOW      # the rule tables keep the default


def test_collector_with_a_playout_opponent(hip_lib):
    """T = 4, N = 8, the collector's default arguments: the three opponent slots of every game played by PlayoutPolicy(env); two rollouts
    run, the player decided, nothing illegal was stepped on either handle; an explicit deferred window is refused here too"""
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy
    env, cenv, sampler, RolloutCollector = _collector(8, 4)
    pol = PlayoutPolicy(env, randoms=1, playouts=2, depth=3)
    col = RolloutCollector(cenv, sampler, 4, opponents=[pol], seed=5)
    assert col.deferred_window == 0
    for _ in range(2):
        st = col.gather_rollouts()
        assert st.actions.shape[:2] == (4, 8) and int(col.n_act.sum()) > 0
        col.after_rollouts()
    assert pol.step_idx > 0 and pol.last_stats is not None and pol.last_stats.shape[1:] == (3, 7)
    assert env.invalid_action_count() == 0 and pol.sim.invalid_action_count() == 0
    with pytest.raises(ValueError, match="lock-step"):
        RolloutCollector(cenv, sampler, 4, opponents=[PlayoutPolicy(env)], seed=5, deferred_window=4)
