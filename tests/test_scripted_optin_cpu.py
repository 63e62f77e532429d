"""The opt-in switches of the rule-based baseline player on the CPU: `args.eval_scripted_baseline` of
reference_api.run_evaluation_protocol -> SubProcEvaluationManager.run_evaluation_episodes(scripted_baseline=True),
train_loop.eval_baselines, and `--eval-scripted-baseline` of tools/train.py.  The games run on the oracle; the bot's decisions there
come from the numpy restatement of the rule (tests/scripted_reference.py) behind `sample_scripted_actions`."""
import ctypes as C
import importlib.util
import os
import random
import types

import numpy as np
import torch

import scripted_reference as sr
from oracle_vec_env import OracleVecEnv
from settlers_of_catan_rl_amd import reference_api as ra
from settlers_of_catan_rl_amd import train_loop as tl
from settlers_of_catan_rl_amd.scripted import ScriptedPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["policy_win_frac", "avg_game_length", "avg_policy_decisions", "avg_victory_points"]


class _LateGames(OracleVecEnv):
    """evaluation games that are nearly over (late random-play positions), with the device env's sample_scripted_actions"""
    made = []

    def __init__(self, n):
        super().__init__(n, seed=13, auto_reset=False)
        self.advance_random(1800)
        self.scripted_rows = 0
        _LateGames.made.append(self)

    def sample_scripted_actions(self, games=None, out=None):
        g = np.arange(self.n) if games is None else games.long().numpy()
        a, rows = sr.decide_all(self.export_state().numpy()[g], self.get_action_masks().numpy()[g])
        assert (rows < 13).all()
        self.scripted_rows += len(g)
        return torch.from_numpy(a.astype(np.int32))


class _NetByGame(object):
    """stands where a net does: the oracle's uniform-random legal policy, keyed by game"""
    wants_games = True

    def to(self, dev):
        return self

    def eval(self):
        return self

    def load_reference_state_dict(self, sd):
        self.sd = sd

    def act(self, f, lists, lens, masks, games=None, **_kw):
        env, out = _LateGames.made[-1], np.zeros((f.shape[0], 18), dtype=np.int32)
        for j, i in enumerate(games.tolist()):
            m = np.ascontiguousarray(masks[j].numpy(), dtype=np.float32)
            env.L.orc_sample_action(env.b.env_ptr(i), 5, i, int(env.steps_taken[i]), m.ctypes.data_as(C.POINTER(C.c_float)),
                                    out[j].ctypes.data_as(C.POINTER(C.c_int32)))
        z = torch.zeros((f.shape[0], 1))
        return z, torch.from_numpy(out).long(), z


class _Central(object):
    def state_dict(self):
        return {"w": torch.zeros(1)}


def _protocol(**switch):
    random.seed(4)
    _LateGames.made = []
    mgr = ra.SubProcEvaluationManager([ra.make_evaluation_manager() for _ in range(2)], device="cpu", seed=0, env_factory=_LateGames,
                                      make_policy=_NetByGame, autocast_dtype=None)
    args = types.SimpleNamespace(num_eval_episodes=4, **switch)
    log, summary = ra.run_evaluation_protocol(mgr, _Central(), [], {"w": torch.ones(1)}, args, 3)
    return log, summary, list(_LateGames.made)


def test_reference_api_protocol_switch(oracle):
    plain, plain_summary, envs = _protocol()
    assert list(plain) == ["update", "random"] and list(plain["random"]) == KEYS and len(envs) == 1 and envs[0].scripted_rows == 0
    off, off_summary, envs = _protocol(eval_scripted_baseline=False)
    assert off == plain and off_summary == plain_summary and len(envs) == 1            # default off: the log as it was
    log, summary, envs = _protocol(eval_scripted_baseline=True)
    assert list(log) == ["update", "random", "scripted"] and list(log["scripted"]) == KEYS
    assert log["random"] == plain["random"] and summary.startswith(plain_summary)
    assert "4 games against scripted. Policy won " in summary and summary.count("games against") == 2
    assert len(envs) == 2 and envs[0].scripted_rows == 0 and envs[1].scripted_rows > 0      # the bot played, on the second call's env only
    s = log["scripted"]
    assert 0.0 <= s["policy_win_frac"] <= 1.0 and 0 < s["avg_policy_decisions"] < s["avg_game_length"]


def test_manager_scripted_baseline_seats(oracle):
    """scripted_baseline=True: policy 0 stays the net of update_policies, the other three are one ScriptedPolicy bound to the call's env"""
    from settlers_of_catan_rl_amd import evaluation as ev
    seen = []
    real = ev.run_evaluation_episodes

    def spy(env, nets, orders, **kw):
        seen.append((env, list(nets)))
        return real(env, nets, orders, **kw)
    mgr = ra.SubProcEvaluationManager([ra.make_evaluation_manager()], device="cpu", seed=0, env_factory=_LateGames, make_policy=_NetByGame,
                                      autocast_dtype=None)
    mgr.update_policies([{"w": torch.zeros(1)}] + [{"w": torch.ones(1)}] * 3)
    ev.run_evaluation_episodes = spy
    try:
        out = mgr.run_evaluation_episodes(2, scripted_baseline=True)
        mgr.run_evaluation_episodes(2)
    finally:
        ev.run_evaluation_episodes = real
    (env, nets), (_, plain_nets) = seen
    assert nets[0] is mgr._nets[0] and isinstance(nets[1], ScriptedPolicy) and nets[1] is nets[2] is nets[3] and nets[1].env is env
    assert plain_nets == mgr._nets and not any(isinstance(x, ScriptedPolicy) for x in plain_nets)
    assert len(out) == 1 and len(out[0]) == 4 and all(len(col) == 2 for col in out[0])


def test_train_loop_eval_baselines():
    assert tl.TrainArgs().eval_scripted_baseline is False and tl.eval_baselines(tl.TrainArgs()) is None
    assert tl.eval_baselines(types.SimpleNamespace()) is None
    assert tl.eval_baselines(tl.TrainArgs(eval_scripted_baseline=True)) == {"scripted": ScriptedPolicy}


def _run_train_tool(monkeypatch, extra):
    """tools/train.py's main() with the device objects replaced by stand-ins -> the keyword arguments its evaluation hands to
    evaluation.run_evaluation_protocol"""
    from settlers_of_catan_rl_amd import dist as cdist, env as env_mod, evaluation, policy, rollout, train
    calls = []

    class Obj(object):
        n = 8

        def __init__(self, *a, **kw):
            pass

        def cuda(self):
            return self

        def eval(self):
            return self

    class Loop(object):
        def __init__(self, env, net, col, tr, targs, league=None, make_net=None, evaluate=None, checkpoint_path=None):
            self.net, self.evaluate, Loop.targs = net, evaluate, targs

        def run_update(self):
            log, summary = self.evaluate(self.net, 1)
            return {"update": 0, "eval": summary}

    def protocol(make_env, central, opponent, episodes, update_num, **kw):
        calls.append(kw)
        return {"update": update_num}, "summary"
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(cdist, "init_from_env", lambda *a, **kw: (0, 0, 1))
    for mod, name in ((env_mod, "VecCatanEnv"), (policy, "CatanPolicy"), (rollout, "RolloutCollector"), (train, "PPOTrainer")):
        monkeypatch.setattr(mod, name, Obj)
    monkeypatch.setattr(tl, "TrainingLoop", Loop)
    monkeypatch.setattr(evaluation, "run_evaluation_protocol", protocol)
    monkeypatch.setattr("sys.argv", ["train.py", "--updates", "1", "--league", "0"] + extra)
    spec = importlib.util.spec_from_file_location("train_tool_under_test", os.path.join(ROOT, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main()
    assert len(calls) == 1
    return calls[0], Loop.targs


def test_train_tool_flag(monkeypatch, capsys):
    kw, targs = _run_train_tool(monkeypatch, [])
    assert kw["baselines"] is None and targs.eval_scripted_baseline is False
    kw, targs = _run_train_tool(monkeypatch, ["--eval-scripted-baseline"])
    assert kw["baselines"] == {"scripted": ScriptedPolicy} and targs.eval_scripted_baseline is True
    capsys.readouterr()
