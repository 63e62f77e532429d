"""Kickstarting from a teacher on the CPU: teacher labels in the rollout collector (oracle-backed env, the numpy twins
of the rule-based player and of the row completion as the teacher), the torch form of the imitation loss against hand numbers, the
trainer with the imitation term, the training loop's schedule and the flags of tools/train.py.

The oracle env has no device loop: the collector runs its tensor-operation loop here; tests/test_gpu_teacher.py compares the two loops."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import action_complete_reference as acr
import scripted_reference as sr
from oracle_vec_env import OracleVecEnv, ScriptedPolicy as RandomPolicy
from settlers_of_catan_rl_amd import ppo, train_loop as tl
from settlers_of_catan_rl_amd.rollout import RolloutCollector, RolloutStorage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGE_KEYS = ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks")


class TwinTeacher(object):
    """scripted_reference.decide + action_complete_reference.complete on the oracle env's games: what ScriptedPolicy.label is on the device"""

    def __init__(self, env):
        self.env, self.calls = env, 0

    def label(self, games=None):
        assert games is None
        env = self.env
        self.calls += 1
        masks = env.get_action_masks().numpy()
        rows, _ = sr.decide_all(env.export_state().numpy(), masks)
        return torch.from_numpy(acr.complete_all(rows, masks, env.get_obs()[0][:, 12:18].numpy()).astype(np.int32))


class SpyEnv(object):
    """delegates to the env and keeps, for every step, the games as they were decided in"""

    def __init__(self, env):
        self.env, self.log = env, []

    def step(self, a):
        env = self.env
        self.log.append((env.export_state().numpy().copy(), env.get_action_masks().numpy().copy(), env.get_obs()[0][:, 12:18].numpy().copy(),
                         env.deciding_player().numpy().copy(), (a[:, 0] >= 0).numpy().copy()))
        return env.step(a)

    def __getattr__(self, name):
        return getattr(self.env, name)


def _collect(n, T, gathers, teacher):
    env = SpyEnv(OracleVecEnv(n, seed=11))
    env.advance_random(700)                                  # late games: ends, re-deals and the carry-over between rollouts
    t = TwinTeacher(env) if teacher else None
    col = RolloutCollector(env, RandomPolicy(env), T, seed=3, teacher=t)
    out = []
    for _ in range(gathers):
        first = len(env.log)
        st = col.gather_rollouts()
        snap = {k: getattr(st, k).clone() for k in STORAGE_KEYS}
        snap["teacher_actions"] = None if st.teacher_actions is None else st.teacher_actions.clone()
        snap["n_act"], snap["log"], snap["iters"] = col.n_act.clone(), env.log[first:], col.iters
        out.append(snap)
        col.after_rollouts()
    return out, col, t


def test_collector_stores_the_labels_of_the_stored_decisions(oracle):
    n, T = 16, 8
    with_t, col, teacher = _collect(n, T, 2, True)
    without, col0, _ = _collect(n, T, 2, False)
    assert col0.storage.teacher_actions is None and col.storage.teacher_actions.dtype == torch.int16
    assert col.storage.teacher_actions.shape == (T, n, 18)
    active = col.active_pid.numpy()
    stored = 0
    for snap, plain in zip(with_t, without):
        for k in STORAGE_KEYS:                               # nothing else in the storage changes with a teacher
            assert torch.equal(snap[k], plain[k]), k
        assert len(snap["log"]) == len(plain["log"])
        # the labels recomputed from the states the stored decisions were taken in
        n_act = np.zeros(n, dtype=np.int64)
        want = np.full((T, n, 18), -99, dtype=np.int64)
        for blobs, masks, res, deciding, live in snap["log"]:
            for g in range(n):
                if live[g] and deciding[g] == active[g]:
                    t = min(int(n_act[g]), T - 1)
                    want[t, g] = acr.complete(sr.decide(blobs[g], masks[g])[0], masks[g], res[g])
                    # (the slot is the one the net's action went into: its packed mask row is this state's)
                    assert torch.equal(col.storage.unpack_action_masks(snap["action_masks"][t, g]), torch.from_numpy(masks[g]))
                    n_act[g] += 1
        assert np.array_equal(n_act, snap["n_act"].numpy())
        got = snap["teacher_actions"].numpy()
        for g in range(n):
            k = min(int(n_act[g]), T)
            assert np.array_equal(got[:k, g], want[:k, g]), (g, got[:k, g], want[:k, g])
            stored += k
    assert stored >= n * T                                   # (two rollouts of T decisions per game, minus the games cut short)
    assert teacher.calls == sum(len(s["log"]) for s in with_t)          # one label call per env iteration
    # stop_teacher: no further label call, the tensor is freed, the collector goes on as one without a teacher
    col.stop_teacher()
    assert col.teacher is None and col.storage.teacher_actions is None
    col.gather_rollouts()
    assert teacher.calls == sum(len(s["log"]) for s in with_t)


def test_a_teacher_is_refused_with_an_lstm_policy(oracle):
    from oracle_vec_env import RecurrentScriptedPolicy
    env = OracleVecEnv(4, seed=1)
    with pytest.raises(ValueError, match="LSTM"):
        RolloutCollector(env, RecurrentScriptedPolicy(env), 4, teacher=TwinTeacher(env))
    with pytest.raises(ValueError, match="label"):
        RolloutCollector(env, RandomPolicy(env), 4, teacher=object())
    assert RolloutStorage(4, 2, "cpu").teacher_actions is None


# ---------------------------------------------------------------------------------------------- the loss
def test_torch_form_against_hand_numbers():
    f32 = lambda x: float(np.float32(x))
    half = f32(-0.6931472)
    # rows: -inf, NaN, then one row of each type; types 0 and 1 straddle log(1/2) by one fp32 step, type 2 sits exactly on it
    lps = [-math.inf, math.nan, float(np.nextafter(np.float32(half), np.float32(0))), float(np.nextafter(np.float32(half), np.float32(-1))), half,
           0.0, -0.25, -1.5, -2.0, -3.25, -0.125, -7.0, -0.5, -1.0, -4.0]
    types = [3, 12] + list(range(13))
    rows = torch.zeros((15, 18), dtype=torch.int64)
    rows[:, 0] = torch.tensor(types)
    rows[:, 1:] = 5                                          # (only column 0 is read)
    lp = torch.tensor(lps, dtype=torch.float32, requires_grad=True)
    block = torch.zeros(33, dtype=torch.float64)
    loss = ppo.imitation_loss(lp, rows, block)
    finite = [f32(x) for x in lps[2:]]
    total = -sum(finite)                                     # (all exactly representable sums of fp32 values in fp64)
    assert float(loss.detach()) == f32(total / 15.0)
    (3.0 * loss).backward()
    g = f32(-1.0 / 15.0)
    assert lp.grad.tolist() == [0.0, 0.0] + [f32(3.0 * g)] * 13
    w = block.tolist()
    assert w[0] == 15.0 and w[1] == 1.0 and w[2] == total and w[3] == 7.0 and w[5] == 2.0 and w[32] == 0.0
    assert w[4] == sum(1 for x in finite if np.float32(x) > np.float32(-0.6931472)) == 5     # the step above log(1/2), 0, -0.25, -0.125, -0.5 - and not log(1/2) itself
    assert w[6:19] == [1.0] * 13 and w[19:32] == [-x for x in finite]
    # a second call accumulates: sums add, the maximum stays, the skipped rows' types are not counted
    loss2 = ppo.imitation_loss(torch.tensor([-8.0, -math.inf]), rows[:2], block)
    assert float(loss2) == 4.0
    w = block.tolist()
    assert w[0] == 17.0 and w[1] == 2.0 and w[2] == total + 8.0 and w[3] == 8.0 and w[5] == 3.0 and w[6 + 3] == 2.0 and w[6 + 12] == 1.0
    assert w[19 + 3] == 0.0 + 8.0
    s = ppo.imitation_summary(block.numpy())
    assert s["rows"] == 17 and s["steps"] == 2 and s["skipped"] == 3 and s["nll"] == (total + 8.0) / 14.0 and s["nll_max"] == 8.0
    assert s["half_share"] == 5.0 / 14.0 and s["rows_by_type"][3] == 2 and s["nll_by_type"][3] == 4.0 and len(s["nll_by_type"]) == 13
    import json
    json.dumps(s)


def test_block_and_rows_are_checked():
    rows = torch.zeros((4, 18), dtype=torch.int64)
    lp = torch.zeros(4)
    for bad in (torch.zeros(32, dtype=torch.float64), torch.zeros(33, dtype=torch.float32), torch.zeros(66, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError):
            ppo.imitation_loss(lp, rows, bad)
    with pytest.raises(ValueError):
        ppo.imitation_loss(lp, rows[:3], torch.zeros(33, dtype=torch.float64))
    assert ppo.reduce_imitation_over_ranks(torch.ones(33, dtype=torch.float64)).tolist() == [1.0] * 33      # (one rank: untouched)


# ---------------------------------------------------------------------------------------------- the trainer
T_TRAIN, N_TRAIN = 16, 64                                    # one fixed rollout of 1 024 rows


@pytest.fixture(scope="module")
def rollout(oracle):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(7)
    env = OracleVecEnv(N_TRAIN, seed=5)
    env.advance_random(200)
    col = RolloutCollector(env, CatanPolicy().eval(), T_TRAIN, seed=2, teacher=TwinTeacher(env))
    return col.gather_rollouts()


@pytest.fixture()
def cpu_backends():
    from test_ppo_diag_cpu import _install_cpu_backends
    saved = _install_cpu_backends()
    yield
    ppo._gae_raw, ppo._adv_normalise, ppo._loss_backend = saved


def _trainer(**cfg):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    torch.manual_seed(123)
    return PPOTrainer(CatanPolicy(), PPOConfig(**cfg), autocast_dtype=None, seed=0)


def _without_labels(st):
    out = RolloutStorage(st.T, st.N, "cpu")
    for k in STORAGE_KEYS:
        setattr(out, k, getattr(st, k))
    return out


def test_zero_coefficient_is_the_parent_path(rollout, cpu_backends):
    from settlers_of_catan_rl_amd.train import PPOConfig
    assert PPOConfig.teacher_coef == 0.0 and PPOConfig.teacher_only is False
    a, b = _trainer(ppo_epoch=1, num_mini_batch=2), _trainer(ppo_epoch=1, num_mini_batch=2, teacher_coef=0.0)
    la, lb = a.update(_without_labels(rollout)), b.update(rollout)
    assert la == lb and a.teacher is None and b.teacher is None
    sa, sb = a.policy.state_dict(), b.policy.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_configurations_that_cannot_run(rollout, cpu_backends):
    with pytest.raises(ValueError, match="teacher_actions"):
        _trainer(ppo_epoch=1, num_mini_batch=1, teacher_coef=1.0).update(_without_labels(rollout))
    with pytest.raises(ValueError, match="target_kl"):
        _trainer(ppo_epoch=1, num_mini_batch=1, teacher_coef=1.0, teacher_only=True, diagnostics=True, target_kl=0.1).update(rollout)
    with pytest.raises(ValueError, match="teacher_coef"):
        _trainer(ppo_epoch=1, num_mini_batch=1, teacher_only=True).update(rollout)


def _nll(pol, st):
    T, total = st.T, st.T * st.N
    with torch.no_grad():
        r = pol.evaluate_actions(st.obs_f[:T].reshape(total, -1), st.lists[:T].reshape(total, 5, -1), st.lens[:T].reshape(total, 5).long(),
                                 st.unpack_action_masks(st.action_masks.reshape(total, -1)), st.actions.reshape(total, -1),
                                 teacher_actions=st.teacher_actions.reshape(total, -1).long())
    assert len(r) == 4 and r[3].shape == (total, 1) and bool(torch.isfinite(r[3]).all())
    return float(-r[3].double().mean()), r


def test_teacher_only_lowers_the_nll_in_twenty_steps(rollout, cpu_backends):
    """pure imitation on one fixed rollout of 1 024 rows: 20 optimiser steps at lr 3e-4 (measured: 1.410 -> 1.086 in the experiment of
    the issue, on other rows of the same play)"""
    tr = _trainer(ppo_epoch=20, num_mini_batch=1, teacher_coef=1.0, teacher_only=True, lr=3e-4)
    before, r = _nll(tr.policy, rollout)
    # without teacher_actions the call is the parent's
    with torch.no_grad():
        T, total = rollout.T, rollout.T * rollout.N
        plain = tr.policy.evaluate_actions(rollout.obs_f[:T].reshape(total, -1), rollout.lists[:T].reshape(total, 5, -1),
                                           rollout.lens[:T].reshape(total, 5).long(),
                                           rollout.unpack_action_masks(rollout.action_masks.reshape(total, -1)), rollout.actions.reshape(total, -1))
    assert len(plain) == 3 and all(torch.equal(x, y) for x, y in zip(plain, r[:3]))
    vl, al, el = tr.update(rollout)
    after, _ = _nll(tr.policy, rollout)
    t = tr.teacher
    print(f"teacher NLL on the rollout: {before:.4f} -> {after:.4f}; read-out: {t['nll']:.4f} mean over the update, {t['half_share']:.3f} p > 1/2, {t['skipped']} skipped")
    assert after < before
    assert t["rows"] == 20 * T_TRAIN * N_TRAIN and t["steps"] == 20 and t["skipped"] == 0 and sum(t["rows_by_type"]) == t["rows"]
    assert after < t["nll"] < before + 1e-3                  # the update's mean lies between its ends
    assert al == 0.0                                         # zero advantages: no policy-gradient term


# ---------------------------------------------------------------------------------------------- the loop and the tool
def test_decay_schedule():
    a = tl.TrainArgs(teacher="scripted", teacher_coef=0.5, teacher_coef_updates=4, teacher_only_updates=2)
    assert [tl.teacher_coef_at(u, a) for u in range(6)] == [0.5, 0.375, 0.25, 0.125, 0.0, 0.0]
    assert tl.teacher_coef_at(100, tl.TrainArgs(teacher="scripted", teacher_coef=0.5)) == 0.5          # no decay asked for
    assert tl.teacher_coef_at(0, tl.TrainArgs()) == 0.0 and tl.teacher_coef_at(0, tl.TrainArgs(teacher_coef=1.0)) == 0.0
    d = tl.TrainArgs()
    assert d.teacher is None and d.teacher_coef == 0.0 and d.teacher_coef_updates == 0 and d.teacher_only_updates == 0
    assert tl.make_teacher(d, object()) is None and tl.make_teacher(tl.TrainArgs(teacher="scripted"), object()) is None
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = object()
    t = tl.make_teacher(a, env)
    assert isinstance(t, ScriptedPolicy) and t.env is env
    with pytest.raises(ValueError):
        tl.make_teacher(tl.TrainArgs(teacher="net", teacher_coef=1.0), env)


class _Env(object):
    n = 10


class _Storage(object):
    games_complete = 0


class _Collector(object):
    N = 10

    def __init__(self, teacher):
        self.teacher, self.seen, self.stopped = teacher, [], 0

    def stop_teacher(self):
        self.teacher, self.stopped = None, self.stopped + 1

    def gather_rollouts(self):
        self.seen.append(self.teacher)
        return _Storage()

    def after_rollouts(self):
        pass


class _Trainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)

        class Cfg:
            entropy_coef, teacher_coef, teacher_only = 0.0, 0.0, False
        self.cfg, self.seen, self.teacher = Cfg(), [], None

    def update(self, st):
        self.seen.append((self.cfg.teacher_coef, self.cfg.teacher_only))
        self.teacher = {"nll": 1.0} if self.cfg.teacher_coef > 0 else None
        return (0.1, 0.2, 0.3)


def test_run_update_drives_the_schedule():
    net = torch.nn.Linear(3, 3)
    args = tl.TrainArgs(num_steps=4, total_env_steps=4 * 10 * 50, teacher="scripted", teacher_coef=0.5, teacher_coef_updates=2, teacher_only_updates=1)
    teacher = object()
    col, tr = _Collector(teacher), _Trainer(net)
    loop = tl.TrainingLoop(_Env(), net, col, tr, args)
    outs = [loop.run_update() for _ in range(4)]
    assert tr.seen == [(0.5, True), (0.25, False), (0.0, False), (0.0, False)]
    assert col.seen == [teacher, teacher, None, None] and col.stopped == 1     # behind the decay the collector stops labelling, once
    assert [("teacher" in o) for o in outs] == [True, True, False, False] and outs[0]["teacher"] == {"nll": 1.0}
    # no teacher configured: the trainer's configuration and the collector are not touched
    col, tr = _Collector(None), _Trainer(net)
    out = tl.TrainingLoop(_Env(), net, col, tr, tl.TrainArgs(num_steps=4, total_env_steps=4 * 10 * 50)).run_update()
    assert tr.seen == [(0.0, False)] and "teacher" not in out
    with pytest.raises(ValueError, match="make_teacher"):
        tl.TrainingLoop(_Env(), net, _Collector(None), _Trainer(net), args).run_update()


def _run_train_tool(monkeypatch, extra):
    """tools/train.py's main() with the device objects replaced by stand-ins -> (the collector's keyword arguments, the TrainArgs)"""
    from settlers_of_catan_rl_amd import dist as cdist, env as env_mod, policy, rollout, train
    made = {}

    class Obj(object):
        n = 8

        def __init__(self, *a, **kw):
            made.setdefault(type(self).__name__, []).append(kw)

        def cuda(self):
            return self

        def eval(self):
            return self

    class Collector(Obj):
        pass

    class Loop(object):
        def __init__(self, env, net, col, tr, targs, **kw):
            Loop.targs = targs

        def run_update(self):
            return {"update": 0, "eval": None}
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(cdist, "init_from_env", lambda *a, **kw: (0, 0, 1))
    for mod, name, cls in ((env_mod, "VecCatanEnv", Obj), (policy, "CatanPolicy", Obj), (rollout, "RolloutCollector", Collector), (train, "PPOTrainer", Obj)):
        monkeypatch.setattr(mod, name, cls)
    monkeypatch.setattr(tl, "TrainingLoop", Loop)
    monkeypatch.setattr("sys.argv", ["train.py", "--updates", "1", "--league", "0"] + extra)
    spec = importlib.util.spec_from_file_location("train_tool_under_test", os.path.join(ROOT, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main()
    return made["Collector"][0], Loop.targs


def test_train_tool_flags(monkeypatch, capsys):
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    kw, targs = _run_train_tool(monkeypatch, [])
    assert "teacher" not in kw and "teacher" not in targs.__dict__ and targs.teacher is None           # the defaults make no call
    kw, targs = _run_train_tool(monkeypatch, ["--teacher", "scripted", "--teacher-coef", "0.5", "--teacher-coef-updates", "30", "--teacher-only-updates", "3"])
    assert isinstance(kw["teacher"], ScriptedPolicy)
    assert (targs.teacher, targs.teacher_coef, targs.teacher_coef_updates, targs.teacher_only_updates) == ("scripted", 0.5, 30, 3)
    kw, targs = _run_train_tool(monkeypatch, ["--teacher", "scripted"])                                 # no coefficient: no teacher is built
    assert "teacher" not in kw
    capsys.readouterr()
