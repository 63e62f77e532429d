"""CPU: the start pool without a GPU - the twin's Philox against the published known-answer vectors, the pick rule by
hand, StartPool (npz, harvesting from records, the tool), the collector's, the training loop's and the evaluator's new arguments on the
oracle env, and the seed check the GPU tests rely on."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import record_reference as rr
import start_pool_reference as spr
from oracle_vec_env import OracleVecEnv, ScriptedPolicy
from settlers_of_catan_rl_amd import _lib, record, spec, start_pool
from settlers_of_catan_rl_amd import evaluation as ev
from settlers_of_catan_rl_amd import train_loop as tl
from settlers_of_catan_rl_amd.rollout import RolloutCollector

CFG = {"max_proposed_trades_per_turn": 4, "dense_reward": False, "validate_actions": True, "auto_reset": False, "win_reward": 500.0,
       "reward_annealing_factor": 1.0, "max_actions_per_turn": None}


def test_philox_known_answers():
    """the three published vectors of Philox4x32-10 (Random123's kat_vectors)"""
    h = lambda *w: tuple(int(x, 16) for x in w)
    assert spr.philox4x32_10((0, 0, 0, 0), (0, 0)) == h("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")
    ones = 0xFFFFFFFF
    assert spr.philox4x32_10((ones,) * 4, (ones,) * 2) == h("408f276d", "41c83b0e", "a20bc7c6", "6d5451fd")
    assert spr.philox4x32_10(h("243f6a88", "85a308d3", "13198a2e", "03707344"), h("a4093822", "299f31d0")) == \
        h("d16cfe09", "94fdcceb", "5001e420", "24126ea1")


def test_pick_rule_by_hand():
    # on a block: word 1's high half against fresh_q16, word 0 scaled to [0, m)
    assert spr.pick_from_block((0x80000000, 0x7FFF0000, 0, 0), 3, 0x8000) is None          # 0x7FFF < 0x8000: stays fresh
    assert spr.pick_from_block((0x80000000, 0x80000000, 0, 0), 3, 0x8000) == 1             # 0x8000 is not: entry floor(3 / 2)
    assert spr.pick_from_block((0xFFFFFFFF, 0xFFFFFFFF, 0, 0), 65536, 65535) == 65535
    assert spr.pick_from_block((0, 0xFFFF0000, 0, 0), 65536, 65535) == 0
    assert spr.pick_from_block((0x55555556, 0, 0, 0), 3, 0) == 1 and spr.pick_from_block((0x55555555, 0, 0, 0), 3, 0) == 0
    for o1 in (0, 1, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFF0000, 0xFFFFFFFF):
        for o0 in (0, 0x12345678, 0xFFFFFFFF):
            assert spr.pick_from_block((o0, o1, 0, 0), 1, 0) == 0                          # m = 1: always entry 0
            assert spr.pick_from_block((o0, o1, 0, 0), 7, 0) is not None                   # fresh_q16 = 0: never fresh
            assert spr.pick_from_block((o0, o1, 0, 0), 7, 65536) is None                   # fresh_q16 = 65 536: always fresh
    # through the block of (seed, id, d): the counter is (d, "POOL", lo32(id), hi32(id)), the key the seed's two words
    for seed, gid, d, m, q in ((23, (5 << 32) + 7, 1234, 3, 0), (2 ** 40 + 5, 63, 0, 64, 32768), (0, 0, 0xFFFFFFFF, 65536, 1)):
        o = spr.philox4x32_10((d, 0x504F4F4C, gid & 0xFFFFFFFF, gid >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        want = None if (o[1] >> 16) < q else (o[0] * m) >> 32
        assert spr.pick(seed, gid, d, m, q) == want and (want is None or 0 <= want < m)
        assert spr.pick(seed, gid, d, 1, 0) == 0 and spr.pick(seed, gid, d, m, 65536) is None
    # the id's two words and the draw counter all matter
    picks = {(gid, d): spr.pick(23, gid, d, 1 << 16, 0) for gid in (7, (5 << 32) + 7, (6 << 32) + 7) for d in (100, 101)}
    assert len(set(picks.values())) == len(picks)


def test_npz_round_trip(tmp_path):
    rng = np.random.RandomState(4)
    a = start_pool.StartPool(rng.randint(-1, 99, (5, 736)), seed=[1, 2, 3, 2 ** 40, -1], game_id=[0, 2 ** 33 + 1, 5, 6, -1], step=[0, 9, 700, 3, -1])
    b = start_pool.StartPool(rng.randint(-1, 99, (2, 736)))
    for i, p in enumerate((a, b)):
        path = str(tmp_path / f"p{i}.npz")
        start_pool.save(p, path)
        with np.load(path, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
        back = start_pool.load(path)
        assert back == p and back.blobs.dtype == np.int32 and len(back) == len(p)
    assert a != b and (b.seed == -1).all() and (b.game_id == -1).all() and (b.step == -1).all()


@pytest.fixture(scope="module")
def two_records():
    """two whole games of the rule-based player, recorded by tests/record_reference.py's host recorder on the oracle env"""
    n, seed, env_id0 = 2, rr.SEED, 40
    env = OracleVecEnv(n, seed=seed, env_id0=env_id0, auto_reset=False)
    recorder = rr.HostRecorder(env, range(n))
    finished = np.zeros(n, dtype=bool)
    for _ in range(rr.STEP_CAP_ONE * 2):
        a = torch.from_numpy(rr.bot_actions(env.export_state().numpy(), env.get_action_masks().numpy()))
        a[torch.from_numpy(finished), 0] = -1
        _, done = recorder.step(a)
        finished |= done.numpy().astype(bool)
        if finished.all():
            break
    assert finished.all()
    out = []
    for g in range(n):
        r = recorder.record(g)
        out.append(record.GameRecord(seed, env_id0 + g, CFG, r["start"], r["final"], r["actions"], len(r["actions"])))
    return out


def _cpu_env(rec):
    return rr.CpuEnv(rec.seed, rec.game_id, **rec.cfg)


def test_from_records_filters_finished_positions_and_duplicates(two_records):
    f = lambda b, name: spec.state_field(b, name)
    every = start_pool.StartPool.from_records(two_records, every=1, make_env=_cpu_env)
    lengths = [r.length for r in two_records]
    assert 0 < len(every) < sum(lengths)
    assert all(int(f(b, "winner")[0]) == 0 and int(f(b, "initial_phase")[0]) == 0 for b in every.blobs)     # the last positions are finished
    assert set(every.game_id.tolist()) == {40, 41} and (every.seed == rr.SEED).all()
    # an entry is the position `step` actions behind the record's start blob
    for k in (0, len(every) // 2, len(every) - 1):
        rec = two_records[int(every.game_id[k]) - 40]
        blob, _, _, _ = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions[:int(every.step[k])])
        assert np.array_equal(blob, every.blobs[k]), k
    # duplicates (compared with rng_draws zeroed) are dropped: the same records twice add nothing
    twice = start_pool.StartPool.from_records(two_records + two_records, every=1, make_env=_cpu_env)
    assert twice == every
    keys = set()
    for b in every.blobs:
        z = b.copy(); f(z, "rng_draws")[...] = 0
        keys.add(z.tobytes())
    assert len(keys) == len(every)
    # with the initial placement kept, the start blob (step 0) and the placement positions are in
    with_initial = start_pool.StartPool.from_records(two_records, every=1, skip_initial=False, make_env=_cpu_env)
    assert len(with_initial) > len(every) and (with_initial.step == 0).sum() == 2
    assert any(int(f(b, "initial_phase")[0]) == 1 for b in with_initial.blobs)
    # every=k takes the positions behind every k-th action only
    tenth = start_pool.StartPool.from_records(two_records, every=10, make_env=_cpu_env)
    assert len(tenth) > 0 and (tenth.step % 10 == 0).all() and len(tenth) <= sum(n // 10 for n in lengths)
    # the filters
    late = start_pool.StartPool.from_records(two_records, every=1, min_leader_vp=8, make_env=_cpu_env)
    assert len(late) > 0 and (late.leader_vps() >= 8).all() and len(late) == int((every.leader_vps() >= 8).sum())
    mid = start_pool.StartPool.from_records(two_records, every=1, min_turn=10, max_turn=20, min_leader_vp=3, max_leader_vp=5, make_env=_cpu_env)
    assert ((mid.turns() >= 10) & (mid.turns() <= 20) & (mid.leader_vps() >= 3) & (mid.leader_vps() <= 5)).all()
    assert len(mid) == int(((every.turns() >= 10) & (every.turns() <= 20) & (every.leader_vps() >= 3) & (every.leader_vps() <= 5)).sum())
    with pytest.raises(ValueError):
        start_pool.StartPool.from_records(two_records, every=0, make_env=_cpu_env)


def test_from_env_takes_the_unfinished_games():
    env = OracleVecEnv(4, seed=3, env_id0=10, auto_reset=False)
    blobs = env.export_state().numpy()
    spec.state_field(blobs[2], "winner")[...] = 3
    env.import_state(blobs)
    pool = start_pool.StartPool.from_env(env)
    assert len(pool) == 3 and pool.game_id.tolist() == [10, 11, 13] and (pool.seed == 3).all() and (pool.step == -1).all()
    assert np.array_equal(pool.blobs, blobs[[0, 1, 3]])


def test_the_tool_prints_one_summary_line(two_records, tmp_path, capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_start_pool
    paths = []
    for i, rec in enumerate(two_records):
        paths.append(str(tmp_path / f"r{i}.npz"))
        record.save(rec, paths[-1])
    out = str(tmp_path / "pool.npz")
    assert make_start_pool.main(paths + ["-o", out, "--every", "5", "--min-leader-vp", "6"], make_env=_cpu_env) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    pool = start_pool.load(out)
    t, v = pool.turns(), pool.leader_vps()
    hist = " ".join(f"{k}:{int((v == k).sum())}" for k in sorted(set(v.tolist())))
    assert lines[0] == f"{out}: {len(pool)} entries, turns {t.min()}..{t.max()}, leader VP {hist}"
    assert re.fullmatch(r".*: \d+ entries, turns \d+\.\.\d+, leader VP (\d+:\d+ ?)+", lines[0]) and v.min() >= 6 and (pool.step % 5 == 0).all()
    assert start_pool.StartPool(np.zeros((0, 736), dtype=np.int32)).summary() == "0 entries"


# ---- the layers above the env, on the oracle env

def _late(env):
    env.advance_random(1750)             # late game: several games end inside a short rollout
    return env


def test_collector_without_a_pool_is_the_collector_it_was():
    """start_pool=None makes no call on the env (OracleVecEnv has none of the start-pool methods) and changes no tensor"""
    n, T = 12, 16
    sts = []
    for kw in ({}, {"start_pool": None, "start_pool_fresh": 0.0}):
        env = _late(OracleVecEnv(n, 13))
        assert not hasattr(env, "set_start_pool")
        col = RolloutCollector(env, ScriptedPolicy(env), T, seed=4, **kw)
        st = col.gather_rollouts()
        assert st.start_pool is None and not col.start_pool_on
        sts.append((st, env.b.export()))
    (a, ea), (b, eb) = sts
    for name in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(ea, eb) and a.games_complete == b.games_complete


class _Trainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        self.cfg = type("Cfg", (), {"entropy_coef": 0.0})()

    def update(self, st):
        return (0.1, 0.2, 0.3)


@pytest.mark.parametrize("how", ["collector", "args", "path"])
def test_the_counts_surface_in_run_update(tmp_path, how):
    """a pool given to the collector, to TrainArgs, or to TrainArgs as the path of a saved pool: the env is reset once under it, and every
    update's result carries the counts of its rollout's deals"""
    n, T = 12, 16
    late, _ = spr.harvest()
    pool = start_pool.StartPool(late[:20])
    env = spr.PoolTwin(n, 13, 0)
    kw = dict(start_pool=pool, start_pool_fresh=0.25)
    if how == "path":
        start_pool.save(pool, str(tmp_path / "pool.npz"))
        kw["start_pool"] = str(tmp_path / "pool.npz")
    col = RolloutCollector(env, ScriptedPolicy(env), T, seed=4, **(kw if how == "collector" else {}))
    assert (env.pool is not None) == (how == "collector")
    net = torch.nn.Linear(3, 3)
    loop = tl.TrainingLoop(env, net, col, _Trainer(net), tl.TrainArgs(num_steps=T, total_env_steps=T * n * 50, **kw))
    assert np.array_equal(env.pool, late[:20]) and env.fresh_q16 == 16384
    assert int(env.deals.sum()) == n and env.counts["pool"] + env.counts["fresh"] == 0       # one reset under the pool; a rollout counts its own deals
    entries = {spr._zero_rng(b) for b in late[:20]}
    from_pool = sum(spr._zero_rng(b) in entries for b in env.blobs())
    assert 0 < from_pool <= n
    total = 0
    for u in range(2):
        ended = len(env.finished)
        out = loop.run_update()
        sp = out["start_pool"]
        assert sp["pool"] + sp["fresh"] == len(env.finished) - ended and sum(sp["per_entry"]) == sp["pool"] and len(sp["per_entry"]) == 20
        json.dumps(sp)
        total += sp["pool"] + sp["fresh"]
    assert total > 0
    # without a pool the result has no such key
    env2 = _late(OracleVecEnv(n, 13))
    col2 = RolloutCollector(env2, ScriptedPolicy(env2), T, seed=4)
    assert "start_pool" not in tl.TrainingLoop(env2, net, col2, _Trainer(net), tl.TrainArgs(num_steps=T, total_env_steps=T * n * 50)).run_update()
    assert tl.TrainArgs().start_pool is None and tl.TrainArgs().start_pool_fresh == 0.0


def _eval_run(n, seed, **kw):
    env = OracleVecEnv(n, seed, auto_reset=False)
    imported = []
    inner = env.import_state
    env.import_state = lambda blobs: (imported.append(blobs.numpy().copy()), inner(blobs))[1]

    def act_fn(net, idx, f, lists, lens, masks):
        out = []
        for j, i in enumerate(idx):
            m = np.ascontiguousarray(masks[j].numpy(), dtype=np.float32)
            a = np.zeros(18, dtype=np.int32)
            env.L.orc_sample_action(env.b.env_ptr(int(i)), seed + 99, int(i), int(env.steps_taken[int(i)]), m.ctypes.data_as(C.POINTER(C.c_float)),
                                    a.ctypes.data_as(C.POINTER(C.c_int32)))
            out.append(a)
        return torch.tensor(np.stack(out), dtype=torch.int64)
    tag = object()
    orders = np.array([[1, 2, 3, 4], [2, 1, 4, 3], [3, 4, 1, 2], [4, 3, 2, 1], [1, 3, 2, 4]][:n])
    res = ev.run_evaluation_episodes(env, [tag, tag, tag, tag], orders, max_steps=40, act_fn=act_fn, **kw)
    return res, imported, env.b.export()


def test_evaluator_start_blobs():
    n, seed = 5, 7
    late, early = spr.harvest()
    blobs = np.stack([late[3], early[1]])
    plain, imp0, end0 = _eval_run(n, seed)
    none, imp1, end1 = _eval_run(n, seed, start_blobs=None)
    assert imp0 == [] and imp1 == [] and list(plain) == list(none) and all(np.array_equal(plain[k], none[k]) for k in plain)
    assert np.array_equal(end0, end1)
    a, imp_a, end_a = _eval_run(n, seed, start_blobs=blobs)
    b, imp_b, end_b = _eval_run(n, seed, start_blobs=start_pool.StartPool(blobs))
    assert len(imp_a) == 1 and np.array_equal(imp_a[0], blobs[np.arange(n) % 2]) and np.array_equal(imp_a[0], imp_b[0])
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(end_a, end_b)           # two runs with the same seeds are identical
    assert not np.array_equal(end_a, end0)
    with pytest.raises(ValueError):
        _eval_run(n, seed, start_blobs=np.zeros((0, 736), dtype=np.int32))


def test_the_env_methods_raise_where_the_library_lacks_the_entry_points():
    import cpu_abi_driver as drv
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    new = {"catan_start_pool_set", "catan_start_pool_clear", "catan_start_pool_read", "catan_start_pool_size"}
    assert new <= set(_lib.declared_symbols()) and new <= _lib._OPTIONAL
    L = drv.cpu_lib()
    assert not any(hasattr(L, name) for name in new)
    env = object.__new__(VecCatanEnv)
    env.L, env.h = L, None
    for call in (lambda: env.set_start_pool(np.zeros((1, 736))), env.clear_start_pool, env.start_pool_counts):
        with pytest.raises(_lib.CatanHipError, match="the loaded library has no catan_start_pool_"):
            call()


# ---- the seed check that keeps the GPU tests honest

def test_seed_check_for_the_gpu_scenarios():
    """Where the seeds, pools and caps of tests/test_gpu_start_pool.py are chosen (tests/start_pool_reference.py): played here on the twin
    under the numpy restatement of the rule-based player, every scenario sees what its GPU test is about."""
    late, early = spr.harvest()
    f = lambda b, name: spec.state_field(b, name)
    assert all(int(f(b, "winner")[0]) == 0 and max(int(v) for v in f(b, "curr_vps")) >= spr.LATE_VP for b in late)
    assert all(int(f(b, "winner")[0]) == 0 and int(f(b, "initial_phase")[0]) == 0 and int(f(b, "turn")[0]) <= 1 for b in early)
    pools = spr.pools()
    assert [len(pools[m]) for m in (1, 3, 64)] == [1, 3, 64]
    assert len({spr._zero_rng(b) for b in pools[64]}) == 64
    assert spr.N_GAMES == 64 and spr.ENV_ID0 >> 32 != 0 and spr.ENV_ID0 & 0xFFFFFFFF != 0
    for m, env_id0 in ((1, spr.ENV_ID0_ZERO), (3, spr.ENV_ID0), (64, spr.ENV_ID0)):          # the lock-step scenarios
        twin = spr.PoolTwin(spr.N_GAMES, spr.SEED, env_id0, pools[m], 0)
        spr.run_twin(twin, spr.STEP_CAP)
        redeals = int(twin.deals.sum()) - spr.N_GAMES
        print("pool", m, "re-deals", redeals, "games re-dealt twice", int((twin.deals >= 3).sum()), "installs", twin.counts["per_entry"][:8])
        assert redeals >= 32 and (twin.deals >= 3).any() and twin.counts["fresh"] == 0
        assert twin.counts["pool"] == redeals + spr.N_GAMES
        if m <= 3:
            assert (twin.counts["per_entry"] > 0).all()
    twin = spr.PoolTwin(spr.N_GAMES, spr.SEED, spr.ENV_ID0, pools[64][:2], 0)               # the two late positions behind a refused set
    spr.run_twin(twin, spr.REFUSED_SET_STEPS)
    assert twin.counts["pool"] >= spr.N_GAMES + 8 and (twin.counts["per_entry"] > 0).all() and twin.counts["fresh"] == 0
    twin = spr.PoolTwin(spr.N_GAMES, spr.SEED, spr.ENV_ID0, pools[3], 32768)               # half fresh
    spr.run_twin(twin, spr.STEP_CAP)
    print("half fresh:", twin.counts)
    assert twin.counts["pool"] >= 8 and twin.counts["fresh"] >= 8
