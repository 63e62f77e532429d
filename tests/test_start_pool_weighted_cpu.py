"""CPU: the start pool's weighted pick and outcome tallies without a GPU - the weighted rule by hand, against the uniform
rule and at the edge of its range, StartPool's weights / outcomes / balanced_weights and their .npz keys, the env methods' host checks,
the collector's and the training loop's new arguments on the oracle twin, the labelling tool, and the seed check the GPU tests rely on."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import start_pool_reference as spr
import start_pool_weighted_reference as wr
from oracle_vec_env import ScriptedPolicy
from settlers_of_catan_rl_amd import _lib, spec, start_pool
from settlers_of_catan_rl_amd import train_loop as tl
from settlers_of_catan_rl_amd.rollout import RolloutCollector

ONES = 0xFFFFFFFF


def test_weighted_rule_by_hand():
    """five entries, weight 0 in the middle and at both ends: cum = [0, 3, 3, 8, 8], W = 8, t = floor(o0 * 8 / 2^32)"""
    cum = wr.prefix_sums([0, 3, 0, 5, 0])
    assert cum == [0, 3, 3, 8, 8]
    blk = lambda o0, o1=ONES: (o0, o1, 0, 0)
    assert wr.pick_from_block_weighted(blk(0), cum, 0) == 1                        # t = 0: cum[0] = 0 is not above it
    assert wr.pick_from_block_weighted(blk(0x5FFFFFFF), cum, 0) == 1               # t = 2
    assert wr.pick_from_block_weighted(blk(0x60000000), cum, 0) == 3               # t = 3: cum[1] = cum[2] = 3 are not above it
    assert wr.pick_from_block_weighted(blk(ONES), cum, 0) == 3                     # t = 7
    assert {wr.pick_from_block_weighted(blk((i * 0x01000193 + 7) & ONES), cum, 0) for i in range(4000)} == {1, 3}
    # the freshness test is the uniform rule's: word 1's high half against fresh_q16
    assert wr.pick_from_block_weighted((0x60000000, 0x7FFF0000, 0, 0), cum, 0x8000) is None
    assert wr.pick_from_block_weighted((0x60000000, 0x80000000, 0, 0), cum, 0x8000) == 3
    assert wr.pick_from_block_weighted(blk(0x60000000), cum, 65536) is None
    # the shares: over the 2^32 values of o0 entry 1 takes 3 / 8 and entry 3 takes 5 / 8 - the boundaries are exact
    assert wr.pick_from_block_weighted(blk(3 * 2 ** 29 - 1), cum, 0) == 1 and wr.pick_from_block_weighted(blk(3 * 2 ** 29), cum, 0) == 3
    with pytest.raises(AssertionError):
        wr.prefix_sums([0, 0, 0])
    with pytest.raises(AssertionError):
        wr.prefix_sums([2 ** 31, 2 ** 31])


@pytest.mark.parametrize("m,fresh_q16,pairs", [(1, 0, 1000), (3, 0, 3000), (64, 32768, 4000), (1000, 0, 1900), (65536, 1, 100)])
def test_all_ones_weights_are_the_uniform_rule(m, fresh_q16, pairs):
    """W = m, cum[k] = k + 1, k = t: 10 000 (id, d) pairs in all"""
    cum = wr.prefix_sums([1] * m)
    rng = np.random.RandomState(m)
    picked = set()
    for _ in range(pairs):
        gid, d = int(rng.randint(0, 2 ** 31)) * int(rng.randint(1, 2 ** 31)), int(rng.randint(0, 2 ** 31)) * 2 + int(rng.randint(0, 2))
        k = wr.weighted_pick(spr.SEED, gid, d, cum, fresh_q16)
        assert k == spr.pick(spr.SEED, gid, d, m, fresh_q16)
        picked.add(k)
    assert len(picked) >= min(m, 50)


def test_the_largest_sum():
    """W = 2^32 - 1: t = o0 - 1 for o0 >= 1 (and 0 for o0 = 0), so t reaches 2^32 - 2 and no further"""
    cum = wr.prefix_sums([2 ** 32 - 2, 1])
    assert cum[-1] == wr.MAX_SUM
    blk = lambda o0: (o0, ONES, 0, 0)
    assert wr.pick_from_block_weighted(blk(ONES), cum, 0) == 1                     # t = 2^32 - 2 = cum[0]: not above it
    assert wr.pick_from_block_weighted(blk(ONES - 1), cum, 0) == 0                 # t = 2^32 - 3
    assert wr.pick_from_block_weighted(blk(0), cum, 0) == 0 and wr.pick_from_block_weighted(blk(1), cum, 0) == 0
    cum = wr.prefix_sums([1, 2 ** 32 - 2])
    assert wr.pick_from_block_weighted(blk(0), cum, 0) == 0 and wr.pick_from_block_weighted(blk(1), cum, 0) == 0      # t = 0 twice
    assert wr.pick_from_block_weighted(blk(2), cum, 0) == 1
    cum = wr.prefix_sums([ONES])
    assert all(wr.pick_from_block_weighted(blk(o0), cum, 0) == 0 for o0 in (0, 1, 2 ** 31, ONES))


def test_balanced_weights_by_hand():
    """p = (focus_wins + prior / 4) / (focus_games + prior), weight = max(floor, round(scale * 4 p (1 - p)))"""
    pool = start_pool.StartPool(np.zeros((5, 736), dtype=np.int32))
    assert pool.weights is None and pool.outcomes is None
    # no outcomes at all: every entry is unplayed, p = 1 / 4, 4 p (1 - p) = 3 / 4
    assert pool.balanced_weights().tolist() == [round(65535 * 0.75)] * 5 == [49151] * 5
    t = np.zeros((6, 8))
    t[0, 5:7] = (2, 1)        # p = 1.5 / 4 = 0.375          -> 4 * 0.375 * 0.625 = 0.9375
    t[1, 5:7] = (6, 3.5)      # p = 4 / 8 = 0.5              -> 1
    t[2, 5:7] = (98, 0)       # p = 0.5 / 100 = 0.005        -> 4 * 0.005 * 0.995 = 0.0199
    t[3, 5:7] = (0, 0)        # unplayed: p = 0.25           -> 0.75
    t[4, 5:7] = (2, 3.5)      # p = 1: only with decayed sums -> 0, the floor
    t[5, 5:7] = (50, 50)      # the fresh deals' row has no weight
    pool.add_outcomes(t)
    w = pool.balanced_weights()
    assert w.dtype == np.uint32 and w.tolist() == [61439, 65535, 1304, 49151, 1]
    assert [round(65535 * x) for x in (0.9375, 1.0, 0.0199, 0.75)] == [61439, 65535, 1304, 49151]
    assert pool.balanced_weights(floor=2000).tolist() == [61439, 65535, 2000, 49151, 2000]
    assert pool.balanced_weights(prior=0.0, floor=1, scale=100).tolist()[:3] == [100, round(100 * 4 * (3.5 / 6) * (2.5 / 6)), 1]
    # the decay multiplies what was accumulated in front of every add
    half = start_pool.StartPool(np.zeros((5, 736), dtype=np.int32), decay=0.5)
    half.add_outcomes(t); half.add_outcomes({"table": t})
    assert np.array_equal(half.outcomes, 1.5 * t)
    pool.add_outcomes(t)
    assert np.array_equal(pool.outcomes, 2 * t)
    with pytest.raises(ValueError):
        start_pool.StartPool(np.zeros((5, 736), dtype=np.int32), decay=1.5)
    with pytest.raises(ValueError):
        pool.add_outcomes(np.zeros((5, 8)))


PARENT_KEYS = {"format_version", "blobs", "source_seed", "source_game_id", "source_step"}


def test_npz_round_trip_with_and_without_the_new_keys(tmp_path):
    rng = np.random.RandomState(4)
    blobs = rng.randint(-1, 99, (4, 736))
    plain = start_pool.StartPool(blobs, seed=[1, 2, 3, -1], game_id=[0, 2 ** 33 + 1, 5, -1], step=[0, 9, 700, -1])
    weighted = start_pool.StartPool(blobs, weights=[0, 5, 2 ** 32 - 7, 1])
    labelled = start_pool.StartPool(blobs, outcomes=rng.rand(5, 8) * 9, decay=0.75)
    both = start_pool.StartPool(blobs, weights=np.array([1, 1, 1, 1]), outcomes=rng.randint(0, 9, (5, 8)))
    want = {"plain": set(), "weighted": {"weights"}, "labelled": {"outcomes", "outcomes_decay"}, "both": {"weights", "outcomes", "outcomes_decay"}}
    for name, p in (("plain", plain), ("weighted", weighted), ("labelled", labelled), ("both", both)):
        path = str(tmp_path / f"{name}.npz")
        start_pool.save(p, path)
        with np.load(path, allow_pickle=False) as z:
            assert set(z.files) == PARENT_KEYS | want[name] and all(z[k].dtype != object for k in z.files)
        back = start_pool.load(path)
        assert back == p and back.decay == p.decay
        assert (back.weights is None) == (p.weights is None) and (back.outcomes is None) == (p.outcomes is None)
    assert weighted.weights.dtype == np.uint32 and weighted.weights.tolist() == [0, 5, 2 ** 32 - 7, 1]
    assert labelled.outcomes.dtype == np.float64 and labelled.outcomes.shape == (5, 8)
    assert plain != weighted and plain != labelled and weighted != both
    # a file as the library wrote it before there were weights or outcomes
    old = str(tmp_path / "old.npz")
    np.savez(old, format_version=np.int64(1), blobs=plain.blobs, source_seed=plain.seed, source_game_id=plain.game_id, source_step=plain.step)
    back = start_pool.load(old)
    assert back == plain and back.weights is None and back.outcomes is None and back.decay == 1.0
    for bad in ([1, 2, 3], [1, 2, 3, -1], [2 ** 32, 0, 0, 0], [0, 0, 0, 0], [2 ** 31, 2 ** 31, 0, 0], [0.5, 1, 1, 1]):
        with pytest.raises(ValueError):
            start_pool.StartPool(blobs, weights=bad)


def test_the_outcome_fields_are_restated_alike():
    assert spec.START_POOL_OUTCOME_FIELDS == wr.FIELDS and spec.START_POOL_OUTCOME_WORDS == 8 and spec.START_POOL_MAX_WEIGHT_SUM == wr.MAX_SUM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "settlers_of_catan_rl_amd", "csrc", "catan_hooks.h")).read()
    offs = {name: int(v) for name, v in re.findall(r"constexpr int (PO_[A-Z_]+) = (\d+);", src)}
    assert (offs["PO_GAMES"], offs["PO_WINS_PLAYER"], offs["PO_FOCUS_GAMES"], offs["PO_FOCUS_WINS"], offs["PO_TURNS_SUM"], offs["PO_WORDS"]) == (0, 1, 5, 6, 7, 8)
    # spec's reading of a table against the twin's own
    twin = wr.OutcomeTwin(4, 1, 0, np.zeros((3, 736), dtype=np.int32))
    twin.enable_outcomes()
    twin.table[:] = np.arange(2 + 4 * 8) % 7
    a, b = spec.start_pool_outcomes_dict(twin.table, 3), twin.start_pool_outcomes()
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
        else:
            assert a[k] == b[k], k
    assert np.isnan(a["focus_win_share"]).any() or (a["focus_games"] > 0).all()
    empty = spec.start_pool_outcomes_dict(np.zeros(2 + 4 * 8, dtype=np.int64), 3)
    assert np.isnan(empty["win_share_by_pid"]).all() and np.isnan(empty["focus_win_share"]).all() and empty["win_share_by_pid"].shape == (3, 4)
    with pytest.raises(ValueError):
        spec.start_pool_outcomes_dict(np.zeros(2 + 3 * 8), 3)


class _StubLib(object):
    """a library that has the entry points and must not be reached"""

    def __init__(self, m):
        self.m, self.calls = m, []

    def catan_start_pool_size(self, h):
        return self.m

    def catan_start_pool_set_weights(self, *a):
        self.calls.append("set_weights")
        return 0

    def catan_start_pool_set(self, *a):
        self.calls.append("set")
        return 0


def test_bad_weights_raise_on_the_host_before_any_call(monkeypatch):
    from settlers_of_catan_rl_amd import env as env_mod
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    monkeypatch.setattr(env_mod, "_stream", lambda: None)
    env = object.__new__(VecCatanEnv)
    env.L, env.h, env.device, env.n = _StubLib(4), None, torch.device("cpu"), 8
    bads = ([1, 2, 3], [1, 2, 3, -1], [2 ** 32, 0, 0, 0], [0, 0, 0, 0], [2 ** 31, 2 ** 31, 0, 0], np.array([0.5, 1, 1, 1]), torch.tensor([1.0, 1, 1, 1]),
            np.ones((2, 2), dtype=np.int64))
    for bad in bads:
        with pytest.raises(ValueError):
            env.set_start_pool_weights(bad)
        with pytest.raises(ValueError):
            env.set_start_pool(np.zeros((4, 736), dtype=np.int32), weights=bad)
    assert env.L.calls == []
    for good in ([0, 0, 0, 1], np.array([2 ** 32 - 2, 1, 0, 0], dtype=np.uint64), torch.tensor([1, 2, 3, 4]), [2 ** 31, 2 ** 31 - 1, 0, 0]):
        env.set_start_pool_weights(good)
    env.set_start_pool_weights(None)
    assert env.L.calls == ["set_weights"] * 5
    w = env._start_pool_weights([2 ** 32 - 2, 1, 0, 0], 4)
    assert w.dtype == torch.int32 and w.numpy().view(np.uint32).tolist() == [2 ** 32 - 2, 1, 0, 0]
    env.L.m = 0
    with pytest.raises(_lib.CatanHipError):
        env.set_start_pool_weights([1])


def test_the_env_methods_raise_where_the_library_lacks_the_entry_points():
    import cpu_abi_driver as drv
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    new = {"catan_start_pool_set_weights", "catan_start_pool_outcomes_words", "catan_start_pool_outcomes_enable", "catan_start_pool_outcomes_read"}
    assert new <= set(_lib.declared_symbols()) and new <= _lib._OPTIONAL
    L = drv.cpu_lib()
    assert not any(hasattr(L, name) for name in new)
    env = object.__new__(VecCatanEnv)
    env.L, env.h = L, None
    for call in (lambda: env.set_start_pool_weights([1]), lambda: env.set_start_pool_weights(None), env.enable_start_pool_outcomes, env.start_pool_outcomes):
        with pytest.raises(_lib.CatanHipError, match="the loaded library has no catan_start_pool_"):
            call()


# ---- the layers above the env, on the oracle twin

class _Trainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        self.cfg = type("Cfg", (), {"entropy_coef": 0.0})()

    def update(self, st):
        return (0.1, 0.2, 0.3)


def _pool20():
    late, _ = spr.harvest()
    return start_pool.StartPool(late[:20])


def test_the_defaults_make_no_call_and_change_nothing():
    """start_pool_outcomes=False and start_pool_sampling="uniform" on PoolTwin, which has neither enable_start_pool_outcomes nor
    set_start_pool_weights: the collector is the collector it was, tensor for tensor, and no checkpoint key is added"""
    n, T = 12, 16
    sts = []
    for kw in ({}, {"start_pool_outcomes": False, "start_pool_sampling": "uniform"}):
        env = spr.PoolTwin(n, 13, 0)
        assert not hasattr(env, "enable_start_pool_outcomes") and not hasattr(env, "set_start_pool_weights")
        col = RolloutCollector(env, ScriptedPolicy(env), T, seed=4, start_pool=_pool20(), start_pool_fresh=0.25, **kw)
        env.reset(); col.reset()
        st = col.gather_rollouts()
        assert set(st.start_pool) == {"pool", "fresh", "per_entry"} and not col.start_pool_outcomes and col.start_pool is None
        sts.append((st, env.blobs(), env.counts))
    (a, ea, ca), (b, eb, cb) = sts
    for name in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(ea, eb) and np.array_equal(a.start_pool["per_entry"], b.start_pool["per_entry"])
    args = tl.TrainArgs(num_steps=T)
    assert (args.start_pool_outcomes, args.start_pool_sampling) == (False, "uniform")
    assert "start_pool_outcomes" not in args.__dict__ and "start_pool_sampling" not in args.__dict__       # (the checkpoint keeps args.__dict__)
    with pytest.raises(ValueError):
        RolloutCollector(spr.PoolTwin(n, 13, 0), None, T, start_pool_outcomes=True)
    with pytest.raises(ValueError):
        RolloutCollector(spr.PoolTwin(n, 13, 0), None, T, start_pool=_pool20(), start_pool_sampling="pfsp")


@pytest.mark.parametrize("sampling", ["uniform", "balanced"])
@pytest.mark.parametrize("how", ["collector", "args"])
def test_the_outcomes_surface_in_the_collector_and_in_run_update(how, sampling):
    """outcomes on, given to the collector or to TrainArgs: every rollout's storage and every update's result carry the tallies of the
    games that finished in it, the focus is the collector's active seat, and under "balanced" the weights installed behind a rollout
    are balanced_weights() of everything tallied so far"""
    n, T = 12, 16
    pool = _pool20()
    env = wr.OutcomeTwin(n, 13, 0)
    kw = dict(start_pool=pool, start_pool_fresh=0.25, start_pool_outcomes=True, start_pool_sampling=sampling)
    col = RolloutCollector(env, ScriptedPolicy(env), T, seed=4, **(kw if how == "collector" else {}))
    net = torch.nn.Linear(3, 3)
    loop = tl.TrainingLoop(env, net, col, _Trainer(net), tl.TrainArgs(num_steps=T, total_env_steps=T * n * 50, **kw))
    assert env.table is not None and np.array_equal(env.focus, col.active_pid.numpy()) and col.start_pool is pool
    unplayed = wr.prefix_sums([49151] * 20)
    assert env.cum == (unplayed if sampling == "balanced" else None)
    total = np.zeros((21, 8))
    for u in range(3):
        ended = len(env.finished)
        out = loop.run_update()
        sp, oc = out["start_pool"], out["start_pool"]["outcomes"]
        json.dumps(sp)
        t = np.array(oc["table"])
        new = env.finished[ended:]
        assert oc["seen"] == len(new) == sp["pool"] + sp["fresh"] and oc["skipped"] == 0
        assert t[:20, 0].sum() == sum(o >= 0 for _g, _b, o in new) and t[20, 0] == oc["fresh"]["games"] == sum(o < 0 for _g, _b, o in new)
        assert np.array_equal(col.storage.start_pool["outcomes"]["table"], t)
        total += t
        if sampling == "balanced":
            assert np.array_equal(pool.outcomes, total) and env.cum == wr.prefix_sums(pool.balanced_weights().tolist())
        else:
            assert pool.outcomes is None and env.cum is None
    assert total[:, 0].sum() > 0 and total[:, 5].sum() == total[:, 0].sum()            # every game has a focus seat here
    if sampling == "balanced":
        assert env.cum != unplayed


def test_the_labelling_tool_prints_one_summary_line(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import label_start_pool
    src, out = str(tmp_path / "pool.npz"), str(tmp_path / "labelled.npz")
    pool = _pool20()
    start_pool.save(pool, src)
    made = []
    make_env = lambda n, seed: made.append(wr.OutcomeTwin(n, seed, 0)) or made[-1]
    assert label_start_pool.main([src, "--games", "16", "--steps", "60", "--seed", "13", "-o", out], make_env=make_env) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    twin = made[0]
    assert twin.n == 16 and twin.fresh_q16 == 0 and twin.cum is None and twin.focus is None
    back = start_pool.load(out)
    rows = twin.table[2:].reshape(21, 8)
    assert np.array_equal(back.blobs, pool.blobs) and np.array_equal(back.outcomes, rows) and back.weights is None
    games, wins = rows[:20, 0], rows[:20, 1:5]
    played = int((games > 0).sum())
    decided = int(((games > 0) & (wins.max(axis=1) * 10 >= games * 9)).sum())
    assert played > 0 and games.sum() == len(twin.finished) and rows[20, 0] == 0
    assert lines[0] == (f"{out}: {played} of 20 entries played, {int(games.sum())} games tallied, {100.0 * decided / played:.1f} % of the played "
                        f"entries have one seat with at least 90 % of the games")
    # the share by hand: entry 0 decided (9 of 10), entry 1 not (8 of 10), entry 2 unplayed
    t = np.zeros((4, 8)); t[0, :2] = (10, 9); t[0, 3] = 1; t[1, 0] = 10; t[1, 2] = 8; t[1, 4] = 2
    assert label_start_pool.summary_line(t).startswith("2 of 3 entries played, 20 games tallied, 50.0 %")


# ---- the seed check that keeps the GPU tests honest

def _zero_runs_have_a_played_neighbour(weights, installs):
    """every zero-weight entry has no install, and the nearest positive-weight entry on one side of it has some"""
    m = len(weights)
    for k in (i for i in range(m) if weights[i] == 0):
        assert installs[k] == 0, k
        lo = next((j for j in range(k - 1, -1, -1) if weights[j] > 0), None)
        hi = next((j for j in range(k + 1, m) if weights[j] > 0), None)
        assert any(j is not None and installs[j] > 0 for j in (lo, hi)), (k, lo, hi)


def test_seed_check_for_the_gpu_scenarios():
    """Where the weights, seeds and caps of tests/test_gpu_start_pool_weighted.py are chosen (tests/start_pool_weighted_reference.py): played
    here on the twin under the numpy restatement of the rule-based player, every scenario sees what its GPU test is about."""
    pools = wr.pools()
    w = wr.weights_64()
    assert len(w) == 64 and sum(w) <= wr.MAX_SUM and w[wr.HEAVY] == 2 ** 31 and all(w[k] == 0 for k in wr.ZEROS_64)
    assert w[0] == 0 and w[63] == 0 and {1, 2, 3} == set(wr.SMALL_64.values())
    assert wr.N_GAMES == 64 and (wr.FOCUS == 0).any() and set(wr.FOCUS.tolist()) == {0, 1, 2, 3, 4}
    # the weighted pool, every deal from it
    twin = wr.OutcomeTwin(wr.N_GAMES, wr.SEED, wr.ENV_ID0, pools[64], 0, w)
    twin.enable_outcomes(wr.FOCUS)
    wr.run_twin(twin, wr.STEP_CAP)
    o = twin.start_pool_outcomes()
    print("weighted: finished", o["seen"], "entries tallied", int((o["games"] > 0).sum()), "most", int(o["games"].max()), "winners", o["table"][:, 1:5].sum(0))
    assert o["skipped"] == 0 and o["fresh"]["games"] == 0 and o["games"].sum() == o["seen"] == len(twin.finished) >= 32
    assert (o["games"] > 0).sum() >= 8 and o["games"].max() >= 2
    assert (o["table"][:, 1:5].sum(0) > 0).sum() >= 2                               # two different PlayerIds win
    assert 0 < o["focus_games"].sum() < o["games"].sum() and 0 < o["focus_wins"].sum() < o["focus_games"].sum()
    assert (twin.deals >= 3).any()                                                   # some game is re-dealt twice
    _zero_runs_have_a_played_neighbour(w, twin.counts["per_entry"])
    assert twin.counts["per_entry"][wr.HEAVY] * 3 > twin.counts["pool"]             # the 2^31 entry takes about half
    assert twin.counts["fresh"] == 0 and twin.counts["pool"] == int(twin.deals.sum())
    # half fresh
    twin = wr.OutcomeTwin(wr.N_GAMES, wr.SEED, wr.ENV_ID0, pools[64], wr.HALF_FRESH_Q16, w)
    twin.enable_outcomes(wr.FOCUS)
    wr.run_twin(twin, wr.STEP_CAP)
    o = twin.start_pool_outcomes()
    print("half fresh: finished", o["seen"], "of fresh origin", o["fresh"]["games"], "counts", twin.counts["pool"], twin.counts["fresh"])
    assert o["fresh"]["games"] >= 1 and o["games"].sum() >= 8 and twin.counts["fresh"] >= 8 and twin.counts["pool"] >= 8
    assert all(twin.counts["per_entry"][k] == 0 for k in wr.ZEROS_64)
    # the last entry alone, and the 65 536-entry table's six edges: the picks the GPU test will see are within them by the rule
    cum = wr.prefix_sums([0] * 63 + [1])
    big = wr.prefix_sums(wr.big_weights().tolist())
    assert big[-1] == 21 and [big[k] - (big[k - 1] if k else 0) for k in wr.BIG_EDGES] == [1, 2, 3, 4, 5, 6]
    import bisect
    seen = set()
    for g in range(wr.N_GAMES):
        for d in range(40):
            assert wr.weighted_pick(wr.SEED, wr.ENV_ID0 + g, d, cum, 0) == 63
            t = (spr.philox4x32_10((d, spr.POOL_STREAM, (wr.ENV_ID0 + g) & ONES, (wr.ENV_ID0 + g) >> 32), (wr.SEED, 0))[0] * 21) >> 32
            seen.add(bisect.bisect_right(big, t))
    assert seen == set(wr.BIG_EDGES)                                                 # bisect_right: the smallest k with big[k] > t
