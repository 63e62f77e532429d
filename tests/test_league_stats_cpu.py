"""League results on the CPU: the plain-Python tally the device tests compare with (tests/league_stats_oracle.py) on hand-written
episodes, the league's serial numbers, records and PFSP sampling, and the training loop's bookkeeping with stub collector and trainer."""
import numpy as np
import pytest
import torch

import episode_stats_oracle as eso
import league_stats_oracle as lso
from settlers_of_catan_rl_amd import league, spec
from settlers_of_catan_rl_amd import train_loop as tl


def _episode(game, decision, winner, vp):
    r = [0] * eso.COLS
    r[eso.GAME], r[eso.DECISION], r[eso.WINNER] = game, decision, winner
    r[eso.VP:eso.VP + 4] = vp
    return r


# ---------------------------------------------------------------- the tally
def test_tally_of_hand_written_episodes():
    # PlayerId 1..4 -> slot; slot 0 is the central policy
    slot = np.array([[0, 1, 2, 3],          # game 0: central = PlayerId 1
                     [2, 0, 3, 1],          # game 1: central = PlayerId 2; slot 1 = PlayerId 4, slot 2 = PlayerId 1, slot 3 = PlayerId 3
                     [3, 2, 1, 0],          # game 2: central = PlayerId 4
                     [1, 0, 2, 3],          # game 3: central = PlayerId 2
                     [0, 1, 1, 3]],         # game 4: no permutation
                    dtype=np.int32)
    net = np.array([[1, -1, -1],            # game 0: net 1 on one seat (PlayerId 2)
                    [0, 0, 0],              # game 1: net 0 on all three seats
                    [1, 0, 1],              # game 2: net 1 on slots 1 and 3 (PlayerIds 3 and 1), net 0 on slot 2 (PlayerId 2)
                    [0, -1, 7],             # game 3: a -1 seat and an index out of range
                    [0, 0, 0]], dtype=np.int32)
    ep = [_episode(0, 10, 1, [10, 4, 5, 6]),      # central wins against net 1's one seat
          _episode(1, 20, 2, [3, 11, 5, 7]),      # central wins against three seats of net 0
          _episode(2, 30, 3, [2, 6, 10, 8]),      # an opponent seat wins: PlayerId 3 = slot 1 = net 1
          _episode(3, 40, 1, [10, 9, 1, 2]),      # PlayerId 1 = slot 1 = net 0 wins
          _episode(4, 50, 1, [10, 0, 0, 0]),      # skipped: the slot row
          _episode(0, 99, 2, [1, 10, 1, 1])]      # beyond the counter of 60 below
    t = lso.table(np.array(ep), 60, slot, net, 2)
    assert t.shape == (3, 6)
    # net 0: games 1, 2, 3 -> seats 3 + 1 + 1
    assert t[0].tolist() == [3, 5, 1, 3, (3 + 7 + 5) + 6 + 10, 3 * 11 + 8 + 9]
    # net 1: games 0, 2 -> seats 1 + 2; its PlayerId 3 won game 2
    assert t[1].tolist() == [2, 3, 1, 1, 4 + (10 + 2), 10 + 2 * 8]
    # totals: seen 5, tallied 4, central wins 2, central VP 10 + 11 + 8 + 9, one game and one seat skipped
    assert t[2].tolist() == [5, 4, 2, 38, 1, 1]
    # the same net on all three seats and the central seat wins: central_wins += 3, games += 1
    one = lso.table(np.array(ep[1:2]), 60, slot, net, 2)
    assert one[0].tolist() == [1, 3, 0, 3, 15, 33] and one[1].tolist() == [0] * 6
    # within per-game counters: game 0's second episode counts at 99
    cnt = np.array([99, 0, 0, 0, 0])
    t2 = lso.table(np.array(ep), cnt, slot, net, 2)
    assert t2[2][lso.T_SEEN] == 2 and t2[1].tolist() == [2, 2, 1, 1, 4 + 10, 10 + 1]
    # no winner
    t3 = lso.table(np.array([_episode(0, 1, 0, [0, 0, 0, 0])]), 60, slot, net, 2)
    assert t3[2].tolist() == [1, 0, 0, 0, 1, 0]
    named = spec.league_stats_table(t, 2)
    assert list(named)[:6] == spec.LEAGUE_STATS_FIELDS and spec.LEAGUE_STATS_WORDS == 6
    assert named["seats"].tolist() == [5, 3] and named["totals"]["games_tallied"] == 4 and named["totals"]["seats_skipped"] == 1
    with pytest.raises(ValueError):
        spec.league_stats_table(t, 3)


# ---------------------------------------------------------------- League
def _league(n, **kw):
    lg = league.League(**kw)
    lg.earlier.extend({"id": i} for i in range(n))
    return lg


def _table(rows):
    """rows: (net_wins, central_wins) per net -> a league table with seats = their sum and a zero totals row"""
    t = torch.zeros((len(rows) + 1, 6), dtype=torch.int64)
    for k, (nw, cw) in enumerate(rows):
        t[k] = torch.tensor([nw + cw, nw + cw, nw, cw, 5 * nw, 5 * cw])
    return t


def test_serials_survive_the_roll_over_and_evicted_records_disappear():
    lg = league.League(num_policies_to_store=3)
    for i in range(3):
        lg.earlier.append({"id": i})
    assert lg.serials() == [0, 1, 2]
    lg.in_play = [0, 2]
    lg.record(_table([(1, 3), (2, 2)]))
    assert sorted(lg.records) == [0, 2]
    lg.earlier.append({"id": 3})                       # evicts the snapshot with serial 0
    assert lg.serials() == [1, 2, 3] and sorted(lg.records) == [2]
    lg.add(torch.nn.Linear(1, 1))
    assert lg.serials() == [2, 3, 4] and lg.records[2][3] == 2.0
    lg.earlier.append({"id": 5}); lg.earlier.append({"id": 6})
    assert lg.serials() == [4, 5, 6] and lg.records == {}
    # rows of a snapshot that left between the draw and the record are dropped
    lg.in_play = [2, 6]
    lg.record(_table([(1, 1), (0, 4)]))
    assert sorted(lg.records) == [6] and lg.records[6].tolist() == [4, 4, 0, 4, 0, 20]


@pytest.mark.parametrize("max_distinct", [None, 4])
def test_reference_sampling_with_records_makes_the_parents_draws(max_distinct):
    """the parent's League.sample, restated: get_prob_dist and the same generator calls in the same order"""
    def parent_sample(rng, n, workers):
        p = league.get_prob_dist(n)
        if max_distinct is None:
            return np.stack([rng.choice(n, 3, p=p) for _ in range(workers)]).astype(np.int64)
        pool = rng.choice(n, max_distinct, p=p)
        return pool[rng.randint(0, max_distinct, size=(workers, 3))].astype(np.int64)
    lg = _league(40, seed=9, max_distinct=max_distinct)
    assert lg.sampling == "reference"
    lg.in_play = [3, 7, 39]
    lg.record(_table([(50, 0), (0, 50), (9, 1)]))
    rng = np.random.RandomState(9)
    for workers in (7, 20):
        assert np.array_equal(lg.sample(workers), parent_sample(rng, 40, workers))
    # ... while PFSP with the same records draws differently
    pf = _league(40, seed=9, max_distinct=max_distinct, sampling="pfsp")
    pf.in_play = [3, 7, 39]
    pf.record(_table([(50, 0), (0, 50), (9, 1)]))
    assert not np.array_equal(pf.sample(200), parent_sample(np.random.RandomState(9), 40, 200))
    with pytest.raises(ValueError):
        league.League(sampling="uniform")


def test_central_share_and_pfsp_probabilities_by_hand():
    lg = _league(3, sampling="pfsp", pfsp_power=2.0, pfsp_mix=0.5, pfsp_prior=1.0)
    assert lg.central_share().tolist() == [0.5, 0.5, 0.5]
    assert np.allclose(lg.probabilities(), 0.5 * league.get_prob_dist(3) + 0.5 / 3, rtol=0, atol=1e-15)
    lg.in_play = [0, 1]
    lg.record(_table([(6, 2), (0, 8)]))                # snapshot 0: central 2 : 6 net; snapshot 1: central 8 : 0; snapshot 2 never met
    x = lg.central_share()
    assert x.tolist() == [(2 + 1) / (2 + 6 + 2), (8 + 1) / (8 + 0 + 2), 0.5] == [0.3, 0.9, 0.5]
    w = np.array([0.7 ** 2, 0.1 ** 2, 0.5 ** 2])       # 0.49, 0.01, 0.25: sum 0.75
    # get_prob_dist(3) from its definition: 1/6 each plus the ramp 0, 1/12, 2/12, normalised
    base = np.full(3, 0.5 / 3) + np.arange(3) * ((2 * 0.5 / 4) / 3)
    base = base / base.sum()
    assert np.allclose(league.get_prob_dist(3), base, rtol=0, atol=1e-15)
    want = 0.5 * base + 0.5 * w / 0.75
    p = lg.probabilities()
    assert np.allclose(p, want, rtol=0, atol=1e-15) and abs(p.sum() - 1.0) < 1e-12
    assert p[0] > p[2] > p[1]                          # the snapshot the central policy loses to is drawn most
    # the draws follow p (exact rule and max_distinct)
    idx = lg.sample(4000)
    freq = np.bincount(idx.reshape(-1), minlength=3) / idx.size
    assert np.abs(freq - p).max() < 0.02               # 12 000 draws: standard error < 0.005
    md = _league(3, sampling="pfsp", max_distinct=64, seed=2)
    md.in_play = [0, 1]
    md.record(_table([(6, 2), (0, 8)]))
    idx = md.sample(4000)
    assert idx.shape == (4000, 3) and np.bincount(idx.reshape(-1), minlength=3).argmin() == 1     # (p = 0.44, 0.17, 0.39)
    # "reference" reports the reference distribution
    ref = _league(3)
    ref.in_play = [0, 1]
    ref.record(_table([(6, 2), (0, 8)]))
    assert np.array_equal(ref.probabilities(), league.get_prob_dist(3)) and ref.central_share().tolist() == [0.3, 0.9, 0.5]


def test_decay_and_reduce_and_zero_weight_fallback():
    lg = _league(2, decay=0.5, pfsp_prior=0.0, sampling="pfsp")
    lg.in_play = [0]
    lg.record(_table([(4, 12)]))
    assert lg.records[0].tolist() == [16, 16, 4, 12, 20, 60]
    lg.record(_table([(2, 0)]))                        # what is on record is halved first
    assert lg.records[0].tolist() == [8 + 2, 8 + 2, 2 + 2, 6, 10 + 10, 30]
    lg.in_play = [1]
    lg.record(_table([(0, 0)]))                        # nothing new: decay only, and no record for a snapshot never met
    assert lg.records[0].tolist() == [5, 5, 2, 3, 10, 15] and 1 not in lg.records
    # a stub reduce: sees the dense [len(earlier), 6] int64 tensor in deque order; its result is what is added
    seen = []

    def reduce(dense):
        seen.append(dense.clone())
        return dense * 3
    lg2 = _league(4, decay=1.0)
    lg2.in_play = [2, 0]
    lg2.record(_table([(1, 2), (3, 4)]), reduce=reduce)
    assert seen[0].shape == (4, 6) and seen[0].dtype == torch.int64
    assert seen[0][2].tolist() == [3, 3, 1, 2, 5, 10] and seen[0][0].tolist() == [7, 7, 3, 4, 15, 20] and int(seen[0][1].sum()) == 0
    assert lg2.records[2].tolist() == [9, 9, 3, 6, 15, 30] and lg2.records[0].tolist() == [21, 21, 9, 12, 45, 60]
    # all weights zero (prior 0 and the central policy won every decided seat): the reference distribution takes their place
    z = _league(3, sampling="pfsp", pfsp_prior=0.0)
    z.in_play = [0, 1, 2]
    z.record(_table([(0, 5), (0, 1), (0, 9)]))
    assert z.central_share().tolist() == [1.0, 1.0, 1.0]
    assert np.allclose(z.probabilities(), league.get_prob_dist(3), rtol=0, atol=1e-15)
    assert z.sample(5).shape == (5, 3)
    with pytest.raises(ValueError):
        _league(3).record(_table([(1, 1)]))            # no assignment on record
    z.in_play = [0]
    with pytest.raises(ValueError):
        z.record(_table([(1, 1), (1, 1)]))             # a table of two nets for one net in play


# ---------------------------------------------------------------- TrainingLoop
class _Env(object):
    n = 10

    def set_reward_annealing_factor(self, f):
        pass


class _Storage(object):
    games_complete = 3
    league_stats = None


class _Collector(object):
    N = 10

    def __init__(self, with_table):
        self.with_table, self.nets, self.league_stats = with_table, 0, with_table

    def gather_rollouts(self):
        st = _Storage()
        if self.with_table:
            t = torch.zeros((self.nets + 1, 6), dtype=torch.int64)
            for k in range(self.nets):
                t[k] = torch.tensor([2, 2, 1, 1, 7, 8])
            t[self.nets] = torch.tensor([2 * self.nets, 2 * self.nets, self.nets, 9, 0, 0])
            st.league_stats = t
        return st

    def after_rollouts(self):
        pass

    def set_opponents(self, nets, idx):
        self.nets = len(nets)


class _Trainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)

        class C:
            entropy_coef = 0.0
        self.cfg = C()

    def update(self, st):
        return (0.1, 0.2, 0.3)


def _loop(with_table, path=None, **lkw):
    net = torch.nn.Linear(3, 3)
    args = tl.TrainArgs(num_steps=4, total_env_steps=4 * 10 * 50, add_policy_every=2)
    return tl.TrainingLoop(_Env(), net, _Collector(with_table), _Trainer(net), args, league=league.League(envs_per_worker=5, seed=1, **lkw),
                           make_net=lambda: torch.nn.Linear(3, 3), checkpoint_path=path)


def test_training_loop_scoreboard_and_checkpoint(tmp_path):
    off = _loop(False, str(tmp_path / "off.pt"))
    outs = [off.run_update() for _ in range(3)]
    assert all("league" not in o for o in outs) and off.league.records == {}
    assert "league_serials" not in torch.load(str(tmp_path / "off.pt"), weights_only=False)      # off: the checkpoint's keys as they were
    on = _loop(True, str(tmp_path / "on.pt"), sampling="pfsp", decay=1.0)
    o0 = on.run_update()
    assert "league" not in o0 and on.league.records == {}        # the first rollout's random-initialised opponents are no snapshots
    o1 = on.run_update()                                         # played against the draw after update 0: snapshot 0 alone
    lg = o1["league"]
    assert sorted(lg) == ["central_share", "pairs", "probabilities", "serials", "totals"]
    assert lg["serials"] == [0] and lg["pairs"] == [2.0] and lg["central_share"] == [(1 + 1) / (1 + 1 + 2)] and lg["probabilities"] == [1.0]
    assert lg["totals"] == dict(zip(spec.LEAGUE_STATS_TOTALS, [2, 2, 1, 9, 0, 0]))
    o2 = on.run_update()                                         # update 2 adds snapshot 1 before the scoreboard is taken
    assert o2["league"]["serials"] == [0, 1] and o2["league"]["pairs"] == [4.0, 0.0] and len(o2["league"]["probabilities"]) == 2
    import json
    json.dumps(o2["league"])
    # save / load round trip of serials and records
    ck = torch.load(str(tmp_path / "on.pt"), weights_only=False)
    assert ck["league_serials"] == [0, 1] and ck["league_records"] == {0: [4.0, 4.0, 2.0, 2.0, 14.0, 16.0]}
    re = _loop(True, sampling="pfsp", decay=1.0)
    re.load(str(tmp_path / "on.pt"))
    assert re.league.serials() == [0, 1] and re.league.records[0].tolist() == on.league.records[0].tolist()
    assert re.league.in_play is not None                         # load draws opponents: the next rollout is on record again
    assert "league" in re.run_update()
    re.league.add(torch.nn.Linear(3, 3))
    assert re.league.serials() == [0, 1, 2]                      # numbering goes on behind the restored serials
    # a checkpoint without the new keys: numbered afresh, no records
    old = {k: v for k, v in ck.items() if not k.startswith("league_")}
    torch.save(old, str(tmp_path / "old.pt"))
    lo = _loop(True)
    lo.load(str(tmp_path / "old.pt"))
    assert lo.league.serials() == [0, 1] and lo.league.records == {} and lo.update_num == 3
    # the reference-tuple checkpoint is unchanged
    on.save_reference_tuple(str(tmp_path / "ref.pt"))
    tup = torch.load(str(tmp_path / "ref.pt"), weights_only=False)
    assert len(tup) == 5 and len(tup[1]) == 2


def test_train_tool_flags(monkeypatch, capsys):
    """--league-stats and --league-sampling reach the collector and the league; PFSP implies the statistics"""
    import importlib.util
    import os
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

    class Col(Obj):
        pass

    class Loop(object):
        def __init__(self, env, net, col, tr, targs, league=None, **kw):
            Loop.league = league

        def run_update(self):
            return {"update": 0, "eval": None, "league": {"serials": [4, 5, 6], "pairs": [1.0, 2.0, 3.0], "central_share": [0.5, 0.25, 0.75],
                                                          "probabilities": [0.2, 0.5, 0.3], "totals": {"games_tallied": 12}}}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        made.clear()
        monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
        monkeypatch.setattr(cdist, "init_from_env", lambda *a, **kw: (0, 0, 1))
        for mod, name, cls in ((env_mod, "VecCatanEnv", Obj), (policy, "CatanPolicy", Obj), (rollout, "RolloutCollector", Col), (train, "PPOTrainer", Obj)):
            monkeypatch.setattr(mod, name, cls)
        monkeypatch.setattr(tl, "TrainingLoop", Loop)
        monkeypatch.setattr("sys.argv", ["train.py", "--updates", "1"] + extra)
        s = importlib.util.spec_from_file_location("train_tool_league_stats", os.path.join(root, "tools", "train.py"))
        tool = importlib.util.module_from_spec(s)
        s.loader.exec_module(tool)
        tool.main()
        return made["Col"][0], Loop.league, capsys.readouterr().out
    kw, lg, _ = run([])
    assert "league_stats" not in kw and lg.sampling == "reference"
    kw, lg, out = run(["--league-stats"])
    assert kw["league_stats"] is True and lg.sampling == "reference"
    assert "lowest 0.250 against snapshot 5, highest 0.750 against snapshot 6" in out
    kw, lg, _ = run(["--league-sampling", "pfsp"])
    assert kw["league_stats"] is True and lg.sampling == "pfsp"
    kw, lg, _ = run(["--league", "0", "--league-stats"])
    assert "league_stats" not in kw and lg is None
