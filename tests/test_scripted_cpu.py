"""The rule-based "builder" player on the CPU: the numpy restatement of the rule (tests/scripted_reference.py) played on
the oracle - legality and termination -, hand-built states with hand-written answers, and the Python contracts around the device
kernel (ScriptedPolicy.act, run_evaluation_protocol(baselines=None))."""
import random

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle_lib
import scripted_reference as sr
from settlers_of_catan_rl_amd import evaluation as ev
from settlers_of_catan_rl_amd import spec
from settlers_of_catan_rl_amd.scripted import ScriptedPolicy

CAP = 4000                       # decisions per game


def play_scripted_game(seed, env_id, scripted_seats=(1, 2, 3, 4), cap=CAP):
    """one oracle game: the rule for `scripted_seats` (PlayerIds), the oracle's uniform-random legal policy for the others.
    -> (winner PlayerId or 0, decisions, per-row counts [14], per-card counts [5])"""
    env = oracle_lib.OracleEnv(seed, env_id)
    env.reset()
    rows, cards = np.zeros(14, dtype=np.int64), np.zeros(5, dtype=np.int64)
    for k in range(cap):
        blob, masks = env.export(), env.masks()
        if sr.deciding_pid0(blob) + 1 in scripted_seats:
            a, row = sr.decide(blob, masks)
            rows[row] += 1
            if row == 8:
                cards[a[4]] += 1
        else:
            a = env.sample_action(seed + 99, env_id, k, masks)
        assert env.is_legal(a), (seed, env_id, k, a.tolist())
        _, done = env.step(a)
        if done:
            return int(spec.state_field(env.export(), "winner")[0]), k + 1, rows, cards
    return 0, cap, rows, cards


def test_all_seats_scripted_games_are_legal_and_end():
    """16 games, the rule on all four seats: every action passes the oracle's legality check (Game.validate_action restated) and every
    game has a winner before 4 000 decisions.  (No seed had to be left out: the first 16 game streams of seed 11 all end.)"""
    total = np.zeros(14, dtype=np.int64)
    for g in range(16):
        winner, n, rows, _ = play_scripted_game(11, g)
        assert 1 <= winner <= 4 and n < CAP, (g, winner, n)
        total += rows
    assert total[13] == 0 and total[2] == 0 and total[12] > 0          # no fall-back; nobody proposes, so nobody responds


# ---------------------------------------------------------------------------------------------- hand-built states
# The board of every hand-built state (tile order): terrain 0 Desert 1 Hills 2 Forest 3 Mountains 4 Pastures 5 Fields, and its tokens.
TILE_RES = [1, 2, 3, 4, 5, 1, 2, 3, 4, 0, 5, 5, 2, 3, 4, 5, 1, 2, 4]
TILE_VAL = [6, 8, 3, 5, 9, 10, 11, 4, 2, 0, 12, 6, 8, 3, 4, 5, 9, 10, 11]
# pips per tile:  5  5  2  4  4   3   2  3  1  0   1  5  5  2  3  4  4   3   2
# corner values used below (tests/golden/topology.npz corner_tile): c0 {0} 5, c1 {0} 5, c2 {0,3} 9, c3 {0,3,4} 13, c4 {0,1,4} 14


def _base(desert_val):
    """a normal turn of player 1 after the roll on an empty board: nothing built, nothing held"""
    env = oracle_lib.OracleEnv(1, 0)
    env.reset()
    b = env.export().copy()

    def put(name, v):
        spec.state_field(b, name)[:] = v
    put("tile_res", TILE_RES)
    val = list(TILE_VAL)
    val[9] = desert_val
    put("tile_val", val)
    put("robber_tile", 9)
    for name in ("corner_bld", "corner_owner", "edge_owner"):
        put(name, 0)
    for p in (1, 2, 3, 4):
        put(f"p{p}_res", 0)
        put(f"p{p}_vis", 0)
    put("bank_res", 19)
    put("settlements_left", 5); put("cities_left", 4)
    put("player_order", [1, 2, 3, 4]); put("player_order_id", 0); put("players_go", 1)
    put("initial_phase", 0); put("init_settlements", 2); put("init_roads", 2)
    put("dice_rolled", 1)
    return b


def _build(b, corner, player, kind=1):
    spec.state_field(b, "corner_bld")[corner] = kind
    spec.state_field(b, "corner_owner")[corner] = player


def _decide(b):
    env = oracle_lib.OracleEnv(1, 0)
    env.import_(b)
    blob, masks = env.export(), env.masks()
    a, row = sr.decide(blob, masks)
    assert env.is_legal(a), a.tolist()
    return a.tolist(), row


def _action(t, **heads):
    a = [0] * 18
    a[0] = t
    for k, v in heads.items():
        a[{"corner": 1, "edge": 2, "tile": 3, "card": 4, "response": 5, "player": 6, "res_a": 15, "res_b": 16, "discard": 17}[k]] = v
    return a


@pytest.fixture(scope="module")
def desert_val():
    env = oracle_lib.OracleEnv(1, 0)
    env.reset()
    b = env.export()
    res, val = spec.state_field(b, "tile_res"), spec.state_field(b, "tile_val")
    return int(val[list(res).index(0)])


def test_row1_discard_the_resource_held_most(desert_val):
    b = _base(desert_val)
    spec.state_field(b, "need_discard")[:] = 1; spec.state_field(b, "n_to_discard")[:] = 1; spec.state_field(b, "to_discard")[0] = 3
    spec.state_field(b, "p3_res")[:] = [2, 3, 1, 3, 0]               # wood and sheep tie at 3: the lower index, wood
    assert _decide(b) == (_action(sr.DISCARD, discard=1), 1)


def test_row3_steal_from_the_fuller_hand_then_the_higher_score(desert_val):
    b = _base(desert_val)
    spec.state_field(b, "robber_tile")[:] = 4; spec.state_field(b, "just_moved_robber")[:] = 1
    _build(b, 3, 2); _build(b, 18, 3)                                # both on tile 4
    spec.state_field(b, "p2_res")[:] = [1, 1, 0, 0, 0]; spec.state_field(b, "p3_res")[:] = [0, 0, 2, 0, 0]
    spec.state_field(b, "curr_vps")[:] = [2, 2, 3, 2]                # two cards each: player 3 has more points; he is "next_next" of player 1
    assert _decide(b) == (_action(sr.STEAL, player=1), 3)
    spec.state_field(b, "p2_res")[:] = [1, 1, 1, 0, 0]               # now player 2 ("next") holds more cards
    assert _decide(b) == (_action(sr.STEAL, player=0), 3)


def test_row4_robber_on_the_best_tile_of_the_others(desert_val):
    b = _base(desert_val)
    spec.state_field(b, "can_move_robber")[:] = 1
    _build(b, 3, 2)                  # player 2: a settlement on tiles 0, 3, 4      -> tile 0: 5 x 1, tile 3: 4 x 1
    _build(b, 8, 3, kind=2)          # player 3: a city on tiles 1, 2, 5           -> tile 1: 5 x 2 = 10, tile 2: 2 x 2
    _build(b, 19, 1)                 # own settlement on tiles 4, 5, 9: those score -1000
    assert _decide(b) == (_action(sr.ROBBER, tile=1), 4)


def test_row6_city_on_the_corner_with_more_pips(desert_val):
    b = _base(desert_val)
    _build(b, 0, 1); _build(b, 4, 1)                                 # corner values 5 and 14
    spec.state_field(b, "p1_res")[:] = [0, 0, 3, 0, 2]
    assert _decide(b) == (_action(sr.CITY, corner=4), 6)


def test_row7_settlement_on_the_corner_with_more_pips(desert_val):
    b = _base(desert_val)
    _build(b, 0, 1)
    spec.state_field(b, "edge_owner")[[4, 2, 0]] = 1                 # corners 0-1-2-3: 2 (value 9) and 3 (value 13) are legal
    spec.state_field(b, "p1_res")[:] = [1, 1, 0, 1, 1]
    assert _decide(b) == (_action(sr.SETTLE, corner=3), 7)


def _with_card(b, card):
    spec.state_field(b, "p1_n_hidden")[:] = 1
    spec.state_field(b, "p1_hidden")[0] = card
    return b


def test_row8_each_card_kind(desert_val):
    assert _decide(_with_card(_base(desert_val), sr.KNIGHT)) == (_action(sr.PLAYDEV, card=sr.KNIGHT), 8)
    assert _decide(_with_card(_base(desert_val), sr.ROAD_BUILDING)) == (_action(sr.PLAYDEV, card=sr.ROAD_BUILDING), 8)
    b = _with_card(_base(desert_val), sr.YEAR_OF_PLENTY)
    spec.state_field(b, "p1_res")[:] = [2, 0, 1, 0, 3]               # fewest: wood (before sheep); with a wood in hand: sheep
    assert _decide(b) == (_action(sr.PLAYDEV, card=sr.YEAR_OF_PLENTY, res_a=1, res_b=3), 8)
    b = _with_card(_base(desert_val), sr.MONOPOLY)
    spec.state_field(b, "p2_res")[:] = [1, 0, 0, 2, 0]; spec.state_field(b, "p3_res")[:] = [0, 0, 0, 2, 1]; spec.state_field(b, "p4_res")[:] = [1, 0, 0, 0, 0]
    assert _decide(b) == (_action(sr.PLAYDEV, card=sr.MONOPOLY, res_a=3), 8)     # the others hold 4 sheep
    # a victory-point card is never played: the turn ends
    assert _decide(_with_card(_base(desert_val), sr.VICTORY_POINT)) == (_action(sr.ENDTURN), 12)


def test_row10_road_under_both_conditions(desert_val):
    # road building in progress: Road is the only legal type.  Settlement on corner 0, road 4 (corners 0-1): edge 2 leads to the free
    # corner 2 (value 9), edge 5 to corner 5, which is next to the settlement (-1)
    b = _base(desert_val)
    _build(b, 0, 1)
    spec.state_field(b, "edge_owner")[4] = 1
    spec.state_field(b, "road_building_active")[:] = 1
    assert _decide(b) == (_action(sr.ROAD, edge=2), 10)
    # a normal turn with wood and brick and no open site (corner 1 is next to the settlement): the same road is bought
    b = _base(desert_val)
    _build(b, 0, 1)
    spec.state_field(b, "edge_owner")[4] = 1
    spec.state_field(b, "p1_res")[:] = [1, 1, 0, 0, 0]
    assert _decide(b) == (_action(sr.ROAD, edge=2), 10)
    # ... with that road in place corner 2 is an open site: the player saves for the settlement and ends the turn
    spec.state_field(b, "edge_owner")[2] = 1
    assert _decide(b) == (_action(sr.ENDTURN), 12)


def test_row11_exchange_from_five_of_a_kind(desert_val):
    b = _base(desert_val)
    spec.state_field(b, "p1_res")[:] = [5, 0, 1, 0, 0]               # five brick at 4:1; wood is the lowest-index resource held least
    assert _decide(b) == (_action(sr.EXCHANGE, res_a=0, res_b=1), 11)
    spec.state_field(b, "p1_res")[:] = [4, 0, 1, 0, 0]               # four can be exchanged, but the bot keeps them
    assert _decide(b) == (_action(sr.ENDTURN), 12)


# ---------------------------------------------------------------------------------------------- Python contracts
class _StubEnv(object):
    def __init__(self, n):
        self.n, self.calls = n, []

    def sample_scripted_actions(self, games=None, out=None):
        self.calls.append(None if games is None else games.clone())
        rows = self.n if games is None else games.numel()
        g = torch.arange(self.n) if games is None else games.long()
        a = torch.zeros((rows, 18), dtype=torch.int32)
        a[:, 0], a[:, 1] = 10, g.to(torch.int32)
        return a


def test_scripted_policy_act_contract():
    env = _StubEnv(6)
    pol = ScriptedPolicy(env)
    assert pol.wants_games is True and pol.include_lstm is False and not hasattr(pol, "inference_copy")
    f = torch.zeros((6, spec.OBS_FLOATS))
    v, a, lp = pol.act(f, None, None, None)
    assert v.shape == (6, 1) and lp.shape == (6, 1) and a.shape == (6, 18) and a.dtype == torch.int64
    assert v.dtype == torch.float32 and float(v.abs().sum()) == 0.0 and float(lp.abs().sum()) == 0.0
    assert env.calls[-1] is None and a[:, 1].tolist() == list(range(6))
    games = torch.tensor([4, 1, 5])
    v, a, lp = pol.act(f[:3], None, None, None, games=games, deterministic=True, generator=None, return_entropy=True)
    assert a.shape == (3, 18) and a[:, 1].tolist() == [4, 1, 5] and v.shape == (3, 1) and lp.shape == (3, 1)
    with pytest.raises(ValueError):
        pol.act(f[:3], None, None, None)                              # without `games` it must be handed all rows
    with pytest.raises(ValueError):
        pol.act(f[:2], None, None, None, games=games)
    other = _StubEnv(2)
    assert pol.rebind(other) is pol and pol.env is other
    with pytest.raises(RuntimeError):
        ScriptedPolicy().act(f, None, None, None)


def test_protocol_without_baselines_is_the_parent_log(monkeypatch):
    """run_evaluation_protocol(baselines=None) on the games of tests/golden/eval_small.npz (the reference's EvaluationManager): the log
    and the summary are what the protocol returned before it knew baselines, to the byte."""
    import rollout_fixture as rf
    from oracle_vec_env import OracleVecEnv
    g = gu.load("eval_small.npz")
    n, seed = int(g["n_games"]), int(g["seed"])
    cenvs = []

    def make_env(m):
        assert m == n
        cenvs.append(rf.CountingEnv(OracleVecEnv(m, seed, auto_reset=False)))
        return cenvs[-1]
    table = {}

    def act_fn(net, idx, f, lists, lens, masks):
        cenv = cenvs[-1]
        if id(cenv) not in table:
            table[id(cenv)] = rf.ReplayPolicy(cenv, [g[f"g{i}_trace"] for i in range(n)])
        t = table[id(cenv)]
        k = torch.minimum(cenv.steps_taken, t.lens)
        return t.table[torch.arange(n), k][idx.cpu()].to(f.device)
    orders = np.stack([g[f"g{i}_order"].astype(np.int64) for i in range(n)])
    monkeypatch.setattr(ev, "sample_orders", lambda m, rng=None: orders)
    log, summary = ev.run_evaluation_protocol(make_env, object(), object(), n, update_num=7, rng=random.Random(0), act_fn=act_fn)
    res = np.array([[int(x) for x in g[f"g{i}_result"]] for i in range(n)])     # winner, victory points, steps, decisions
    want = {"update": 7, "random": {"policy_win_frac": float(np.mean(res[:, 0] == 0)), "avg_game_length": float(np.mean(res[:, 2])),
                                    "avg_policy_decisions": float(np.mean(res[:, 3])), "avg_victory_points": float(np.mean(res[:, 1]))}}
    assert log == want and list(log) == ["update", "random"] and list(log["random"]) == list(want["random"])
    r = want["random"]
    assert summary == ("\n\n---------------------- EVALUATION (after {} updates) ----------------------\n"
                       "{} games against random. Policy won {}/{}. Avg. game length: {}. Avg num policy decisions: {}. "
                       "Avg victory points for policy: {}. \n\n").format(7, n, int(np.sum(res[:, 0] == 0)), n, r["avg_game_length"],
                                                                       r["avg_policy_decisions"], r["avg_victory_points"])
    assert len(cenvs) == 1


def test_protocol_baselines_add_a_log_entry_each():
    """a baseline is played after the protocol's own games, on an env of its own that it is bound to, against three copies of itself
    (the decisions come from the test hook act_fn here: what is checked is the protocol around them)"""
    import ctypes as C
    from oracle_vec_env import OracleVecEnv
    bound, envs = [], []

    class Baseline(object):
        wants_games = True

        def rebind(self, env):
            bound.append(env)

    def make_env(m):
        envs.append(OracleVecEnv(m, 3, auto_reset=False))
        return envs[-1]

    def act_fn(net, idx, f, lists, lens, masks):
        env, out = envs[-1], np.zeros((len(idx), 18), dtype=np.int32)
        for j, i in enumerate(idx.tolist()):
            m = np.ascontiguousarray(masks[j].numpy(), dtype=np.float32)
            env.L.orc_sample_action(env.b.env_ptr(i), 5, i, int(env.steps_taken[i]), m.ctypes.data_as(C.POINTER(C.c_float)),
                                    out[j].ctypes.data_as(C.POINTER(C.c_int32)))
        return torch.from_numpy(out).long()
    kw = dict(rng=random.Random(1), max_steps=3, act_fn=act_fn)
    log, summary = ev.run_evaluation_protocol(make_env, object(), object(), 2, baselines={"scripted": Baseline}, **kw)
    assert list(log) == ["update", "random", "scripted"] and list(log["scripted"]) == list(log["random"])
    assert len(envs) == 2 and bound == [envs[1]]
    assert summary.count("games against") == 2 and "2 games against scripted. Policy won 0/2." in summary
    with pytest.raises(ValueError):
        ev.run_evaluation_protocol(make_env, object(), object(), 2, baselines={"random": Baseline()}, **kw)
