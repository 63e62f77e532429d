"""The rule-based "trader" player on the CPU: hand-built states with hand-written answers for its three rows and its
goal, the numpy restatement of the rule (tests/trader_reference.py) played on the oracle - legality, termination, at most three
proposals a turn, accepted trades, the builder's action wherever no new row fires -, its completed rows through the net's heads, and the
Python contracts around the device kernel (styles, TraderPolicy, make_teacher / eval_baselines)."""
import numpy as np
import pytest
import torch

import action_complete_reference as acr
import oracle_lib
import scripted_reference as sr
import trader_reference as tr
from oracle_vec_env import OracleVecEnv
from settlers_of_catan_rl_amd import spec, train_loop
from settlers_of_catan_rl_amd.scripted import ScriptedPolicy, TraderPolicy

BRICK, WOOD, ORE, SHEEP, WHEAT = range(5)
NEW_ROWS = ("2T", "11P", "11E")

# ---------------------------------------------------------------------------------------------- hand-built states
# the board of tests/test_scripted_cpu.py's hand-built states; only the topology matters here
TILE_RES = [1, 2, 3, 4, 5, 1, 2, 3, 4, 0, 5, 5, 2, 3, 4, 5, 1, 2, 4]
TILE_VAL = [6, 8, 3, 5, 9, 10, 11, 4, 2, 0, 12, 6, 8, 3, 4, 5, 9, 10, 11]


def _put(b, name, v):
    spec.state_field(b, name)[:] = v


@pytest.fixture(scope="module")
def base(oracle):
    """a normal turn of player 1 after the roll on an empty board: nothing built, nothing held; order 1, 2, 3, 4 (labels from player 1:
    player 2 is 0, 3 is 1, 4 is 2); every player at 2 victory points"""
    env = oracle_lib.OracleEnv(1, 0)
    env.reset()
    b = env.export().copy()
    res, val = spec.state_field(b, "tile_res"), spec.state_field(b, "tile_val")
    desert_val = int(val[list(res).index(0)])
    _put(b, "tile_res", TILE_RES)
    tv = list(TILE_VAL)
    tv[9] = desert_val
    _put(b, "tile_val", tv)
    _put(b, "robber_tile", 9)
    for name in ("corner_bld", "corner_owner", "edge_owner"):
        _put(b, name, 0)
    for p in (1, 2, 3, 4):
        _put(b, f"p{p}_res", 0); _put(b, f"p{p}_vis", 0); _put(b, f"p{p}_harbours", 0)
    _put(b, "bank_res", 19)
    _put(b, "settlements_left", 5); _put(b, "cities_left", 4)
    _put(b, "player_order", [1, 2, 3, 4]); _put(b, "player_order_id", 0); _put(b, "players_go", 1)
    _put(b, "initial_phase", 0); _put(b, "init_settlements", 2); _put(b, "init_roads", 2)
    _put(b, "dice_rolled", 1)
    _put(b, "curr_vps", 2)
    return b


def _build(b, corner, player, kind=1):
    spec.state_field(b, "corner_bld")[corner] = kind
    spec.state_field(b, "corner_owner")[corner] = player


def _decide(b):
    env = oracle_lib.OracleEnv(1, 0)
    env.import_(b)
    blob, masks = env.export(), env.masks()
    a, row = tr.decide(blob, masks)
    assert env.is_legal(a), a.tolist()
    return a.tolist(), row


def _action(t, **cols):
    a = [0] * 18
    a[0] = t
    for k, v in cols.items():
        a[{"response": 5, "player": 6, "give": 7, "want": 11, "res_a": 15, "res_b": 16}[k]] = v
    return a


def _offer(base, give, recv, hand=(1, 0, 0, 2, 0)):
    """player 2, on its turn, offers `give` for `recv` (r0 lists) to player 1, who owns a settlement on corner 0 and holds `hand`:
    brick and two sheep.  Player 1's goals: City (deficit 5), Road (needs the wood: 1), DevCard (ore, wheat: 2) - the road."""
    b = base.copy()
    _build(b, 0, 1)
    _put(b, "players_go", 2)
    _put(b, "p1_res", hand)
    _put(b, "p2_res", [2, 2, 2, 2, 2])
    _put(b, "must_respond", 1); _put(b, "trade_proposer", 2); _put(b, "trade_target", 1)
    _put(b, "trade_n_give", len(give)); _put(b, "trade_n_recv", len(recv))
    spec.state_field(b, "trade_give")[:len(give)] = [r + 1 for r in give]
    spec.state_field(b, "trade_recv")[:len(recv)] = [r + 1 for r in recv]
    return b


def test_row2t_accepts_what_lowers_the_deficit(base):
    assert _decide(_offer(base, [WOOD], [SHEEP])) == (_action(sr.RESPOND, response=tr.ACCEPT), "2T")     # wood completes the road


def test_row2t_one_reject_for_each_condition(base):
    reject = (_action(sr.RESPOND, response=sr.REJECT), "2T")
    assert _decide(_offer(base, [WOOD], [ORE])) == reject                       # accept is illegal: no ore to pay with
    assert _decide(_offer(base, [WOOD], [SHEEP, SHEEP])) == reject              # two cards asked for one (both held, the road still completes)
    b = _offer(base, [WOOD], [SHEEP])
    spec.state_field(b, "curr_vps")[1] = 8                                      # the proposer is at 8 victory points
    assert _decide(b) == reject
    spec.state_field(b, "curr_vps")[1] = 7
    assert _decide(b)[0][5] == tr.ACCEPT
    assert _decide(_offer(base, [ORE], [SHEEP])) == reject                      # ore does not lower the road's deficit (the goal comes from h, not h')
    # no goal: no settlement (City), a site on the own road 0-1 but no settlement piece left (Settlement, and Road because of the site), an empty pile
    b = _offer(base, [WOOD], [SHEEP])
    _put(b, "corner_bld", 0); _put(b, "corner_owner", 0)
    spec.state_field(b, "edge_owner")[4] = 1
    spec.state_field(b, "settlements_left")[0] = 0
    _put(b, "pile_len", 0)
    assert tr.goal_of(b, 0, [1, 0, 0, 2, 0]) is None
    assert _decide(b) == reject
    _put(b, "pile_len", 5)                                                      # ... with a pile the goal is a card: wood does not help it either
    assert _decide(b) == reject


def _seller(base, k, vps=(2, 3, 2, 2), woods=(1, 1, 1)):
    """player 1 (settlement on corner 0; brick and two sheep: the road lacks its wood, a sheep is spare) with k proposals made this
    turn; players 2, 3, 4 hold `woods` and stand at vps[1:]"""
    b = base.copy()
    _build(b, 0, 1)
    _put(b, "p1_res", [1, 0, 0, 2, 0])
    for p, w in zip((2, 3, 4), woods):
        spec.state_field(b, f"p{p}_res")[WOOD] = w
    _put(b, "curr_vps", vps)
    _put(b, "trades_this_turn", k)
    return b


def test_row11p_asks_the_candidates_weakest_first_once_each(base):
    def propose(label):
        return (_action(sr.PROPOSE, player=label, give=SHEEP + 1, want=WOOD + 1), "11P")
    # candidates by (victory points, label): player 3 (2, label 1), player 4 (2, label 2), player 2 (3, label 0)
    assert _decide(_seller(base, 0)) == propose(1)
    assert _decide(_seller(base, 1)) == propose(2)
    assert _decide(_seller(base, 2)) == propose(0)
    assert _decide(_seller(base, 3)) == (_action(sr.ENDTURN), 12)               # k past the candidates: the builder's row
    assert _decide(_seller(base, 0, vps=(2, 3, 8, 2))) == propose(2)            # player 3 at 8 points is no candidate
    assert _decide(_seller(base, 1, vps=(2, 3, 8, 2))) == propose(0)
    assert _decide(_seller(base, 2, vps=(2, 3, 8, 2))) == (_action(sr.ENDTURN), 12)
    assert _decide(_seller(base, 0, woods=(1, 0, 0))) == propose(0)             # only player 2 holds wood
    assert _decide(_seller(base, 0, woods=(0, 0, 0))) == (_action(sr.ENDTURN), 12)


def _banker(base, sheep, harbours=()):
    b = base.copy()
    _build(b, 0, 1)
    _put(b, "p1_res", [1, 0, 0, sheep, 0])                                      # the road lacks its wood; nobody else holds a card
    for i in harbours:
        spec.state_field(b, "p1_harbours")[i] = 1
    return b


def test_row11e_exchanges_spare_cards_at_the_players_rate(base):
    exchange = (_action(sr.EXCHANGE, res_a=SHEEP, res_b=WOOD), "11E")
    assert _decide(_banker(base, 4)) == exchange                                # 4:1
    assert _decide(_banker(base, 3)) == (_action(sr.ENDTURN), 12)
    assert _decide(_banker(base, 3, harbours=[0])) == exchange                  # 3:1 with the generic harbour
    assert _decide(_banker(base, 2, harbours=[0])) == (_action(sr.ENDTURN), 12)
    assert _decide(_banker(base, 2, harbours=[SHEEP + 1])) == exchange          # 2:1 with the sheep harbour
    assert _decide(_banker(base, 3, harbours=[WOOD + 1])) == (_action(sr.ENDTURN), 12)    # another resource's harbour does not count
    # refused for spare < rate although head 9 offers the resource: four sheep held, one of them is the card's own (goal DevCard:
    # ore and sheep held, the wheat missing), three spare at 4:1 - and the builder's row 11 wants five
    b = base.copy()
    _build(b, 0, 1)
    _put(b, "p1_res", [0, 0, 1, 4, 0])
    assert tr.goal_of(b, 0, [0, 0, 1, 4, 0]) == tr.GOALS.index("devcard")
    assert _decide(b) == (_action(sr.ENDTURN), 12)
    spec.state_field(b, "p1_res")[SHEEP] = 5
    assert _decide(b) == (_action(sr.EXCHANGE, res_a=SHEEP, res_b=WHEAT), "11E")


def test_goal_each_row_of_the_table_and_the_tie_order(base):
    def goal(b, h):
        g = tr.goal_of(b, 0, list(h))
        return None if g is None else tr.GOALS[g]
    town = base.copy()
    _build(town, 0, 1)
    assert goal(town, (0, 0, 3, 0, 2)) == "city"
    assert goal(town, (0, 0, 3, 0, 1)) == "city"                                # City 1 = DevCard 1 (the sheep): table order
    assert goal(town, (0, 0, 1, 1, 1)) == "devcard"                             # DevCard 0 < City 3
    spec.state_field(town, "cities_left")[0] = 0
    assert goal(town, (0, 0, 3, 0, 2)) == "devcard"
    site = base.copy()
    _build(site, 0, 1)
    spec.state_field(site, "edge_owner")[[4, 2]] = 1                            # corners 0-1-2: corner 2 is an open site
    assert goal(site, (1, 1, 0, 1, 0)) == "settlement"                          # Settlement 1, DevCard 2, City 5; Road is not available
    assert goal(site, (1, 1, 0, 0, 0)) == "settlement"                          # Settlement 2 < DevCard 3: the road (0) is not considered
    spec.state_field(site, "settlements_left")[0] = 0
    assert goal(site, (1, 1, 0, 0, 0)) == "devcard"                             # ... nor is it without a piece to settle with
    assert goal(base, (1, 0, 0, 0, 0)) == "road"                                # an empty board: Road 1 < DevCard 3
    assert goal(base, (1, 0, 0, 1, 1)) == "road"                                # Road 1 = DevCard 1: table order
    assert goal(base, (0, 0, 1, 1, 0)) == "devcard"                             # DevCard 1 < Road 2
    full = base.copy()
    spec.state_field(full, "edge_owner")[:15] = 1                               # fifteen roads, no free corner next to them left open ...
    for c in range(54):
        _build(full, c, 2)                                                      # ... every corner taken
    _put(full, "pile_len", 0)
    assert goal(full, (1, 1, 1, 1, 1)) is None


# ---------------------------------------------------------------------------------------------- all-trader games on the oracle
N_GAMES, SEED = 16, 11
# the largest number of decisions any of the 16 games needs under the twin is 921 (measured on the oracle, printed by the fixture): twice that
CAP = 1842


def play_all_trader(max_trades=None, n=N_GAMES, seed=SEED, cap=CAP, keep_every=0):
    """n oracle games without re-deal, the twin on every seat, lock-step until every game has ended or `cap` decisions were taken.
    OracleVecEnv.step asserts the oracle's legality check on every action."""
    env = OracleVecEnv(n, seed=seed, auto_reset=False)
    if max_trades is not None:
        env.b.set_config(max_trades_per_turn=max_trades)
    tally = tr.Tally()
    over = np.zeros(n, dtype=bool)
    length = np.zeros(n, dtype=np.int64)
    turn_key, in_turn, most = [None] * n, np.zeros(n, dtype=np.int64), 0
    same_as_builder = 0
    keep = {k: [] for k in ("f", "lists", "lens", "masks", "rows")}
    for it in range(cap):
        if over.all():
            break
        blobs, masks = env.export_state().numpy(), env.get_action_masks().numpy()
        obs = env.get_obs() if keep_every and it % keep_every == 0 else None
        actions = np.full((n, 18), -1, dtype=np.int32)
        for i in np.flatnonzero(~over):
            a, row = tr.decide(blobs[i], masks[i])
            tally.add(a, row, masks[i])
            key = (int(spec.state_field(blobs[i], "turn")[0]), int(spec.state_field(blobs[i], "players_go")[0]))
            if key != turn_key[i]:
                turn_key[i], in_turn[i] = key, 0
            if row == "11P":
                in_turn[i] += 1
                most = max(most, int(in_turn[i]))
            if row not in NEW_ROWS:
                assert np.array_equal(a, sr.decide(blobs[i], masks[i])[0]), (i, it, row)
                same_as_builder += 1
            actions[i] = a
            if obs is not None:
                keep["f"].append(obs[0][i].numpy()); keep["lists"].append(obs[1][i].numpy()); keep["lens"].append(obs[2][i].numpy())
                keep["masks"].append(masks[i]); keep["rows"].append(a.astype(np.int64))
        _, done = env.step(torch.from_numpy(actions))
        length[~over] += 1
        over |= done.numpy().astype(bool)
    return dict(over=over, length=length, counts=tally.c, most_proposals=most, same_as_builder=same_as_builder,
                keep={k: np.stack(v) for k, v in keep.items()} if keep_every else None)


@pytest.fixture(scope="module")
def games(oracle):
    out = play_all_trader(keep_every=8)
    print("all-trader games: decisions per game", out["length"].tolist(), "counters", out["counts"])
    return out


def test_all_trader_games_are_legal_and_end_inside_the_cap(games):
    assert games["over"].all(), games["length"].tolist()
    assert int(games["length"].max()) * 2 <= CAP + 1, int(games["length"].max())       # the cap is twice what the twin needs, not more
    assert games["counts"]["fallbacks"] == 0


def test_all_trader_games_trade(games):
    c = games["counts"]
    assert c["accepts"] >= 1 and c["proposals"] == c["responses"] == c["accepts"] + c["rejects_illegal"] + c["rejects_other"], c
    assert c["goal_exchanges"] >= 1, c
    assert games["most_proposals"] == 3                                                # reached, never passed


def test_no_turn_holds_more_than_three_proposals_without_a_limit(oracle):
    out = play_all_trader(max_trades=-1)
    assert out["over"].all() and out["most_proposals"] == 3 and out["counts"]["accepts"] >= 1, (out["length"], out["most_proposals"])


def test_outside_the_new_rows_the_action_is_the_builders(games):
    """(asserted decision by decision inside the play; here: that it was asserted often, and that the new rows fired too)"""
    c = games["counts"]
    assert games["same_as_builder"] == c["decisions"] - c["proposals"] - c["responses"] - c["goal_exchanges"] > 1000


def test_completed_trader_rows_have_finite_log_probs(games):
    d = games["keep"]
    raw = d["rows"]
    assert (raw[:, 0] == sr.PROPOSE).sum() >= 1 and ((raw[:, 0] == sr.RESPOND) & (raw[:, 5] == tr.ACCEPT)).sum() >= 1
    done = acr.complete_all(raw, d["masks"], d["f"][:, 12:18])
    torch.manual_seed(0)
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    net = CatanPolicy().eval()
    with torch.no_grad():
        lp = net.evaluate_actions(torch.from_numpy(d["f"]), torch.from_numpy(d["lists"]), torch.from_numpy(d["lens"]).long(),
                                  torch.from_numpy(d["masks"]), torch.from_numpy(done))[1][:, 0]
    assert bool(torch.isfinite(lp).all()), raw[~torch.isfinite(lp).numpy()][:4]
    prop = raw[:, 0] == sr.PROPOSE
    assert np.array_equal(done[prop][:, 6:15], raw[prop][:, 6:15])                     # a Propose row's own columns are never filled in


# ---------------------------------------------------------------------------------------------- Python contracts
class _StubEnv(object):
    def __init__(self, n):
        self.n, self.calls = n, []

    def sample_scripted_actions(self, games=None, out=None, **kw):
        self.calls.append(kw)
        rows = self.n if games is None else games.numel()
        a = torch.zeros((rows, 18), dtype=torch.int32)
        a[:, 0] = 10
        return a

    def complete_action_rows(self, actions, games=None):
        return actions


def test_policy_styles():
    f = torch.zeros((3, spec.OBS_FLOATS))
    env = _StubEnv(3)
    ScriptedPolicy(env).act(f, None, None, None)
    assert env.calls[-1] == {}                                                  # the builder's call is the one it always was
    TraderPolicy(env).act(f, None, None, None)
    assert env.calls[-1] == {"style": "trader"}
    TraderPolicy(env).label()
    assert env.calls[-1] == {"style": "trader"}
    ScriptedPolicy(env, style="trader").label()
    assert env.calls[-1] == {"style": "trader"}
    ScriptedPolicy(env).label()
    assert env.calls[-1] == {}
    assert ScriptedPolicy().style == "builder" and TraderPolicy().style == "trader" and TraderPolicy(style="builder").style == "builder"
    assert isinstance(TraderPolicy(), ScriptedPolicy) and TraderPolicy.wants_games is True and TraderPolicy.include_lstm is False
    with pytest.raises(ValueError, match="style"):
        ScriptedPolicy(env, style="banker")
    with pytest.raises(RuntimeError, match="TraderPolicy"):
        TraderPolicy().act(f, None, None, None)                                 # unbound
    with pytest.raises(RuntimeError, match="TraderPolicy"):
        TraderPolicy().label()
    other = _StubEnv(2)
    pol = TraderPolicy()
    assert pol.rebind(other) is pol and pol.env is other


def test_env_style_check_needs_no_device():
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    assert VecCatanEnv.SCRIPTED_STYLES == {"builder": 0, "trader": 1} and len(VecCatanEnv.TRADE_COUNT_KEYS) == 8
    assert VecCatanEnv.TRADE_COUNT_KEYS == tr.COUNT_KEYS
    with pytest.raises(ValueError, match="style"):
        VecCatanEnv.__new__(VecCatanEnv).sample_scripted_actions(style="banker")          # refused before anything of the env is touched


def test_make_teacher_and_eval_baselines():
    A = train_loop.TrainArgs
    env = _StubEnv(2)
    assert A().eval_trader_baseline is False and A().teacher is None
    assert train_loop.eval_baselines(A()) is None
    assert train_loop.eval_baselines(A(eval_scripted_baseline=True)) == {"scripted": ScriptedPolicy}
    assert train_loop.eval_baselines(A(eval_trader_baseline=True)) == {"trader": TraderPolicy}
    assert list(train_loop.eval_baselines(A(eval_scripted_baseline=True, eval_trader_baseline=True))) == ["scripted", "trader"]
    assert train_loop.make_teacher(A(), env) is None
    assert train_loop.make_teacher(A(teacher="trader"), env) is None            # no coefficient, no teacher
    t = train_loop.make_teacher(A(teacher="trader", teacher_coef=0.5), env)
    assert type(t) is TraderPolicy and t.env is env and t.style == "trader"
    t = train_loop.make_teacher(A(teacher="scripted", teacher_coef=0.5), env)
    assert type(t) is ScriptedPolicy and t.style == "builder"
    with pytest.raises(ValueError, match="trader"):
        train_loop.make_teacher(A(teacher="banker", teacher_coef=0.5), env)


def test_the_library_declares_the_new_entry_points():
    from settlers_of_catan_rl_amd import _lib
    assert {"catan_sample_scripted_actions_style", "catan_scripted_trade_counts"} <= set(_lib.declared_symbols())
    assert _lib.TRANSLATION_UNITS == ("catan_abi.hip", "catan_players.hip", "catan_hooks.hip")
