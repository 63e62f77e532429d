"""The tournament's host side without a GPU: the lineup builders, the seat rule's balance, run_tournament on the oracle
twin (tests/tournament_reference.py) and fit_ratings against expected counts and the test's own likelihood."""
import itertools
import math

import numpy as np
import pytest
import torch

import tournament_reference as tr
from settlers_of_catan_rl_amd import spec
from settlers_of_catan_rl_amd import tournament as tn
from settlers_of_catan_rl_amd.scripted import RandomPolicy


# ---------------------------------------------------------------- lineups
def test_all_lineups_counts_and_multisets():
    for m in (4, 5, 6, 9):
        a = tn.all_lineups(m)
        assert a.shape == (math.comb(m, 4), 4) and a.dtype == np.int64
        assert len({tuple(r) for r in a.tolist()}) == len(a) and all(len(set(r)) == 4 and list(r) == sorted(r) for r in a.tolist())
    for m in (1, 2, 3):
        a = tn.all_lineups(m)
        assert a.shape == (math.comb(m + 3, 4), 4)
        assert sorted(map(tuple, a.tolist())) == sorted(itertools.combinations_with_replacement(range(m), 4))
    assert tn.all_lineups(1).tolist() == [[0, 0, 0, 0]]
    assert math.comb(36, 4) <= 65536 < math.comb(37, 4)
    assert len(tn.all_lineups(36)) == 58905
    with pytest.raises(ValueError, match="65536"):
        tn.all_lineups(37)


def test_versus_anchors():
    a = tn.versus_anchors([5, 6], [0, 1, 2])
    assert a.tolist() == [[5, 0, 0, 0], [5, 1, 1, 1], [5, 2, 2, 2], [5, 0, 1, 2], [6, 0, 0, 0], [6, 1, 1, 1], [6, 2, 2, 2], [6, 0, 1, 2]]
    assert tn.versus_anchors([3], [0, 1]).tolist() == [[3, 0, 0, 0], [3, 1, 1, 1]]
    assert tn.versus_anchors([4], [0, 1, 2, 3]).tolist()[-1] == [4, 0, 1, 2]
    with pytest.raises(ValueError, match="65536"):
        tn.versus_anchors(range(3, 3 + 16385), [0, 1, 2])
    assert len(tn.versus_anchors(range(3, 3 + 16384), [0, 1, 2])) == 65536
    with pytest.raises(ValueError):
        tn.check_lineups(np.zeros((65537, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        tn.check_lineups([[0, 1, 2]])
    with pytest.raises(ValueError):
        tn.check_lineups([[0, 1, 2, 4]], 4)


# ---------------------------------------------------------------- the seat rule
@pytest.mark.parametrize("L", [1, 5, 7, 24, 64])
@pytest.mark.parametrize("s0", [0, 12345, (1 << 40) + 17])
def test_seat_rule_balance(L, s0):
    """over 24 L consecutive s every (lineup, permutation) exactly once; the package's restatement agrees with the reference's"""
    seen = {}
    for s in range(s0, s0 + 24 * L):
        # (E = 1: s is the game id itself)
        lineup, perm = tr.seat(s, 0, 1, L)
        assert sorted(perm) == [0, 1, 2, 3]
        assert (lineup, perm) == tn.seating(s, L)
        seen[(lineup, perm)] = seen.get((lineup, perm), 0) + 1
    assert len(seen) == 24 * L and set(seen.values()) == {1}


def test_seat_rule_indices_and_order():
    assert [tr.permutation(i) for i in range(24)] == list(itertools.permutations(range(4)))
    assert tr.episode_index(7, 3, 5) == 38 and tr.episode_index(7, 3, 0) == 7 + (3 << 32)
    assert tn.episode_index(7, 3, 5) == 38 and tn.episode_index(7, 3, 0) == 7 + (3 << 32)
    assert tr.seat(9, 2, 2, 5) is None and tr.seat(9, 1, 2, 5) is not None
    # n games x E episodes are the contiguous s range [id0 E, (id0 + n) E): the a-priori counts per lineup
    assert tn.expected_games(16, 2, 5).tolist() == [7, 7, 6, 6, 6]
    assert tn.expected_games(3, 2, 4, env_id0=10).tolist() == [np.sum(np.arange(20, 26) % 4 == l) for l in range(4)]


# ---------------------------------------------------------------- run_tournament on the twin
N, SEED, ID0, E = 3, 11, 40, 2
LINEUPS = np.array([[0, 1, 2, 2], [1, 1, 0, 2], [2, 0, 0, 1], [0, 1, 2, 0], [2, 2, 2, 2]], dtype=np.int64)


class WatchedTwin(tr.TourneyTwin):
    """the twin, with the episode number of every game kept from what the caller can see: the done flags step returns and the masks it
    hands to reset"""

    def __init__(self, *a, **kw):
        tr.TourneyTwin.__init__(self, *a, **kw)
        self.k = np.full(self.n, -1, dtype=np.int64)
        self.resets = []

    def reset(self, mask=None):
        sel = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.k += sel
        if mask is not None:
            self.resets.append(sel.copy())
        tr.TourneyTwin.reset(self, mask)

    def step(self, actions):
        reward, done = tr.TourneyTwin.step(self, actions)
        self.k += done.numpy().astype(np.int64)
        return reward, done


class CheckedRandom(RandomPolicy):
    """scripted.RandomPolicy that asserts, for every row it is handed, that its game's deciding seat carries this player's id - by the
    reference's seat rule and the episode numbers WatchedTwin observed"""

    def __init__(self, me, lineups, episodes):
        RandomPolicy.__init__(self)
        self.me, self.lineups, self.episodes, self.rows = me, lineups, episodes, 0

    def act(self, f, lists, lens, masks, games=None, **kw):
        env = self.env
        deciding = env.deciding_player().numpy()
        assert games is not None and len(games) == f.shape[0]
        for g in games.tolist():
            s = tr.seat(env.env_id0 + g, int(env.k[g]), self.episodes, len(self.lineups))
            assert s is not None, f"game {g} is retired (episode {env.k[g]}) and was handed to player {self.me}"
            lineup, pos = s
            assert self.lineups[lineup][pos[deciding[g] - 1]] == self.me, (g, int(env.k[g]), lineup, pos, int(deciding[g]), self.me)
        self.rows += len(games)
        return RandomPolicy.act(self, f, lists, lens, masks, games=games, **kw)


@pytest.fixture(scope="module")
def twin_run(oracle):
    env = WatchedTwin(N, SEED, ID0)
    players = [CheckedRandom(i, LINEUPS, E) for i in range(3)]
    res = tn.run_tournament(env, players, LINEUPS, E, max_steps=100000)
    return env, players, res


def test_run_tournament_hands_every_player_its_own_rows(twin_run):
    env, players, res = twin_run
    assert all(p.rows > 0 for p in players)
    assert sum(p.rows for p in players) <= res["passes"] * N


def test_run_tournament_table_is_the_twins(twin_run):
    env, players, res = twin_run
    want = np.array(env.table, dtype=np.int64)
    assert res["table"].shape == (len(LINEUPS) + 1, spec.TOURNAMENT_WORDS) and res["table"].dtype == torch.int64
    assert np.array_equal(res["table"].numpy(), want)
    assert env.lineups is None                          # the runner disabled the tournament behind its last read


def test_retirement_after_exactly_e_episodes(twin_run):
    env, players, res = twin_run
    t = res["table"].numpy()
    tot = dict(zip(spec.TOURNAMENT_TOTALS, t[-1].tolist()))
    assert int(t[:-1, tr.GAMES].sum()) == N * E == tot["seen"] == tot["seated"]
    assert tot["retired"] == N and tot["skipped_unseated"] == 0 and tot["draws"] == 0 and tot["tallied"] == N * E
    assert t[:-1, tr.GAMES].tolist() == tn.expected_games(N, E, len(LINEUPS), ID0).tolist()
    assert (env.k == E).all() and not env.resets          # every game ended by itself, twice
    assert (t[:-1, tr.WINS:tr.WINS + 4].sum(1) == t[:-1, tr.GAMES]).all() and (t[:-1, tr.WINS_BY_TURN:tr.WINS_BY_TURN + 4].sum(1) == t[:-1, tr.GAMES]).all()
    # the summary: every decided game has four seats, one of them the winner's
    assert sum(p["wins"] for p in res["players"]) == N * E
    for p in res["players"]:
        mult = (LINEUPS == p["player"]).sum(1)
        games = int(t[:-1, tr.GAMES][mult > 0].sum())
        assert p["games"] == games and p["fair_share"] == pytest.approx(float((t[:-1, tr.GAMES] * mult).sum()) / 4 / games)


def test_a_capped_game_is_booked_as_a_draw(oracle):
    """max_steps 40: no uniform-random game ends that early, so every game is reset at the loop's first look behind the cap (pass 64)
    and again 64 passes later - two draws per game, and the game retires"""
    env = WatchedTwin(N, SEED, ID0)
    res = tn.run_tournament(env, [CheckedRandom(i, LINEUPS, E) for i in range(3)], LINEUPS, E, max_steps=40)
    t = res["table"].numpy()
    tot = dict(zip(spec.TOURNAMENT_TOTALS, t[-1].tolist()))
    assert res["passes"] == 4 * tn.CHECK_EVERY
    assert [int(r.sum()) for r in env.resets] == [N, 0, N]         # (behind the cap every look resets the games past it: none at pass 96)
    assert tot == {"seen": N * E, "tallied": 0, "draws": N * E, "skipped_unseated": 0, "seated": N * E, "retired": N}
    assert t[:-1, tr.DRAWS].tolist() == t[:-1, tr.GAMES].tolist() == tn.expected_games(N, E, len(LINEUPS), ID0).tolist()
    assert int(t[:-1, tr.WINS:].sum()) == 0
    assert all(p["games"] == 0 and math.isnan(p["share"]) for p in res["players"])


def test_run_tournament_refuses_an_endless_one(oracle):
    with pytest.raises(ValueError, match="episodes_per_game"):
        tn.run_tournament(tr.TourneyTwin(2, 1), [RandomPolicy()], [[0, 0, 0, 0]], 0)


def test_tally_of_episode_records():
    """the reference's own pieces against each other: table_of_episodes over hand-made records"""
    ep = np.zeros((3, 26), dtype=np.int64)
    for i, (g, d, w, turn) in enumerate([(0, 10, 2, 30), (1, 12, 4, 40), (0, 25, 1, 50)]):
        ep[i, :4] = [g, d, w, turn]
        ep[i, 6:10] = [3, 10, 4, 5] if w == 2 else [10, 2, 2, 2] if w == 1 else [1, 2, 3, 10]
        ep[i, 10:14] = [4, 2, 1, 3]
    t = tr.table_of_episodes(ep, 20, 2, 3, 1)           # E = 1: game 0's second episode (decision 25) lies behind the counter anyway
    assert t[3].tolist()[:6] == [2, 2, 0, 0, 2, 2]
    t = tr.table_of_episodes(ep, 30, 2, 3, 1)
    assert t[3].tolist()[:6] == [3, 2, 0, 1, 2, 2]      # ... and within it is a finished game without a seating
    lineup, pos = tr.seat(0, 0, 1, 3)
    assert t[lineup][tr.GAMES] == 1 and t[lineup][tr.WINS + pos[1]] == 1 and t[lineup][tr.WINS_BY_TURN + 1] == 1 and t[lineup][tr.TURNS] == 30
    assert [t[lineup][tr.VP + pos[p]] for p in range(4)] == [3, 10, 4, 5]


def test_train_loop_eval_ladder_is_opt_in():
    import types
    from settlers_of_catan_rl_amd import train_loop as tl
    assert tl.TrainArgs().eval_ladder is False and tl.eval_ladder(tl.TrainArgs()) is None and tl.eval_ladder(types.SimpleNamespace()) is None
    assert callable(tl.eval_ladder(tl.TrainArgs(eval_ladder=True, eval_ladder_episodes=1)))
    assert tn.versus_anchors([3], [0, 1, 2]).tolist() == [[3, 0, 0, 0], [3, 1, 1, 1], [3, 2, 2, 2], [3, 0, 1, 2]]      # the ladder's lineups


# ---------------------------------------------------------------- ratings
def _expected_table(lineups, strength, games_per_lineup):
    t = np.zeros((len(lineups) + 1, spec.TOURNAMENT_WORDS), dtype=np.float64)
    for l, row in enumerate(lineups):
        s = strength[row]
        t[l, spec.TOURNAMENT_GAMES] = games_per_lineup
        t[l, spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4] = games_per_lineup * s / s.sum()
    return t


def _log_likelihood(theta_free, free, m, anchor, lineups, wins, prior):
    """the test's own: sum_l sum_j w_lj (theta_lj - log sum_m exp theta_lm) plus prior / 2 wins for each side of (i, anchor)"""
    theta = np.zeros(m)
    theta[free] = theta_free
    ll = 0.0
    for row, w in zip(lineups, wins):
        ll += float(np.dot(w, theta[row])) - float(w.sum()) * math.log(float(np.exp(theta[row]).sum()))
    for i in free:
        ll += prior / 2.0 * (theta[i] + theta[anchor]) - prior * math.log(math.exp(theta[i]) + math.exp(theta[anchor]))
    return ll


STRENGTH = np.exp(np.array([0.0, 0.7, -1.1, 0.25, 1.6]))


def test_fit_recovers_known_strengths_from_expected_counts():
    """expected counts, not samples: the maximum likelihood of exact proportions is the generating strengths.  1e-9: the iteration stops
    at steps below 1e-12 and converges linearly, which leaves the distance to the fixed point a few orders above the last step"""
    lineups = tn.all_lineups(5)
    fit = tn.fit_ratings(_expected_table(lineups, STRENGTH, 1000.0), lineups, 5, anchor=0, prior_games=0)
    assert fit["converged"] and fit["iterations"] < tn.MM_MAX_ITERATIONS
    err = np.abs(fit["log_strength"] - np.log(STRENGTH))
    print("iterations", fit["iterations"], "max |error| of the log-strengths", err.max())
    assert err.max() < 1e-9
    assert np.allclose(fit["rating"], 400.0 * np.log10(STRENGTH), atol=1e-6) and fit["stderr"][0] == 0.0


def _sampled_table(lineups, seed, games):
    rs = np.random.RandomState(seed)
    t = np.zeros((len(lineups) + 1, spec.TOURNAMENT_WORDS), dtype=np.int64)
    for l, row in enumerate(lineups):
        s = STRENGTH[row]
        w = rs.multinomial(games, s / s.sum())
        t[l, spec.TOURNAMENT_GAMES], t[l, spec.TOURNAMENT_DRAWS] = games + 3, 3           # draws carry no information
        t[l, spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4] = w
    return t


@pytest.mark.parametrize("prior", [0.0, 1.0])
def test_standard_errors_against_a_finite_difference_hessian(prior):
    lineups = np.concatenate([tn.all_lineups(5), tn.versus_anchors([4], [0, 1, 2])])      # repeated players in a lineup too
    t = _sampled_table(lineups, 5, 40)
    anchor, m = 2, 5
    fit = tn.fit_ratings(t, lineups, m, anchor=anchor, prior_games=prior)
    assert fit["converged"]
    free = [i for i in range(m) if i != anchor]
    wins = t[:len(lineups), spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4].astype(np.float64)
    x0 = fit["log_strength"][free]
    f = lambda x: _log_likelihood(x, free, m, anchor, lineups, wins, prior)
    h, k = 1e-3, len(free)
    # the gradient vanishes at the estimate (central differences, h^2 truncation)
    grad = [(f(x0 + h * np.eye(k)[i]) - f(x0 - h * np.eye(k)[i])) / (2 * h) for i in range(k)]
    assert np.abs(grad).max() < 1e-4
    hess = np.zeros((k, k))
    for i in range(k):
        for j in range(k):
            ei, ej = h * np.eye(k)[i], h * np.eye(k)[j]
            hess[i, j] = (f(x0 + ei + ej) - f(x0 + ei - ej) - f(x0 - ei + ej) + f(x0 - ei - ej)) / (4 * h * h)
    want = np.sqrt(np.diag(np.linalg.inv(-hess))) * 400.0 / math.log(10.0)
    rel = np.abs(fit["stderr"][free] / want - 1.0)
    print("prior", prior, "stderr", fit["stderr"], "finite differences", want, "max relative difference", rel.max())
    assert rel.max() < 1e-5 and fit["stderr"][anchor] == 0.0


def test_rating_differences_do_not_depend_on_the_anchor():
    lineups = tn.all_lineups(5)
    t = _sampled_table(lineups, 9, 25)
    fits = [tn.fit_ratings(t, lineups, 5, anchor=a, prior_games=0) for a in range(5)]
    for fit in fits:
        assert fit["converged"] and fit["rating"][fit["anchor"]] == 0.0
        d = (fit["rating"][:, None] - fit["rating"][None, :]) - (fits[0]["rating"][:, None] - fits[0]["rating"][None, :])
        assert np.abs(d).max() < 1e-7, np.abs(d).max()


def test_a_winless_player_stays_finite_with_the_default_prior():
    lineups = tn.all_lineups(4)
    t = np.zeros((2, spec.TOURNAMENT_WORDS), dtype=np.int64)
    t[0, spec.TOURNAMENT_GAMES] = 60
    t[0, spec.TOURNAMENT_WINS:spec.TOURNAMENT_WINS + 4] = [30, 20, 10, 0]
    fit = tn.fit_ratings(t, lineups, 4)
    assert fit["converged"] and np.isfinite(fit["rating"]).all() and np.isfinite(fit["stderr"]).all()
    assert fit["rating"][3] < fit["rating"][2] < fit["rating"][1] < fit["rating"][0] == 0.0
    plain = tn.fit_ratings(t, lineups, 4, prior_games=0)
    assert plain["rating"][3] == -np.inf and np.isfinite(plain["rating"][:3]).all()
    text = tn.report(tn.summarise(t, lineups, 4), names=["a", "b", "c", "d"], ratings=fit)
    assert "rating" in text and len(text.splitlines()) == 6
