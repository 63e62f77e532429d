"""The tournament's hooks on the device (catan_tourney_*, csrc/catan_hooks.hip) against the plain-Python seat rule and
tally of tests/tournament_reference.py.

Expected tables never come from the library: they are tallied from the episode records of episode_stats_oracle.replay (the oracle
replay of 96 games x 4 000 decisions that tests/test_gpu_episode_stats.py and tests/test_gpu_league_stats.py share).  The replay
starts at the handle's first deal, so a handle is enabled, reset (which seats every game and deals it again) and then given its first
deal back by import_state: the seating stays, the games are the replay's.  All comparisons are integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_oracle as eso
import guarded
import league_stats_oracle as lso
import tournament_reference as tr
from settlers_of_catan_rl_amd import _lib, spec
from settlers_of_catan_rl_amd import tournament as tn

pytestmark = pytest.mark.gpu

N, SEED, STEPS = 96, 7, 4000
PLAYERS = 7
LDS_MAX = spec.TOURNAMENT_LDS_MAX_LINEUPS
TOTALS = spec.TOURNAMENT_TOTALS


def _env(n, seed, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=seed, **kw)


def _lineups(L):
    return np.random.RandomState(L % 9973).randint(0, PLAYERS, size=(L, 4)).astype(np.int32)


def _seated(L, E, n=N, seed=SEED):
    """-> a fresh handle with the tournament on, every game seated for its episode 0 and back at its first deal"""
    env = _env(n, seed)
    first = env.export_state()
    env.enable_tournament(_lineups(L), PLAYERS, E)
    assert int(env.tournament_table().abs().sum()) == 0 and int((env.tournament_seating()[0] != -1).sum()) == 0
    env.reset()
    env.import_state(first)
    return env


def _assert_table(got, want, what):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in zip(*np.nonzero(got != want))]
    assert not bad, f"{what}: (row, column, device, expected) {bad[:12]}"


def _assert_seating(env, finished, L, E, what):
    """the arrays the runner reads: game g is in its episode finished[g], or retired"""
    lineup_of, pos_of_pid = (x.cpu().numpy() for x in env.tournament_seating())
    for g in range(env.n):
        s = tr.seat(env.env_id0 + g, int(finished[g]), E, L)
        want = (-1, (-1, -1, -1, -1)) if s is None else s
        assert (int(lineup_of[g]), tuple(int(x) for x in pos_of_pid[g])) == want, (what, g, int(finished[g]))


def _finished(ep, counts, n=N):
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (n,))
    ep = ep[ep[:, eso.DECISION] <= counts[ep[:, eso.GAME]]]
    return np.bincount(ep[:, eso.GAME], minlength=n)


@pytest.fixture(scope="module")
def episodes(oracle):
    return eso.replay(N, SEED, STEPS)[0]


@pytest.mark.parametrize("E", [0, 2])
@pytest.mark.parametrize("L", [1, 5, LDS_MAX, LDS_MAX + 1, spec.TOURNAMENT_MAX_LINEUPS])
def test_lockstep_table_equals_the_tally(episodes, hip_lib, L, E):
    env = _seated(L, E)
    _assert_seating(env, np.zeros(N, dtype=np.int64), L, E, "behind the first reset")
    env.random_rollout(0, STEPS)
    got = env.tournament_table().numpy()
    want = tr.table_of_episodes(episodes, STEPS, N, L, E)
    tot = dict(zip(TOTALS, want[L].tolist()))
    print("L", L, "E", E, "totals", tot)
    assert tot["seen"] >= 150 and tot["draws"] == 0
    assert (tot["skipped_unseated"] > 0 and tot["retired"] > 0) if E else (tot["skipped_unseated"] == 0 == tot["retired"] and tot["tallied"] == tot["seen"])
    _assert_table(got, want, f"lock-step L={L} E={E}")
    _assert_seating(env, _finished(episodes, STEPS), L, E, "behind the rollout")
    assert env.missed_speculation_count() == 0 and env.invalid_action_count() == 0


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("window", [1, 8])
def test_deferred_table_equals_the_tally(episodes, hip_lib, fused, window):
    L, E = 5, 0
    env = _seated(L, E)
    env.set_deferred_fused(fused)
    env.random_rollout_deferred(2600, window)
    got = env.tournament_table().numpy()
    cnt = env.policy_counters().cpu().numpy()
    assert cnt.max() <= STEPS and env.invalid_action_count() == 0
    want = tr.table_of_episodes(episodes, cnt, N, L, E)
    print("fused", fused, "window", window, "seen", got[L][0], "expected", want[L][0])
    assert want[L][tr.T_SEEN] >= 50
    _assert_table(got, want, f"deferred rollout fused={fused} window={window}")
    _assert_seating(env, _finished(episodes, cnt), L, E, "behind the deferred rollout")


def test_reset_mask_books_draws_and_reseats_the_selected_games(episodes, hip_lib):
    L, E = 5, 0
    env = _seated(L, E)
    env.random_rollout(0, STEPS)
    k = _finished(episodes, STEPS)
    before = env.tournament_table().numpy()
    mask = torch.from_numpy((np.arange(N) % 3 == 1))
    env.reset(mask)
    after = env.tournament_table().numpy()
    want = before.copy()
    for g in np.flatnonzero(mask.numpy()):
        lineup, _ = tr.seat(g, int(k[g]), E, L)
        want[lineup, tr.GAMES] += 1
        want[lineup, tr.DRAWS] += 1
    sel = int(mask.sum())
    want[L, tr.T_SEEN] += sel; want[L, tr.T_DRAWS] += sel; want[L, tr.T_SEATED] += sel
    _assert_table(after, want, "reset(mask)")
    _assert_seating(env, k + mask.numpy().astype(np.int64), L, E, "behind reset(mask)")


def test_with_episode_statistics_and_league_results_on(episodes, hip_lib):
    """each of the three equals its own oracle, and they agree on the number of finished games"""
    L, E, nets = 5, 0, 5
    slot, net = lso.maps(N, nets, 21, bad_game=17)
    env = _seated(L, E)
    env.enable_episode_stats()
    env.enable_league_stats(slot, net, nets)
    env.random_rollout(0, STEPS)
    tour, league, ep = env.tournament_table().numpy(), env.league_stats().numpy(), env.episode_stats_words()
    _assert_table(tour, tr.table_of_episodes(episodes, STEPS, N, L, E), "tournament, all three on")
    _assert_table(league, lso.table(episodes, STEPS, slot, net, nets), "league results, all three on")
    assert list(ep) == eso.counters(episodes, STEPS)
    assert tour[L][tr.T_SEEN] == league[nets][lso.T_SEEN] == eso.named(ep)["episodes"] > 0


def test_enable_refusals_and_their_messages(hip_lib):
    Lb = hip_lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lineups = np.ascontiguousarray(_lineups(5))
    lp = lineups.ctypes.data_as(C.c_void_p)
    out = (C.c_uint64 * (6 * 16))()
    a, b = C.c_void_p(), C.c_void_p()
    err = lambda: Lb.catan_last_error()
    assert Lb.catan_tourney_words() == spec.TOURNAMENT_WORDS == 16
    assert Lb.catan_tourney_enable(None, lp, 5, PLAYERS, 0, st) == -1 and b"null handle" in err()
    e0 = _env(64, 1, auto_reset=False)
    assert Lb.catan_tourney_enable(e0.h, lp, 5, PLAYERS, 0, st) == -1 and b"auto_reset" in err()
    em = _env(1, 1)
    em.seed_mt19937(3, 4)
    assert Lb.catan_tourney_enable(em.h, lp, 5, PLAYERS, 0, st) == -1 and b"MT19937" in err()
    env = _env(64, 9)
    for bad in (0, -1, 65537):
        assert Lb.catan_tourney_enable(env.h, lp, bad, PLAYERS, 0, st) == -1 and b"L must be" in err()
    assert Lb.catan_tourney_enable(env.h, None, 5, PLAYERS, 0, st) == -1 and b"null lineups" in err()
    assert Lb.catan_tourney_enable(env.h, lp, 5, int(lineups.max()), 0, st) == -1 and b"names player" in err()       # an id == M
    neg = lineups.copy(); neg[3, 2] = -1
    assert Lb.catan_tourney_enable(env.h, neg.ctypes.data_as(C.c_void_p), 5, PLAYERS, 0, st) == -1 and b"lineup 3 names player -1" in err()
    assert Lb.catan_tourney_enable(env.h, lp, 5, PLAYERS, -2, st) == -1 and b"E must be" in err()
    # none of them switched it on: reading is refused, not answered with zeros
    assert Lb.catan_tourney_read(env.h, out, 0, st) == -1 and b"no tournament" in err()
    assert Lb.catan_tourney_seating(env.h, C.byref(a), C.byref(b)) == -1 and b"no tournament" in err()
    assert Lb.catan_tourney_read(env.h, None, 0, st) == -1 and b"null argument" in err()
    # an open deferred sequence
    env.step_deferred(env.sample_random_actions(0), 4)
    assert Lb.catan_tourney_enable(env.h, lp, 5, PLAYERS, 0, st) == -1 and b"catan_step_flush" in err()
    env.step_flush()
    assert Lb.catan_tourney_enable(env.h, lp, 5, PLAYERS, 0, st) == 0
    env.step_deferred(env.sample_random_actions(1), 4)
    assert Lb.catan_tourney_read(env.h, out, 0, st) == -1 and b"catan_step_flush" in err()
    assert Lb.catan_tourney_disable(env.h, st) == -1 and b"catan_step_flush" in err()
    env.step_flush()
    assert Lb.catan_tourney_read(env.h, out, 0, st) == 0 and list(out) == [0] * 96
    assert Lb.catan_tourney_seating(env.h, C.byref(a), C.byref(b)) == 0 and a.value and b.value
    assert Lb.catan_tourney_disable(env.h, st) == 0 and Lb.catan_tourney_disable(env.h, st) == 0
    assert Lb.catan_tourney_read(env.h, out, 0, st) == -1 and b"no tournament" in err()
    # the python layer checks the shape before the library sees a pointer
    with pytest.raises(ValueError):
        env.enable_tournament(lineups[:, :3], PLAYERS)


def test_a_refused_enable_leaves_the_earlier_tournament_as_it_was(hip_lib):
    """a lineup that names player M is refused on the host, before anything of the tournament in force is touched: its table (made
    non-zero by a second reset, which books every seated game as a draw) and its seating read as before"""
    L = 5
    env = _env(64, 9)
    env.enable_tournament(_lineups(L), PLAYERS)
    env.reset()
    env.reset()
    before, seats = env.tournament_table().numpy(), [x.clone() for x in env.tournament_seating()]
    assert before[L][tr.T_DRAWS] == 64 and before[L][tr.T_SEATED] == 128
    bad = np.ascontiguousarray(_lineups(3))
    bad[2, 1] = PLAYERS
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.catan_tourney_enable(env.h, bad.ctypes.data_as(C.c_void_p), 3, PLAYERS, 0, st) == -1
    assert b"lineup 2 names player 7" in hip_lib.catan_last_error()
    _assert_table(env.tournament_table().numpy(), before, "behind the refused enable")
    assert all(torch.equal(a, b) for a, b in zip(env.tournament_seating(), seats))


RT_N, RT_SEED, RT_E, RT_CAP = 16, 3, 2, 1500
RT_LINEUPS = np.array([[0, 1, 2, 2], [0, 2, 2, 2], [1, 2, 2, 2], [0, 1, 1, 2], [0, 0, 1, 2]], dtype=np.int64)     # 0 builder, 1 trader, 2 random


def _run_tournament():
    from settlers_of_catan_rl_amd.scripted import RandomPolicy, ScriptedPolicy, TraderPolicy
    env = _env(RT_N, RT_SEED)
    return tn.run_tournament(env, [ScriptedPolicy(), TraderPolicy(), RandomPolicy()], RT_LINEUPS, RT_E, max_steps=RT_CAP)


@pytest.fixture(scope="module")
def tournament_runs(hip_lib):
    return _run_tournament(), _run_tournament()


def test_run_tournament_plays_the_a_priori_schedule(tournament_runs):
    res = tournament_runs[0]
    t = res["table"].numpy()
    tot = dict(zip(TOTALS, t[-1].tolist()))
    print(tn.report(res, names=["builder", "trader", "random"]), "\ntotals", tot, "passes", res["passes"])
    assert t[:-1, tr.GAMES].tolist() == tn.expected_games(RT_N, RT_E, len(RT_LINEUPS)).tolist()
    assert tot["seen"] == tot["seated"] == RT_N * RT_E and tot["retired"] == RT_N and tot["skipped_unseated"] == 0
    assert tot["tallied"] + tot["draws"] == RT_N * RT_E
    assert (t[:-1, tr.WINS:tr.WINS + 4].sum(1) == t[:-1, tr.GAMES] - t[:-1, tr.DRAWS]).all()


def test_two_tournaments_end_in_identical_tables(tournament_runs):
    a, b = tournament_runs
    assert torch.equal(a["table"], b["table"]) and a["passes"] == b["passes"]


def test_the_builder_wins_more_than_any_random_seat(tournament_runs):
    res = tournament_runs[0]
    t = res["table"].numpy()
    builder = res["players"][0]["wins"]
    random_seats = [int(t[l, tr.WINS + j]) for l in range(len(RT_LINEUPS)) for j in range(4) if RT_LINEUPS[l, j] == 2]
    print("builder", builder, "random seats", random_seats)
    assert all(builder > w for w in random_seats)


def test_eval_ladder_logs_rating_error_and_games(hip_lib):
    """train_loop.eval_ladder with the uniform-random sampler in the net's place: the three keys, a rating below the builder's 0"""
    import math
    from settlers_of_catan_rl_amd import train_loop as tl
    from settlers_of_catan_rl_amd.scripted import RandomPolicy
    ladder = tl.eval_ladder(tl.TrainArgs(eval_ladder=True, eval_ladder_episodes=1))
    out = ladder(RandomPolicy(), _env(16, 4), max_steps=600)
    print(out)
    assert sorted(out) == ["games", "rating", "stderr"] and 0 < out["games"] <= 16
    assert math.isfinite(out["rating"]) and out["rating"] < 0 and math.isfinite(out["stderr"]) and out["stderr"] > 0


def test_never_enabled_nothing_of_it_and_no_write_outside_its_arrays(hip_lib):
    """Two handles of one seed play the same 3 000 random-policy steps and then 100 caller-stepped ones, one with the tournament on.
    Off: no table, no seating.  On: the games, rewards and done flags are the other handle's bit for bit - the hooks write the three
    per-game arrays and the table and nothing of a game - and the margins around the caller's reward buffer come back untouched."""
    n, steps = 96, 3000
    off, on = _env(n, 5), _env(n, 5)
    with pytest.raises(_lib.CatanHipError, match="no tournament"):
        off.tournament_table()
    with pytest.raises(_lib.CatanHipError, match="no tournament"):
        off.tournament_seating()
    on.enable_tournament(_lineups(5), PLAYERS, 0)
    whole, view = guarded.sentinel_output(n * 4, torch.float32, tail=256, lead=256, sentinel=guarded.SENTINEL32)
    on.reward = view.view(n, 4)
    for env in (off, on):
        env.reset()
        env.random_rollout(0, steps)
    for t in range(100):
        acts = off.sample_random_actions(steps + t)
        assert torch.equal(acts, on.sample_random_actions(steps + t))
        r0, d0 = off.step(acts)
        r1, d1 = on.step(acts)
        assert torch.equal(r0, r1) and torch.equal(d0, d1)
    assert torch.equal(off.export_state(), on.export_state())
    assert guarded.intact(whole, view) and guarded.written(whole, view, guarded.SENTINEL32)
    tot = dict(zip(TOTALS, on.tournament_table()[-1].tolist()))
    assert tot["seen"] >= 100 and tot["seated"] == n + tot["seen"]
    with pytest.raises(_lib.CatanHipError, match="no tournament"):
        off.tournament_table()
