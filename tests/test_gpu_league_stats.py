"""League results counted on the device (catan_league_stats_*, csrc/catan_league_stats.hip) against a plain-Python tally.

Expected tables never come from the library's statistics code: tests/league_stats_oracle.py tallies the episode records of
episode_stats_oracle.replay (the oracle replay of 96 games x 4 000 decisions that tests/test_gpu_episode_stats.py shares) or the
states export_state returns.  The maps come from fixed RandomStates: random seat permutations, some -1 seats, one game whose slot row
is no permutation.  All comparisons are integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_oracle as eso
import league_stats_oracle as lso
from settlers_of_catan_rl_amd import _lib, spec

pytestmark = pytest.mark.gpu

N, SEED, STEPS = 96, 7, 4000
NETS = 5
BAD_GAME = 17
SLOT, NET = lso.maps(N, NETS, 21, bad_game=BAD_GAME)
# the focus player of the finished-game statistics: the central seat (none in the game without one)
CENTRAL = np.where(np.arange(N) == BAD_GAME, 0, np.argmax(SLOT == 0, axis=1) + 1).astype(np.int32)
LDS_MAX = spec.LEAGUE_STATS_LDS_MAX_NETS


def _env(n, seed, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=seed, **kw)


def _assert_table(got, want, what):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in zip(*np.nonzero(got != want))]
    assert not bad, f"{what}: (row, column, device, expected) {bad[:12]}"


@pytest.fixture(scope="module")
def episodes(oracle):
    return eso.replay(N, SEED, STEPS)[0]


@pytest.fixture(scope="module")
def lockstep(hip_lib):
    """96 games, 4 000 lock-step steps of the library's random policy with BOTH statistics on"""
    env = _env(N, SEED)
    env.enable_episode_stats(CENTRAL)
    env.enable_league_stats(SLOT, NET, NETS)
    env.random_rollout(0, STEPS)
    return dict(table=env.league_stats().numpy(), episode=env.episode_stats_words(), missed=env.missed_speculation_count())


def test_lockstep_table_equals_the_tally(episodes, lockstep):
    want = lso.table(episodes, STEPS, SLOT, NET, NETS)
    tot = want[NETS]
    print("seen", lockstep["table"][NETS][0], "expected", tot[0], "tallied", tot[1], "skipped games", tot[4])
    assert tot[lso.T_SEEN] >= 150 and tot[lso.T_SKIPPED_GAMES] > 0 and (want[:NETS, lso.NET_WINS] > 0).all()
    _assert_table(lockstep["table"], want, "lock-step")
    assert lockstep["missed"] == 0


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("window", [1, 8])
def test_deferred_table_equals_the_tally(episodes, hip_lib, fused, window):
    env = _env(N, SEED)
    env.set_deferred_fused(fused)
    env.enable_league_stats(SLOT, NET, NETS)
    env.random_rollout_deferred(2600, window)
    got = env.league_stats().numpy()
    cnt = env.policy_counters().cpu().numpy()
    assert cnt.max() <= STEPS and env.invalid_action_count() == 0
    want = lso.table(episodes, cnt, SLOT, NET, NETS)
    print("fused", fused, "window", window, "seen", got[NETS][0], "expected", want[NETS][0])
    assert want[NETS][lso.T_SEEN] >= 50
    _assert_table(got, want, f"deferred rollout fused={fused} window={window}")


def test_both_statistics_at_once(episodes, lockstep):
    """each equals its own oracle, and with the central seat as the focus player the two agree where they count the same thing"""
    want_ep = eso.counters(episodes, STEPS, CENTRAL)
    assert list(lockstep["episode"]) == want_ep
    _assert_table(lockstep["table"], lso.table(episodes, STEPS, SLOT, NET, NETS), "lock-step, both on")
    e, tot = eso.named(lockstep["episode"]), lockstep["table"][NETS]
    assert e["episodes"] == tot[lso.T_SEEN] and e["focus_wins"] == tot[lso.T_CENTRAL_WINS] and e["focus_vp_sum"] == tot[lso.T_CENTRAL_VP]
    assert e["focus_episodes"] == tot[lso.T_TALLIED] < tot[lso.T_SEEN]


@pytest.fixture(scope="module")
def finished_handle(hip_lib):
    """96 games without auto-reset played by the library's random sampler, finished games idling with type -1 as the evaluation loop
    idles them -> (env, winner [n], vp [n][4]) from export_state"""
    env = _env(N, 31, auto_reset=False)
    over = torch.zeros(N, dtype=torch.bool, device="cuda")
    idle = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    for t in range(2600):
        a = env.sample_random_actions(t)
        a[:, 0] = torch.where(over, idle, a[:, 0])
        _, done = env.step(a)
        over |= done.bool()
    blobs = env.export_state().cpu().numpy()
    winner = spec.state_field(blobs, "winner")[:, 0].astype(np.int64)
    vp = np.stack([spec.state_field(blobs, f"p{p}_vp")[:, 0] for p in (1, 2, 3, 4)], axis=1).astype(np.int64)
    assert int((winner > 0).sum()) >= 20 and int((winner > 0).sum()) == int(over.sum()) and env.invalid_action_count() == 0
    return env, winner, vp


def _size_maps(num_nets, finished_game):
    slot, net = lso.maps(N, num_nets, 100 + num_nets % 97, minus_one_every=11, bad_game=5)
    if num_nets == spec.LEAGUE_STATS_MAX_NETS:           # sparse indices over the whole range, its last row included
        pool = np.array([0, 1, 40000, 65534, 65535], dtype=np.int32)
        net = np.where(net >= 0, pool[net % len(pool)], net).astype(np.int32)
    net[finished_game] = [num_nets, -2, 0]               # out of range on either side, in a game that is tallied
    return slot, net


@pytest.mark.parametrize("num_nets", [1, 3, LDS_MAX, LDS_MAX + 1, spec.LEAGUE_STATS_MAX_NETS])
def test_table_sizes_and_list_lengths(finished_handle, num_nets):
    """catan_league_stats_count, the kernel's direct entry: the LDS table up to its threshold, global atomics beyond; lists that fill
    less than a wave, exactly one, one and a lane, and the whole handle; an explicit list with a repeated game"""
    env, winner, vp = finished_handle
    first = int([g for g in np.nonzero(winner > 0)[0] if g != 5][0])
    slot, net = _size_maps(num_nets, first)
    lists = [(m, None) for m in (1, 63, 64, 65, 96)]
    lists.append((65, np.random.RandomState(3).permutation(N)[:65]))
    rep = np.array([first] * 2 + [0, 95, 40], dtype=np.int64)
    lists.append((len(rep), rep))
    for m, games in lists:
        env.enable_league_stats(slot, net, num_nets, count_only=True)
        env.league_stats_count(None if games is None else torch.from_numpy(games), count=m)
        got = env.league_stats().numpy()
        want = lso.table_of_states(winner, vp, range(m) if games is None else games, slot, net, num_nets)
        assert got.shape == (num_nets + 1, 6)
        _assert_table(got, want, f"num_nets={num_nets} m={m} explicit={games is not None}")
    tot = want[num_nets]
    assert tot[lso.T_SEEN] == len(rep) and want[0, lso.SEATS] >= 2 and tot[lso.T_SKIPPED_SEATS] >= 4     # the repeated game counted twice
    # the whole handle once more, on top of the list above: the table accumulates
    env.league_stats_count()
    both = want + lso.table_of_states(winner, vp, range(N), slot, net, num_nets)
    assert both[num_nets][lso.T_SKIPPED_SEATS] >= 2 and both[num_nets][lso.T_SKIPPED_GAMES] > 0
    _assert_table(env.league_stats().numpy(), both, f"num_nets={num_nets}: two counts")
    env.enable_league_stats(None, None, 0, on=False)


def test_reenable_and_read(hip_lib):
    env = _env(64, 9)
    slot, net = lso.maps(64, 4, 5)
    env.enable_league_stats(slot, net, 4)
    assert int(env.league_stats().abs().sum()) == 0
    env.random_rollout(0, 2500)
    a = env.league_stats()
    assert a.shape == (5, 6) and a.dtype == torch.int64 and int(a[4, 0]) > 0
    assert torch.equal(env.league_stats(reset=True), a)          # read(reset = 1) returns the table, then zeroes it
    assert int(env.league_stats().abs().sum()) == 0
    env.random_rollout(2500, 1500)
    assert int(env.league_stats()[4, 0]) > 0
    slot2, net2 = lso.maps(64, 300, 6)
    env.enable_league_stats(slot2, net2, 300)                    # other maps, a larger table: zeroed
    b = env.league_stats()
    assert b.shape == (301, 6) and int(b.abs().sum()) == 0
    env.random_rollout(4000, 1500)
    b = env.league_stats()
    assert int(b[300, 0]) > 0 and 0 < int(b[:300, 1].sum()) <= 3 * int(b[300, 1]) and int(b[300, 5]) == 0
    env.enable_league_stats(slot, net, 4)                        # ... and back to a smaller one
    assert env.league_stats().shape == (5, 6) and int(env.league_stats().abs().sum()) == 0
    env.enable_league_stats(None, None, 0, on=False)
    with pytest.raises(_lib.CatanHipError):
        env.league_stats()


def test_error_returns(hip_lib):
    L = hip_lib
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = (C.c_uint64 * (6 * 6))()
    assert L.catan_league_stats_words() == spec.LEAGUE_STATS_WORDS == 6
    slot, net = (torch.from_numpy(x).cuda() for x in lso.maps(64, 5, 1))
    sp, npn = C.c_void_p(slot.data_ptr()), C.c_void_p(net.data_ptr())
    err = lambda: L.catan_last_error()
    # a null handle
    assert L.catan_league_stats_enable(None, 1, sp, npn, 5, st) == -1 and b"null handle" in err()
    assert L.catan_league_stats_read(None, out, 0, st) == -1 and b"null argument" in err()
    assert L.catan_league_stats_count(None, None, 1, st) == -1 and b"null handle" in err()
    # auto_reset = 0: nothing is re-dealt; the count-only mode is the one such a handle takes
    e0 = _env(64, 1, auto_reset=False)
    assert L.catan_league_stats_enable(e0.h, spec.LEAGUE_STATS_REDEALS, sp, npn, 5, st) == -1 and b"auto_reset" in err()
    assert L.catan_league_stats_count(e0.h, None, 64, st) == -1 and b"not enabled" in err()
    assert L.catan_league_stats_enable(e0.h, spec.LEAGUE_STATS_COUNT_ONLY, sp, npn, 5, st) == 0
    assert L.catan_league_stats_count(e0.h, None, 0, st) == -1 and b"m must be" in err()
    assert L.catan_league_stats_count(e0.h, None, 65, st) == -1 and b"exceeds" in err()
    assert L.catan_league_stats_count(e0.h, None, 64, st) == 0 and L.catan_league_stats_read(e0.h, out, 0, st) == 0
    assert list(out)[30:] == [64, 0, 0, 0, 64, 0]                # fresh games: seen and skipped, no winner yet
    # a handle under the MT19937 contract
    em = _env(1, 1)
    em.seed_mt19937(3, 4)
    assert L.catan_league_stats_enable(em.h, 1, sp, npn, 5, st) == -1 and b"MT19937" in err()
    env = _env(64, 9)
    # off: reading is refused, not answered with zeros
    assert L.catan_league_stats_read(env.h, out, 0, st) == -1 and b"not enabled" in err()
    assert L.catan_league_stats_read(env.h, None, 0, st) == -1 and b"null argument" in err()
    # num_nets and the maps
    for bad in (0, -3, 65537):
        assert L.catan_league_stats_enable(env.h, 1, sp, npn, bad, st) == -1 and b"num_nets" in err()
    assert L.catan_league_stats_enable(env.h, 1, None, npn, 5, st) == -1 and b"null map" in err()
    assert L.catan_league_stats_enable(env.h, 1, sp, None, 5, st) == -1 and b"null map" in err()
    assert L.catan_league_stats_enable(env.h, 4, sp, npn, 5, st) == -1 and b"mode bits" in err()
    assert L.catan_league_stats_read(env.h, out, 0, st) == -1 and b"not enabled" in err()       # none of them switched it on
    # an open deferred sequence
    env.step_deferred(env.sample_random_actions(0), 4)
    assert L.catan_league_stats_enable(env.h, 1, sp, npn, 5, st) == -1 and b"catan_step_flush" in err()
    env.step_flush()
    assert L.catan_league_stats_enable(env.h, 1, sp, npn, 5, st) == 0
    env.step_deferred(env.sample_random_actions(1), 4)
    assert L.catan_league_stats_read(env.h, out, 0, st) == -1 and b"catan_step_flush" in err()
    assert L.catan_league_stats_count(env.h, None, 64, st) == -1 and b"catan_step_flush" in err()
    env.step_flush()
    assert L.catan_league_stats_read(env.h, out, 0, st) == 0 and list(out) == [0] * 36
    assert L.catan_league_stats_enable(env.h, 0, None, None, 0, st) == 0                         # off takes no maps
    # the python layer checks the shapes before the library sees a pointer
    with pytest.raises(ValueError):
        env.enable_league_stats(slot[:, :3], net, 5)
    with pytest.raises(ValueError):
        env.enable_league_stats(slot, net[:32], 5)


@pytest.mark.parametrize("fused", [True, False])
def test_collector_leaves_the_table_of_every_gather(hip_lib, fused):
    """RolloutCollector(league_stats=True, episode_stats=True) with the rule-based player and a small net as opponents, in the device
    loop and in the tensor-operation loop: the totals agree with the finished-game statistics (the active seat is both the focus
    player and the central seat), and every tallied game adds three seats."""
    import rollout_fixture as rf
    from test_gpu_collector import SamplerPolicy
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    n, T, seed = 96, 16, 5
    env = _env(n, seed)
    env.random_rollout(0, 1700)                  # (late enough for games to end inside a short rollout)
    cenv = rf.CountingEnv(env)
    torch.manual_seed(3)
    nets = [ScriptedPolicy(env), CatanPolicy().cuda().eval()]
    col = RolloutCollector(cenv, SamplerPolicy(cenv), T, seed=seed, episode_stats=True, league_stats=True)
    col.fused_bookkeeping = fused
    assert col.gather_rollouts().league_stats is None                     # no opponents installed: no table
    col.after_rollouts()
    opp_index = torch.from_numpy(np.random.RandomState(8).randint(0, 2, size=(n, 3)))
    col.set_opponents(nets, opp_index)
    seen = 0
    for g in range(3):
        st = col.gather_rollouts()
        t, e = st.league_stats, st.episode_stats
        assert t.shape == (3, 6)
        tot = t[2].tolist()
        print("fused", fused, "gather", g, "totals", tot, "episodes", e["episodes"], "seats", t[:2, 1].tolist())
        assert tot[0] == e["episodes"] == tot[1] and tot[2] == e["focus_wins"] and tot[3] == e["focus_vp_sum"] and tot[4] == tot[5] == 0
        assert int(t[:2, 1].sum()) == 3 * tot[1]
        assert int(t[:2, 2].sum()) + tot[2] == tot[1]                     # every tallied game has one winner: an opponent seat or the central one
        seen += tot[0]
        col.after_rollouts()
    assert seen > 0 and env.invalid_action_count() == 0
    col.set_opponents(nets[:1], torch.zeros((n, 3), dtype=torch.int64))   # a re-enable between rollouts: a table of one net
    assert col.gather_rollouts().league_stats.shape == (2, 6)
