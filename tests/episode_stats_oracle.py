"""Expected finished-game statistics from the CPU oracle, without any of the library's statistics code: every game is replayed one
decision at a time (mask -> orc_sample_action with the game's own decision number -> orc_step), and whenever a step ends a game its
final state is exported and read through spec.STATE_FIELDS before the game is reset, as orc_batch_run_random resets it.  One replay
to `max_decisions` serves every schedule: an episode that ended with the game's d-th decision lies within a counter c iff d <= c
(lock-step: c = the number of steps; deferred: the game's policy counter)."""
import ctypes as C
import functools

import numpy as np

import oracle_lib
from settlers_of_catan_rl_amd import spec

# columns of an episode record
GAME, DECISION, WINNER, TURN, LR, LA, VP, ORDER, SLEFT, CLEFT, NPLAYED = 0, 1, 2, 3, 4, 5, 6, 10, 14, 18, 22
COLS = 26


@functools.lru_cache(maxsize=4)
def replay(n, seed, max_decisions, env_id0=0):
    """-> (episodes int64 [k][COLS], final blobs int32 [n][736]) of games env_id0 .. env_id0 + n - 1 after max_decisions decisions each.
    Cached and shared between tests: treat both arrays as read-only."""
    ob = oracle_lib.OracleBatch(n, seed, env_id0=env_id0)
    L = ob.L
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    m = np.zeros(oracle_lib.MASK_WORDS, dtype=np.float32)
    a = np.zeros(oracle_lib.ACTION_WORDS, dtype=np.int32)
    rew = np.zeros(4, dtype=np.float32)
    blob = np.zeros(oracle_lib.STATE_WORDS, dtype=np.int32)
    mp, ap, rp, bp = m.ctypes.data_as(f32p), a.ctypes.data_as(i32p), rew.ctypes.data_as(f32p), blob.ctypes.data_as(i32p)
    done = C.c_int(0)
    dref = C.byref(done)
    f = lambda name: spec.state_field(blob, name)
    rows = []
    for i in range(n):
        env = ob.env_ptr(i)
        for s in range(max_decisions):
            L.orc_masks(env, mp)
            L.orc_sample_action(env, seed, env_id0 + i, s, mp, ap)
            assert L.orc_step(env, ap, rp, dref) == 0
            if done.value:
                L.orc_export(env, bp)
                rows.append([i, s + 1, int(f("winner")[0]), int(f("turn")[0]), int(f("lr_player")[0]), int(f("la_player")[0])]
                            + [int(f(f"p{p}_vp")[0]) for p in (1, 2, 3, 4)] + [int(x) for x in f("player_order")]
                            + [int(x) for x in f("settlements_left")] + [int(x) for x in f("cities_left")]
                            + [int(f(f"p{p}_n_played")[0]) for p in (1, 2, 3, 4)])
                L.orc_game_reset(env)
    ep = np.array(rows, dtype=np.int64).reshape(-1, COLS)
    ep.setflags(write=False)
    blobs = ob.export()
    blobs.setflags(write=False)
    return ep, blobs


def counters(ep, counts, focus=None):
    """The counter block (spec.EPISODE_STATS_FIELDS order, list of ints) of the episodes of `ep` that lie within counts[game];
    focus: PlayerId per game (0: none) or None."""
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (int(ep[:, GAME].max()) + 1 if len(ep) else 1,)) if np.ndim(counts) == 0 \
        else np.asarray(counts, dtype=np.int64)
    ep = ep[ep[:, DECISION] <= counts[ep[:, GAME]]]
    out = {name: (0 if k == 1 else [0] * k) for name, k in spec.EPISODE_STATS_FIELDS}
    for r in ep:
        w = int(r[WINNER])
        assert 1 <= w <= 4
        vp, order = [int(x) for x in r[VP:VP + 4]], [int(x) for x in r[ORDER:ORDER + 4]]
        turn = int(r[TURN])
        out["episodes"] += 1
        out["wins_by_player"][w - 1] += 1
        out["wins_by_turn_order"][order.index(w)] += 1
        out["turns_sum"] += turn
        out["turns_sumsq"] += turn * turn
        out["turns_max"] = max(out["turns_max"], turn)
        out["turns_hist"][min(turn // spec.EPISODE_STATS_HIST_BIN_TURNS, 15)] += 1
        for p in range(4):
            out["vp_sum_by_player"][p] += vp[p]
        out["winner_vp_sum"] += vp[w - 1]
        out["loser_vp_sum"] += sum(vp) - vp[w - 1]
        out["winner_has_longest_road"] += int(r[LR] == w)
        out["winner_has_largest_army"] += int(r[LA] == w)
        out["games_with_longest_road"] += int(r[LR] != 0)
        out["games_with_largest_army"] += int(r[LA] != 0)
        out["winner_settlements_sum"] += 5 - int(r[SLEFT + w - 1])
        out["winner_cities_sum"] += 4 - int(r[CLEFT + w - 1])
        out["dev_cards_played_sum"] += int(r[NPLAYED:NPLAYED + 4].sum())
        fp = 0 if focus is None else int(focus[int(r[GAME])])
        if fp:
            out["focus_episodes"] += 1
            out["focus_vp_sum"] += vp[fp - 1]
            if fp == w:
                out["focus_wins"] += 1
                out["focus_turn_order_wins"][order.index(fp)] += 1
    flat = []
    for name, k in spec.EPISODE_STATS_FIELDS:
        flat += [out[name]] if k == 1 else out[name]
    return flat


def named(words):
    """counter block -> {name: int or list} (no derived means), for readable assertion messages"""
    d, o = {}, 0
    for name, k in spec.EPISODE_STATS_FIELDS:
        d[name] = words[o] if k == 1 else list(words[o:o + k])
        o += k
    return d
