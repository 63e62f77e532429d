"""Test infrastructure for the start pool's weighted pick and outcome tallies: the weighted rule in plain Python
integers on top of start_pool_reference.philox4x32_10, written from the design text, and OutcomeTwin - PoolTwin with the weighted
rule, the per-game origin and the outcome table.  Shares no code with the package.  The scenarios of
tests/test_gpu_start_pool_weighted.py stand here and are checked on the CPU by tests/test_start_pool_weighted_cpu.py."""
import numpy as np
import torch

import scripted_reference as sr
import start_pool_reference as spr
from start_pool_reference import (ENV_ID0, M32, N_GAMES, POOL_STREAM, RNG_WORD, SEED, STATE_WORDS, STEP_CAP, bot_actions, pools,  # noqa: F401
                                  run_twin)

MAX_SUM = 2 ** 32 - 1
FIELDS = ["games", "wins_p1", "wins_p2", "wins_p3", "wins_p4", "focus_games", "focus_wins", "turns_sum"]       # a row of the table
ROW = len(FIELDS)


def prefix_sums(weights):
    """-> the inclusive prefix sums as Python ints; the contract's bounds are checked here"""
    w = [int(x) for x in weights]
    assert all(0 <= x <= M32 for x in w)
    cum, run = [], 0
    for x in w:
        run += x
        cum.append(run)
    assert 1 <= run <= MAX_SUM, run
    return cum


def pick_from_block_weighted(o, cum, fresh_q16):
    """None = the fresh deal stays, else the smallest k with cum[k] > t, t = the high word of o[0] * W"""
    if (o[1] >> 16) < fresh_q16:
        return None
    t = (o[0] * cum[-1]) >> 32
    for k, c in enumerate(cum):
        if c > t:
            return k
    raise AssertionError("t < W: some prefix sum is above it")


def weighted_pick(seed, game_id, d, cum, fresh_q16):
    o = spr.philox4x32_10((d, POOL_STREAM, game_id & M32, (game_id >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    return pick_from_block_weighted(o, cum, fresh_q16)


class OutcomeTwin(spr.PoolTwin):
    """PoolTwin whose pick is the weighted one (weights None: PoolTwin's), which keeps per game the entry its episode started from
    (`origin`, -1: a fresh deal) and - once enabled - tallies every finished game into `table`, int64 [2 + (m + 1) * 8]: seen, skipped,
    then a row (FIELDS) per entry and a last row for the games that were dealt fresh."""

    def __init__(self, n, seed, env_id0, pool=None, fresh_q16=0, weights=None, auto_reset=True, dense_reward=False):
        self.cum, self.origin, self.focus, self.table = None, np.full(n, -1, dtype=np.int64), None, None
        spr.PoolTwin.__init__(self, n, seed, env_id0, pool, fresh_q16, auto_reset=auto_reset, dense_reward=dense_reward)
        if weights is not None:
            self.set_weights(weights)

    def set_pool(self, pool, fresh_q16=0):
        spr.PoolTwin.set_pool(self, pool, fresh_q16)
        self.cum = None                           # a new pool is uniform ...
        self.origin[:] = -1                       # ... and the games in flight are not booked to it
        if self.table is not None:
            self.table = np.zeros(2 + (len(self.pool) + 1) * ROW, dtype=np.int64)

    def set_weights(self, weights):
        if weights is None:
            self.cum = None
            return
        assert len(weights) == len(self.pool)
        self.cum = prefix_sums(weights)

    def enable_outcomes(self, focus=None, on=True):
        if not on:
            self.table, self.focus = None, None
            return
        if self.table is None:
            self.origin[:] = -1
        self.table = np.zeros(2 + (len(self.pool) + 1) * ROW, dtype=np.int64)
        self.focus = None if focus is None else np.asarray(focus, dtype=np.int64).copy()

    # ---- the calls of VecCatanEnv
    def set_start_pool(self, blobs, fresh_share=0.0, weights=None):
        if not 0.0 <= float(fresh_share) <= 1.0:
            raise ValueError("fresh_share")
        b = blobs.cpu().numpy() if torch.is_tensor(blobs) else np.asarray(blobs)
        self.set_pool(b, int(round(float(fresh_share) * 65536)))
        self.set_weights(weights)

    def clear_start_pool(self):
        self.pool, self.cum, self.table, self.focus = None, None, None, None
        self.origin[:] = -1

    def set_start_pool_weights(self, weights):
        self.set_weights(None if weights is None else [int(x) for x in np.asarray(weights).tolist()])

    def enable_start_pool_outcomes(self, focus_pid=None, on=True):
        f = focus_pid.cpu().numpy() if torch.is_tensor(focus_pid) else focus_pid
        self.enable_outcomes(f, on)

    def start_pool_counts(self, reset=False):
        out = {"pool": int(self.counts["pool"]), "fresh": int(self.counts["fresh"]), "per_entry": self.counts["per_entry"].copy()}
        if reset:
            self.counts = {"pool": 0, "fresh": 0, "per_entry": np.zeros(len(self.pool), dtype=np.int64)}
        return out

    def start_pool_outcomes(self, reset=False):
        m = len(self.pool)
        rows = self.table[2:].reshape(m + 1, ROW).copy()
        out = {"seen": int(self.table[0]), "skipped": int(self.table[1]), "table": rows}
        for i, name in enumerate(FIELDS):
            out[name] = rows[:m, i].copy()
        out["fresh"] = {name: int(rows[m, i]) for i, name in enumerate(FIELDS)}
        share = np.full((m, 4), np.nan)
        fshare = np.full(m, np.nan)
        for k in range(m):
            if rows[k, 0] > 0:
                share[k] = rows[k, 1:5] / float(rows[k, 0])
            if rows[k, 5] > 0:
                fshare[k] = rows[k, 6] / float(rows[k, 5])
        out["win_share_by_pid"], out["focus_win_share"] = share, fshare
        if reset:
            self.table[:] = 0
        return out

    def sample_scripted_actions(self):
        return torch.from_numpy(bot_actions(self.blobs(), self.masks()))

    def import_state(self, blobs):
        spr.PoolTwin.import_state(self, blobs)
        self.origin[:] = -1                       # a state that did not come from the pick

    # ---- the deal and the tally
    def _deal_and_pick(self, g):
        self.L.orc_game_reset(self.b.env_ptr(g))
        self.deals[g] += 1
        self.origin[g] = -1
        if self.pool is None:
            return
        d = int(self.export_game(g)[RNG_WORD]) & M32
        if self.cum is None:
            k = spr.pick(self.seed, self.env_id0 + g, d, len(self.pool), self.fresh_q16)
        else:
            k = weighted_pick(self.seed, self.env_id0 + g, d, self.cum, self.fresh_q16)
        if k is None:
            self.counts["fresh"] += 1
            return
        blob = self.pool[k].copy()
        blob[RNG_WORD] = np.array(d, dtype=np.uint32).astype(np.int32)
        self.L.orc_import(self.b.env_ptr(g), blob.ctypes.data_as(spr.C.POINTER(spr.C.c_int32)))
        self.counts["pool"] += 1
        self.counts["per_entry"][k] += 1
        self.origin[g] = k

    def _tally(self, g, blob):
        if self.table is None:
            return
        m = len(self.pool)
        self.table[0] += 1
        winner, turn, o = int(sr._f(blob, "winner")[0]), int(sr._f(blob, "turn")[0]), int(self.origin[g])
        if not 1 <= winner <= 4 or not -1 <= o < m:
            self.table[1] += 1
            return
        row = self.table[2 + (m if o < 0 else o) * ROW:][:ROW]
        row[0] += 1
        row[winner] += 1
        f = 0 if self.focus is None else int(self.focus[g])
        if 1 <= f <= 4:
            row[5] += 1
            row[6] += int(f == winner)
        row[7] += turn

    def step(self, actions):
        a = actions if torch.is_tensor(actions) else torch.from_numpy(np.asarray(actions))
        reward, done = spr.OracleVecEnv.step(self, a)
        for g in np.flatnonzero(done.numpy()):
            blob = self.export_game(int(g))
            self.finished.append((int(g), blob, int(self.origin[g])))
            self._tally(int(g), blob)
            if self.deal_finished:
                self._deal(int(g))
        return reward, done


# ---- the scenarios of tests/test_gpu_start_pool_weighted.py; tests/test_start_pool_weighted_cpu.py::test_seed_check asserts what they rely on
HEAVY, HEAVY_WEIGHT = 17, 2 ** 31
ZEROS_64 = (0, 5, 31, 32, 63)                    # both ends, the middle, and one with positive neighbours on both sides
SMALL_64 = {40: 1, 41: 3, 42: 2}                 # next to nothing beside the others: never picked in a short run, never wrong either


def weights_64():
    """the weighted 64-entry scenario: zeros, three tiny weights, one weight of 2^31 and the rest (k % 3 + 1) * 2^24 - the sum is below 2^32"""
    w = [(k % 3 + 1) << 24 for k in range(64)]
    for k in ZEROS_64:
        w[k] = 0
    for k, v in SMALL_64.items():
        w[k] = v
    w[HEAVY] = HEAVY_WEIGHT
    assert sum(w) <= MAX_SUM
    return w


FOCUS = (np.arange(N_GAMES) % 5).astype(np.int32)           # PlayerId 1..4 and, for every fifth game, no focus player
HALF_FRESH_Q16 = 32768
BIG_M = 65536
BIG_EDGES = (0, 63, 64, 4095, 4096, 65535)       # the edges of every round of a 64-ary search over 65 536 entries


def big_weights():
    w = np.zeros(BIG_M, dtype=np.int64)
    for i, k in enumerate(BIG_EDGES):
        w[k] = 1 + i
    return w
