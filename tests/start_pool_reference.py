"""Test infrastructure for the start pool: Philox4x32-10 and the pick rule in plain Python integers, written from the
design text, and PoolTwin - tests/oracle_vec_env.py with the install applied by export / import of single oracle games.  Shares no
code with the package.  The scenarios of tests/test_gpu_start_pool.py (seeds, pools, caps) stand here and are checked on the CPU by
tests/test_start_pool_cpu.py."""
import ctypes as C
import functools

import numpy as np
import torch

import scripted_reference as sr
from oracle_vec_env import OracleVecEnv

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57        # the two round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85        # the key schedule's increments
POOL_STREAM = 0x504F4F4C                              # "POOL": counter word 1 of the pick's block
RNG_WORD = 735                                        # rng_draws, the blob's last word
STATE_WORDS = 736


def philox4x32_10(counter, key):
    """counter (c0, c1, c2, c3), key (k0, k1) -> the four output words after ten rounds"""
    c0, c1, c2, c3 = (int(x) & M32 for x in counter)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def pick_from_block(o, m, fresh_q16):
    """the rule on an output block: None = the fresh deal stays, else the entry"""
    if (o[1] >> 16) < fresh_q16:
        return None
    return (o[0] * m) >> 32


def pick(seed, game_id, d, m, fresh_q16):
    o = philox4x32_10((d, POOL_STREAM, game_id & M32, (game_id >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    return pick_from_block(o, m, fresh_q16)


class PoolTwin(OracleVecEnv):
    """OracleVecEnv whose deals go through the pick rule, with VecCatanEnv's start-pool calls.  The oracle's own auto-reset is off: a
    finished game is kept (`finished`: game and final blob, in the order the games ended), dealt by the oracle, exported, and - where
    the rule picks an entry - replaced by that entry's blob with the fresh deal's rng_draws.  No pool: every deal stays fresh and
    nothing is counted."""

    def __init__(self, n, seed, env_id0, pool=None, fresh_q16=0, auto_reset=True, dense_reward=False):
        OracleVecEnv.__init__(self, n, seed=seed, env_id0=env_id0, dense_reward=dense_reward, auto_reset=False)
        self.deal_finished = auto_reset
        self.finished, self.deal_log, self.deals = [], [], np.zeros(n, dtype=np.int64)
        self.pool = None
        if pool is not None:
            self.set_pool(pool, fresh_q16)

    def set_pool(self, pool, fresh_q16=0):
        self.pool = np.asarray(pool, dtype=np.int32).reshape(-1, STATE_WORDS).copy()
        self.fresh_q16 = int(fresh_q16)
        self.counts = {"pool": 0, "fresh": 0, "per_entry": np.zeros(len(self.pool), dtype=np.int64)}

    # ---- the calls of VecCatanEnv
    def set_start_pool(self, blobs, fresh_share=0.0):
        if not 0.0 <= float(fresh_share) <= 1.0:
            raise ValueError("fresh_share")
        b = blobs.cpu().numpy() if torch.is_tensor(blobs) else np.asarray(blobs)
        self.set_pool(b, int(round(float(fresh_share) * 65536)))

    def clear_start_pool(self):
        self.pool = None

    def start_pool_counts(self, reset=False):
        out = {"pool": int(self.counts["pool"]), "fresh": int(self.counts["fresh"]), "per_entry": self.counts["per_entry"].copy()}
        if reset:
            self.set_pool(self.pool, self.fresh_q16)
        return out

    def export_game(self, g):
        b = np.zeros(STATE_WORDS, dtype=np.int32)
        self.L.orc_export(self.b.env_ptr(g), b.ctypes.data_as(C.POINTER(C.c_int32)))
        return b

    def _deal(self, g):
        self._deal_and_pick(g)
        self.deal_log.append((g, self.export_game(g)))          # every deal in order: the game and the state it starts from

    def _deal_and_pick(self, g):
        self.L.orc_game_reset(self.b.env_ptr(g))
        self.deals[g] += 1
        if self.pool is None:
            return
        d = int(self.export_game(g)[RNG_WORD]) & M32
        k = pick(self.seed, self.env_id0 + g, d, len(self.pool), self.fresh_q16)
        if k is None:
            self.counts["fresh"] += 1
            return
        blob = self.pool[k].copy()
        blob[RNG_WORD] = np.array(d, dtype=np.uint32).astype(np.int32)
        self.L.orc_import(self.b.env_ptr(g), blob.ctypes.data_as(C.POINTER(C.c_int32)))
        self.counts["pool"] += 1
        self.counts["per_entry"][k] += 1

    def reset(self, mask=None):
        for g in range(self.n):
            if mask is None or bool(mask[g]):
                self._deal(g)

    def step(self, actions):
        a = actions if torch.is_tensor(actions) else torch.from_numpy(np.asarray(actions))
        reward, done = OracleVecEnv.step(self, a)
        for g in np.flatnonzero(done.numpy()):
            self.finished.append((int(g), self.export_game(int(g))))
            if self.deal_finished:
                self._deal(int(g))
        return reward, done

    def blobs(self):
        return self.export_state().numpy()

    def masks(self):
        return self.get_action_masks().numpy()


def bot_actions(blobs, masks):
    return sr.decide_all(blobs, masks)[0].astype(np.int32)


# ---- the scenarios of tests/test_gpu_start_pool.py; tests/test_start_pool_cpu.py::test_seed_check asserts what they rely on
N_GAMES, SEED, ENV_ID0 = 64, 23, (5 << 32) + 7        # the high and the low word of the global ids are both non-zero
ENV_ID0_ZERO = 0
STEP_CAP = 250                  # lock-step steps of a scenario; every scenario starts with reset() under its pool
RANDOM_STEPS = 300              # the random-policy scenario (catan_random_rollout)
REFUSED_SET_STEPS = 40          # the steps behind a refused catan_start_pool_set, under the pool of pools()[64][:2] installed before it
POOL_SRC_GAMES, POOL_SRC_SEED, POOL_SRC_ID0, POOL_SRC_CAP = 24, 5, 1000, 1400
LATE_VP, N_LATE, N_EARLY = 8, 60, 4


def _zero_rng(blob):
    b = blob.copy()
    b[RNG_WORD] = 0
    return b.tobytes()


@functools.lru_cache(maxsize=None)
def harvest():
    """-> (late [N_LATE, 736], early [N_EARLY, 736]): unfinished positions of bot-played oracle games whose leader has at least LATE_VP
    points (one per game and turn at most), and positions right behind the initial placement"""
    env = OracleVecEnv(POOL_SRC_GAMES, seed=POOL_SRC_SEED, env_id0=POOL_SRC_ID0, auto_reset=False)
    late, early, seen = [], [], set()
    finished = np.zeros(POOL_SRC_GAMES, dtype=bool)
    was_initial = np.ones(POOL_SRC_GAMES, dtype=bool)
    last_turn = np.full(POOL_SRC_GAMES, -1)
    f = lambda b, name: sr._f(b, name)
    for _ in range(POOL_SRC_CAP):
        blobs = env.export_state().numpy()
        a = torch.from_numpy(bot_actions(blobs, env.get_action_masks().numpy()))
        a[torch.from_numpy(finished), 0] = -1
        _, done = env.step(a)
        finished |= done.numpy().astype(bool)
        blobs = env.export_state().numpy()
        for g in range(POOL_SRC_GAMES):
            b = blobs[g]
            if finished[g] or int(f(b, "winner")[0]) != 0:
                continue
            initial = bool(f(b, "initial_phase")[0])
            key = _zero_rng(b)
            if was_initial[g] and not initial and len(early) < N_EARLY and key not in seen:
                early.append(b.copy()); seen.add(key)
            was_initial[g] = initial
            turn = int(f(b, "turn")[0])
            if max(int(v) for v in f(b, "curr_vps")) >= LATE_VP and turn != last_turn[g] and len(late) < N_LATE and key not in seen:
                late.append(b.copy()); seen.add(key); last_turn[g] = turn
        if (len(late) >= N_LATE and len(early) >= N_EARLY) or finished.all():
            break
    assert len(late) == N_LATE and len(early) == N_EARLY, (len(late), len(early))
    return np.stack(late), np.stack(early)


def pools():
    """-> {1: [1, 736], 3: [3, 736], 64: [64, 736]}"""
    late, early = harvest()
    return {1: late[7:8].copy(), 3: np.stack([late[0], late[31], early[0]]), 64: np.concatenate([late, early])}


def run_twin(twin, steps, stop=None):
    """reset() under the twin's pool, then `steps` bot steps -> the action rows fed, per step (the GPU tests feed the device's own rows
    instead and compare after each)"""
    twin.reset()
    rows = []
    for t in range(steps):
        a = bot_actions(twin.blobs(), twin.masks())
        rows.append(a)
        twin.step(a)
        if stop is not None and stop(twin):
            break
    return rows
