"""Test infrastructure for the game recorder: a host-side recorder over tests/oracle_vec_env.py, a one-game env over
oracle/libcatan_cpu.so for replays, and the shapes the CPU seed check and the GPU tests share.  Shares no code with the package's
recorder: the records it makes are plain dicts of numpy arrays."""
import ctypes as C

import numpy as np
import torch

import cpu_abi_driver
import scripted_reference as sr
from settlers_of_catan_rl_amd._lib import CatanCfg

# ---- what tests/test_gpu_record.py runs, and tests/test_record_cpu.py checks on the CPU beforehand (the seed is chosen THERE)
N_GAMES, SEED, ENV_ID0 = 64, 11, 0
# 16 slots on both 32-game tiles of k_step, with the tiles' first and last games
ARMED_GAMES = [0, 5, 11, 17, 23, 29, 30, 31, 32, 33, 38, 44, 50, 56, 62, 63]
# decisions per game, the rule-based player in all four seats, inside which every armed game finishes once / twice (re-dealt in between):
# the longest first episode of this seed takes 785 decisions, the longest two together 1 437 (tests/test_record_cpu.py asserts the caps)
STEP_CAP_ONE, STEP_CAP_TWO = 900, 1600
OVERFLOW_CAPACITY = 64


class HostRecorder(object):
    """Wraps OracleVecEnv.step: for every game of `games` it logs the applied action rows (no-ops excluded) with the step's reward /
    done, keeps the blob in front of the first logged action and the blob after the action that ended the game - taken before the
    env's auto-reset deals the game again, which this wrapper therefore does itself."""

    def __init__(self, env, games):
        self.env, self.games = env, list(games)
        self.auto_reset, env.auto_reset = env.auto_reset, False
        blobs = env.export_state().numpy()
        self.rec = {g: dict(start=blobs[g].copy(), actions=[], reward=[], done=[], final=None) for g in self.games}

    def step(self, actions):
        a = actions.numpy().astype(np.int32)
        reward, done = self.env.step(actions)
        blobs = self.env.export_state().numpy()
        for g in self.games:
            r = self.rec[g]
            if a[g, 0] < 0 or r["final"] is not None:
                continue
            r["actions"].append(a[g].copy()); r["reward"].append(reward[g].numpy().copy()); r["done"].append(bool(done[g]))
            if done[g]:
                r["final"] = blobs[g].copy()
        if self.auto_reset:
            for g in np.flatnonzero(done.numpy()):
                self.env.L.orc_game_reset(self.env.b.env_ptr(int(g)))
        return reward, done

    def record(self, g):
        r = self.rec[g]
        return dict(seed=self.env.seed, game_id=self.env.env_id0 + g, start=r["start"], final=r["final"],
                    actions=np.array(r["actions"], dtype=np.int32).reshape(-1, 18), reward=np.array(r["reward"], dtype=np.float32).reshape(-1, 4),
                    done=np.array(r["done"], dtype=bool))


class CpuEnv(object):
    """ONE game on oracle/libcatan_cpu.so (the env ABI of include/catan_hip.h over the CPU oracle), created with n = 1, the record's seed
    and env_id0 = the game id; the duck-typed interface record.replay takes as `env`."""

    def __init__(self, seed, game_id, validate_actions=True, dense_reward=False, win_reward=500.0, reward_annealing_factor=1.0,
                 max_proposed_trades_per_turn=4, max_actions_per_turn=None, **_ignored):
        self.L = cpu_abi_driver.cpu_lib()
        cfg = CatanCfg()
        self.L.catan_cfg_default(C.byref(cfg))
        cfg.validate_actions, cfg.dense_reward, cfg.auto_reset = int(validate_actions), int(dense_reward), 0
        cfg.win_reward, cfg.reward_annealing_factor = float(win_reward), float(reward_annealing_factor)
        cfg.max_proposed_trades_per_turn = -1 if max_proposed_trades_per_turn is None else int(max_proposed_trades_per_turn)
        cfg.max_actions_per_turn = -1 if max_actions_per_turn is None else int(max_actions_per_turn)
        self.h = C.c_void_p()
        assert self.L.catan_create(C.byref(self.h), 0, 1, int(seed), int(game_id), C.byref(cfg)) == 0, self.L.catan_last_error()
        self._rew, self._done = np.zeros((1, 4), dtype=np.float32), np.zeros((1,), dtype=np.uint8)

    @staticmethod
    def _p(a):
        return C.c_void_p(a.ctypes.data)

    def import_state(self, blobs):
        b = np.ascontiguousarray(np.asarray(blobs, dtype=np.int32).reshape(1, 736).T)
        assert self.L.catan_state_import(self.h, self._p(b), None, 1, None) == 0

    def export_state(self):
        b = np.zeros((736, 1), dtype=np.int32)
        assert self.L.catan_state_export(self.h, self._p(b), None, 1, None) == 0
        return torch.from_numpy(b.T.copy())

    def deciding_player(self):
        s = np.zeros((1,), dtype=np.int32)
        assert self.L.catan_deciding_seat(self.h, self._p(s), None) == 0
        return torch.from_numpy(s)

    def masks(self):
        m = np.zeros((1, 325), dtype=np.float32)
        assert self.L.catan_masks(self.h, self._p(m), None) == 0
        return m

    def invalid_action_count(self):
        return int(self.L.catan_invalid_action_count(self.h, None))

    def step(self, actions):
        a = np.ascontiguousarray(actions.numpy().astype(np.int32).reshape(1, 18))
        assert self.L.catan_step(self.h, self._p(a), self._p(self._rew), self._p(self._done), None) == 0
        return torch.from_numpy(self._rew.copy()), torch.from_numpy(self._done.copy())

    def close(self):
        if self.h:
            self.L.catan_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def replay_on_cpu(seed, game_id, start, actions, **cfg):
    """-> (final blob, reward [L, 4], done [L], rejected [L]): the start blob stepped through libcatan_cpu"""
    env = CpuEnv(seed, game_id, **cfg)
    env.import_state(start)
    rew, done, rejected = [], [], []
    for a in np.asarray(actions, dtype=np.int32).reshape(-1, 18):
        bad0 = env.invalid_action_count()
        r, d = env.step(torch.from_numpy(a.copy()).view(1, 18))
        rew.append(r[0].numpy()); done.append(bool(d[0])); rejected.append(env.invalid_action_count() != bad0)
    final = env.export_state()[0].numpy()
    env.close()
    return final, np.array(rew, dtype=np.float32).reshape(-1, 4), np.array(done, dtype=bool), np.array(rejected, dtype=bool)


def bot_actions(blobs, masks):
    """the numpy restatement of the rule-based player for every game -> int32 [n, 18]"""
    return sr.decide_all(blobs, masks)[0].astype(np.int32)
