"""Test infrastructure for the tournament: the seat rule and the tally in plain Python integers, written from the
design text, and TourneyTwin - tests/oracle_vec_env.py whose auto-reset and reset(mask) call them, with VecCatanEnv's tournament calls.
Shares no code with the package.  The tally works on episode records: the columns of episode_stats_oracle.replay."""
import ctypes as C

import numpy as np
import torch

import episode_stats_oracle as eso
from oracle_vec_env import OracleVecEnv
from settlers_of_catan_rl_amd import spec

WORDS = 16
GAMES, DRAWS, WINS, VP, WINS_BY_TURN, TURNS = 0, 1, 2, 6, 10, 14
T_SEEN, T_TALLIED, T_DRAWS, T_SKIPPED_UNSEATED, T_SEATED, T_RETIRED = range(6)
M64 = (1 << 64) - 1


def permutation(idx):
    """the idx-th permutation of (0, 1, 2, 3) in lexicographic order, by its factorial digits"""
    free, out = [0, 1, 2, 3], []
    for radix in (6, 2, 1):
        out.append(free.pop(idx // radix))
        idx %= radix
    return tuple(out + free)


def episode_index(game_id, k, E):
    game_id, k, E = int(game_id), int(k), int(E)             # (Python integers: the products pass 2^63)
    return (game_id * E + k if E else game_id + (k << 32)) & M64


def seat(game_id, k, E, L):
    """-> (lineup, pos_of_pid) of the k-th episode (from 0) of the game with that global id; None: retired (k >= E > 0)"""
    if E and k >= E:
        return None
    s = episode_index(game_id, k, E)
    return s % L, permutation((s // L) % 24)


def new_table(L):
    return [[0] * WORDS for _ in range(L + 1)]


def tally(table, L, seating, winner, vp, order, turn):
    """one finished game: seating as `seat` returns it (None: unseated), winner PlayerId (0: none), vp[4] by PlayerId-1, order the
    player_order (PlayerIds), turn the final turn number"""
    tot = table[L]
    tot[T_SEEN] += 1
    if seating is None:
        tot[T_SKIPPED_UNSEATED] += 1
        return
    lineup, pos = seating
    row = table[lineup]
    row[GAMES] += 1
    if not 1 <= winner <= 4:
        row[DRAWS] += 1
        tot[T_DRAWS] += 1
        return
    tot[T_TALLIED] += 1
    row[WINS + pos[winner - 1]] += 1
    for p in range(4):
        row[VP + pos[p]] += int(vp[p])
    row[WINS_BY_TURN + [int(x) for x in order].index(winner)] += 1
    row[TURNS] += int(turn)


def table_of_episodes(ep, counts, n, L, E, env_id0=0, initial_reset=True):
    """-> int64 [L + 1][16]: what a handle of n games shows that was enabled, reset (initial_reset: every game seated once) and then
    finished the episodes of `ep` (rows of episode_stats_oracle.replay, in each game's own order) with DECISION <= counts[game]"""
    ep = np.asarray(ep, dtype=np.int64).reshape(-1, eso.COLS)
    counts = np.broadcast_to(np.asarray(counts, dtype=np.int64), (n,))
    t = new_table(L)
    k = [0] * n
    for g in range(n):
        if initial_reset:
            t[L][T_SEATED] += 1
    for r in ep:
        g = int(r[eso.GAME])
        if r[eso.DECISION] > counts[g]:
            continue
        tally(t, L, seat(env_id0 + g, k[g], E, L), int(r[eso.WINNER]), r[eso.VP:eso.VP + 4], r[eso.ORDER:eso.ORDER + 4], int(r[eso.TURN]))
        if E and k[g] >= E:
            continue                                   # retired: it stays unseated, nothing is counted again
        k[g] += 1
        if E and k[g] == E:
            t[L][T_RETIRED] += 1
        else:
            t[L][T_SEATED] += 1
    return np.array(t, dtype=np.int64)


class TourneyTwin(OracleVecEnv):
    """OracleVecEnv with VecCatanEnv's tournament calls.  The oracle's own auto-reset is off: a finished game is booked from its exported
    final state, dealt by the oracle and seated anew; reset(mask) books the seated games it selects (as draws, no winner) and seats every
    selected game."""

    def __init__(self, n, seed, env_id0=0):
        OracleVecEnv.__init__(self, n, seed=seed, env_id0=env_id0, auto_reset=False)
        self.lineups = None

    # ---- the calls of VecCatanEnv
    def enable_tournament(self, lineups, num_players, episodes_per_game=0):
        a = np.asarray(lineups, dtype=np.int64)
        if a.ndim != 2 or a.shape[1] != 4 or not 1 <= a.shape[0] <= 65536 or a.min() < 0 or a.max() >= num_players or episodes_per_game < 0:
            raise ValueError("enable_tournament")
        self.lineups, self.E = a.copy(), int(episodes_per_game)
        self.lineup_of = np.full(self.n, -1, dtype=np.int32)
        self.pos_of_pid = np.full((self.n, 4), -1, dtype=np.int32)
        self.episode = np.zeros(self.n, dtype=np.int64)
        self.table = new_table(len(a))

    def disable_tournament(self):
        self.lineups = None

    def tournament_table(self, reset=False):
        out = torch.tensor(self.table, dtype=torch.int64)
        if reset:
            self.table = new_table(len(self.lineups))
        return out

    def tournament_seating(self):
        return torch.from_numpy(self.lineup_of), torch.from_numpy(self.pos_of_pid)       # (views: the twin writes them in place)

    def sample_random_actions(self, step_idx):
        m = self.b.masks()
        a = np.zeros((self.n, 18), dtype=np.int32)
        for g in range(self.n):
            self.L.orc_sample_action(self.b.env_ptr(g), self.seed, self.env_id0 + g, int(step_idx), m[g].ctypes.data_as(C.POINTER(C.c_float)),
                                     a[g].ctypes.data_as(C.POINTER(C.c_int32)))
        return torch.from_numpy(a)

    # ---- the hooks
    def _seating_of(self, g):
        return None if self.lineup_of[g] < 0 else (int(self.lineup_of[g]), tuple(int(x) for x in self.pos_of_pid[g]))

    def _tally(self, g):
        b = np.zeros(spec.STATE_WORDS, dtype=np.int32)
        self.L.orc_export(self.b.env_ptr(g), b.ctypes.data_as(C.POINTER(C.c_int32)))
        f = lambda name: spec.state_field(b, name)
        tally(self.table, len(self.lineups), self._seating_of(g), int(f("winner")[0]), [int(f(f"p{p}_vp")[0]) for p in (1, 2, 3, 4)],
              f("player_order"), int(f("turn")[0]))

    def _seat(self, g):
        L, E, k = len(self.lineups), self.E, int(self.episode[g])
        s = seat(self.env_id0 + g, k, E, L)
        if s is None:
            self.lineup_of[g], self.pos_of_pid[g] = -1, -1
            if k == E:
                self.episode[g] = E + 1
                self.table[L][T_RETIRED] += 1
            return
        self.lineup_of[g], self.pos_of_pid[g] = s[0], s[1]
        self.episode[g] = k + 1
        self.table[L][T_SEATED] += 1

    def reset(self, mask=None):
        for g in range(self.n):
            if mask is None or bool(mask[g]):
                if self.lineups is not None and self.lineup_of[g] >= 0:
                    self._tally(g)
                self.L.orc_game_reset(self.b.env_ptr(g))
                if self.lineups is not None:
                    self._seat(g)

    def step(self, actions):
        reward, done = OracleVecEnv.step(self, actions if torch.is_tensor(actions) else torch.from_numpy(np.asarray(actions)))
        for g in np.flatnonzero(done.numpy()):
            g = int(g)
            if self.lineups is not None:
                self._tally(g)
            self.L.orc_game_reset(self.b.env_ptr(g))
            if self.lineups is not None:
                self._seat(g)
        return reward, done
