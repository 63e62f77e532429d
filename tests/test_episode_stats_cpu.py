"""Host side of the finished-game statistics: the dict built from a counter block, TrainingLoop.run_update passing it on, and the
ctypes table loading the CPU library, which has no such entry points."""
import ctypes as C

import pytest
import torch

from settlers_of_catan_rl_amd import _lib, spec
from settlers_of_catan_rl_amd import train_loop as tl


def _block(**kw):
    words, o = [0] * spec.EPISODE_STATS_WORDS, 0
    for name, n in spec.EPISODE_STATS_FIELDS:
        v = kw.pop(name, None)
        if v is not None:
            words[o:o + n] = [v] if n == 1 else list(v)
        o += n
    assert not kw
    return words


def test_layout_is_the_headers():
    assert spec.EPISODE_STATS_WORDS == 48 and [n for n, _ in spec.EPISODE_STATS_FIELDS][:3] == ["episodes", "wins_by_player", "wins_by_turn_order"]
    offs, o = {}, 0
    for name, n in spec.EPISODE_STATS_FIELDS:
        offs[name] = o
        o += n
    # include/catan_hip_tuning.h, csrc/catan_stats.hip (ES_*)
    assert (offs["turns_sum"], offs["turns_max"], offs["turns_hist"], offs["vp_sum_by_player"], offs["winner_vp_sum"]) == (9, 11, 12, 28, 32)
    assert (offs["winner_has_longest_road"], offs["winner_settlements_sum"], offs["dev_cards_played_sum"]) == (34, 38, 40)
    assert (offs["focus_episodes"], offs["focus_turn_order_wins"]) == (41, 44)


def test_derived_means_of_a_hand_written_block():
    # four games: turns 40, 60, 100, 200; winners' seats 0, 0, 2, 3; the focus player took part in three and won one from seat 2
    d = spec.episode_stats_dict(_block(
        episodes=4, wins_by_player=[1, 0, 2, 1], wins_by_turn_order=[2, 0, 1, 1], turns_sum=400, turns_sumsq=40 ** 2 + 60 ** 2 + 100 ** 2 + 200 ** 2,
        turns_max=200, turns_hist=[0, 2, 0, 1, 0, 0, 1] + [0] * 9, vp_sum_by_player=[30, 20, 34, 28], winner_vp_sum=41, loser_vp_sum=71,
        winner_has_longest_road=3, winner_has_largest_army=1, games_with_longest_road=4, games_with_largest_army=2,
        winner_settlements_sum=12, winner_cities_sum=9, dev_cards_played_sum=30, focus_episodes=3, focus_wins=1, focus_vp_sum=21,
        focus_turn_order_wins=[0, 0, 1, 0]))
    assert d["episodes"] == 4 and d["wins_by_player"] == [1, 0, 2, 1] and d["turns_hist"][:4] == [0, 2, 0, 1] and d["turns_max"] == 200
    assert d["mean_turns"] == 100.0
    assert abs(d["std_turns"] - (((40 - 100) ** 2 + (60 - 100) ** 2 + 0 + 100 ** 2) / 4) ** 0.5) < 1e-9
    assert d["win_rate_by_turn_order"] == [0.5, 0.0, 0.25, 0.25] and d["win_rate_by_player"] == [0.25, 0.0, 0.5, 0.25]
    assert d["mean_winner_vp"] == 10.25 and d["mean_loser_vp"] == 71 / 12
    assert d["longest_road_decides"] == 0.75 and d["largest_army_decides"] == 0.25 and d["mean_dev_cards_played"] == 7.5
    assert d["focus_win_rate"] == 1 / 3 and d["focus_mean_vp"] == 7.0 and d["focus_turn_order_wins"] == [0, 0, 1, 0]
    # nothing counted: counters 0, every mean None (not a division by zero)
    z = spec.episode_stats_dict([0] * 48)
    assert z["episodes"] == 0 and z["mean_turns"] is None and z["focus_win_rate"] is None and z["win_rate_by_turn_order"] == [None] * 4
    # episodes without a focus player
    assert spec.episode_stats_dict(_block(episodes=2, turns_sum=10, turns_sumsq=52))["focus_win_rate"] is None
    with pytest.raises(ValueError):
        spec.episode_stats_dict([0] * 47)


class _Env(object):
    n = 10
    def set_reward_annealing_factor(self, f): pass


class _Storage(object):
    games_complete = 3
    def __init__(self, stats): self.episode_stats = stats


class _BareStorage(object):          # a collector's storage from before the feature
    games_complete = 3


class _Collector(object):
    N = 10
    def __init__(self, storages): self.storages = list(storages)
    def gather_rollouts(self): return self.storages.pop(0)
    def after_rollouts(self): pass


class _Trainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        class Cfg: entropy_coef = 0.0
        self.cfg = Cfg()
    def update(self, st): return (0.1, 0.2, 0.3)


def test_run_update_passes_the_episodes_on():
    net = torch.nn.Linear(3, 3)
    stats = spec.episode_stats_dict(_block(episodes=5, focus_episodes=5, focus_wins=2))
    col = _Collector([_Storage(stats), _Storage(None), _BareStorage()])
    loop = tl.TrainingLoop(_Env(), net, col, _Trainer(net), tl.TrainArgs(num_steps=4, total_env_steps=4 * 10 * 50))
    out = loop.run_update()
    assert out["episodes"] is stats and out["episodes"]["focus_win_rate"] == 0.4 and out["games_complete"] == 3
    assert "episodes" not in loop.run_update()          # statistics off: the result is the one it was
    assert "episodes" not in loop.run_update()


def test_the_table_loads_the_cpu_library_without_the_new_entry_points():
    import cpu_abi_driver as drv
    new = {"catan_episode_stats_words", "catan_episode_stats_enable", "catan_episode_stats_read"}
    assert new <= set(_lib.declared_symbols()) and new <= _lib._OPTIONAL
    L = drv.cpu_lib()
    assert not any(hasattr(L, name) for name in new)
    shared = [name for name in drv.ENTRY_POINTS if name in _lib._SIGS]
    bound = _lib.bind(C.CDLL(drv.CPU_LIB), shared + sorted(new))
    assert bound == shared and len(shared) >= 20
    with pytest.raises(AttributeError):
        _lib.bind(C.CDLL(drv.CPU_LIB), ["catan_random_rollout_deferred"])     # a required entry point it lacks still raises
