"""CPU: the three-unit layout of the library (csrc/catan_players.hip and csrc/catan_hooks.hip beside csrc/catan_abi.hip) and the players'
shared policy base class.

The library carries three gfx950 code objects.  k_sample_scripted, the builder's kernel, is a function of the first - the one that holds
k_step and the learner's kernels, and that must stay what it is without the other players and without the opt-in hooks -, the kernels of
the teacher, the trader and the playout player are functions of the second and of the second only, and the kernels of the recorder and of
the start pool are functions of the third and of the third only.  Read off the code objects' symbol tables (llvm-readelf, as
tools/kernel_resources.py reads them); no GPU needed."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

from settlers_of_catan_rl_amd import _lib, scripted
from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, ScriptedPolicy, TraderPolicy

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FIRST = ("k_sample_scripted",)
FIRST_ENV = ("k_step", "k_masks", "k_export", "k_import", "k_episode_stats", "k_league_stats", "k_sample_scripted")
SECOND = ("k_sample_trader", "k_complete_action_rows", "k_collector_label", "k_imitation_loss", "k_playout_slots", "k_playout_expand",
          "k_playout_hold", "k_playout_score")
THIRD = ("k_record_bind", "k_record_arm", "k_record_append", "k_record_seal", "k_record_open", "k_pool_count_finished", "k_pool_scan",
         "k_pool_install_list_x", "k_pool_install_sel_x", "k_pool_origin_clear", "k_pool_outcomes")
GONE = ("k_pool_masks", "k_pool_install_list", "k_pool_install_sel")


@pytest.fixture(scope="module")
def kernels_per_code_object():
    """-> one set per code object, in link order: the names (`k_...`, unmangled, no namespace) of its function symbols in namespace catan"""
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf on this box")
    _lib.build_library()
    out = []
    for co in _lib.device_code_objects():
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            syms = subprocess.run([READELF, "-sW", f.name], stdout=subprocess.PIPE, check=True).stdout.decode()
        names = set()
        for line in syms.splitlines():
            p = line.split()
            if len(p) == 8 and p[3] == "FUNC":
                m = re.match(r"_ZN5catan(\d+)", p[7])           # catan::<name>: the length, then the name
                if m:
                    start = m.end()
                    names.add(p[7][start:start + int(m.group(1))])
        out.append(names)
    return out


def test_the_library_has_two_code_objects(kernels_per_code_object):
    assert _lib.TRANSLATION_UNITS == ("catan_abi.hip", "catan_players.hip", "catan_hooks.hip")
    assert len(kernels_per_code_object) == 3


def test_the_builder_kernel_is_in_the_first_code_object(kernels_per_code_object):
    first = kernels_per_code_object[0]
    assert all(k in first for k in FIRST), sorted(k for k in FIRST if k not in first)
    assert "k_step" in first and "k_masks" in first          # ... the one the env's own kernels live in


def test_the_players_kernels_are_in_the_second_code_object_only(kernels_per_code_object):
    first, second, third = kernels_per_code_object
    assert all(k in second for k in SECOND), sorted(k for k in SECOND if k not in second)
    assert not any(k in first | third for k in SECOND), sorted(k for k in SECOND if k in first | third)
    assert not any(k in second for k in FIRST)


def test_the_hooks_kernels_are_in_the_third_code_object_only(kernels_per_code_object):
    first, second, third = kernels_per_code_object
    hooks = {k for names in kernels_per_code_object for k in names if k.startswith(("k_record_", "k_pool_"))}
    assert hooks == set(THIRD), sorted(hooks ^ set(THIRD))
    assert hooks <= third and not hooks & (first | second), sorted(hooks & (first | second))
    assert all(k in first for k in FIRST_ENV), sorted(k for k in FIRST_ENV if k not in first)
    assert not any(k in names for k in GONE for names in kernels_per_code_object)


# ---- the base class of scripted.py: rebind, the bound-env check, act and label, for every player

class _Env(object):
    """a stand-in that answers every row with EndTurn"""

    def __init__(self, n):
        self.n, self.env_id0, self.device, self.completed = n, 0, torch.device("cpu"), 0

    def _rows(self, games):
        a = torch.zeros((self.n if games is None else int(games.numel()), 18), dtype=torch.int32)
        a[:, 0] = 10
        return a

    def sample_scripted_actions(self, games=None, **kw):
        return self._rows(games)

    def playout_actions(self, sim_env, games=None, **kw):
        a = self._rows(games)
        return a, torch.zeros(a.shape[0], dtype=torch.int32), torch.zeros((a.shape[0], 4, 7), dtype=torch.int64)

    def complete_action_rows(self, actions, games=None):
        self.completed += 1
        return actions


class _Playout(PlayoutPolicy):
    def _make_sim(self, env, games):
        return _Env(games)


PLAYERS = (ScriptedPolicy, TraderPolicy, _Playout)


def _obs(rows):
    return torch.zeros(rows, 4), None, None, None


@pytest.mark.parametrize("cls", PLAYERS)
def test_unbound_players_raise_with_their_own_name(cls):
    assert issubclass(cls, scripted.GamesPolicy) and cls.wants_games is True and cls.include_lstm is False
    name = cls.__name__
    with pytest.raises(RuntimeError, match=rf"^{name} is not bound to an env \({name}\(env\) or rebind\(env\)\)$"):
        cls().act(*_obs(4))
    with pytest.raises(RuntimeError, match=rf"^{name} is not bound to an env \({name}\(env\) or rebind\(env\)\)$"):
        cls().label()


@pytest.mark.parametrize("cls", PLAYERS)
def test_bound_players_check_the_rows_of_a_pass(cls):
    env, name = _Env(4), cls.__name__
    pol = cls()
    assert pol.rebind(env) is pol and pol.env is env
    with pytest.raises(ValueError, match=rf"^{name}\.act without `games` decides all 4 games of its env, the pass has 3 rows$"):
        pol.act(*_obs(3))
    with pytest.raises(ValueError, match=rf"^{name}\.act: 2 games for 3 rows$"):
        pol.act(*_obs(3), games=torch.tensor([0, 1]))
    v, a, lp = pol.act(*_obs(4))
    assert a.dtype == torch.int64 and a.shape == (4, 18) and a[:, 0].tolist() == [10] * 4
    assert v.shape == (4, 1) and lp.shape == (4, 1) and v.dtype == torch.float32 and not v.any() and not lp.any() and v is not lp
    _, a, _ = pol.act(*_obs(2), games=torch.tensor([3, 1]))
    assert a.shape == (2, 18)
    lab = pol.label(games=torch.tensor([2]))
    assert lab.dtype == torch.int32 and lab.shape == (1, 18) and env.completed == 1
    assert pol.label().shape == (4, 18) and env.completed == 2
