"""Board layouts on the host: validation of the configs (spec.normalise_board_config, VecCatanEnv.set_board_config's first step),
spec.board_config_from_state, and the self-consistency of tests/golden/board_configs.npz (tools/gen_golden_boards.py)."""
import numpy as np
import pytest

import board_layouts as bl
import golden_util as gu
from settlers_of_catan_rl_amd import spec

TERRAIN = list(spec.TERRAIN_TO_PLACE)
NAMES = [spec.TERRAIN_NAMES[t] for t in TERRAIN]


def test_default_and_names_versus_codes():
    assert spec.normalise_board_config(None) == (True, None, None)
    assert spec.normalise_board_config({}) == (True, None, None)
    assert spec.normalise_board_config({"randomise_number_placement": False}) == (False, None, None)
    by_code = spec.normalise_board_config({"fixed_terrain_placements": TERRAIN})
    by_name = spec.normalise_board_config({"fixed_terrain_placements": NAMES})
    lower = spec.normalise_board_config({"fixed_terrain_placements": [n.lower() for n in NAMES]})
    qualified = spec.normalise_board_config({"fixed_terrain_placements": ["Terrain." + n for n in NAMES]})
    assert by_code == by_name == lower == qualified == (True, TERRAIN, None)
    # the reference's Terrain is an IntEnum: anything with __index__ in 0..5 is taken by value
    assert spec.terrain_code(np.int8(5)) == 5 and spec.TERRAIN_NAMES[5] == "Fields" and spec.TERRAIN_NAMES[2] == "Forest"
    r, t, n = spec.normalise_board_config({"fixed_number_order": spec.DEFAULT_NUMBER_ORDER[::-1]})
    assert (r, t, n) == (True, None, spec.DEFAULT_NUMBER_ORDER[::-1])


@pytest.mark.parametrize("cfg, match", [
    ({"fixed_terrain_placements": TERRAIN[:-1]}, "19 terrains"),
    ({"fixed_terrain_placements": [1] + TERRAIN[1:]}, "counts of TERRAIN_TO_PLACE"),            # no desert, four hills
    ({"fixed_terrain_placements": ["Desert", "Desert"] + NAMES[2:]}, "counts of TERRAIN_TO_PLACE"),
    ({"fixed_terrain_placements": ["Sea"] + NAMES[1:]}, "unknown terrain name"),
    ({"fixed_terrain_placements": [6] + TERRAIN[1:]}, "outside 0..5"),
    ({"fixed_terrain_placements": [True] + TERRAIN[1:]}, "a terrain is a name"),
    ({"fixed_number_order": spec.DEFAULT_NUMBER_ORDER[:-1]}, "permutation of DEFAULT_NUMBER_ORDER"),
    ({"fixed_number_order": [7] + spec.DEFAULT_NUMBER_ORDER[1:]}, "permutation of DEFAULT_NUMBER_ORDER"),
    ({"fixed_number_order": [6] + spec.DEFAULT_NUMBER_ORDER[1:]}, "permutation of DEFAULT_NUMBER_ORDER"),   # three 6s, one 5
    ({"fixed_terrain": TERRAIN}, "unknown board config keys"),
    ([("randomise_number_placement", False)], "a board config is a dict"),
])
def test_wrong_configs_are_value_errors(cfg, match):
    with pytest.raises(ValueError, match=match):
        spec.normalise_board_config(cfg)


def test_more_than_sixteen_layouts_are_refused_on_the_host():
    """VecCatanEnv.set_board_config checks the count before it touches the library (no device needed to reach the check)"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv.__new__(VecCatanEnv)
    env.n = 4
    with pytest.raises(ValueError, match="at most 16"):
        VecCatanEnv.set_board_config(env, [{}] * 17)
    with pytest.raises(ValueError, match="unknown terrain name"):
        VecCatanEnv.set_board_config(env, [{}, {"fixed_terrain_placements": ["Sea"] * 19}])


def test_c_layout_of_a_board_config():
    import ctypes as C
    from settlers_of_catan_rl_amd import _lib
    assert C.sizeof(_lib.CatanBoardCfg) == 56
    assert _lib.CatanBoardCfg.terrain.offset == 12 and _lib.CatanBoardCfg.numbers.offset == 31


def test_fixture_layouts_and_their_blobs():
    """every fixture blob carries its layout's board; the fixed token orders are never rejected (layout 2 puts a 6 and an 8
    side by side on every board, layout 1 whenever the desert does not separate them), and the reference's default order
    unshuffled (layout 3) is dealt as it stands"""
    g = gu.load(bl.FIXTURE)
    lays = bl.layouts(g)
    assert len(lays) == 4
    assert "fixed_terrain_placements" in lays[0] and "fixed_number_order" not in lays[0]
    assert "fixed_number_order" in lays[1] and "fixed_terrain_placements" not in lays[1]
    assert "fixed_number_order" in lays[2] and "fixed_terrain_placements" in lays[2]
    assert lays[3] == {"randomise_number_placement": False}
    nbr = bl.tile_nbr_masks()
    blobs = g["reset_blobs"]
    assert blobs.shape[:3] == (4, len(g["seeds"]), int(g["pairs"])) and blobs.shape[0] * blobs.shape[1] * blobs.shape[2] == 192
    reds = [0, 0, 0, 0]
    for li, cfg in enumerate(lays):
        for b in blobs[li].reshape(-1, spec.STATE_WORDS):
            assert bl.board_problem(b, cfg, nbr) is None, (li, bl.board_problem(b, cfg, nbr))
            reds[li] += bl.touching_reds(b, nbr)
    assert reds[0] == 0 and reds[2] == 48 and reds[1] > 0
    # fixed terrain: one board; shuffled tokens: (almost) every board different
    assert len({tuple(spec.state_field(b, "tile_val")) for b in blobs[0].reshape(-1, spec.STATE_WORDS)}) > 40
    assert len({tuple(spec.state_field(b, "tile_res")) for b in blobs[2].reshape(-1, spec.STATE_WORDS)}) == 1
    # the trajectories cross game ends and every re-deal carries the layout (the final blob is a re-dealt game's)
    for k in (0, 1):
        assert int(g[f"traj{k}_dones"].sum()) >= 2
        assert bl.board_problem(g[f"traj{k}_final_blob"], lays[int(g[f"traj{k}_layout"])], nbr, fresh=False) is None
    assert int(g["mt_dones"].sum()) >= 1 and bl.board_problem(g["mt_final"], lays[int(g["mt_layout"])], nbr, fresh=False) is None


def test_board_config_from_state_round_trips():
    g = gu.load(bl.FIXTURE)
    lays = bl.layouts(g)
    nbr = bl.tile_nbr_masks()
    for li in range(4):
        for b in g["reset_blobs"][li].reshape(-1, spec.STATE_WORDS)[:12]:
            cfg = spec.board_config_from_state(b)
            assert set(cfg) == set(spec.BOARD_CONFIG_KEYS)
            assert bl.board_problem(b, cfg, nbr) is None          # the board of the blob is the one its layout fixes
            randomise, terrain, numbers = spec.normalise_board_config(cfg)
            assert terrain == [int(x) for x in spec.state_field(b, "tile_res")]
            if "fixed_number_order" in lays[li]:
                assert numbers == lays[li]["fixed_number_order"]
            if "fixed_terrain_placements" in lays[li]:
                assert terrain == lays[li]["fixed_terrain_placements"]
            # and once more through the names
            named = dict(cfg, fixed_terrain_placements=[spec.TERRAIN_NAMES[t] for t in terrain])
            assert spec.normalise_board_config(named) == (randomise, terrain, numbers)


def test_configured_board_config_reaches_the_rollout_and_evaluation_envs(monkeypatch):
    """reference_api.configure(env_kwargs={"board_config": ...}) is passed to the env of the rollouts (with the other env_kwargs) and to
    every evaluation env (the layout only)"""
    from settlers_of_catan_rl_amd import env as env_mod, reference_api as ra
    seen = []

    class Built(Exception):
        pass

    def fake_env(n, **kw):
        seen.append((n, kw))
        raise Built()

    monkeypatch.setattr(env_mod, "VecCatanEnv", fake_env)
    layout = {"fixed_number_order": spec.DEFAULT_NUMBER_ORDER}
    monkeypatch.setitem(ra._DEFAULTS, "env_kwargs", {"board_config": layout, "dense_reward": True})
    with pytest.raises(Built):
        ra.SubProcGameManager([ra.make_game_manager(3, 8), ra.make_game_manager(3, 8)])
    with pytest.raises(Built):
        ra.SubProcEvaluationManager([ra.make_evaluation_manager()] * 2).run_evaluation_episodes(4)
    (n0, kw0), (n1, kw1) = seen
    assert n0 == 6 and kw0["board_config"] is layout and kw0["dense_reward"] is True and kw0["auto_reset"] is True
    assert n1 == 4 and kw1["board_config"] is layout and "dense_reward" not in kw1 and kw1["auto_reset"] is False
