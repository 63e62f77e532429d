"""Canonical layouts shared by the host shim, the parity tests and the golden generators.

Three flat formats pin parity between the upstream reference (`/root/reference`, Python),
the CPU oracle (`oracle/catan_oracle.c`) and the HIP path (`csrc/catan_kernels.hip`):

* STATE BLOB  - int32[STATE_WORDS]: the full per-game state in reference-like, unpacked form
  (mirrors `Game.save_current_state`, reference game/game.py:1013-1091, plus the wrapper fields
  env/wrapper.py:30-34).  The device keeps a packed layout; `catan_state_export` unpacks to this.
* MASKS       - float32[325]: the 12 arrays of `EnvWrapper.get_action_masks`
  (env/wrapper.py:172-185) flattened row-major in head order.
* OBS         - float32[1787] + int32[5][OBS_LIST_PAD] card-id lists + lengths
  (env/wrapper.py:52-83, key order of RL/ppo/process_batch.py:10-13).
* ACTION      - int32[18]: the 12-head composite action of env/wrapper.py:114-166 flattened
  (heads 7 and 8 are 4-long sequences).
"""
from collections import OrderedDict

N_CORNERS, N_EDGES, N_TILES, N_PLAYERS = 54, 72, 19, 4
N_ACTION_TYPES = 13

# ---------------------------------------------------------------- action (int32[18])
ACTION_WORDS = 18
A_TYPE, A_CORNER, A_EDGE, A_TILE, A_CARD, A_RESPONSE, A_PLAYER = 0, 1, 2, 3, 4, 5, 6
A_GIVE, A_RECV, A_RES_A, A_RES_B, A_DISCARD = 7, 11, 15, 16, 17
# head index -> (offset, length) in the flat action
ACTION_HEAD_SLICES = [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 4), (11, 4), (15, 1), (16, 1), (17, 1)]

# ---------------------------------------------------------------- masks (float32[325])
MASK_SHAPES = [(13,), (3, 54), (73,), (19,), (5,), (2,), (3, 3), (6,), (6,), (4, 5), (5,), (5,)]
MASK_SIZES = []
for _s in MASK_SHAPES:
    _n = 1
    for _d in _s:
        _n *= _d
    MASK_SIZES.append(_n)
MASK_OFFSETS = [sum(MASK_SIZES[:i]) for i in range(len(MASK_SIZES))]
MASK_WORDS = sum(MASK_SIZES)
assert MASK_WORDS == 325
MASK_PACKED_WORDS = 11  # ceil(325 / 32) uint32 words, bit i of the flat mask -> word i>>5, bit i&31

# ---------------------------------------------------------------- obs
OBS_FLOAT_KEYS = OrderedDict([
    ("proposed_trade", (12,)),
    ("current_resources", (6,)),
    ("tile_representations", (19, 60)),
    ("current_player_main", (152,)),
    ("next_player_main", (159,)),
    ("next_next_player_main", (159,)),
    ("next_next_next_player_main", (159,)),
])
OBS_FLOAT_OFFSETS = OrderedDict()
_o = 0
for _k, _shape in OBS_FLOAT_KEYS.items():
    OBS_FLOAT_OFFSETS[_k] = _o
    _n = 1
    for _d in _shape:
        _n *= _d
    _o += _n
OBS_FLOATS = _o
assert OBS_FLOATS == 1787
OBS_LIST_KEYS = ["current_player_played_dev", "current_player_hidden_dev", "next_player_played_dev",
                 "next_next_player_played_dev", "next_next_next_player_played_dev"]
OBS_LIST_PAD = 25  # a player can hold at most the whole 25-card deck
# key order used by the reference rollout storage (RL/ppo/process_batch.py:10-13)
OBS_KEYS = ["proposed_trade", "current_resources", "tile_representations", "current_player_main",
            "current_player_played_dev", "current_player_hidden_dev", "next_player_main", "next_player_played_dev",
            "next_next_player_main", "next_next_player_played_dev", "next_next_next_player_main",
            "next_next_next_player_played_dev"]

# ---------------------------------------------------------------- state blob (int32)
def _player_fields(p):
    return [(f"p{p}_res", 5), (f"p{p}_vis", 5), (f"p{p}_opp_min", 15), (f"p{p}_opp_max", 15),
            (f"p{p}_harbours", 6), (f"p{p}_n_hidden", 1), (f"p{p}_hidden", 25), (f"p{p}_n_played", 1),
            (f"p{p}_played", 25), (f"p{p}_vp", 1)]


STATE_FIELDS = [("tile_res", 19), ("tile_val", 19), ("robber_tile", 1), ("harbour_type", 9),
                ("corner_bld", 54), ("corner_owner", 54), ("edge_owner", 72)]
for _p in (1, 2, 3, 4):
    STATE_FIELDS += _player_fields(_p)
STATE_FIELDS += [
    ("bank_res", 5), ("settlements_left", 4), ("cities_left", 4), ("pile_len", 1), ("pile", 25),
    ("player_order", 4), ("player_order_id", 1), ("players_go", 1),
    ("initial_phase", 1), ("init_settlements", 4), ("init_roads", 4), ("init_second_corner", 4),
    ("dice_rolled", 1), ("played_dev", 1), ("must_use_dev", 1), ("must_respond", 1),
    ("trade_proposer", 1), ("trade_target", 1), ("trade_n_give", 1), ("trade_give", 4),
    ("trade_n_recv", 1), ("trade_recv", 4),
    ("road_building_active", 1), ("road_building_count", 1),
    ("can_move_robber", 1), ("just_moved_robber", 1),
    ("need_discard", 1), ("n_to_discard", 1), ("to_discard", 4),
    ("die1", 1), ("die2", 1),
    ("trades_this_turn", 1), ("actions_this_turn", 1), ("turn", 1),
    ("bought_this_turn", 5),
    ("lr_player", 1), ("lr_count", 1), ("la_player", 1), ("la_count", 1),
    ("cur_longest_path", 4), ("cur_army_size", 4),
    ("curr_vps", 4), ("winner", 1),
    ("rng_draws", 1),
]
STATE_OFFSETS = OrderedDict()
_o = 0
for _name, _n in STATE_FIELDS:
    STATE_OFFSETS[_name] = (_o, _n)
    _o += _n
STATE_WORDS = _o


def state_field(blob, name):
    """View of one named field of a state blob (last axis = STATE_WORDS)."""
    off, n = STATE_OFFSETS[name]
    return blob[..., off:off + n]


def describe_state_diff(a, b, limit=12):
    """Human-readable list of differing fields between two blobs (for test failure messages)."""
    out = []
    for name, (off, n) in STATE_OFFSETS.items():
        xa, xb = a[off:off + n], b[off:off + n]
        if (xa != xb).any():
            out.append(f"{name}: {xa.tolist()} != {xb.tolist()}")
            if len(out) >= limit:
                break
    return "\n".join(out)


# ---------------------------------------------------------------- board layouts (reference game/components/board.py:23-47)
# A layout is a dict with the keyword names of the reference's Board(...) / Game(board_config=...): randomise_number_placement,
# fixed_terrain_placements (19 terrains in tile order), fixed_number_order (18 tokens along NUMBER_PLACEMENT_INDS, desert skipped).
TERRAIN_NAMES = ["Desert", "Hills", "Forest", "Mountains", "Pastures", "Fields"]        # the reference's Terrain values 0..5
TERRAIN_TO_PLACE = [0] + [1] * 3 + [5] * 4 + [2] * 4 + [3] * 3 + [4] * 4
DEFAULT_NUMBER_ORDER = [5, 2, 6, 3, 8, 10, 9, 12, 11, 4, 8, 10, 9, 4, 5, 6, 3, 11]
NUMBER_PLACEMENT_INDS = [0, 3, 7, 12, 16, 17, 18, 15, 11, 6, 2, 1, 4, 8, 13, 14, 10, 5, 9]
BOARD_CONFIG_KEYS = ("randomise_number_placement", "fixed_terrain_placements", "fixed_number_order")
MAX_BOARD_CONFIGS = 16


def terrain_code(t):
    """A terrain as its Terrain value: the value itself, the reference's Terrain member, or its name ("Hills", "hills")."""
    if isinstance(t, str):
        name = t.split(".")[-1].strip().lower()
        for code, n in enumerate(TERRAIN_NAMES):
            if n.lower() == name:
                return code
        raise ValueError(f"unknown terrain name {t!r} (one of {TERRAIN_NAMES})")
    if isinstance(t, bool) or not hasattr(t, "__index__"):
        raise ValueError(f"a terrain is a name or a Terrain value 0..5, not {t!r}")
    code = int(t)
    if not 0 <= code <= 5:
        raise ValueError(f"terrain value {code} outside 0..5 ({TERRAIN_NAMES})")
    return code


def normalise_board_config(cfg):
    """-> (randomise_number_placement: bool, terrain: list of 19 Terrain values or None, numbers: list of 18 or None).  None or {}
    is the reference's default Board().  Raises ValueError for unknown keys and for multisets other than TERRAIN_TO_PLACE /
    DEFAULT_NUMBER_ORDER (the check the reference's constructor means to make, board.py:37-42)."""
    cfg = {} if cfg is None else cfg
    if not isinstance(cfg, dict):
        raise ValueError(f"a board config is a dict with the keys {BOARD_CONFIG_KEYS}, not {type(cfg).__name__}")
    unknown = set(cfg) - set(BOARD_CONFIG_KEYS)
    if unknown:
        raise ValueError(f"unknown board config keys {sorted(unknown)} (Board's keywords: {BOARD_CONFIG_KEYS})")
    randomise = bool(cfg.get("randomise_number_placement", True))
    terrain = cfg.get("fixed_terrain_placements")
    if terrain is not None:
        terrain = [terrain_code(t) for t in terrain]
        if len(terrain) != N_TILES or sorted(terrain) != sorted(TERRAIN_TO_PLACE):
            raise ValueError(f"fixed_terrain_placements must be 19 terrains with the counts of TERRAIN_TO_PLACE "
                             f"(1 desert, 3 hills, 4 forest, 3 mountains, 4 pastures, 4 fields), got {terrain}")
    numbers = cfg.get("fixed_number_order")
    if numbers is not None:
        numbers = [int(v) for v in numbers]
        if sorted(numbers) != sorted(DEFAULT_NUMBER_ORDER):
            raise ValueError(f"fixed_number_order must be a permutation of DEFAULT_NUMBER_ORDER {DEFAULT_NUMBER_ORDER}, got {numbers}")
    return randomise, terrain, numbers


def board_config_from_state(blob):
    """The layout of an exported game (a state blob): its terrain in tile order and its tokens in placement order, read from
    tile_res / tile_val - `env.set_board_config(spec.board_config_from_state(blob))` deals that board from then on."""
    res = [int(v) for v in state_field(blob, "tile_res")]
    val = [int(v) for v in state_field(blob, "tile_val")]
    return {"randomise_number_placement": True, "fixed_terrain_placements": res,
            "fixed_number_order": [val[t] for t in NUMBER_PLACEMENT_INDS if res[t] != 0]}



# ---------------------------------------------------------------- finished-game statistics (include/catan_hip_tuning.h catan_episode_stats_*)
# the block of uint64 counters, in order: (name, words); csrc/catan_stats.hip holds the same layout as ES_* offsets
EPISODE_STATS_FIELDS = [
    ("episodes", 1), ("wins_by_player", 4), ("wins_by_turn_order", 4), ("turns_sum", 1), ("turns_sumsq", 1), ("turns_max", 1),
    ("turns_hist", 16), ("vp_sum_by_player", 4), ("winner_vp_sum", 1), ("loser_vp_sum", 1),
    ("winner_has_longest_road", 1), ("winner_has_largest_army", 1), ("games_with_longest_road", 1), ("games_with_largest_army", 1),
    ("winner_settlements_sum", 1), ("winner_cities_sum", 1), ("dev_cards_played_sum", 1),
    ("focus_episodes", 1), ("focus_wins", 1), ("focus_vp_sum", 1), ("focus_turn_order_wins", 4),
]
EPISODE_STATS_WORDS = sum(n for _, n in EPISODE_STATS_FIELDS)      # 48
EPISODE_STATS_HIST_BIN_TURNS = 32                                 # turns_hist: bin = min(turn // 32, 15)


def episode_stats_dict(words):
    """The counter block catan_episode_stats_read fills (EPISODE_STATS_WORDS integers) -> a dict: every counter by name (an int, or a
    list of ints for the indexed ones) plus the derived means, None where nothing was counted:
    mean_turns, std_turns, mean_winner_vp, mean_loser_vp (per losing player), win_rate_by_player / win_rate_by_turn_order (lists),
    longest_road_decides / largest_army_decides (share of the games whose winner holds it), mean_dev_cards_played (per game),
    focus_win_rate, focus_mean_vp."""
    w = [int(x) for x in words]
    if len(w) != EPISODE_STATS_WORDS:
        raise ValueError(f"an episode-statistics block has {EPISODE_STATS_WORDS} words, got {len(w)}")
    out, o = OrderedDict(), 0
    for name, n in EPISODE_STATS_FIELDS:
        out[name] = w[o] if n == 1 else w[o:o + n]
        o += n
    ep, fe = out["episodes"], out["focus_episodes"]
    per = lambda x, d: (x / d) if d else None
    out["mean_turns"] = per(out["turns_sum"], ep)
    var = per(out["turns_sumsq"], ep)
    out["std_turns"] = max(var - out["mean_turns"] ** 2, 0.0) ** 0.5 if ep else None
    out["mean_winner_vp"] = per(out["winner_vp_sum"], ep)
    out["mean_loser_vp"] = per(out["loser_vp_sum"], 3 * ep)
    out["win_rate_by_player"] = [per(x, ep) for x in out["wins_by_player"]]
    out["win_rate_by_turn_order"] = [per(x, ep) for x in out["wins_by_turn_order"]]
    out["longest_road_decides"] = per(out["winner_has_longest_road"], ep)
    out["largest_army_decides"] = per(out["winner_has_largest_army"], ep)
    out["mean_dev_cards_played"] = per(out["dev_cards_played_sum"], ep)
    out["focus_win_rate"] = per(out["focus_wins"], fe)
    out["focus_mean_vp"] = per(out["focus_vp_sum"], fe)
    return out


# ---------------------------------------------------------------- league results (include/catan_hip_tuning.h catan_league_stats_*)
# one row of uint64 sums per opponent net, in order; csrc/catan_league_stats.hip holds the same layout as LS_* offsets
LEAGUE_STATS_FIELDS = ["games", "seats", "net_wins", "central_wins", "net_vp_sum", "central_vp_sum"]
LEAGUE_STATS_WORDS = len(LEAGUE_STATS_FIELDS)                      # 6
# ... and the last row, the totals over every finished game
LEAGUE_STATS_TOTALS = ["games_seen", "games_tallied", "central_wins", "central_vp_sum", "games_skipped", "seats_skipped"]
LEAGUE_STATS_MAX_NETS = 65536
LEAGUE_STATS_LDS_MAX_NETS = 127                                   # up to here the kernel accumulates in LDS (LEAGUE_STATS_LDS_MAX_NETS there)
LEAGUE_STATS_REDEALS, LEAGUE_STATS_COUNT_ONLY = 1, 2              # mode bits of catan_league_stats_enable


# ---------------------------------------------------------------- start pool outcomes (include/catan_hip_tuning.h catan_start_pool_outcomes_*)
# one row of uint64 sums per pool entry and a last row for the fresh deals, behind the two head words; csrc/catan_hooks.h
# holds the same layout as PO_* offsets
START_POOL_OUTCOME_HEAD = ["seen", "skipped"]
START_POOL_OUTCOME_FIELDS = ["games", "wins_p1", "wins_p2", "wins_p3", "wins_p4", "focus_games", "focus_wins", "turns_sum"]
START_POOL_OUTCOME_WORDS = len(START_POOL_OUTCOME_FIELDS)          # 8
START_POOL_MAX_WEIGHT_SUM = 2 ** 32 - 1


def start_pool_outcomes_dict(words, m):
    """The table catan_start_pool_outcomes_read fills (2 + (m + 1) * 8 integers) -> OrderedDict: "seen", "skipped", "table" (int64 [m + 1, 8],
    the last row the fresh deals'), every START_POOL_OUTCOME_FIELDS name -> int64 [m], "fresh" -> a dict of the same names for the last row,
    and the derived float64 arrays "win_share_by_pid" [m, 4] and "focus_win_share" [m], NaN where no game was tallied."""
    import numpy as np
    t = np.asarray(words, dtype=np.int64).reshape(-1)
    m = int(m)
    if t.size != 2 + (m + 1) * START_POOL_OUTCOME_WORDS:
        raise ValueError(f"an outcome table of {m} entries has {2 + (m + 1) * START_POOL_OUTCOME_WORDS} words, got {t.size}")
    rows = t[2:].reshape(m + 1, START_POOL_OUTCOME_WORDS).copy()
    out = OrderedDict((("seen", int(t[0])), ("skipped", int(t[1])), ("table", rows)))
    for i, name in enumerate(START_POOL_OUTCOME_FIELDS):
        out[name] = rows[:m, i].copy()
    out["fresh"] = OrderedDict((name, int(rows[m, i])) for i, name in enumerate(START_POOL_OUTCOME_FIELDS))
    with np.errstate(divide="ignore", invalid="ignore"):
        games, fgames = rows[:m, 0].astype(np.float64), rows[:m, 5].astype(np.float64)
        out["win_share_by_pid"] = np.where(games[:, None] > 0, rows[:m, 1:5] / games[:, None], np.nan)
        out["focus_win_share"] = np.where(fgames > 0, rows[:m, 6] / fgames, np.nan)
    return out


def league_stats_table(words, num_nets):
    """The table catan_league_stats_read fills ((num_nets + 1) * LEAGUE_STATS_WORDS integers, or anything that reshapes to
    [num_nets + 1, LEAGUE_STATS_WORDS]) -> OrderedDict: every LEAGUE_STATS_FIELDS name -> int64 array [num_nets], and "totals" -> a
    dict of the LEAGUE_STATS_TOTALS names."""
    import numpy as np
    t = np.asarray(words, dtype=np.int64).reshape(-1)
    if t.size != (int(num_nets) + 1) * LEAGUE_STATS_WORDS:
        raise ValueError(f"a league table of {num_nets} nets has {(int(num_nets) + 1) * LEAGUE_STATS_WORDS} words, got {t.size}")
    t = t.reshape(int(num_nets) + 1, LEAGUE_STATS_WORDS)
    out = OrderedDict((name, t[:-1, i].copy()) for i, name in enumerate(LEAGUE_STATS_FIELDS))
    out["totals"] = OrderedDict((name, int(t[-1, i])) for i, name in enumerate(LEAGUE_STATS_TOTALS))
    return out


# ---------------------------------------------------------------- tournament (include/catan_hip_tuning.h catan_tourney_*)
# one row of uint64 sums per lineup; csrc/catan_hooks.h holds the same layout as TY_* offsets.  Everything behind "draws" is summed over
# the row's decided games; wins_pos / vp_pos are by lineup position, wins_turn by the winner's place in the turn order
TOURNAMENT_FIELDS = ["games", "draws", "wins_pos0", "wins_pos1", "wins_pos2", "wins_pos3", "vp_pos0", "vp_pos1", "vp_pos2", "vp_pos3",
                     "wins_turn0", "wins_turn1", "wins_turn2", "wins_turn3", "turns_sum", "spare"]
TOURNAMENT_WORDS = len(TOURNAMENT_FIELDS)                          # 16
TOURNAMENT_GAMES, TOURNAMENT_DRAWS, TOURNAMENT_WINS, TOURNAMENT_VP, TOURNAMENT_WINS_BY_TURN, TOURNAMENT_TURNS = 0, 1, 2, 6, 10, 14
# ... and the last row, the totals (TT_* there)
TOURNAMENT_TOTALS = ["seen", "tallied", "draws", "skipped_unseated", "seated", "retired"]
TOURNAMENT_MAX_LINEUPS = 65536
TOURNAMENT_LDS_MAX_LINEUPS = 63                                    # up to here the tally accumulates in LDS (TOURNEY_LDS_MAX_LINEUPS there)


# ---------------------------------------------------------------- state check (include/catan_hip_tuning.h catan_state_check)
# the rules a state blob is checked against, in bit order: bit r of a blob's uint64 word = rule r is broken.  The header restates the
# list; csrc/catan_hooks.hip holds it as SC_* bit numbers.  Necessary conditions of a legal position, not sufficient ones.
STATE_CHECK_RULES = [
    "range_board", "range_players", "range_turn", "terrain_multiset", "token_multiset", "harbour_permutation", "building_owner",
    "distance_rule", "pieces_left", "resource_conservation", "card_conservation", "army", "largest_army", "longest_road",
    "victory_points", "winner", "turn_order", "roads_attached", "initial_phase", "dice", "discard", "trade", "estimates", "bought",
    "road_building", "harbour_flags",
]
STATE_CHECK_BIT = {name: i for i, name in enumerate(STATE_CHECK_RULES)}
DEV_CARD_COUNTS = [14, 5, 2, 2, 2]                                # knights, victory points, year of plenty, road building, monopoly
RESOURCE_CARDS_EACH = 19
# harbour id (a harbour_type word) -> index of the player's harbour flag: 0 the generic 3:1, r the 2:1 harbour of Resource r
# (reference game/components/board.py:29-33)
HARBOUR_FLAG_OF_ID = [3, 4, 5, 2, 1, 0, 0, 0, 0]


# ---------------------------------------------------------------- playout player (include/catan_hip_tuning.h catan_playout_actions)
# the int64 row of one (row, candidate), in order; csrc/catan_players.h holds the same layout as PS_* offsets
PLAYOUT_STAT_FIELDS = ["valid", "sims", "finished", "wins", "score_sum", "vp_sum", "steps_sum"]
PLAYOUT_STAT_WORDS = len(PLAYOUT_STAT_FIELDS)                      # 7
PLAYOUT_MAX_CANDIDATES, PLAYOUT_MAX_PLAYOUTS = 8, 64
PLAYOUT_WIN_SCORE, PLAYOUT_VP_SCORE = 1000, 10                    # score of a playout = 1000 [p won] + 10 (vp_p - best other vp)
PLAYOUT_DRAW_SHIFT = 22                                           # playout k runs (1 + k) << 22 draws behind its root (forward_search.py's stride)
