"""Host-side mirror of the reference env interface over libcatan_hip.so.

* `VecCatanEnv`  - N games on one GPU; torch tensors in, torch tensors out (zero-copy device pointers).
* `EnvWrapper`   - single-game view with the reference's signatures (`reset() -> obs`, `step(action) ->
                   (obs, reward_dict, done, info)`, `get_action_masks() -> list of 12 np.ndarray`,
                   `save_state()/restore_state()`), reference env/wrapper.py:11-50,168-185,711-721, so that
                   RL/ppo/game_manager.py style callers keep working.
PyTorch is only plumbing here (device memory + streams); all game logic runs in the HIP kernels.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, spec


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _DeviceArray(object):
    """int32 device memory the library owns, described for torch.as_tensor (the CUDA array interface, version 2)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i4", "data": (int(ptr), False), "version": 2, "strides": None}


def _device_view(ptr, shape, device):
    """-> an int32 tensor over the library's memory at `ptr` (no copy)"""
    with torch.cuda.device(device):
        return torch.as_tensor(_DeviceArray(ptr, shape), device=device)


def board_cfg_struct(cfg):
    """a board layout dict (spec.normalise_board_config) -> catan_board_cfg_t"""
    randomise, terrain, numbers = spec.normalise_board_config(cfg)
    c = _lib.CatanBoardCfg()
    c.randomise_number_placement = int(randomise)
    c.has_fixed_terrain, c.has_fixed_numbers = int(terrain is not None), int(numbers is not None)
    for i, v in enumerate(terrain or []):
        c.terrain[i] = v
    for i, v in enumerate(numbers or []):
        c.numbers[i] = v
    return c


class VecCatanEnv(object):
    takes_game_lists = True      # export_state / import_state accept a list of game ids

    def __init__(self, num_envs, seed=0, env_id0=0, device=None, max_proposed_trades_per_turn=4, win_reward=500.0,
                 dense_reward=False, validate_actions=True, auto_reset=True, max_actions_per_turn=None, board_config=None,
                 board_config_index=None):
        """board_config / board_config_index: board layouts, as `set_board_config` takes them; the games are then dealt with them
        from the start of their streams (as the reference's Game(board_config=...) deals its first board)."""
        if not torch.cuda.is_available():
            raise _lib.CatanHipError("VecCatanEnv needs a HIP device (no CPU fallback)")
        self.L = _lib.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.n = int(num_envs)
        self.seed, self.env_id0 = int(seed), int(env_id0)
        self._reward_annealing_factor = 1.0
        self._record_slots = 0
        cfg = _lib.CatanCfg()
        self.L.catan_cfg_default(C.byref(cfg))
        cfg.max_proposed_trades_per_turn = -1 if max_proposed_trades_per_turn is None else int(max_proposed_trades_per_turn)
        cfg.win_reward = float(win_reward)
        cfg.dense_reward = int(bool(dense_reward))
        cfg.validate_actions = int(bool(validate_actions))
        cfg.auto_reset = int(bool(auto_reset))
        if max_actions_per_turn is not None and (max_actions_per_turn != max_actions_per_turn or max_actions_per_turn < 0):
            raise ValueError("max_actions_per_turn must be None (no limit) or a non-negative number")
        # env/wrapper.py:14-17,233: None -> np.inf; the test is `actions_this_turn > max_actions_per_turn` on an integer counter
        cfg.max_actions_per_turn = -1 if (max_actions_per_turn is None or max_actions_per_turn == float("inf")) \
            else int(min(max_actions_per_turn // 1, 2 ** 31 - 1))
        self.cfg = cfg
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.catan_create(C.byref(h), self.device.index or 0, self.n, seed, env_id0, C.byref(cfg)))
        self.h = h
        self.reward = torch.zeros((self.n, 4), dtype=torch.float32, device=self.device)
        self.done = torch.zeros((self.n,), dtype=torch.uint8, device=self.device)
        self.reward64 = None
        if board_config is not None:
            self.set_board_config(board_config, board_config_index)
            # catan_create dealt random boards: deal again from draw 0 of every game's stream, now with the layouts
            with torch.cuda.device(self.device):
                blobs = self.export_state()
                spec.state_field(blobs, "rng_draws").zero_()
                self.import_state(blobs)
                del blobs
                self.reset()
        elif board_config_index is not None:
            raise ValueError("board_config_index without board_config")

    def _entry(self, name):
        """-> an entry point that older builds of the library lack (_lib._OPTIONAL)"""
        if not hasattr(self.L, name):
            raise _lib.CatanHipError(f"the loaded library has no {name}")
        return getattr(self.L, name)

    def _per_game_i32(self, name, t, cols=None):
        """-> the env's own int32 device copy of a per-game argument, [n] or [n, cols]: the library reads it whenever a game finishes"""
        t = torch.as_tensor(t, device=self.device).to(torch.int32).contiguous().clone()
        if t.shape != ((self.n,) if cols is None else (self.n, cols)):
            raise ValueError(f"{name}: one PlayerId per game ({self.n}), got shape {tuple(t.shape)}" if cols is None
                             else f"{name}: shape ({self.n}, {cols}) expected, got {tuple(t.shape)}")
        return t

    def _read_u64(self, name, words, reset):
        """-> uint64 [words] (host): the counter block that entry point `name` copies out, zeroed behind the copy if `reset`; waits for the stream"""
        out = np.zeros(words, dtype=np.uint64)
        _lib.check(self._entry(name)(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset)), _stream()))
        return out

    def set_board_config(self, config_or_list, index=None):
        """Board layouts (include/catan_hip.h catan_set_board_configs): one layout or a list of up to 16, each a dict with the
        keyword names of the reference's Board (randomise_number_placement, fixed_terrain_placements - names or Terrain values -,
        fixed_number_order); index: each game's entry (n values, None = entry 0 for all).  They apply from each game's next deal;
        None or [] removes the table (fully random deals, as before)."""
        cfgs = [] if config_or_list is None else ([config_or_list] if isinstance(config_or_list, dict) else list(config_or_list))
        if len(cfgs) > spec.MAX_BOARD_CONFIGS:
            raise ValueError(f"at most {spec.MAX_BOARD_CONFIGS} board layouts per env, got {len(cfgs)}")
        arr = (_lib.CatanBoardCfg * max(1, len(cfgs)))(*[board_cfg_struct(c) for c in cfgs])
        idx = None
        if index is not None:
            if not cfgs:
                raise ValueError("a board config index without board configs")
            idx = torch.as_tensor(index, device=self.device)
            if idx.shape != (self.n,):
                raise ValueError(f"board config index: one entry per game ({self.n}), got shape {tuple(idx.shape)}")
            if bool(((idx < 0) | (idx >= len(cfgs))).any()):
                raise ValueError(f"board config index: entries must be in 0..{len(cfgs) - 1}")
            idx = idx.to(torch.uint8).contiguous()
        _lib.check(self._entry("catan_set_board_configs")(self.h, arr, len(cfgs), _ptr(idx), _stream()))

    def set_step_wave_games(self, games):
        """scheduling knob of k_step: 64 / 32 / 16 games per wave (results do not depend on it)"""
        _lib.check(self.L.catan_set_step_wave_games(self.h, int(games)))

    def enable_reward64(self):
        """Every later step also leaves its rewards UNROUNDED (the reference's Python floats, env/wrapper.py:85-112) in
        `self.reward64` (float64 [n][4]); rollout collection sums those over a turn before rounding, as
        RL/ppo/game_manager.py:94-95 does."""
        if self.reward64 is None:
            self.reward64 = torch.zeros((self.n, 4), dtype=torch.float64, device=self.device)
            _lib.check(self.L.catan_set_reward_f64_buffer(self.h, _ptr(self.reward64)))
        return self.reward64

    def enable_episode_stats(self, focus_pid=None, on=True):
        """Finished games are counted on the device from now on, from their final states and just before their re-deal
        (include/catan_hip_tuning.h catan_episode_stats_enable); the counters start at zero.  focus_pid: PlayerId 1..4 per game (0: none) of the
        seat whose own results are wanted - the env keeps an int32 copy on the device, later edits of the argument are not seen.
        on=False stops counting."""
        fn = self._entry("catan_episode_stats_enable")
        focus = self._per_game_i32("focus_pid", focus_pid) if on and focus_pid is not None else None
        _lib.check(fn(self.h, int(bool(on)), _ptr(focus), _stream()))
        self._episode_focus = focus              # (the library reads it whenever a game finishes)

    def episode_stats_words(self, reset=False):
        """-> the raw counter block (list of spec.EPISODE_STATS_WORDS ints); waits for the current stream"""
        assert int(self.L.catan_episode_stats_words()) == spec.EPISODE_STATS_WORDS
        return [int(x) for x in self._read_u64("catan_episode_stats_read", spec.EPISODE_STATS_WORDS, reset)]

    def episode_stats(self, reset=False):
        """-> dict (spec.episode_stats_dict): the counters of the games finished since statistics were enabled (or last read with reset=True)
        by name, plus the derived means (mean_turns, win_rate_by_turn_order, focus_win_rate, ...).  A game's length in decisions is not
        among them: the state does not hold it."""
        return spec.episode_stats_dict(self.episode_stats_words(reset))

    def enable_league_stats(self, slot_of_pid, net_of_slot, num_nets, on=True, count_only=False):
        """Per-opponent results of the finished games are counted on the device from now on (include/catan_hip_tuning.h "league results");
        the table starts at zero.  slot_of_pid [n,4]: the policy slot 0..3 (0: the central policy) PlayerId p+1 of each game plays;
        net_of_slot [n,3]: the net in [0, num_nets) on slots 1..3, -1 for a seat that is not tallied.  The env keeps int32 copies on the
        device (the library reads them whenever a game finishes); later edits of the arguments are not seen.
        count_only: nothing is tallied at the re-deals, only by league_stats_count (the one mode a handle without auto_reset takes).
        on=False stops counting."""
        fn = self._entry("catan_league_stats_enable")
        if not on:
            _lib.check(fn(self.h, 0, None, None, 0, _stream()))
            self._league_maps, self._league_nets = None, 0
            return
        maps = [self._per_game_i32("slot_of_pid", slot_of_pid, 4), self._per_game_i32("net_of_slot", net_of_slot, 3)]
        mode = spec.LEAGUE_STATS_COUNT_ONLY if count_only else spec.LEAGUE_STATS_REDEALS
        _lib.check(fn(self.h, mode, _ptr(maps[0]), _ptr(maps[1]), int(num_nets), _stream()))
        self._league_maps, self._league_nets = maps, int(num_nets)

    def league_stats(self, reset=False):
        """-> int64 [num_nets + 1, spec.LEAGUE_STATS_WORDS] (host): a row per net (spec.LEAGUE_STATS_FIELDS) and the totals row
        (spec.LEAGUE_STATS_TOTALS) of the games finished since the table was enabled (or last read with reset=True); waits for the
        current stream.  spec.league_stats_table names the columns."""
        rows = getattr(self, "_league_nets", 0) + 1
        assert int(self.L.catan_league_stats_words()) == spec.LEAGUE_STATS_WORDS
        out = self._read_u64("catan_league_stats_read", rows * spec.LEAGUE_STATS_WORDS, reset)
        return torch.from_numpy(out.astype(np.int64).reshape(rows, spec.LEAGUE_STATS_WORDS))

    def league_stats_count(self, games=None, count=None):
        """Adds the CURRENT records of `games` (game ids; None: games 0..count-1, count None: every game) to the league table - for
        handles whose finished games stay where they are (auto_reset=False: evaluation).  A game listed twice is counted twice."""
        g = None if games is None else torch.as_tensor(games, device=self.device).to(torch.int32).contiguous()
        m = int(g.numel()) if g is not None else (self.n if count is None else int(count))
        _lib.check(self.L.catan_league_stats_count(self.h, _ptr(g), m, _stream()))

    # ---- tournament (include/catan_hip_tuning.h "tournament"; tournament.py)
    def enable_tournament(self, lineups, num_players, episodes_per_game=0):
        """From the next reset() on every game plays one of `lineups` - int [L, 4] player ids in [0, num_players), repeats allowed, up to
        65536 rows - seated by the library's rule (no draw), every finished game is booked by who sat where, and a game
        retires (tournament_seating: lineup -1; step it with the no-op) once it has played episodes_per_game episodes (0: unlimited).
        Every game is unseated and the table zero until the caller's reset()."""
        fn = self._entry("catan_tourney_enable")
        a = np.ascontiguousarray(np.asarray(lineups.cpu() if torch.is_tensor(lineups) else lineups), dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"tournament lineups: shape [L, 4] expected, got {tuple(a.shape)}")
        _lib.check(fn(self.h, a.ctypes.data_as(C.c_void_p), int(a.shape[0]), int(num_players), int(episodes_per_game), _stream()))
        self._tourney_lineups, self._tourney_seating = int(a.shape[0]), None

    def disable_tournament(self):
        """frees the tournament's buffers: nothing of it is launched from here on"""
        _lib.check(self._entry("catan_tourney_disable")(self.h, _stream()))
        self._tourney_lineups, self._tourney_seating = 0, None

    def tournament_table(self, reset=False):
        """-> int64 [L + 1, spec.TOURNAMENT_WORDS] (host): a row per lineup (spec.TOURNAMENT_FIELDS) and the totals row
        (spec.TOURNAMENT_TOTALS) since enable_tournament (or the last read with reset=True); waits for the current stream"""
        rows = getattr(self, "_tourney_lineups", 0) + 1
        assert int(self._entry("catan_tourney_words")()) == spec.TOURNAMENT_WORDS
        out = self._read_u64("catan_tourney_read", rows * spec.TOURNAMENT_WORDS, reset)
        return torch.from_numpy(out.astype(np.int64).reshape(rows, spec.TOURNAMENT_WORDS))

    def tournament_seating(self):
        """-> (lineup_of int32 [n], pos_of_pid int32 [n, 4]): views of the library's own device arrays - the lineup each game plays (-1:
        unseated) and the lineup position PlayerId p+1 plays - current on this stream behind reset() and step(); valid until the
        tournament is enabled again or disabled"""
        if getattr(self, "_tourney_seating", None) is None:
            lp, pp = C.c_void_p(), C.c_void_p()
            _lib.check(self._entry("catan_tourney_seating")(self.h, C.byref(lp), C.byref(pp)))
            self._tourney_seating = (_device_view(lp.value, (self.n,), self.device), _device_view(pp.value, (self.n, 4), self.device))
        return self._tourney_seating

    # ---- game records (include/catan_hip_tuning.h "game records"; record.py)
    def enable_recording(self, games, capacity=8192):
        """Binds one record slot to each game of `games` (ids, each at most once; up to 4096) with room for `capacity` actions (up to
        65535); the slots start idle (arm_recording).  An empty list frees everything.  Until armed, and while off, a step costs nothing."""
        g = torch.as_tensor(games, device=self.device).to(torch.int32).contiguous().reshape(-1)
        _lib.check(self._entry("catan_record_enable")(self.h, _ptr(g) if g.numel() else None, int(g.numel()), int(capacity), _stream()))
        self._record_slots, self._record_capacity, self._record_cfg = int(g.numel()), int(capacity), {}

    def arm_recording(self, slots=None, at_deal=False):
        """slots (None: all): start recording now - the current state is the start blob - or, at_deal, from the game's next re-deal
        (auto_reset envs).  Arming discards what the slot held.  The record keeps the reward annealing factor of this moment."""
        from . import record as _record
        arr, k = None, 0
        if slots is not None:
            a = np.ascontiguousarray(np.asarray(slots).reshape(-1), dtype=np.int32)
            arr, k = a.ctypes.data_as(C.c_void_p), int(a.size)
        _lib.check(self._entry("catan_record_arm")(self.h, arr, k, _record.RECORD_AT_DEAL if at_deal else _record.RECORD_NOW, _stream()))
        cfg = _record.cfg_dict(self.cfg, self._reward_annealing_factor)
        for s in (range(self._record_slots) if slots is None else a.tolist()):
            self._record_cfg[int(s)] = cfg

    def recording_status(self):
        """-> int64 [m, 4] (host): state (record.IDLE / WAIT_DEAL / RECORDING / SEALED), game, length, flags per slot; waits for the stream"""
        out = np.zeros((max(self._record_slots, 1), 4), dtype=np.uint32)
        _lib.check(self._entry("catan_record_status")(self.h, out.ctypes.data_as(C.c_void_p), _stream()))
        return torch.from_numpy(out[:self._record_slots].astype(np.int64))

    def recordings(self, slots=None, sealed_only=True):
        """-> list of record.GameRecord, one per sealed slot of `slots` (None: all); sealed_only=False: also the slots still recording
        (final_blob None).  Waits for the stream."""
        from . import record as _record
        status = self.recording_status().numpy()
        out = []
        for s in (range(self._record_slots) if slots is None else [int(x) for x in np.asarray(slots).reshape(-1)]):
            state, game, length, flags = (int(v) for v in status[s])
            if state != _record.SEALED and (sealed_only or state != _record.RECORDING):
                continue
            if flags & _record.F_GUARD_BROKEN:
                raise _lib.CatanHipError(f"record slot {s}: the guard word behind its log was overwritten")
            rows = min(length, self._record_capacity)
            start, fin = np.zeros(spec.STATE_WORDS, dtype=np.int32), np.zeros(spec.STATE_WORDS, dtype=np.int32)
            acts, hdr = np.zeros((max(rows, 1), spec.ACTION_WORDS), dtype=np.int32), np.zeros(4, dtype=np.uint32)
            vp = lambda x: x.ctypes.data_as(C.c_void_p)
            _lib.check(self._entry("catan_record_read")(self.h, s, vp(start), vp(fin), vp(acts), vp(hdr), _stream()))
            assert int(hdr[0]) == state and int(hdr[2]) == length, (hdr, status[s])      # (nothing ran in between)
            out.append(_record.GameRecord(self.seed, self.env_id0 + game, self._record_cfg[s], start, fin if state == _record.SEALED else None,
                                          acts[:rows], length, bool(flags & _record.F_TRUNCATED), bool(flags & _record.F_FROM_DEAL)))
        return out

    # ---- start pool (include/catan_hip_tuning.h "start pool"; start_pool.py)
    def set_start_pool(self, blobs, fresh_share=0.0, weights=None, check=False):
        """From now on a game that is re-dealt (auto_reset) or dealt by reset() starts from one of `blobs` - [m, 736], numpy or tensor, the
        orientation of export_state, up to 65536 unfinished positions - except for the share `fresh_share` of deals, which stay fresh.
        The game keeps its own draw counter: the same position in two games rolls different dice.  The env keeps its own copy; the
        counters (start_pool_counts) start at zero.  A second call replaces the pool.  weights: see set_start_pool_weights (None: every
        entry is equally likely; a new pool never inherits the weights of the one it replaces).
        check=True: the blobs go through the state check first (position.check_blobs); a ValueError names the first eight that break a
        rule and the pool in force stays as it was.  The default launches nothing new."""
        fn = self._entry("catan_start_pool_set")
        share = float(fresh_share)
        if not 0.0 <= share <= 1.0:                      # (also refuses nan)
            raise ValueError(f"fresh_share must be in [0, 1], got {fresh_share}")
        b = blobs if torch.is_tensor(blobs) else torch.from_numpy(np.array(blobs, dtype=np.int32))      # (a copy: the source may be read-only)
        b = b.to(device=self.device, dtype=torch.int32)
        if b.dim() == 1:
            b = b[None]
        if b.dim() != 2 or b.shape[1] != spec.STATE_WORDS:
            raise ValueError(f"start pool blobs: shape [m, {spec.STATE_WORDS}] expected, got {tuple(b.shape)}")
        bt = b.t().contiguous()
        w = None if weights is None else self._start_pool_weights(weights, int(b.shape[0]))      # (refused before any call)
        if check:
            from . import position
            position.require_legal(bt, "set_start_pool")
        _lib.check(fn(self.h, _ptr(bt) if bt.numel() else None, int(b.shape[0]), int(round(share * 65536)), _stream()))
        if w is not None:
            _lib.check(self._entry("catan_start_pool_set_weights")(self.h, _ptr(w), _stream()))

    def _start_pool_weights(self, weights, m):
        """-> the weights as a device tensor of m uint32 values (held in int32 storage), checked on the host"""
        self._entry("catan_start_pool_set_weights")
        w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights)
        if w.dtype.kind not in "iu":
            raise ValueError(f"start pool weights must be integers, got {w.dtype}")
        if w.shape != (m,):
            raise ValueError(f"start pool weights: one per entry ({m}), got shape {tuple(w.shape)}")
        vals = [int(x) for x in w.tolist()]
        if any(x < 0 or x > 0xFFFFFFFF for x in vals):
            raise ValueError("start pool weights must be in 0..2^32-1")
        if not 1 <= sum(vals) <= spec.START_POOL_MAX_WEIGHT_SUM:
            raise ValueError(f"start pool weights must sum to 1..2^32-1, got {sum(vals)}")
        return torch.from_numpy(np.array(vals, dtype=np.uint32).view(np.int32)).to(self.device)

    def set_start_pool_weights(self, weights):
        """The installed pool's entries are drawn in proportion to `weights` from now on: an integer array or tensor of m values in
        0..2^32-1 whose sum is in 1..2^32-1 (ValueError otherwise, before any call).  An entry of weight 0 is never installed; all-ones
        weights draw exactly what the uniform pool draws.  None: uniform again.  Waits for the env's streams."""
        fn = self._entry("catan_start_pool_set_weights")
        if weights is None:
            _lib.check(fn(self.h, None, _stream()))
            return
        m = max(int(self._entry("catan_start_pool_size")(self.h)), 0)
        if m == 0:
            raise _lib.CatanHipError("set_start_pool_weights: no start pool is installed (set_start_pool)")
        _lib.check(fn(self.h, _ptr(self._start_pool_weights(weights, m)), _stream()))

    def enable_start_pool_outcomes(self, focus_pid=None, on=True):
        """The finished games are tallied on the device from now on by the pool entry they started from (include/catan_hip_tuning.h
        "start pool: weighted picks and per-entry outcomes"); the table starts at zero and every game the env holds counts as freshly
        dealt until its next deal - enable in front of the reset() that deals from the pool.  focus_pid: PlayerId 1..4 per game (0:
        none) of the seat whose own results are wanted; the env keeps an int32 copy on the device.  on=False stops the tallies."""
        fn = self._entry("catan_start_pool_outcomes_enable")
        focus = self._per_game_i32("focus_pid", focus_pid) if on and focus_pid is not None else None
        _lib.check(fn(self.h, int(bool(on)), _ptr(focus), _stream()))
        self._start_pool_focus = focus           # (the library reads it whenever a game finishes)

    def start_pool_outcomes(self, reset=False):
        """-> dict (spec.start_pool_outcomes_dict): "seen", "skipped", "table" (int64 [m + 1, 8]: a row per entry and the fresh deals' row),
        the per-entry arrays by field name (spec.START_POOL_OUTCOME_FIELDS), the "fresh" row by name, and the derived win_share_by_pid
        [m, 4] and focus_win_share [m] (NaN where no game was tallied), of the games finished since outcomes were enabled (or last read
        with reset=True); waits for the current stream"""
        assert int(self._entry("catan_start_pool_outcomes_words")()) == spec.START_POOL_OUTCOME_WORDS
        m = max(int(self._entry("catan_start_pool_size")(self.h)), 0)
        out = self._read_u64("catan_start_pool_outcomes_read", 2 + (m + 1) * spec.START_POOL_OUTCOME_WORDS, reset)
        return spec.start_pool_outcomes_dict(out.astype(np.int64), m)

    def clear_start_pool(self):
        """every later deal is fresh again, draw for draw as on an env that never had a pool"""
        _lib.check(self._entry("catan_start_pool_clear")(self.h, _stream()))

    def start_pool_counts(self, reset=False):
        """-> {"pool": deals that took a pool position, "fresh": deals that stayed fresh while the pool was installed, "per_entry": int64 [m]
        installs of each entry} since set_start_pool (or the last read with reset=True); waits for the current stream"""
        m = max(int(self._entry("catan_start_pool_size")(self.h)), 0)
        out = self._read_u64("catan_start_pool_read", 2 + m, reset)
        return {"pool": int(out[0]), "fresh": int(out[1]), "per_entry": out[2:].astype(np.int64)}

    def close(self):
        if getattr(self, "h", None):
            self.L.catan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference-shaped calls, batched
    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        _lib.check(self.L.catan_reset(self.h, _ptr(m), _stream()))

    # ---- RNG contract (A): a single-game handle on the reference's two Mersenne Twisters (include/catan_hip.h)
    def seed_mt19937(self, numpy_seed, python_seed):
        """as `np.random.seed(numpy_seed); random.seed(python_seed)` in front of the reference's EnvWrapper"""
        _lib.check(self.L.catan_seed_mt19937(self.h, int(numpy_seed) & 0xFFFFFFFF, int(python_seed) & 0xFFFFFFFF, _stream()))

    def mt19937_from_process_globals(self):
        """installs COPIES of this process's np.random / random generator states (np.random.get_state(), random.getstate()): what
        `np.random.seed(s); random.seed(s)` left there.  The library's kernels advance the copies; the process's own generators stay put."""
        import random
        kind, key, pos = np.random.get_state()[:3]
        if kind != "MT19937":
            raise ValueError("np.random is not the legacy MT19937 RandomState")
        key = np.ascontiguousarray(key, dtype=np.uint32)
        _lib.check(self.L.catan_mt19937_set_state(self.h, 0, key.ctypes.data_as(C.c_void_p), int(pos), _stream()))
        st = random.getstate()[1]
        pkey = np.array(st[:624], dtype=np.uint32)
        _lib.check(self.L.catan_mt19937_set_state(self.h, 1, pkey.ctypes.data_as(C.c_void_p), int(st[624]), _stream()))

    def reset_board_only(self):
        """Board.reset alone: the draws of the reference's Board() constructor (game/components/board.py:47)"""
        _lib.check(self.L.catan_reset_board_only(self.h, _stream()))

    def step(self, actions):
        """actions: int32 [n][18] (a negative type = no-op).  Returns (reward [n][4] float32 indexed by PlayerId-1,
        done [n] uint8) - views of buffers owned by the env, overwritten by the next step."""
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        assert a.shape == (self.n, spec.ACTION_WORDS), a.shape
        _lib.check(self.L.catan_step(self.h, _ptr(a), _ptr(self.reward), _ptr(self.done), _stream()))
        return self.reward, self.done

    STEP_COMPLETE, STEP_WAITING, STEP_NONE = 0, 1, 2       # include/catan_hip.h

    def step_deferred(self, actions, window=32, status_out=None):
        """catan_step_deferred (include/catan_hip.h): the same actions as `step`, but a game whose step needs the slow path
        (longest road, re-deal) completes it on side streams and WAITS meanwhile.  Returns (reward, done, status): status[g] == 0:
        reward / done are the result of game g's last applied action and its state is current; 1: game g is waiting (its entry
        of the next call's actions is ignored, its state must not be read).  `step_flush()` closes the sequence."""
        a = actions if (actions.dtype == torch.int32 and actions.is_contiguous() and actions.device == self.device) else \
            actions.to(device=self.device, dtype=torch.int32).contiguous()
        assert a.shape == (self.n, spec.ACTION_WORDS), a.shape
        if status_out is None:
            if getattr(self, "status", None) is None:
                self.status = torch.zeros((self.n,), dtype=torch.uint8, device=self.device)
            status_out = self.status
        _lib.check(self.L.catan_step_deferred(self.h, _ptr(a), int(window), _ptr(self.reward), _ptr(self.done), _ptr(status_out), _stream()))
        return self.reward, self.done, status_out

    def step_flush(self):
        """catan_step_flush: completes every outstanding deferred step.  status 0: a game that was waiting (reward / done valid);
        2: nothing was outstanding for it."""
        if getattr(self, "status", None) is None:
            self.status = torch.zeros((self.n,), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.catan_step_flush(self.h, _ptr(self.reward), _ptr(self.done), _ptr(self.status), _stream()))
        return self.reward, self.done, self.status

    def get_action_masks(self, out=None, games=None):
        """float32 [n][325]; slice with spec.MASK_OFFSETS / MASK_SHAPES for the 12 heads.  games (int32 [k]): catan_masks_of - row j
        = the masks of game games[j] (the first k rows of `out`)."""
        if out is None:
            out = torch.empty((self.n if games is None else games.numel(), spec.MASK_WORDS), dtype=torch.float32, device=self.device)
        if games is not None:
            _lib.check(self.L.catan_masks_of(self.h, _ptr(out), _ptr(games), games.numel(), _stream()))
            return out
        _lib.check(self.L.catan_masks(self.h, _ptr(out), _stream()))
        return out

    def get_action_masks_packed(self):
        """int32 [n][11]: the same masks as 325-bit rows (bit i of the flat mask = word i >> 5, bit i & 31)"""
        out = torch.empty((self.n, 11), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_masks_packed_copy(self.h, _ptr(out), _stream()))
        return out

    def get_action_masks_by_head(self):
        flat = self.get_action_masks()
        return [flat[:, o:o + s].reshape((self.n,) + shp)
                for o, s, shp in zip(spec.MASK_OFFSETS, spec.MASK_SIZES, spec.MASK_SHAPES)]

    def deciding_player(self):
        out = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_deciding_seat(self.h, _ptr(out), _stream()))
        return out

    def players_turn_sim(self):
        """worker.py:146-151: trade target > players_go, ignoring the discard phase (forward-search simulations)"""
        out = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_players_turn_sim(self.h, _ptr(out), _stream()))
        return out

    def sample_random_actions(self, step_idx, out=None):
        if out is None:
            out = torch.empty((self.n, spec.ACTION_WORDS), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_sample_random_actions(self.h, int(step_idx), _ptr(out), _stream()))
        return out

    SCRIPTED_STYLES = {"builder": 0, "trader": 1}      # CATAN_SCRIPTED_* (include/catan_hip_tuning.h)

    def sample_scripted_actions(self, games=None, out=None, style="builder"):
        """catan_sample_scripted_actions (include/catan_hip_tuning.h): the rule-based player's action for the deciding player of
        every game -> int32 [rows][18].  games (int32 [k]): row j is game games[j], as in get_action_masks(games=...); None: all n games.
        style: "builder"  or "trader" (8.14: it answers offers, proposes and exchanges for a goal).
        The masks must be current (they are after reset / step / import_state)."""
        if style not in self.SCRIPTED_STYLES:
            raise ValueError(f"sample_scripted_actions: style must be one of {sorted(self.SCRIPTED_STYLES)}, got {style!r}")
        if games is not None:
            games = games if (games.dtype == torch.int32 and games.is_contiguous() and games.device == self.device) else \
                games.to(device=self.device, dtype=torch.int32).contiguous()
        rows = self.n if games is None else games.numel()
        if out is None:
            out = torch.empty((rows, spec.ACTION_WORDS), dtype=torch.int32, device=self.device)
        assert out.shape == (rows, spec.ACTION_WORDS) and out.dtype == torch.int32 and out.is_contiguous(), (out.shape, out.dtype)
        if rows and style == "builder":
            _lib.check(self.L.catan_sample_scripted_actions(self.h, _ptr(games), rows, _ptr(out), _stream()))
        elif rows:
            _lib.check(self.L.catan_sample_scripted_actions_style(self.h, self.SCRIPTED_STYLES[style], _ptr(games), rows, _ptr(out), _stream()))
        return out

    TRADE_COUNT_KEYS = ("decisions", "proposals", "responses", "accepts", "rejects_illegal", "rejects_other", "goal_exchanges", "fallbacks")

    def scripted_trade_counts(self, reset=False):
        """catan_scripted_trade_counts: what the "trader" style decided since creation (or the last reset), counted on the device ->
        {key: int} over TRADE_COUNT_KEYS; all zero before the first trader call.  Synchronises the stream."""
        out = (C.c_uint64 * 8)()
        _lib.check(self.L.catan_scripted_trade_counts(self.h, out, 1 if reset else 0, _stream()))
        return {k: int(out[i]) for i, k in enumerate(self.TRADE_COUNT_KEYS)}

    def complete_action_rows(self, actions, games=None):
        """catan_complete_action_rows (include/catan_hip_tuning.h): the columns of each action row that its type does
        not use become the lowest legal index of the mask their head would apply, so that the row can be teacher-forced through
        CatanPolicy.evaluate_actions (the samplers leave them 0, which is often illegal there: -inf x 0 = NaN).  actions: int32
        [rows][18] on the device, edited IN PLACE and returned; games as in sample_scripted_actions.  The masks must be current."""
        if games is not None:
            games = games if (games.dtype == torch.int32 and games.is_contiguous() and games.device == self.device) else \
                games.to(device=self.device, dtype=torch.int32).contiguous()
        rows = self.n if games is None else games.numel()
        assert actions.shape == (rows, spec.ACTION_WORDS) and actions.dtype == torch.int32 and actions.is_contiguous() and actions.is_cuda, \
            (actions.shape, actions.dtype)
        if rows:
            _lib.check(self.L.catan_complete_action_rows(self.h, _ptr(games), rows, _ptr(actions), _stream()))
        return actions

    def playout_actions(self, sim_env, games=None, *, candidates, playouts, depth, playout_style, determinise, step_idx, return_stats=False):
        """catan_playout_actions (include/catan_hip_tuning.h) with this env as the root: per row the candidate move whose
        playouts on `sim_env` (a scratch VecCatanEnv with auto_reset=False and this env's limits) score best for the deciding player.
        candidates: (builder, trader, randoms); games as in sample_scripted_actions.  -> actions int32 [rows][18], or with return_stats
        (actions, chosen int32 [rows], stats int64 [rows][C][spec.PLAYOUT_STAT_WORDS]).  Nothing of this env changes."""
        if playout_style not in self.SCRIPTED_STYLES:
            raise ValueError(f"playout_actions: playout_style must be one of {sorted(self.SCRIPTED_STYLES)}, got {playout_style!r}")
        if games is not None:
            games = games if (games.dtype == torch.int32 and games.is_contiguous() and games.device == self.device) else \
                games.to(device=self.device, dtype=torch.int32).contiguous()
        rows = self.n if games is None else games.numel()
        builder, trader, randoms = (int(x) for x in candidates)
        cfg = _lib.CatanPlayoutCfg(builder, trader, randoms, int(playouts), int(depth), self.SCRIPTED_STYLES[playout_style], int(bool(determinise)),
                                   int(step_idx) & 0xFFFFFFFF)
        out = torch.empty((rows, spec.ACTION_WORDS), dtype=torch.int32, device=self.device)
        chosen = stats = None
        if return_stats:
            chosen = torch.empty((rows,), dtype=torch.int32, device=self.device)
            stats = torch.empty((rows, max(builder + trader + randoms, 0), spec.PLAYOUT_STAT_WORDS), dtype=torch.int64, device=self.device)
        if rows:
            _lib.check(self.L.catan_playout_actions(self.h, sim_env.h, _ptr(games), rows, C.byref(cfg), _ptr(out), _ptr(chosen), _ptr(stats), _stream()))
        return (out, chosen, stats) if return_stats else out

    def scripted_fallback_count(self):
        """decisions of sample_scripted_actions that only the rule's fall-back row could take (expected 0)"""
        return int(self.L.catan_scripted_fallback_count(self.h, _stream()))

    def random_rollout(self, step_idx0, steps):
        _lib.check(self.L.catan_random_rollout(self.h, int(step_idx0), int(steps), _stream()))

    def randomise_uncertainty(self, controlling_player):
        """Game.randomise_uncertainty for every game with controlling_player[i] in 1..4 (0: untouched), game.py:1207-1282"""
        cp = torch.as_tensor(controlling_player, device=self.device).to(torch.int32).contiguous()
        assert cp.shape == (self.n,)
        _lib.check(self.L.catan_randomise_uncertainty(self.h, _ptr(cp), _stream()))

    def missed_speculation_count(self):
        """finished games of lock-step steps that had no speculatively dealt successor (expected 0)"""
        return int(self.L.catan_missed_speculation_count(self.h, _stream()))

    def inconsistent_deal_count(self):
        return int(self.L.catan_inconsistent_deal_count(self.h, _stream()))

    def random_rollout_deferred(self, iters, window):
        """`iters` iterations of the deferred loop (include/catan_hip.h): games that need the slow path (longest road,
        re-deal) sit out until their window of `window` iterations closes; per-game trajectories are the lock-step ones."""
        _lib.check(self.L.catan_random_rollout_deferred(self.h, int(iters), int(window), _stream()))

    def policy_counters(self):
        """-> int64 [n]: decisions taken by every game in deferred rollouts (its policy-stream index)"""
        out = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_policy_counters(self.h, _ptr(out), _stream()))
        return out.long() & 0xFFFFFFFF

    def set_policy_counters(self, counters=None):
        c = None if counters is None else torch.as_tensor(counters, device=self.device).to(torch.int32).contiguous()
        _lib.check(self.L.catan_set_policy_counters(self.h, _ptr(c), _stream()))

    def set_deferred_fused(self, on):
        """which form of the deferred loop runs (include/catan_hip_tuning.h): results are identical, game for game"""
        _lib.check(self.L.catan_set_deferred_fused(self.h, int(bool(on))))

    @property
    def deferred_fused(self):
        return bool(self.L.catan_deferred_fused(self.h))

    def set_lr_budgets(self, lockstep, deferred):
        _lib.check(self.L.catan_set_lr_budgets(self.h, int(lockstep), int(deferred)))

    def slow_path_counts(self):
        """-> cumulative (tier-1 longest-road requests, requests handed to tier 2, k_lr_finish launches)"""
        out = (C.c_uint64 * 3)()
        _lib.check(self.L.catan_slow_path_counts(self.h, _stream(), out))
        return int(out[0]), int(out[1]), int(out[2])

    def set_lr_rounds(self, lockstep, deferred):
        _lib.check(self.L.catan_set_lr_rounds(self.h, int(lockstep), int(deferred)))

    def random_rollout_timed(self, step_idx0, steps, window=0):
        """-> dict of summed per-kernel milliseconds (hipEvents on the launch stream); window > 0: the deferred loop."""
        ms = (C.c_float * 5)()
        _lib.check(self.L.catan_random_rollout_timed(self.h, int(step_idx0), int(steps), int(window), _stream(), ms))
        return dict(zip(("k_sample_random", "k_step", "k_lr_finish", "k_lr_heavy", "k_reset_list"), [float(x) for x in ms]))

    def export_state(self, env_idx=None):
        """-> int32 [cnt][736] canonical blobs (host-friendly orientation)."""
        idx = None
        cnt = self.n
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, dtype=torch.int64, device=self.device).contiguous()
            cnt = idx.numel()
        blob = torch.empty((spec.STATE_WORDS, cnt), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_state_export(self.h, _ptr(blob), _ptr(idx), cnt, _stream()))
        return blob.t().contiguous()

    def import_state(self, blobs, env_idx=None, check=False):
        """blobs: [cnt, 736] (the orientation of export_state) into the games env_idx (None: games 0..cnt-1).  check=True: the blobs go
        through the state check first (position.check_blobs); a ValueError names the first eight that break a rule, and nothing else is
        launched: the games stay as they were.  The default launches nothing new."""
        b = blobs if torch.is_tensor(blobs) else torch.as_tensor(np.asarray(blobs))
        b = b.to(device=self.device, dtype=torch.int32)
        if b.dim() == 1:
            b = b[None]
        cnt = b.shape[0]
        idx = None
        if env_idx is not None:
            idx = torch.as_tensor(env_idx, dtype=torch.int64, device=self.device).contiguous()
            assert idx.numel() == cnt
        bt = b.t().contiguous()
        if check:
            from . import position
            position.require_legal(bt, "import_state")
        _lib.check(self.L.catan_state_import(self.h, _ptr(bt), _ptr(idx), cnt, _stream()))

    def check_blobs(self, blobs):
        """-> uint64 [cnt] device tensor: bit r set where blob i of `blobs` ([cnt, 736]) breaks rule spec.STATE_CHECK_RULES[r]
        (position.explain names them).  Only reads the blobs."""
        from . import position
        return position.check_blobs(blobs, self.device)

    def check_states(self, env_idx=None):
        """The state check of the live games env_idx (None: all): exports them and checks the blobs -> uint64 [cnt] device tensor, all
        zero while the engine's own state obeys the rules.  Not inside an open deferred sequence (export_state)."""
        from . import position
        return position.check_blobs(self.export_state(env_idx), self.device)

    def fork_from(self, src_env, src_idx, dst_idx=None, draw_offset=None):
        """catan_state_fork (include/catan_hip_tuning.h): this env's game dst_idx[j] (None: game j) becomes a copy of src_env's game
        src_idx[j]; draw_offset[j] (None: 0) is added to the copy's draw counter modulo 2^32.  What export_state -> an edit of the
        rng_draws word -> import_state does, without the blobs.  The same destination id twice is undefined."""
        si = torch.as_tensor(src_idx, dtype=torch.int64, device=self.device).contiguous()
        cnt = si.numel()
        di = off = None
        if dst_idx is not None:
            di = torch.as_tensor(dst_idx, dtype=torch.int64, device=self.device).contiguous()
            assert di.numel() == cnt
        if draw_offset is not None:
            off = torch.as_tensor(draw_offset, device=self.device)
            assert off.numel() == cnt
            off = off.long() & 0xFFFFFFFF                                      # the low 32 bits, as the kernel reads them (uint32)
            off = torch.where(off >= 2 ** 31, off - 2 ** 32, off).to(torch.int32).contiguous()
        _lib.check(self.L.catan_state_fork(self.h, src_env.h, _ptr(si), _ptr(di), _ptr(off), cnt, _stream()))

    def get_obs(self, out=None):
        from . import obs as _obs
        return _obs.get_obs(self, out)

    def get_obs_rows(self, dtype=torch.float32, out=None, rows=None, t=None, sel=None, dense=True, games=None):
        from . import obs as _obs
        return _obs.get_obs_rows(self, dtype, out, rows, t, sel, dense, games)

    def longest_path(self, players):
        """Game.get_longest_path for PlayerId players[i] of game i (diagnostic/test entry)."""
        p = torch.as_tensor(players, dtype=torch.int32, device=self.device).contiguous()
        out = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        _lib.check(self.L.catan_longest_path(self.h, _ptr(p), _ptr(out), _stream()))
        return out

    def invalid_action_count(self):
        return int(self.L.catan_invalid_action_count(self.h, _stream()))

    def set_reward_annealing_factor(self, f):
        _lib.check(self.L.catan_set_reward_annealing(self.h, float(f)))
        self._reward_annealing_factor = float(f)


class _GameView(object):
    """The `env.game.*` attributes the reference's callers read: players_need_to_discard,
    players_to_discard, must_respond_to_trade, proposed_trade["target_player"], players_go (game_manager.py:152-159),
    initial_settlements_placed / initial_roads_placed (evaluation/evaluation_manager.py:84-88) and
    randomise_uncertainty(player_id) (forward_search_policy/worker.py:46)."""

    def __init__(self, wrapper):
        self._w = wrapper

    def _field(self, name):
        return spec.state_field(self._w._blob(), name)

    @property
    def players_need_to_discard(self):
        return bool(self._field("need_discard")[0])

    @property
    def players_to_discard(self):
        n = int(self._field("n_to_discard")[0])
        return [int(x) for x in self._field("to_discard")[:n]]

    @property
    def must_respond_to_trade(self):
        return bool(self._field("must_respond")[0])

    @property
    def proposed_trade(self):
        if not self.must_respond_to_trade:
            return None
        ng, nr = int(self._field("trade_n_give")[0]), int(self._field("trade_n_recv")[0])
        return {"player_proposing": int(self._field("trade_proposer")[0]),
                "target_player": int(self._field("trade_target")[0]),
                "player_proposing_res": [int(x) for x in self._field("trade_give")[:ng]],
                "target_player_res": [int(x) for x in self._field("trade_recv")[:nr]]}

    @property
    def players_go(self):
        return int(self._field("players_go")[0])

    @property
    def initial_placement_phase(self):
        return bool(self._field("initial_phase")[0])

    @property
    def initial_settlements_placed(self):
        v = self._field("init_settlements")
        return {pid: int(v[pid - 1]) for pid in (1, 2, 3, 4)}

    @property
    def initial_roads_placed(self):
        v = self._field("init_roads")
        return {pid: int(v[pid - 1]) for pid in (1, 2, 3, 4)}

    def randomise_uncertainty(self, controlling_player_id):
        self._w.vec.randomise_uncertainty(torch.tensor([int(controlling_player_id)]))
        self._w._cache = None


class EnvWrapper(object):
    """Single-game view with the reference EnvWrapper signatures (env/wrapper.py:11-50)."""

    def __init__(self, interactive=False, max_actions_per_turn=None, max_proposed_trades_per_turn=4, validate_actions=True,
                 debug_mode=False, win_reward=500, dense_reward=False, policies=None, seed=0, env_id=0, rng="philox", board_config=None):
        """The reference's keyword arguments in the reference's order (env/wrapper.py:12-13) plus the game's Philox stream
        (seed, env_id).  Anything else is a TypeError, as with the reference; `interactive` / `debug_mode` / `policies` drive
        the reference's pygame display and its text log (game/game.py:30-37), which are out of scope: only their defaults.
        rng="mt19937": RNG contract (A) - the game draws from copies of THIS PROCESS's np.random / random generators as they are now
        (`np.random.seed(s); random.seed(s); env = EnvWrapper(rng="mt19937")` replays the unpatched reference draw for draw,
        tests/test_gpu_golden.py::test_mt19937_known_answer_on_the_hip_path); the constructor takes the draws of Board() and Game().
        board_config: Game(board_config=...)'s layout (game/game.py:16-17; VecCatanEnv.set_board_config), an extension keyword."""
        if interactive or debug_mode or policies is not None:
            raise NotImplementedError("EnvWrapper(interactive / debug_mode / policies): the reference's display and text log "
                                      "are not part of the batched HIP path")
        self.vec = VecCatanEnv(1, seed=seed, env_id0=env_id, max_proposed_trades_per_turn=max_proposed_trades_per_turn,
                               win_reward=win_reward, dense_reward=dense_reward, validate_actions=validate_actions,
                               auto_reset=False, max_actions_per_turn=max_actions_per_turn, board_config=board_config)
        self.max_actions_per_turn = float("inf") if max_actions_per_turn is None else max_actions_per_turn
        self.max_proposed_trades_per_turn = max_proposed_trades_per_turn
        self.win_reward, self.dense_reward = win_reward, dense_reward
        self.vec.enable_reward64()       # step() hands back the reference's Python floats (unrounded doubles)
        self.validate_actions = validate_actions
        self.game = _GameView(self)
        self._cache = None
        self._fresh = True          # catan_create already reset the game: the first reset() must not draw again
        if rng == "mt19937":
            self.vec.mt19937_from_process_globals()
            self.vec.reset_board_only()          # Board() (game/components/board.py:47)
            self.vec.reset()                     # Game.__init__ -> reset (game/game.py:40)
            self._fresh = False                  # EnvWrapper.reset() deals again, as the reference's does
        elif rng != "philox":
            raise ValueError("rng: 'philox' or 'mt19937'")
        self._reward_annealing_factor = 1.0

    @property
    def reward_annealing_factor(self):
        return self._reward_annealing_factor

    @reward_annealing_factor.setter
    def reward_annealing_factor(self, f):
        self._reward_annealing_factor = f
        self.vec.set_reward_annealing_factor(f)

    def _blob(self):
        if self._cache is None:
            self._cache = self.vec.export_state()[0].cpu().numpy()
        return self._cache

    def reset(self):
        if self._fresh:
            self._fresh = False
        else:
            self.vec.reset()
        self._cache = None
        return self._get_obs()

    def get_action_masks(self):
        flat = self.vec.get_action_masks()[0].cpu().numpy().astype(np.float64)
        return [flat[o:o + s].reshape(shp).copy()
                for o, s, shp in zip(spec.MASK_OFFSETS, spec.MASK_SIZES, spec.MASK_SHAPES)]

    def step(self, action):
        flat = np.zeros((spec.ACTION_WORDS,), dtype=np.int32)
        for h, (off, ln) in enumerate(spec.ACTION_HEAD_SLICES):
            v = np.asarray(action[h]).reshape(-1)
            flat[off:off + min(ln, len(v))] = v[:ln]
        bad0 = self.vec.invalid_action_count() if self.validate_actions else 0
        reward, done = self.vec.step(torch.from_numpy(flat).view(1, spec.ACTION_WORDS))
        self._cache = None
        if self.validate_actions and self.vec.invalid_action_count() != bad0:
            raise RuntimeError("invalid action (Game.validate_action rejects it; game/game.py:264-525)")   # reference env/wrapper.py:38-41
        r = self.vec.reward64[0].cpu().numpy()
        rew = {pid: float(r[pid - 1]) for pid in (1, 2, 3, 4)}
        return self._get_obs(), rew, bool(done[0].item()), {"log": None}

    def _get_obs(self):
        from . import obs as _obs   # the observation encoder is a separate kernel + binding
        return _obs.single_env_obs(self.vec)

    def save_state(self):
        return {"blob": self._blob().copy()}

    def restore_state(self, state):
        self.vec.import_state(state["blob"][None])
        self._cache = None

    @property
    def winner(self):
        w = int(spec.state_field(self._blob(), "winner")[0])
        return None if w == 0 else type("Winner", (), {"id": w})()

    @property
    def curr_vps(self):
        v = spec.state_field(self._blob(), "curr_vps")
        return {pid: int(v[pid - 1]) for pid in (1, 2, 3, 4)}
