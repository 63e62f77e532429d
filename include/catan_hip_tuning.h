/*
 * catan_hip_tuning.h - scheduling knobs, counters and profilers of the env kernels in libcatan_hip.so.  Benchmarks, sweeps and
 * diagnostics only (bench.py, tools): results never depend on any of them, and nothing a reference-side binding needs is
 * declared here (that is catan_hip.h).  Three sections are no knobs: "search support" (catan_state_fork), which the forward search uses,
 * "finished-game statistics" (catan_episode_stats_*), which the rollout collector uses, and "rule-based player"
 * (catan_sample_scripted_actions), a fixed-strength opponent: the reference has no such interface to replace, and catan_hip.h stays the
 * reference's boundary.  "league results" (catan_league_stats_*) is a fourth: the collector's per-opponent scoreboard; "game records"
 * (catan_record_*) a fifth: whole games recorded on the device for a step-by-step replay; "teacher labels" (catan_complete_action_rows,
 * catan_collector_label) a sixth: the rule-based player's actions as an imitation target for the learner.
 */
#ifndef CATAN_HIP_TUNING_H
#define CATAN_HIP_TUNING_H

#include "catan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scheduling knob of k_step (results do not depend on it): games per wave, 64 / 32 / 16.  With fewer games per wave there are
 * 2 / 4 waves per SIMD at 65 536 games, so that one wave's record transfers overlap the other waves' dependent-instruction
 * chains.  Default DEFAULT_STEP_WAVE_GAMES (csrc/catan_abi.hip), or the environment variable CATAN_STEP_WAVE_GAMES at creation. */
int catan_set_step_wave_games(catan_env_t* env, int32_t games);
/* tier-1 longest-road search budget (iterations) before a request is handed to tier 2: lock-step / deferred mode */
int catan_set_lr_budgets(catan_env_t* env, int32_t lockstep, int32_t deferred);
/* cumulative slow-path counters since creation (synchronises the stream): out3 = { longest-road requests handled by tier 1
 * (k_lr_finish), requests handed on to tier 2 (k_lr_heavy), k_lr_finish launches } - bench.py derives the bytes a launch moves */
int catan_slow_path_counts(catan_env_t* env, catan_stream_t stream, uint64_t* out3);
/* tier-2 longest-road search: iterations per bulk-synchronous round (work is re-shared between rounds): lock-step / deferred */
int catan_set_lr_rounds(catan_env_t* env, int32_t lockstep, int32_t deferred);
/* Game.get_longest_path(player): game/game.py:843-862 for players[i] (PlayerId) in game i -> out[i].  Diagnostic/test
 * entry; inside catan_step the same search runs as part of update_longest_road. */
int catan_longest_path(catan_env_t* env, const int32_t* players, int32_t* out, catan_stream_t stream);

/* ---- search support ----
 * dst game dst_idx[j] (NULL: game j) becomes a copy of src game src_idx[j], j < cnt.  The game stream's draw counter of the copy is the
 * source's plus draw_offset[j] modulo 2^32 (NULL: unchanged).  The destination's packed masks are valid when the call returns.
 * Equal BY DEFINITION to catan_state_export(src, src_idx) -> add draw_offset to the blob's rng_draws word -> catan_state_import(dst, dst_idx):
 * EnvWrapper.save_state() / restore_state(), env/wrapper.py:711-721, between two envs.
 * src_idx, dst_idx and draw_offset are DEVICE arrays.  A source game may appear any number of times (K simulations of one root: consecutive j
 * read the same lines).  The SAME destination id twice in one call is undefined: the copies race.  Ids are not validated on the host;
 * an entry whose source or destination id lies outside its handle copies nothing.
 * Each handle keeps its own configuration (catan_cfg_t, board-layout table); only the game moves: the 704-byte packed record as it is -
 * the longest-path cache included, which an import would invalidate and recompute to the same values - and the 44 bytes of packed masks
 * (recomputed instead when the two handles' max_proposed_trades_per_turn / max_actions_per_turn differ).  The rest of the destination's
 * side row is left as catan_state_import leaves it.
 * CATAN_EINVAL, nothing launched: a null handle or src_idx, cnt <= 0, cnt > n of dst with dst_idx NULL, dst == src, handles on different
 * devices, an open deferred sequence on either handle, a handle under the MT19937 contract on either side. */
int catan_state_fork(catan_env_t* dst, const catan_env_t* src, const int64_t* src_idx, const int64_t* dst_idx,
                     const uint32_t* draw_offset, int64_t cnt, catan_stream_t stream);

/* ---- finished-game statistics ----
 * Gathered on the device.  With auto_reset = 1 a finished game is re-dealt inside the call that ended it -
 * RL/ppo/game_manager.py:112-113 (`if done: ... env.reset()`) throws the finished game away the same way - and all the caller sees
 * of it is done = 1 and the winner's win_reward.  While statistics are enabled, every finished game is counted ONCE, from its final
 * state and just before its re-deal, on every schedule (catan_step, catan_random_rollout, catan_step_deferred / catan_step_flush,
 * catan_random_rollout_deferred in both forms); a game is counted when its re-deal is consumed, i.e. at the latest when the call that
 * reports its done flag (or the flush) returns.  Off, the default, not one kernel more is launched.
 * The block is catan_episode_stats_words() = 48 uint64 counters, all sums over the finished games unless stated otherwise:
 *    [0]      episodes
 *    [1..4]   wins_by_player          index = PlayerId-1
 *    [5..8]   wins_by_turn_order      index = the winner's position in player_order (0 = first mover)
 *    [9]      turns_sum               Game.turn of the final state
 *    [10]     turns_sumsq
 *    [11]     turns_max               a MAXIMUM
 *    [12..27] turns_hist              16 bins of 32 turns: bin = min(turn / 32, 15) (the last bin is open-ended)
 *    [28..31] vp_sum_by_player        index = PlayerId-1
 *    [32]     winner_vp_sum           [33] loser_vp_sum (the three losers together)
 *    [34]     winner_has_longest_road [35] winner_has_largest_army
 *    [36]     games_with_longest_road [37] games_with_largest_army  (somebody holds it at the end)
 *    [38]     winner_settlements_sum  settlements the winner has on the board (5 - settlements left)
 *    [39]     winner_cities_sum       cities (4 - cities left)
 *    [40]     dev_cards_played_sum    all four players
 *    [41]     focus_episodes          finished games with a focus player      [42] focus_wins      [43] focus_vp_sum
 *    [44..47] focus_turn_order_wins   index = the focus player's position in player_order, in the games he won
 * focus_pid: DEVICE int32 [n], PlayerId 1..4 per game, 0 = none, or NULL (the focus counters stay 0): the seat whose results are wanted -
 * a collector's central policy sits on another PlayerId in every game.  The array is the caller's, is read when a game finishes and must
 * stay valid until statistics are disabled or the handle destroyed.
 * A game's length in DECISIONS is not counted: the state holds actions_this_turn only, a per-game decision count would be a new field
 * for the step kernel to maintain.
 * catan_episode_stats_enable(on != 0) zeroes the block (again on every call); on == 0 stops counting.  catan_episode_stats_read copies the
 * block to HOST memory, zeroes it behind the copy when reset != 0, and synchronises the stream.  Use the stream of the handle's step calls.
 * CATAN_EINVAL: a handle with auto_reset = 0 (nothing is re-dealt: read the final states), a handle under the MT19937 contract, an open
 * deferred sequence (both calls), and catan_episode_stats_read while statistics are off. */
int32_t catan_episode_stats_words(void);
int catan_episode_stats_enable(catan_env_t* env, int on, const int32_t* focus_pid, catan_stream_t stream);
int catan_episode_stats_read(catan_env_t* env, uint64_t* out_host, int reset, catan_stream_t stream);

/* ---- league results ----
 * Who beat whom, counted on the device (csrc/catan_league_stats.hip).  A league rollout seats the central policy (policy slot 0) and up to
 * three opponent nets (slots 1..3) in every game.  While enabled with CATAN_LEAGUE_STATS_REDEALS, every finished game is tallied ONCE, from
 * its final state and just before its re-deal, at the very hook of the finished-game statistics above and on every schedule; both may be on
 * together and neither knows of the other.  Off, the default, not one kernel more is launched.
 * The maps are the caller's DEVICE arrays, are read whenever a game finishes and must stay valid until disable or catan_destroy:
 *    slot_of_pid  int32 [n][4]   the policy slot 0..3 that PlayerId p+1 of game g plays (a permutation of 0..3 per game)
 *    net_of_slot  int32 [n][3]   the net, in [0, num_nets), that plays slots 1..3 of game g; -1: the seat is not tallied
 * The table is (num_nets + 1) rows of catan_league_stats_words() = 6 uint64 sums.  Row k < num_nets, over the opponent SEATS net k held in
 * tallied games (a game is tallied if it has a winner 1..4 and a valid slot row):
 *    [0] games          finished games with net k in them (once per game, however many seats it held)
 *    [1] seats          seats it held in them
 *    [2] net_wins       ... that won
 *    [3] central_wins   ... whose game the central seat won
 *    [4] net_vp_sum     victory points of those seats
 *    [5] central_vp_sum the central seat's victory points, once per seat
 * Counting per seat keeps the pair score balanced when a net holds several seats of a game: against an equally strong net every seat wins
 * a quarter of the games, so central_wins == net_wins in expectation whether the net holds one seat or three.
 * Row num_nets, the totals:
 *    [0] finished games seen            [1] of them tallied          [2] central wins          [3] central victory points
 *    [4] games skipped (no winner, no or an invalid slot row)        [5] seats skipped (net index neither -1 nor in [0, num_nets))
 * Every index read from the maps is checked before it addresses anything.
 * catan_league_stats_enable: `on` is 0 (stop counting) or mode bits.  CATAN_LEAGUE_STATS_REDEALS tallies the re-dealt games as described
 * and needs auto_reset = 1; CATAN_LEAGUE_STATS_COUNT_ONLY alone launches nothing at the re-deals and is accepted on any handle: the table
 * is then filled by catan_league_stats_count only (evaluation handles with auto_reset = 0, whose final states stay where they are).  Every
 * call with on != 0 zeroes the table, re-allocating it when num_nets grew.
 * catan_league_stats_count tallies, with the same kernel, the CURRENT records of games[0..m-1] (DEVICE int32; NULL: games 0..m-1, m <= n)
 * into the same table, in either mode; a game listed twice is counted twice.
 * catan_league_stats_read copies the table, (num_nets + 1) * 6 words, to HOST memory, zeroes it behind the copy when reset != 0, and
 * synchronises the stream.  Use the stream of the handle's step calls.
 * CATAN_EINVAL: a null handle; CATAN_LEAGUE_STATS_REDEALS on a handle with auto_reset = 0; an open deferred sequence; a handle under the
 * MT19937 contract; num_nets < 1 or > 65536; a null map with on != 0; unknown mode bits; read and count while off; count with m < 1, or
 * m > n with games == NULL. */
#define CATAN_LEAGUE_STATS_REDEALS 1
#define CATAN_LEAGUE_STATS_COUNT_ONLY 2
int32_t catan_league_stats_words(void);
int catan_league_stats_enable(catan_env_t* env, int on, const int32_t* slot_of_pid, const int32_t* net_of_slot, int32_t num_nets,
                              catan_stream_t stream);
int catan_league_stats_read(catan_env_t* env, uint64_t* out_host, int reset, catan_stream_t stream);
int catan_league_stats_count(catan_env_t* env, const int32_t* games, int64_t m, catan_stream_t stream);

/* ---- tournament ----
 * Round-robin games of M players in lineups of four, seated and booked on the device (csrc/catan_hooks.hip).  The
 * caller passes L lineups (1..65536), each four player ids in [0, M), repeats allowed, and E, the episodes every game slot plays (0:
 * unlimited).  Per game the handle keeps
 *    lineup_of   int32 [n]      the lineup the game's current episode plays, -1: unseated
 *    pos_of_pid  int32 [n][4]   the lineup position 0..3 that PlayerId p+1 plays (-1: unseated)
 * and an episode count.  Game g opens its k-th episode (from 0) with s = (env_id0 + g) * E + k, or (env_id0 + g) + k * 2^32 when E == 0,
 * modulo 2^64: lineup s mod L, seats by the ((s div L) mod 24)-th permutation of (0, 1, 2, 3) in lexicographic order.  No draw is made;
 * every 24 L consecutive s meet every (lineup, permutation) once; the seating is that of every schedule and every sharding.  With
 * k == E > 0 the game becomes unseated for good (retired): the caller steps it with the no-op from then on.
 * Seated: by catan_reset (the selected games) and behind every re-deal of a finished game.  Booked: every finished game in front of its
 * re-deal, and every seated game catan_reset is about to deal again - without a winner, a draw.
 * The table is (L + 1) rows of catan_tourney_words() = 16 uint64 sums.  Row l < L, the games of lineup l:
 *    [0] games   [1] draws   [2..5] wins by lineup position   [6..9] victory points by lineup position
 *    [10..13] wins by the winner's place in the turn order   [14] turns   [15] spare
 * (everything from [2] on over the decided games).  Row L, the totals:
 *    [0] games seen   [1] tallied (seated, a winner)   [2] draws   [3] finished without a seating (retired games)   [4] episodes seated
 *    [5] games retired
 * catan_tourney_enable copies the lineups from HOST memory, leaves every game unseated and the table zero, and waits for the stream; the
 * caller's next catan_reset seats the games.  Enabled again it starts over.  catan_tourney_disable frees everything; off, the default,
 * not one kernel more is launched and no buffer exists.  catan_tourney_read copies the table, (L + 1) * 16 words, to HOST memory, zeroes
 * it behind the copy when reset != 0, and synchronises the stream.  catan_tourney_seating gives the two DEVICE arrays above, valid until
 * the next enable or disable; read them on the stream of the handle's step calls.
 * CATAN_EINVAL: a null handle or argument; a handle with auto_reset = 0; a handle under the MT19937 contract; an open deferred sequence
 * (not catan_tourney_seating); L outside 1..65536, M < 1, E < 0, a player id outside [0, M); read and seating while off. */
int32_t catan_tourney_words(void);
int catan_tourney_enable(catan_env_t* env, const int32_t* lineups_host, int32_t L, int32_t M, int32_t E, catan_stream_t stream);
int catan_tourney_disable(catan_env_t* env, catan_stream_t stream);
int catan_tourney_read(catan_env_t* env, uint64_t* out_host, int32_t reset, catan_stream_t stream);
int catan_tourney_seating(catan_env_t* env, int32_t** lineup_of_dev, int32_t** pos_of_pid_dev);

/* ---- state check ----
 * The rules a state blob obeys in every position legal play reaches, checked on the device before anything reads the blob as player
 * ids, tile numbers, card counts or loop bounds (csrc/catan_hooks.hip k_state_check).  Opt-in: nothing calls it unless
 * the caller does.
 * blob is a DEVICE int32 [736][cnt], the orientation of catan_state_import; viol is a DEVICE uint64 [cnt]: bit r of viol[i] is set when
 * blob i breaks rule r.  n_bad may be NULL; otherwise it is a DEVICE uint64 to which the number of blobs with viol != 0 is ADDED (the
 * caller zeroes it), so one 8-byte read answers "all good?".  No handle: no rule depends on catan_cfg_t.  One lane per blob, 2 944 bytes
 * read and 8 written per blob, at most one atomic per wave; no synchronisation.
 * CATAN_EINVAL, nothing launched: a null blob or viol, cnt <= 0.
 * THE KERNEL IS TOTAL: every int32 in every word is accepted.  A word with a range rule (bits 0..2) that lies outside its range sets
 * the range bit and IS READ AS THE LOWEST VALUE OF ITS RANGE by every other rule; no word is an index, a shift count or a loop bound
 * before that.  Cards behind a list's length and trade resources behind a count are not looked at (catan_state_import ignores them,
 * the export writes -1 there).  Words without a range rule are only compared, or summed in 64 bits.
 * Player ids are 1..4 and 0 is nobody.  The rules, in bit order (spec.STATE_CHECK_RULES):
 *    0 range_board     tile_res 0..5, tile_val 2..12, robber_tile 0..18, harbour_type 0..8, corner_bld 0..2, corner_owner / edge_owner 0..4
 *    1 range_players   n_hidden / n_played / pile_len 0..25 and the cards inside those lengths 0..4; res, vis, bank_res, opp_min, opp_max
 *                      >= 0; harbour flags 0..1; settlements_left 0..5, cities_left 0..4
 *    2 range_turn      player_order entries and players_go 1..4; winner, lr_player, la_player, trade_proposer, trade_target and the four
 *                      to_discard words 0..4; player_order_id 0..3; dice 0..6; n_to_discard, trade_n_give, trade_n_recv 0..4 and the
 *                      resources inside those counts 1..5; road_building_count 0..2; every flag word 0..1; init_settlements / init_roads
 *                      0..2; init_second_corner -1..53
 *    3 terrain_multiset       1 desert, 3 hills, 4 forest, 3 mountains, 4 pastures, 4 fields
 *    4 token_multiset         the desert holds 7, the other tiles the 18 tokens of the default order
 *    5 harbour_permutation    harbour_type is a permutation of the harbour ids 0..8
 *    6 building_owner         corner_bld != 0  <=>  corner_owner != 0
 *    7 distance_rule          no two neighbouring corners are both built
 *    8 pieces_left            per player: settlements on the board = 5 - settlements_left, cities = 4 - cities_left
 *    9 resource_conservation  bank + the four hands = 19 of each resource
 *   10 card_conservation      pile + hidden + played cards = 14 / 5 / 2 / 2 / 2 of card 0..4
 *   11 army                   cur_army_size[p] = the knights among p's played cards
 *   12 largest_army           a holder: la_count = his army >= 3 and no army is larger; none: every army < 3 and la_count = 0
 *   13 longest_road           a holder: lr_count = his cur_longest_path >= 5 and none is larger; none: lr_count = 0
 *   14 victory_points         pP_vp = settlements + 2 cities + 2 [holds LR] + 2 [holds LA] + played victory-point cards = curr_vps[P-1]
 *   15 winner                 0: every curr_vps < 10; w: curr_vps[w-1] >= 10
 *   16 turn_order             player_order is a permutation of 1..4 and players_go = player_order[player_order_id]
 *   17 roads_attached         every road shares a corner with a building or another road of its owner
 *   18 initial_phase          in it: init_settlements[p] / init_roads[p] = p's buildings / roads and dice_rolled = 0; after it: both are
 *                             2 for everyone and every building touches a road of its owner
 *   19 dice                   dice_rolled => both dice 1..6
 *   20 discard                need_discard = (n_to_discard > 0); the first n_to_discard ids are distinct players who each hold more
 *                             than 7 cards; the ids behind them are 0
 *   21 trade                  must_respond: proposer and target are two different players and the proposer holds what he offers;
 *                             otherwise proposer, target and both counts are 0
 *   22 estimates              slot l of player p is the (l+1)-th player behind p in player_order: opp_min <= that hand <= opp_max
 *   23 bought                 sum of bought_this_turn <= n_hidden of players_go
 *   24 road_building          road_building_count > 0 => road_building_active
 *   25 harbour_flags          pP_harbours[k] <=> P has a building at a harbour slot whose id maps to k (ids 0..4: Ore, Sheep, Wheat, Wood,
 *                             Brick, i.e. flags 3, 4, 5, 2, 1; ids 5..8: flag 0, the 3:1 harbours)
 * Necessary, not sufficient: a blob that passes need not be reachable by legal play.  Deliberately no rules: a cap on roads per player
 * (the reference has none), vis <= res, cur_longest_path = a fresh search (the reference keeps stale values). */
#define CATAN_STATE_CHECK_RULES 26
int32_t catan_state_check_rules(void);
int catan_state_check(const int32_t* blob, int64_t cnt, uint64_t* viol, uint64_t* n_bad, catan_stream_t stream);

/* ---- game records ----
 * Whole games recorded on the device and replayed step by step (csrc/catan_hooks.hip).  A game's draws come from Philox
 * keyed by (seed, global game id) and counted in the state itself (blob word rng_draws), so a start blob, the applied actions, the seed,
 * the game id and catan_cfg_t reproduce the game bit for bit on a fresh one-game handle (settlers_of_catan_rl_amd/record.py: replay).
 * Off, the default, not one kernel more is launched and no existing kernel's code differs.
 * m slots, each bound to one game; no game holds two.  A slot holds a header - state (0 IDLE, 1 WAIT_DEAL, 2 RECORDING, 3 SEALED), game,
 * length (actions applied), flags -, a start and a final blob (what catan_state_export gives for the game, 736 int32 each) and a log of
 * `capacity` actions of 18 int16 words with a guard word behind it: 16 + 2 x 2 944 + 36 x capacity + 4 bytes of device memory per slot
 * (300 820 bytes at capacity 8 192).
 * What is logged: every action row a stepping call (catan_step, catan_random_rollout, catan_step_deferred) applies to the slot's game while
 * the slot is RECORDING, a rejected (mask-illegal) one included - a replay rejects it again.  Not logged: the explicit no-op (negative type)
 * and, inside a deferred sequence, the row of a game that is waiting (catan_step_deferred ignores it).  Past `capacity` nothing is written,
 * CATAN_RECORD_TRUNCATED is set and the length keeps counting.  The words of a legal action are head indices below 73 and are stored exactly;
 * a word of an illegal action outside the int16 range is saturated to it (and stays illegal).
 * A RECORDING slot is SEALED - final blob written - when its game's last step is complete: with auto_reset = 1 just before the game's re-deal
 * (the hook of the finished-game statistics), else at the end of the stepping call (or catan_step_flush) that reports done = 1 for it.
 * A SEALED slot stays sealed until it is armed again: one slot holds one game at a time.
 * catan_record_enable: games is a DEVICE int32 [m] of game ids, 1 <= m <= 4096, 1 <= capacity <= 65535; every slot starts IDLE.  m = 0 frees
 *   everything and switches the recorder off.  A second enable replaces the first.  It synchronises the handle's streams.
 * catan_record_arm: slots is a HOST int32 [k] (NULL: all m slots).  CATAN_RECORD_NOW: the current state is the start blob and the slot
 *   records from the next applied action.  CATAN_RECORD_AT_DEAL (needs auto_reset = 1): the slot waits (WAIT_DEAL) for its game's next
 *   re-deal, takes the freshly dealt game as its start blob and sets CATAN_RECORD_FROM_DEAL.  Arming a slot discards what it held.
 * catan_record_status: out_host is a HOST uint32 [m][4]: state, game, length, flags.  It synchronises the stream.
 *   CATAN_RECORD_GUARD_BROKEN in the flags: the guard word behind the slot's log was overwritten (never expected).
 * catan_record_read: copies one SEALED or RECORDING slot to HOST memory: start_blob / final_blob int32 [736] (a RECORDING slot has no final
 *   blob: untouched), actions int32 [min(length, capacity)][18], out_host_header uint32 [4].  Null blob / action pointers are skipped.
 *   It synchronises the stream.
 * CATAN_EINVAL, nothing launched: a null handle; a handle under the MT19937 contract; an open deferred sequence (all four calls); m or
 * capacity out of range; a game id outside [0, n) or a game listed twice (checked on the device, one synchronisation, nothing stays
 * enabled); an unknown mode; CATAN_RECORD_AT_DEAL with auto_reset = 0; a slot outside [0, m); arm, status or read while recording is not
 * enabled; read of an IDLE or WAIT_DEAL slot.
 * Not supported: handles under the MT19937 contract, and catan_random_rollout_deferred in both of its forms (and the deferred form of
 * catan_random_rollout_timed) - its actions never exist outside k_step -, which returns CATAN_EINVAL while any slot is WAIT_DEAL or
 * RECORDING. */
#define CATAN_RECORD_NOW 0
#define CATAN_RECORD_AT_DEAL 1
#define CATAN_RECORD_TRUNCATED 1
#define CATAN_RECORD_FROM_DEAL 2
#define CATAN_RECORD_GUARD_BROKEN 4
int catan_record_enable(catan_env_t* env, const int32_t* games, int32_t m, int32_t capacity, catan_stream_t stream);
int catan_record_arm(catan_env_t* env, const int32_t* slots, int32_t k, int32_t mode, catan_stream_t stream);
int catan_record_status(catan_env_t* env, uint32_t* out_host, catan_stream_t stream);
int catan_record_read(catan_env_t* env, int32_t slot, int32_t* start_blob, int32_t* final_blob, int32_t* actions, uint32_t* out_host_header,
                      catan_stream_t stream);

/* ---- start pool ----
 * Re-dealt games started from a pool of saved positions instead of a fresh deal (csrc/catan_hooks.hip).  With no
 * pool installed, the default, not one kernel more is launched and no existing kernel's code differs.
 * catan_start_pool_set: blobs is a DEVICE int32 [736][m] (the orientation of catan_state_import), 1 <= m <= 65 536; the call keeps its own
 *   copy in the handle's packed form - per entry the record (704 bytes) and the position's side row under the handle's limits (128
 *   bytes): m x (704 + 128) bytes of device memory plus (2 + m) x 8 bytes of counters (52.5 MiB at m = 65 536) - so blobs may be freed when
 *   the call returns.  fresh_q16 in 0..65 536 is the share of deals that stay fresh, in 1/65 536ths.  The finished-position check runs on the
 *   device and synchronises the stream once; a second set replaces the pool and zeroes the counters (and then synchronises the handle's
 *   streams).  A call that fails leaves a previously installed pool as it was.
 * catan_start_pool_clear: from here on every deal is fresh again, draw for draw as on a handle that never had a pool.
 * catan_start_pool_read: out_host is a HOST uint64 [2 + m]: [0] deals that took a pool position, [1] deals that stayed fresh while the pool
 *   was installed, [2 + k] installs of entry k; integer sums.  reset != 0 zeroes them behind the copy.  It synchronises the stream.
 * catan_start_pool_size: m of the installed pool, 0 without one, -1 for a null handle.
 * The install.  Every re-deal (auto_reset = 1: inside catan_step, catan_random_rollout, catan_step_deferred / catan_step_flush) and every
 * game catan_reset deals is first dealt exactly as without a pool - the deal consumes its draws - and then, with d the game's draw counter
 * as the deal left it, id its global id (env_id0 + game) and seed the handle's:
 *   o = philox4x32_10(counter = (d, 0x504F4F4C, lo32(id), hi32(id)), key = (lo32(seed), hi32(seed)))
 *   (o[1] >> 16) < fresh_q16: the fresh deal stays.  Otherwise entry k = (o[0] * m) >> 32 is installed.
 * The game's own draws use counter word 1 = 0 and the random policy's word 1 = 1, so the block is disjoint from both and no draw is
 * consumed.  After an install catan_state_export of the game equals pool blob k with rng_draws replaced by d: the same position in two
 * games rolls different dice.  The pick depends on (seed, id, d) alone, so lock-step and deferred schedules of any window pick alike.
 * catan_create's own deal precedes any pool; catan_reset_board_only never installs.
 * Interplay.  A board-layout table (catan_set_board_configs) shapes only the deals that stay fresh: a pool position carries its own
 * board.  The finished-game statistics and the league scoreboard count a pool-started game like any other; its `turns` include the turns
 * the position already had.  A record armed CATAN_RECORD_AT_DEAL takes the installed position as its start blob.  The fresh deal under an
 * install still consumes its draws, deliberately: d and everything behind it are the same whether the deal stayed or not.
 * CATAN_EINVAL, nothing installed or changed: a null handle or null blobs (what catan_state_import refuses); m or fresh_q16 out of range; an
 * open deferred sequence (set, clear and read); a handle under the MT19937 contract; a blob of a finished game (winner != 0); read without
 * a pool.
 * Not supported: handles under the MT19937 contract, and - while a pool is installed - catan_random_rollout_deferred in both of its forms
 * and the deferred form of catan_random_rollout_timed, which return CATAN_EINVAL: there the re-deal kernel draws the fresh game's first
 * action and its place in the next pass's lists from the state the install would then replace. */
int catan_start_pool_set(catan_env_t* env, const int32_t* blobs, int32_t m, int32_t fresh_q16, catan_stream_t stream);
int catan_start_pool_clear(catan_env_t* env, catan_stream_t stream);
int catan_start_pool_read(catan_env_t* env, uint64_t* out_host, int32_t reset, catan_stream_t stream);
int32_t catan_start_pool_size(const catan_env_t* env);

/* ---- start pool: weighted picks and per-entry outcomes ----
 * (csrc/catan_hooks.hip).  Both are opt-in: with no weights set and outcomes off the install is the one described above,
 * draw for draw.
 * catan_start_pool_set_weights: weights_dev is a DEVICE uint32 [m] for the installed pool; NULL goes back to the uniform pick.  The call
 *   builds the inclusive prefix sums cum[k] = w[0] + ... + w[k] on the device (summed in 64 bits), synchronises the stream once to read
 *   their total W, and refuses W == 0 and W > 2^32 - 1 with CATAN_EINVAL, leaving the weights in force as they were.  The new table is
 *   built beside the old one and swapped in after the handle's streams have drained.  The rule: where the deal does not stay fresh,
 *   t = umulhi(o[0], W) and the entry is the smallest k with cum[k] > t (o, d and the freshness test are those of the install above).  An
 *   entry of weight 0 is never installed; with every weight 1 the rule is the uniform one bit for bit.  catan_start_pool_set drops the
 *   weights: a new pool is uniform.
 * catan_start_pool_outcomes_enable: from now on every finished game of a handle with auto_reset is added, just before its re-deal, to a
 *   table of 2 + (m + 1) x catan_start_pool_outcomes_words() uint64 sums, by the entry its episode started from.  focus_pid_dev is a
 *   caller-owned DEVICE int32 [n] (PlayerId 1..4 per game, 0: none) that is read whenever a game finishes, or NULL.  The call zeroes the
 *   table and, when it switches outcomes on, marks every game as freshly dealt: enable before the reset that deals from the pool.  It needs
 *   a pool.  on == 0 stops the tallies.  catan_start_pool_set over a pool with outcomes on keeps them on with a zeroed table of the new
 *   size and marks every game in flight as freshly dealt; catan_start_pool_clear switches them off.  catan_state_import and
 *   catan_state_fork mark the games they overwrite as freshly dealt (one small launch more, only while outcomes are on).
 * catan_start_pool_outcomes_read: out_host is a HOST uint64 [2 + (m + 1) x 8]:
 *     [0] finished games seen   [1] of them skipped (a padding game, a winner outside 1..4, an origin outside [-1, m))
 *   then a row of 8 per entry k < m and, as row m, for the games that were dealt fresh (the baseline):
 *     [0] games finished   [1..4] games won by PlayerId 1..4   [5] games with a focus PlayerId in 1..4   [6] of those, won by the focus
 *     player   [7] sum of the final turn number (the field catan_episode_stats sums as turns_sum)
 *   All are integer sums, independent of the order of arrival.  reset != 0 zeroes the table behind the copy.  It synchronises the stream.
 * All three refuse an open deferred sequence, and set_weights / outcomes_enable handles under the MT19937 contract.  A tally of the games
 * of a handle without auto_reset (a _count form like catan_league_stats_count) is not built. */
int catan_start_pool_set_weights(catan_env_t* env, const uint32_t* weights_dev, catan_stream_t stream);
int32_t catan_start_pool_outcomes_words(void);
int catan_start_pool_outcomes_enable(catan_env_t* env, int on, const int32_t* focus_pid_dev, catan_stream_t stream);
int catan_start_pool_outcomes_read(catan_env_t* env, uint64_t* out_host, int32_t reset, catan_stream_t stream);

/* ---- rule-based player ----
 * The "builder" bot (csrc/catan_scripted.hip): a deterministic scripted policy - the same state always gives the same
 * action, every action is legal under the game's masks, it never proposes a trade - decided by one lane-per-game kernel.  It decides for
 * the deciding player of catan_deciding_seat (discarder, then trade target, then players_go).
 * actions: DEVICE int32 [n_rows][18].  games == NULL: row j is game j and n_rows <= n; otherwise games is a DEVICE int32 [n_rows] and row j
 * is game games[j], as in catan_masks_of (any number of rows; a game may be listed more than once).
 * The handle's packed masks are REQUIRED to be current, exactly as for catan_sample_random_actions: the kernel reads them and does not
 * recompute them (they are current after catan_create, catan_reset, catan_step, catan_state_import, catan_state_fork and for every game
 * that is not waiting inside a catan_step_deferred sequence).  A negative or out-of-range id, and a game that waits for its deferred
 * step, gets EndTurn - the answer to the placeholder mask row catan_masks_of gives such a game; catan_step_deferred ignores it.
 * catan_scripted_fallback_count: decisions since creation that no row of the rule but its last ("any legal type") could take - expected
 * 0; synchronises the stream; -1 on a null handle or a HIP error.
 * CATAN_EINVAL, nothing launched: a null handle, null actions, n_rows <= 0, n_rows > n with games == NULL. */
int catan_sample_scripted_actions(catan_env_t* env, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream);
int64_t catan_scripted_fallback_count(catan_env_t* env, catan_stream_t stream);
/* The player's STYLES.  catan_sample_scripted_actions_style(env, style, ...) is catan_sample_scripted_actions with the
 * style chosen per call:
 *   CATAN_SCRIPTED_BUILDER (0)  the builder: the same kernel, the same bits as catan_sample_scripted_actions;
 *   CATAN_SCRIPTED_TRADER  (1)  the "trader" (csrc/catan_players.hip): the builder's table with its Respond row replaced (an offer is
 *                               accepted when it brings the hand closer to the player's goal: a city, a settlement, a road or a
 *                               development card) and two rows in front of its Exchange row (a one-for-one proposal to the weakest
 *                               opponent holding the wanted card, at most three a turn; a bank / harbour exchange of spare cards for
 *                               the goal).  Where none of the three fires its action is the builder's.  Deterministic, always legal.
 * The arguments, the required state of the masks and the answer to a bad or waiting game (EndTurn) are those of
 * catan_sample_scripted_actions.  CATAN_EINVAL, nothing launched: an unknown style, and the refusals of catan_sample_scripted_actions.
 * catan_scripted_trade_counts: the trader's decisions since creation (or the last reset), counted on the device: out[0] decisions,
 * [1] proposals, [2] offers decided, [3] accepted, [4] rejected because the player could not pay (accept illegal), [5] rejected by the
 * rule, [6] goal exchanges, [7] fall-backs (expected 0).  Bad and waiting games count nothing.  Synchronises the stream; reset != 0
 * zeroes the block behind the read.  All zero before the first trader call.  catan_scripted_fallback_count counts the builder only. */
enum { CATAN_SCRIPTED_BUILDER = 0, CATAN_SCRIPTED_TRADER = 1 };
int catan_sample_scripted_actions_style(catan_env_t* env, int32_t style, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream);
int catan_scripted_trade_counts(catan_env_t* env, uint64_t out[8], int32_t reset, catan_stream_t stream);

/* ---- the playout player (csrc/catan_players.hip) ----
 * A flat Monte-Carlo player that needs no net: per row it takes C candidate moves (the builder's, the trader's, `randoms` uniform-random
 * legal ones, in this order), plays each out K times for `depth` env steps with the rule-based player of `playout_style` in every seat,
 * on copies of the root game in a second handle, and answers with the candidate whose playouts score best for the root's deciding player p:
 *     score of one playout = 1000 * [the game finished and p won] + 10 * (vp_p - max over q != p of vp_q)      (an integer)
 * summed over the K playouts; ties go to the lowest candidate index.  A candidate that is bytewise equal to a lower-numbered one of its
 * row is a duplicate: it is not played and never chosen.
 *   root     the games that are decided; nothing of it is written, counted or drawn (it is only the source of catan_state_fork)
 *   sim      a scratch handle on the same device, created with auto_reset = 0 and the root's max_proposed_trades_per_turn and
 *            max_actions_per_turn, with at least n_rows * C * K games.  Slot (j*C + c)*K + k holds playout k of candidate c of row j.
 *            Its games are overwritten by every call and its counters (catan_scripted_trade_counts, catan_invalid_action_count,
 *            catan_inconsistent_deal_count ...) are the playouts'.  Give it a seed / env_id0 whose game ids are disjoint from the root's.
 *   games    device int32 [n_rows] or NULL, as for catan_sample_scripted_actions: NULL = row j is game j; a game may be listed twice
 *            (two independent rows); a negative or out-of-range id gets EndTurn, chosen -1 and an all-zero stats block
 *   actions  device int32 [n_rows][18]: the chosen candidates' rows
 *   chosen   device int32 [n_rows] or NULL: the chosen candidates' indices
 *   stats    device int64 [n_rows][C][CATAN_PLAYOUT_STAT_WORDS] or NULL: per candidate valid (0: a duplicate, whose row is all zero),
 *            sims, finished, wins, score sum, p's victory-point sum, steps really taken (spec.PLAYOUT_STAT_FIELDS)
 * Enqueued on `stream`, in this order: the fork with draw_offset (1 + k) << 22; the candidates, sampled on the sim handle in the slots
 * (j, c, 0); k_playout_expand; catan_randomise_uncertainty for p if `determinise`; the candidates' step; depth - 1 times the sampler of
 * playout_style, k_playout_hold (finished, duplicate and bad slots get the no-op type -1) and catan_step; k_playout_score.  The call adds
 * no host wait of its own; the first call on a sim handle allocates its workspace and, inside the samplers, their counters (one
 * synchronous memset each, once per handle).  Deterministic: equal root states, handles and cfg give equal bits.
 * Cost follows the SIM HANDLE's size, not only the call's: catan_sample_random_actions, k_playout_expand and every catan_step run over all
 * of sim's games (the slots behind n_rows * C * K get the no-op), and the builder's and the trader's candidate samplers each run over all
 * n_rows * C slots (j, c, 0) though each owns one column.  Size the sim handle for the passes it serves.
 * Neither handle may be inside an open catan_step_deferred sequence (the fork would copy games that wait for their step): a caller
 * that steps the root with catan_step_deferred flushes first, or steps with catan_step (rollout.RolloutCollector does the latter).
 * CATAN_EINVAL, nothing launched: a null handle, cfg or actions; root == sim; handles on different devices; sim with auto_reset = 1 or
 * with other turn / trade limits than root; n_rows <= 0, n_rows > root's games with games == NULL, or n_rows * C * K > sim's games;
 * builder or trader outside 0..1, randoms < 0, C outside 1..8, playouts outside 1..64, depth < 1, an unknown playout_style; a handle
 * under the MT19937 contract or inside an open catan_step_deferred sequence. */
enum { CATAN_PLAYOUT_STAT_WORDS = 7 };
typedef struct {
    int32_t builder, trader, randoms;   /* candidates: C = builder + trader + randoms, 1..8 */
    int32_t playouts;                   /* K, 1..64 */
    int32_t depth;                      /* D >= 1: env steps per playout, the candidate's own step included */
    int32_t playout_style;              /* CATAN_SCRIPTED_BUILDER / _TRADER: who plays every seat */
    int32_t determinise;                /* 1: catan_randomise_uncertainty for the root's deciding player */
    uint32_t step_idx;                  /* Philox step index of the random candidates */
} catan_playout_cfg_t;
int catan_playout_actions(catan_env_t* root, catan_env_t* sim, const int32_t* games, int64_t n_rows, const catan_playout_cfg_t* cfg,
                          int32_t* actions, int32_t* chosen, int64_t* stats, catan_stream_t stream);

/* ---- teacher labels (csrc/catan_players.hip) ----
 * catan_complete_action_rows makes any legal action row teacher-forceable through the net's heads.  The samplers (this player,
 * catan_sample_random_actions) fill only the columns their action type uses; the heads evaluate EVERY column of every row and multiply
 * the unused ones by 0, and column value 0 is often illegal under an unused head's mask (log-prob -inf, -inf x 0 = NaN).  The rule, per
 * row of type t in 0..12 (head h -> column: 1 -> 1, 2 -> 2, 3 -> 3, 4 -> 4, 5 -> 5, 6 -> 6, 9 -> 15, 10 -> 16, 11 -> 17):
 *   used, NEVER written: column 1 by Settlement / City, 2 Road, 3 MoveRobber, 4 PlayDev, 5 Respond, 6 Propose / Steal, 15 Exchange or
 *   PlayDev with YoP / Monopoly, 16 Exchange or PlayDev with YoP, 17 Discard, 7..14 Propose;
 *   every other column becomes the LOWEST LEGAL INDEX of the mask the head applies to the row (0 if that mask is empty): head 1 row 2 of
 *   its (3, 54) block, head 6 row 2 of (3, 3), head 9 row 1 of (4, 5) (row 0 for Exchange; a PlayDev row ANDs row 2 for Monopoly, 3 for
 *   YoP, else 1 - the card being column 4 after its own completion), the other heads their one row;
 *   the trade lists of a row that is not Propose, with res = the deciding player's current_resources (obs_f[12:18]): column 7 = 0 if res
 *   sums to 0, else the lowest r >= 1 with res[r] > 0; columns 8..10 = 0; column 11 = 0 if res sums to 0, else 1; columns 12..14 = 0.
 * games / n_rows as for catan_sample_scripted_actions; actions: DEVICE int32 [n_rows][18], 8-BYTE ALIGNED (the 72-byte rows are read and
 * written as 8-byte pairs; any device allocation is), edited in place.  The handle's packed masks
 * must be current.  A row is left exactly as given when its type is outside 0..12, its game id is negative or out of range, or its game
 * waits inside a catan_step_deferred sequence.  CATAN_EINVAL, nothing launched: as for catan_sample_scripted_actions. */
int catan_complete_action_rows(catan_env_t* env, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream);
/* Teacher labels in the rollout collector (catan_collector_pre / catan_collector_post of catan_hip.h).
 * labels: int32 [n][18], a teacher's action row per game for the state the net decided in.  st_teacher: int16 [T][n][18], 4-BYTE ALIGNED
 * (the 36-byte rows are written as nine 4-byte words); it gets the row of game g at the slot catan_collector_post stores the net's
 * action of the same decision in - t = min(n_act[g], T - 1), for a game whose action the env consumes in this iteration and whose
 * deciding seat is the active one.
 * Called IN FRONT OF catan_collector_post with its counters4 / flags4 / active_pid / deciding / waiting_before: it reads n_act before
 * the increment.  waiting_before may be NULL (catan_step); any other NULL pointer, n <= 0 or T <= 0: CATAN_EINVAL. */
int catan_collector_label(int64_t n, int32_t T, const int64_t* counters4, const uint8_t* flags4, const int64_t* active_pid, const int32_t* deciding,
                          const int32_t* labels, int16_t* st_teacher, const uint8_t* waiting_before, catan_stream_t stream);

/* the rollout loops with a hipEvent around every kernel launch (recorded on the stream the kernel runs on); window <= 0: the
 * lock-step loop (step_idx0 as in catan_random_rollout), window > 0: the deferred loop (step_idx0 ignored).  kernel_ms is a HOST
 * float[5] receiving the summed milliseconds of k_sample_random (which also sorts the games by action type), k_step,
 * k_lr_finish, k_lr_heavy, k_reset_list / k_install_list (bench.py roofline). */
int catan_random_rollout_timed(catan_env_t* env, uint32_t step_idx0, int64_t steps, int32_t window, catan_stream_t stream, float* kernel_ms);
/* diagnostics of the lock-step step: finished games whose speculatively dealt successor was missing and which
 * were re-dealt on the critical path instead; expected 0 (k_step's may-end filter is a superset of the games a step can end) */
int64_t catan_missed_speculation_count(catan_env_t* env, catan_stream_t stream);

/* diagnostics: copies `bytes` (multiple of 16) device to device with one kernel (k_calib_copy) - a launch with exactly
 * known HBM traffic, used to calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters (profiles/README.md) */
int catan_calib_copy(void* dst, const void* src, int64_t bytes, catan_stream_t stream);

/* phase profile (diagnostics): enable (zeroes the counters) / read.  out16 (62 words) = 8 sums then 8 maxima, 4 tier-1
 * counters, then per action type (14) the sum / count / maximum of k_step's validate+apply time.
 * Slots 0, 1, 2, 6, 7: k_step phases per wave in 100 MHz wall-clock ticks (stage-in, validate+apply, request push,
 * done/reward+masks, write-back); slots 3, 4, 5: k_reset_list (philox draws, re-deals, serial shuffle ticks);
 * tools/phase_profile.py prints them. */
int catan_profile_enable(catan_env_t* env, int on);
int catan_profile_read(catan_env_t* env, uint64_t* out16);
/* catan_profile_enable(env, 2): contention-free variant for k_step - every wave stores its own phase durations of the LAST
 * launch; out: HOST uint32 [max(ceil(n/256)*16 + 17, 7128)][8] (k_step's waves first - slots 0,1,2,6,7 as above in 100 MHz ticks, slot 5 = sort bin + 1: bins
 * 0..12 = action types, 13..16 = play_dev with card 1..4; 17 = one partial wave per bin of the sort; rows 4128.. / 6128..: k_lr_finish's requests / k_lr_heavy's
 * workgroups of the last launch at 65 536 games) */
int catan_profile_read_waves(catan_env_t* env, uint32_t* out);
/* catan_profile_enable(env, 3): as 2, but slot 2 = the wave's START time (low 32 bits of the 100 MHz wall clock at entry; the
 * phases 0, 1, 6, 7 follow it back to back) and slot 3 = where the wave ran (HW_REG_HW_ID bits 0..27 | HW_REG_XCC_ID << 28):
 * the launch's timeline - dispatch ramp, waves that share a SIMD, the tail (tools/step_timeline.py). */

/* hipRuntimeGetVersion() of the HIP runtime this process runs on, or -1 (policy._Branches keys its hipGraph work-around on it: DESIGN.md 4.6) */
int32_t catan_hip_runtime_version(void);

/* Algorithmic HBM bytes of one fused env step per stepped game, from the static_assert-ed layout constants of csrc/catan_state.h
 * (action row in, hot record in, masks + reward + done out, the ideal write-back): bench.py's roofline numerator. */
int32_t catan_step_algorithmic_bytes(void);
/* ... and of the fused-sampling step (the game's action and decision counter out of its side row, the next action and the new masks back into it) */
int32_t catan_step_fused_algorithmic_bytes(void);
/* Which form of the deferred rollout loop catan_random_rollout_deferred runs (results are identical, game for game):
 *   1 (default since round 6)  fused sampling: k_step draws each completed game's next action into its side row and appends the game to the next
 *                pass's lists (per bin CATAN_FUSED_SUBS sub-lists with a counter each, so that the launch's waves do not queue up on one address);
 *                ONE kernel per pass on the main stream, tier 1 forks once per two passes
 *   0            a sampling + sorting kernel in front of every k_step (rounds 1-5) */
int catan_set_deferred_fused(catan_env_t* env, int32_t on);
int32_t catan_deferred_fused(const catan_env_t* env);

/* Environment switches, read once per handle at catan_create (csrc/catan_abi.hip: sched_from_env; setting one afterwards does not reach an existing
 * handle).  A/B diagnostics of the schedules: results never depend on them; defaults are the measured best, DESIGN.md 4.0 /
 * profiles/r05_s5_pass_experiments.txt:
 *   CATAN_STEP_WAVE_GAMES=64|32|16, CATAN_DEFERRED_FUSED=0|1   as the setters above
 *   CATAN_STEP_BIN_ORDER=0        k_step's bins over the launch's waves in index order instead of longest-lasting first
 *   CATAN_FUSED_SUBS=s            sub-lists per sort bin in the fused-sampling loop: 1, 2, 4, 8 (default) or 16
 *   CATAN_T1_GROUP=1              the sampler form of the library's own deferred loop: one tier-1 launch per pass (on three rotating slots) instead of
 *                                 one per two passes
 *   CATAN_T1_DELAY_US=k           the fused-sampling loop: tier 1 staggered k microseconds behind the group's last k_step (default 4; 0: not staggered)
 *   CATAN_LR_SPLIT=0 | 2          tier 1 as search + lane-per-game completion never / in every schedule (default: where a launch has two passes)
 *   CATAN_LR_GRID=g               workgroups of k_lr_finish in every schedule, g >= 64 (default 4 096 inside a lock-step step and in the fused-sampling
 *                                 loop, 3 072 in the other deferred schedules)
 *   CATAN_LR_MID_BUDGET=b         budget of the middle tier of a deferred window (default 256; 0: every tier-2 request straight to k_lr_heavy)
 *   CATAN_LR_MID_HEAVY_GRID=g     workgroups of k_lr_heavy behind the middle tier, 8..256 (default 32) */

#ifdef __cplusplus
}
#endif

#endif /* CATAN_HIP_TUNING_H */
