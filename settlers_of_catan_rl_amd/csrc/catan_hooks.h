// catan_hooks.h - what catan_abi.hip sees of catan_hooks.hip: the launch functions of the recorder's kernels, of the
// start pool's (8.11), of its weighted pick and outcome tallies (8.12), of the tournament's (8.16) and of the state check's (8.17), and the layouts both sides share.  catan_hooks.hip is the
// library's third translation unit and third gfx950 code object; the ABI's entry points - argument checks, the handles' fields,
// allocation, the order of the launches and synchronisations - stand in catan_abi_hooks.h, one of catan_abi.hip's host files, and launch
// through these functions.
//
// What a launch function returns.  Those an entry point calls and checks on the spot return hipGetLastError().  Those of the hooks
// that enqueue_redeal and the stepping calls run (append, seal, open, install, outcomes, origin_clear, tally, seat) return hipPeekAtLastError(): the
// hooks are void, the status stays pending for the hipGetLastError at the end of the caller's sequence, where it has always been read.
#pragma once
#include <hip/hip_runtime.h>
#include "catan_game.h"
#include "catan_state_check.h"

namespace catan {

// ---- recorder
constexpr u32 REC_IDLE = 0, REC_WAIT_DEAL = 1, REC_RECORDING = 2, REC_SEALED = 3;
constexpr u32 REC_F_TRUNCATED = 1, REC_F_FROM_DEAL = 2, REC_F_GUARD_BROKEN = 4;   // (the last one is set by the host reads only)
constexpr u32 RECORD_GUARD = 0x5EA1C0DEu;
constexpr int RECORD_MAX_SLOTS = 4096, RECORD_MAX_CAPACITY = 65535, RECORD_HDR_WORDS = 4;
constexpr int RECORD_LIST_GRID = 8;      // one lane per listed game, 512 per round, grid-stride beyond (as EPISODE_STATS_GRID)
enum { REC_H_STATE = 0, REC_H_GAME = 1, REC_H_LENGTH = 2, REC_H_FLAGS = 3 };

struct RecordBuf {
    u32* hdr;          // [m][RECORD_HDR_WORDS]
    i32* slot_of;      // [N] game -> slot, -1: none
    i32* start;        // [m][STATE_WORDS]
    i32* fin;          // [m][STATE_WORDS]
    short* log;        // [m][log_stride]: capacity rows of ACTION_WORDS int16, then the guard word
    i32* arm_list;     // [m] scratch: the slots of a catan_record_arm call
    int m, capacity;
    long log_stride;   // int16 elements per slot = capacity * ACTION_WORDS + 2
};

hipError_t record_launch_bind(long n, const i32* games, const RecordBuf& rb, u32* bad, hipStream_t stream);
hipError_t record_launch_arm(const Ctx& c, const RecordBuf& rb, const i32* slots, int k, int now, hipStream_t stream);
hipError_t record_launch_append(const Ctx& c, const RecordBuf& rb, const i32* actions, const u8* busy, hipStream_t stream);
// list != null: the games of a re-deal list (its length at *count_p); list == null: every slot, over the call's done flags
hipError_t record_launch_seal(const Ctx& c, const RecordBuf& rb, const u32* count_p, const i32* list, const u8* done, const u8* status, const i32* actions, hipStream_t stream);
hipError_t record_launch_open(const Ctx& c, const RecordBuf& rb, const u32* count_p, const i32* list, hipStream_t stream);

// ---- start pool
constexpr u32 POOL_STREAM = 0x504F4F4Cu;          // "POOL": the c1 word of the pick's Philox block
constexpr int POOL_MAX_ENTRIES = 65536;
constexpr u32 POOL_Q16_ONE = 65536u;
constexpr int POOL_LIST_GRID = 64;                // one wave per listed game, grid-stride beyond
constexpr int POOL_SEL_GRID_MAX = 4096;           // ... per game of the handle, up to this many waves
constexpr int POOL_COPY_LANES = FORK_REC_CHUNKS + 3;
static_assert(MPK_STRIDE % 4 == 0 && MASK_WORDS > 8 && MASK_WORDS <= ROW_ACT && POOL_COPY_LANES <= 64,
              "an entry's mask words are two 16-byte chunks and three words at the head of a side row; a wave copies one game");

struct StartPoolBuf {
    u32* rec;                    // [m][REC]
    u32* mask;                   // [m][MPK_STRIDE]: side rows as k_masks writes them, words 0 .. MASK_WORDS-1 are read
    unsigned long long* cnt;     // [2 + m]: pool deals, fresh deals, installs per entry
    int m;
    u32 fresh_q16;               // 0..65 536
};

// ---- its weighted pick and outcome tallies
// Columns of an entry's row of the outcome table (restated in include/catan_hip_tuning.h and spec.py START_POOL_OUTCOME_FIELDS); row m is
// the fresh deals', and two head words stand in front of the rows
constexpr int PO_GAMES = 0;              // games finished
constexpr int PO_WINS_PLAYER = 1;        // +PlayerId-1 (4)
constexpr int PO_FOCUS_GAMES = 5;        // games with a focus PlayerId in 1..4
constexpr int PO_FOCUS_WINS = 6;         // ... that the focus player won
constexpr int PO_TURNS_SUM = 7;          // sum of the final W_TURN (k_episode_stats' game length)
constexpr int PO_WORDS = 8;
constexpr int PO_HEAD_SEEN = 0, PO_HEAD_SKIPPED = 1, PO_HEAD = 2;
constexpr int POOL_OUTCOMES_GRID = 8;    // as LEAGUE_STATS_GRID: a pass finishes tens of games
constexpr int POOL_SCAN_THREADS = 1024;
static_assert(POOL_MAX_ENTRIES <= POOL_SCAN_THREADS * 64, "one workgroup scans the weights: at most 64 per thread");

struct PoolPick {
    const u32* cum;              // [m] inclusive prefix sums of the weights, or nullptr (uniform)
    u32 W;                       // their sum, cum[m - 1]
    i32* origin;                 // [n] or nullptr (outcomes off)
};

// records: m records as k_import leaves them; bad: device word, counts the finished positions (winner != 0)
hipError_t pool_launch_count_finished(const u32* records, int m, u32* bad, hipStream_t stream);
hipError_t pool_launch_scan(const u32* w, u32* cum, unsigned long long* total, int m, hipStream_t stream);
// The install behind a re-deal.  count_p != null: the games of `list` (its length at *count_p); count_p == null: the games with
// sel[g] != 0, or every game (sel == null).  pp.cum chooses the weighted pick, pp.origin the origin word.
hipError_t pool_launch_install(const Ctx& c, u32* mpk, const StartPoolBuf& pb, const PoolPick& pp, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream);
// origin int32 [n]; idx: device list of cnt games, or null (games 0..cnt-1)
hipError_t pool_launch_origin_clear(i32* origin, long n, const long* idx, long cnt, hipStream_t stream);
// focus: device int32 [n] PlayerId per game (0: none), or null; table: 2 + (m + 1) x PO_WORDS uint64 sums
hipError_t pool_launch_outcomes(const Ctx& c, const u32* count_p, const i32* list, const i32* origin, const i32* focus, unsigned long long* table, int m, hipStream_t stream);

// ---- tournament
// Columns of a lineup's row of the table (restated in include/catan_hip_tuning.h and spec.py TOURNAMENT_FIELDS); row L is the totals'.
// Every column but the first two is a sum over the row's DECIDED games (games - draws).
constexpr int TY_GAMES = 0;              // finished games of the lineup
constexpr int TY_DRAWS = 1;              // ... without a winner: reset before their end
constexpr int TY_WINS = 2;               // +lineup position (4)
constexpr int TY_VP = 6;                 // +lineup position (4): victory points
constexpr int TY_WINS_BY_TURN = 10;      // +the winner's place in player_order (4)
constexpr int TY_TURNS = 14;             // sum of the final W_TURN
constexpr int TY_SPARE = 15;
constexpr int TY_WORDS = 16;
constexpr int TT_SEEN = 0;               // games the tally was handed
constexpr int TT_TALLIED = 1;            // of them seated, with a winner 1..4
constexpr int TT_DRAWS = 2;              // seated, without a winner
constexpr int TT_SKIPPED_UNSEATED = 3;   // finished without a seating (retired games, padding games)
constexpr int TT_SEATED = 4;             // episodes opened by the seat hook
constexpr int TT_RETIRED = 5;            // games retired by it: each game once
constexpr int TOURNEY_MAX_LINEUPS = 65536;
// The LDS budget of the on-chip table: 8 KiB = 64 rows of 16 uint64, i.e. up to 63 lineups and the totals (all_lineups(6) is 15 rows,
// versus_anchors of a candidate and three anchors 4); a larger table - all_lineups(8) is 70 - goes to HBM directly.
constexpr int TOURNEY_LDS_ROWS = 64;
constexpr int TOURNEY_LDS_MAX_LINEUPS = TOURNEY_LDS_ROWS - 1;
constexpr int TOURNEY_GRID = 8;          // as LEAGUE_STATS_GRID: a pass finishes tens of games
constexpr int TOURNEY_SEL_GRID_MAX = 1024;   // catan_reset's forms: one lane per game of the handle, up to this many waves

struct TourneyBuf {
    const i32* lineups;          // [L][4] player ids
    i32* lineup_of;              // [n] the game's lineup, -1: unseated
    i32* pos_of_pid;             // [n][4] the lineup position 0..3 that PlayerId p+1 plays (-1: unseated)
    u32* episode;                // [n] episodes opened so far; E + 1 once retired
    unsigned long long* table;   // [(L + 1)][TY_WORDS]
    int L;
    u32 E;                       // episodes per game slot, 0: unlimited
};

// The tally in front of a re-deal and the seating behind it.  count_p != null: the games of `list` (its length at *count_p); count_p ==
// null: the games with sel[g] != 0, or every game (sel == null) - catan_reset's forms, where an unseated game is no finished one and is
// passed over.
hipError_t tourney_launch_tally(const Ctx& c, const TourneyBuf& tb, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream);
hipError_t tourney_launch_seat(const Ctx& c, const TourneyBuf& tb, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream);

// ---- state check
// blob: device int32 [STATE_WORDS][cnt]; viol: device uint64 [cnt]; n_bad: device word that the number of blobs with viol != 0 is added to, or null
hipError_t state_check_launch(const i32* blob, long cnt, u64* viol, unsigned long long* n_bad, hipStream_t stream);

}  // namespace catan
