// catan_players.h - what catan_abi.hip sees of catan_players.hip: the launch functions of the teacher's kernels, the
// trader (8.14) and the playout player (8.15), and the layouts both sides share.  catan_players.hip is the library's second translation
// unit and second gfx950 code object (the reason stands at its top); the ABI's entry points - argument checks, the handles' fields, the
// order of the launches - stand in catan_abi_players.h, one of catan_abi.hip's host files, and launch through these functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace catan {

// ---- teacher
constexpr int IMIT_WORDS = 33, IMIT_PART = 30;       // the read-out block of k_imitation_loss; partial q of a workgroup = word q + 2
constexpr int IMIT_BLOCKS = 256, IMIT_THREADS = 256; // its grid is capped at IMIT_BLOCKS workgroups; workspace = IMIT_PART * IMIT_BLOCKS + 1 doubles

// records: the handle's game records (Ctx::R), n its games, mpk its side rows; busy: null outside a deferred sequence
hipError_t teacher_launch_complete(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                   int32_t* actions, hipStream_t stream);
hipError_t teacher_launch_label(long n, int T, const long long* n_act, const uint8_t* live, const long long* active_pid, const int32_t* deciding,
                                const uint8_t* waiting_before, const int32_t* labels, short* st_teacher, hipStream_t stream);
hipError_t teacher_launch_imitation(const float* lp, const long long* teacher, long B, float* loss, float* dlp, double* block, double* workspace,
                                    hipStream_t stream);

// ---- trader
// the counter block of the trader (catan_scripted_trade_counts): one uint64 each
enum { TC_DECISIONS = 0, TC_PROPOSALS = 1, TC_RESPONSES = 2, TC_ACCEPTS = 3, TC_REJECT_ILLEGAL = 4, TC_REJECT_OTHER = 5, TC_EXCHANGES = 6,
       TC_FALLBACKS = 7, TC_WORDS = 8 };

// records, n, mpk, busy: as above; counts: device uint64 [TC_WORDS]
hipError_t trader_launch_sample(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                int32_t* actions, unsigned long long* counts, hipStream_t stream);

// ---- playout player
// the int64 row of one (row, candidate): restated in include/catan_hip_tuning.h and spec.PLAYOUT_STAT_FIELDS
enum { PS_VALID = 0, PS_SIMS = 1, PS_FINISHED = 2, PS_WINS = 3, PS_SCORE_SUM = 4, PS_VP_SUM = 5, PS_STEPS_SUM = 6, PS_WORDS = 7 };
constexpr int PLAYOUT_MAX_CANDIDATES = 8, PLAYOUT_MAX_PLAYOUTS = 64;

// The shape of one call.  Sim slot s = (j*C + c)*K + k holds playout k of candidate c of row j; `used` = rows*C*K slots are in use.
struct PlayoutShape {
    long rows;          // rows of the call
    long used;          // rows * C * K
    long sim_n;         // games of the sim handle (>= used)
    int C, K;           // candidates per row (builder + trader + randoms), playouts per candidate
    int n_builder;      // candidates [0, n_builder) are the builder's, [n_builder, n_builder + n_trader) the trader's, the rest random
    int n_trader;
    int determinise;
};

// The sim handle's workspace (device arrays, allocated once per handle for its sim_n games at the first call)
struct PlayoutWs {
    long long* src_idx;     // [sim_n]      the root game slot s is forked from, -1: a bad row (catan_state_fork copies nothing)
    uint32_t* draw_off;     // [sim_n]      (1 + k) << 22
    int32_t* slot0;         // [sim_n]      entry j*C + c: the slot (j, c, 0), the `games` of the candidate samplers
    int32_t* by_builder;    // [sim_n][18]  row j*C + c: the builder's action in slot (j, c, 0)
    int32_t* by_trader;     // [sim_n][18]  ... the trader's
    int32_t* by_random;     // [sim_n][18]  row s: the random sampler's action in slot s
    int32_t* act;           // [sim_n][18]  the action rows of the step in flight
    int32_t* cand;          // [sim_n][18]  cand[rows][C][18]
    int32_t* ctrl;          // [sim_n]      catan_randomise_uncertainty's controlling players
    int32_t* steps;         // [sim_n]      steps slot s really took
    int32_t* rpid;          // [sim_n]      entry j: the root's deciding PlayerId, 0: a bad row
    uint8_t* held;          // [sim_n]      the latch: 1 = slot s steps no more
    uint8_t* dup;           // [sim_n]      entry j*C + c: candidate c of row j repeats a lower-numbered one
};

hipError_t playout_launch_slots(const PlayoutShape& sh, const int32_t* games, long root_n, const PlayoutWs& ws, hipStream_t stream);
// sim_records: the sim handle's game records (Ctx::R)
hipError_t playout_launch_expand(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, hipStream_t stream);
// done: the uint8 [sim_n] of the step before
hipError_t playout_launch_hold(const PlayoutShape& sh, const uint8_t* done, const PlayoutWs& ws, hipStream_t stream);
// actions int32 [rows][18]; chosen int32 [rows] or null; stats int64 [rows][C][PS_WORDS] or null
hipError_t playout_launch_score(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, int32_t* actions, int32_t* chosen,
                                long long* stats, hipStream_t stream);

}  // namespace catan
