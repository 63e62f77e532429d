// catan_stats.hip - finished-game statistics gathered on the device (catan_episode_stats_*, include/catan_hip_tuning.h).
//
// With auto_reset a finished game is re-dealt inside the call that ended it (RL/ppo/game_manager.py:112-113 throws the finished
// env away the same way), so its final state is never seen by the caller.  Every finished game is appended to one of the re-deal
// lists pend.resets[sa][0..2] by the kernel that completes its last step (finish_step), and its record in HBM is the FINAL one
// until the consumer of that list (k_reset_list / k_install_list) overwrites it: k_step writes chunks 16..27 of the hot record
// (words 64..111: W_TURN, the control block, the four player blocks) back for every game it stepped, finished or not, and the
// slow-path completions (k_lr_finish, k_lr_complete, the tier-2 completion of k_lr_heavy) write the whole hot record back.
// k_episode_stats runs on the consumer's stream immediately in front of it and walks the same (list, counter) pair, so it sees
// every final state exactly once on every schedule.  The shadow records of speculative successors are in no such list.
//
// Included behind every other kernel file: no existing kernel's code changes with it.
#pragma once

namespace catan {

// Layout of the per-handle block of uint64 counters (catan_episode_stats_words() of them; restated in include/catan_hip_tuning.h and
// settlers_of_catan_rl_amd/spec.py EPISODE_STATS_FIELDS)
constexpr int ES_EPISODES = 0;
constexpr int ES_WINS_PLAYER = 1;        // +PlayerId-1 (4)
constexpr int ES_WINS_ORDER = 5;         // +the winner's position in player_order (4)
constexpr int ES_TURNS_SUM = 9;
constexpr int ES_TURNS_SUMSQ = 10;
constexpr int ES_TURNS_MAX = 11;         // a maximum, not a sum
constexpr int ES_TURNS_HIST = 12;        // +min(turn / ES_HIST_BIN_TURNS, 15) (16)
constexpr int ES_VP_PLAYER = 28;         // +PlayerId-1 (4)
constexpr int ES_WINNER_VP = 32;
constexpr int ES_LOSER_VP = 33;          // the three losers' points together
constexpr int ES_WINNER_LR = 34;         // the winner holds the longest road
constexpr int ES_WINNER_LA = 35;         // ... the largest army
constexpr int ES_GAMES_LR = 36;          // somebody holds the longest road
constexpr int ES_GAMES_LA = 37;
constexpr int ES_WINNER_SETTLEMENTS = 38;   // settlements the winner has on the board (5 - settlements left)
constexpr int ES_WINNER_CITIES = 39;        // cities (4 - cities left)
constexpr int ES_DEV_PLAYED = 40;        // development cards played, all four players
constexpr int ES_FOCUS_EPISODES = 41;    // finished games with a focus player
constexpr int ES_FOCUS_WINS = 42;
constexpr int ES_FOCUS_VP = 43;
constexpr int ES_FOCUS_ORDER_WINS = 44;  // +the focus player's position in player_order, where he won (4)
constexpr int ES_WORDS = 48;
constexpr int ES_HIST_BIN_TURNS = 32;
constexpr int EPISODE_STATS_GRID = 8;    // a pass finishes tens of games: 8 one-wave workgroups take 512 per round, grid-stride beyond
static_assert(ES_WORDS <= 64, "one lane per counter issues the wave's atomics");

// One lane per finished game of `list` (its length at *count_p: the arguments of k_reset_list / k_install_list).  Each lane adds its
// games' contributions up in registers, the wave sums every counter with a butterfly (the maximum with a max), lane k keeps
// counter k, and the wave issues ONE atomic per non-zero counter: ES_WORDS different addresses from ES_WORDS different lanes.
// focus: int32 [n] PlayerId per game (0: none), or null.
__global__ __launch_bounds__(64) void k_episode_stats(Ctx c, const u32* __restrict__ count_p, const i32* __restrict__ list,
                                                      const i32* __restrict__ focus, unsigned long long* __restrict__ stats) {
    const int lane = threadIdx.x;
    const u32 count = *count_p;
    if ((u32)blockIdx.x * 64u >= count) return;          // (wave-uniform: nothing listed for this wave)
    unsigned long long acc[ES_WORDS];
#pragma unroll
    for (int k = 0; k < ES_WORDS; k++) acc[k] = 0ull;
    for (u32 r = (u32)blockIdx.x * 64u + (u32)lane; r < count; r += gridDim.x * 64u) {
        const long e = list[r];
        if (e < 0 || e >= c.N) continue;
        const St s(c.R, c.N, e);
        const int winner = s.b(B_WINNER);
        if (winner < 1 || winner > 4) continue;          // (a listed game always has one: finish_step lists it when it sets B_WINNER)
        const int w0 = winner - 1;
        const int seatof = s.b(B_SEATOF);
        const unsigned long long turn = s.w(W_TURN);
        const int lr = s.b(B_LR_PLAYER), la = s.b(B_LA_PLAYER);
        int vp[4], total_vp = 0, played = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) { vp[p] = s.pb(p, P_VP); total_vp += vp[p]; played += s.pb(p, P_NPLAYED); }
        const int wseat = (seatof >> (2 * w0)) & 3;
        const int hbin = (int)(turn / ES_HIST_BIN_TURNS < 15 ? turn / ES_HIST_BIN_TURNS : 15);
        acc[ES_EPISODES] += 1;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            acc[ES_WINS_PLAYER + p] += w0 == p ? 1 : 0;
            acc[ES_WINS_ORDER + p] += wseat == p ? 1 : 0;
            acc[ES_VP_PLAYER + p] += (unsigned long long)vp[p];
        }
        acc[ES_TURNS_SUM] += turn;
        acc[ES_TURNS_SUMSQ] += turn * turn;
        acc[ES_TURNS_MAX] = acc[ES_TURNS_MAX] > turn ? acc[ES_TURNS_MAX] : turn;
#pragma unroll
        for (int b = 0; b < 16; b++) acc[ES_TURNS_HIST + b] += hbin == b ? 1 : 0;
        acc[ES_WINNER_VP] += (unsigned long long)vp[w0];
        acc[ES_LOSER_VP] += (unsigned long long)(total_vp - vp[w0]);
        acc[ES_WINNER_LR] += lr == winner ? 1 : 0;
        acc[ES_WINNER_LA] += la == winner ? 1 : 0;
        acc[ES_GAMES_LR] += lr != 0 ? 1 : 0;
        acc[ES_GAMES_LA] += la != 0 ? 1 : 0;
        acc[ES_WINNER_SETTLEMENTS] += (unsigned long long)(5 - s.pb(w0, P_SLEFT));
        acc[ES_WINNER_CITIES] += (unsigned long long)(4 - s.pb(w0, P_CLEFT));
        acc[ES_DEV_PLAYED] += (unsigned long long)played;
        const int f = focus != nullptr && e < c.n ? focus[e] : 0;
        if (f >= 1 && f <= 4) {
            const int fseat = (seatof >> (2 * (f - 1))) & 3;
            acc[ES_FOCUS_EPISODES] += 1;
            acc[ES_FOCUS_WINS] += f == winner ? 1 : 0;
            acc[ES_FOCUS_VP] += (unsigned long long)vp[f - 1];
#pragma unroll
            for (int p = 0; p < 4; p++) acc[ES_FOCUS_ORDER_WINS + p] += (f == winner && fseat == p) ? 1 : 0;
        }
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int k = 0; k < ES_WORDS; k++) {
        unsigned long long v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(v, d);
            v = k == ES_TURNS_MAX ? (v > o ? v : o) : v + o;
        }
        if (lane == k) mine = v;
    }
    if (lane < ES_WORDS && mine != 0ull) {
        if (lane == ES_TURNS_MAX) atomicMax(&stats[lane], mine);
        else atomicAdd(&stats[lane], mine);
    }
}

}  // namespace catan
