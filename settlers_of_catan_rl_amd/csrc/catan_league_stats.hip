// catan_league_stats.hip - per-opponent results of the finished games, counted on the device (catan_league_stats_*,
// include/catan_hip_tuning.h "league results").
//
// A league rollout seats the central policy (policy slot 0) and up to three opponent nets (slots 1..3) in every game; which PlayerId plays
// which slot is the collector's policy_of_pid, which net plays a slot its opp_index.  k_league_stats runs at the hook of k_episode_stats
// (catan_stats.hip: on the stream of the kernel that consumes a re-deal list, immediately in front of it, while the listed records are still
// the final states) and adds every finished game to a table of uint64 counters with one row per net and a row of totals.
//
// Included behind every other kernel file: no existing kernel's code changes with it.
#pragma once

namespace catan {

// Columns of a net's row (restated in include/catan_hip_tuning.h and settlers_of_catan_rl_amd/spec.py LEAGUE_STATS_FIELDS) ...
constexpr int LS_GAMES = 0;              // finished games the net sat in (once per game, however many seats it held)
constexpr int LS_SEATS = 1;              // seats it held in them: the unit of every counter below
constexpr int LS_NET_WINS = 2;           // ... that won
constexpr int LS_CENTRAL_WINS = 3;       // ... whose game the central seat won
constexpr int LS_NET_VP = 4;             // victory points of those seats
constexpr int LS_CENTRAL_VP = 5;         // the central seat's points, once per seat
// ... and of the totals row (row num_nets)
constexpr int LT_SEEN = 0;               // finished games seen
constexpr int LT_TALLIED = 1;            // of them tallied: a winner 1..4 and a slot row that is a permutation of 0..3
constexpr int LT_CENTRAL_WINS = 2;
constexpr int LT_CENTRAL_VP = 3;
constexpr int LT_SKIPPED_GAMES = 4;      // no winner, no slot row (a padding game) or an invalid one
constexpr int LT_SKIPPED_SEATS = 5;      // seats of tallied games whose net index is neither -1 nor in [0, num_nets)
constexpr int LS_WORDS = 6;
constexpr int LEAGUE_STATS_GRID = 8;     // as EPISODE_STATS_GRID: a pass finishes tens of games
// The LDS budget of the on-chip table: 6 KiB = 128 rows of 6 uint64, i.e. up to 127 nets and the totals.  A league rollout has at most
// max_distinct (a few tens of) nets in play; the exact reference rule can put hundreds in play, and those tables go to HBM directly.
constexpr int LEAGUE_STATS_LDS_ROWS = 128;
constexpr int LEAGUE_STATS_LDS_MAX_NETS = LEAGUE_STATS_LDS_ROWS - 1;
constexpr int LEAGUE_STATS_MAX_NETS = 65536;

// One lane per finished game of `list` (count_p != null: its length, the arguments of k_reset_list / k_install_list; null: `count` itself;
// list == null: game r is entry r).  A lane reads its game's two map rows and, from the record, the winner and the four P_VP bytes.
// LDS_TABLE: the workgroup (one wave) accumulates in an LDS copy of the table and then issues ONE global atomic per non-zero entry;
// otherwise (num_nets > LEAGUE_STATS_LDS_MAX_NETS) every contribution is a global atomic of its own.  All counters are integer sums:
// the result does not depend on the order of arrival.
// slot_of_pid: int32 [n][4], the policy slot 0..3 of PlayerId p+1; net_of_slot: int32 [n][3], the net of slots 1..3 (-1: not tallied).
template <bool LDS_TABLE>
__global__ __launch_bounds__(64) void k_league_stats(Ctx c, const u32* __restrict__ count_p, u32 count, const i32* __restrict__ list,
                                                     const i32* __restrict__ slot_of_pid, const i32* __restrict__ net_of_slot, int num_nets,
                                                     unsigned long long* __restrict__ table) {
    __shared__ unsigned long long lds[LDS_TABLE ? LEAGUE_STATS_LDS_ROWS * LS_WORDS : 1];
    const int lane = threadIdx.x;
    if (count_p != nullptr) count = *count_p;
    if ((u32)blockIdx.x * 64u >= count) return;          // (wave-uniform: nothing listed for this wave)
    const int words = (num_nets + 1) * LS_WORDS;         // (the host launches LDS_TABLE only where this fits)
    unsigned long long* const acc = LDS_TABLE ? lds : table;
    if (LDS_TABLE) {
        for (int i = lane; i < words; i += 64) lds[i] = 0ull;
        __syncthreads();
    }
    unsigned long long* const tot = acc + (size_t)num_nets * LS_WORDS;
    for (u32 r = (u32)blockIdx.x * 64u + (u32)lane; r < count; r += gridDim.x * 64u) {
        const long e = list != nullptr ? (long)list[r] : (long)r;
        if (e < 0 || e >= c.N) continue;
        atomicAdd(&tot[LT_SEEN], 1ull);
        int winner = 0, central = -1, seat_of_slot[4] = { -1, -1, -1, -1 }, used = 0;
        if (e < c.n) {                                    // (the maps have n rows; a padding game has none)
            const St s(c.R, c.N, e);
            winner = s.b(B_WINNER);
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int sl = slot_of_pid[e * 4 + p];
                if (sl >= 0 && sl <= 3) {
                    used |= 1 << sl;
#pragma unroll
                    for (int j = 0; j < 4; j++) seat_of_slot[j] = sl == j ? p : seat_of_slot[j];
                }
            }
            central = seat_of_slot[0];
        }
        if (winner < 1 || winner > 4 || used != 15) { atomicAdd(&tot[LT_SKIPPED_GAMES], 1ull); continue; }
        const St s(c.R, c.N, e);
        int vp[4];
#pragma unroll
        for (int p = 0; p < 4; p++) vp[p] = s.pb(p, P_VP);
        int cvp = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) cvp = central == p ? vp[p] : cvp;
        const unsigned long long cwin = central == winner - 1 ? 1ull : 0ull;
        atomicAdd(&tot[LT_TALLIED], 1ull);
        if (cwin) atomicAdd(&tot[LT_CENTRAL_WINS], 1ull);
        if (cvp) atomicAdd(&tot[LT_CENTRAL_VP], (unsigned long long)cvp);
        int net[3];
#pragma unroll
        for (int j = 0; j < 3; j++) net[j] = net_of_slot[e * 3 + j];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int k = net[j];
            if (k == -1) continue;
            if (k < 0 || k >= num_nets) { atomicAdd(&tot[LT_SKIPPED_SEATS], 1ull); continue; }
            const int seat = seat_of_slot[j + 1];
            int svp = 0;
#pragma unroll
            for (int p = 0; p < 4; p++) svp = seat == p ? vp[p] : svp;
            bool first = true;
#pragma unroll
            for (int i = 0; i < 3; i++) first = first && !(i < j && net[i] == k);
            unsigned long long* const row = acc + (size_t)k * LS_WORDS;
            if (first) atomicAdd(&row[LS_GAMES], 1ull);
            atomicAdd(&row[LS_SEATS], 1ull);
            if (seat == winner - 1) atomicAdd(&row[LS_NET_WINS], 1ull);
            if (cwin) atomicAdd(&row[LS_CENTRAL_WINS], 1ull);
            if (svp) atomicAdd(&row[LS_NET_VP], (unsigned long long)svp);
            if (cvp) atomicAdd(&row[LS_CENTRAL_VP], (unsigned long long)cvp);
        }
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int i = lane; i < words; i += 64) {
            const unsigned long long v = lds[i];
            if (v != 0ull) atomicAdd(&table[i], v);
        }
    }
}

}  // namespace catan
