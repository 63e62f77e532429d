// catan_players.hip - the players that read the games themselves, and what makes a training signal of them: the teacher's kernels
// (DESIGN.md 8.13), the rule-based "trader" (8.14) and the flat Monte-Carlo playout player (8.15).  All opt-in: nothing here is launched
// unless a teacher, the trader's style or a playout player is configured.
//
// The library's SECOND translation unit (compiled beside catan_abi.hip by _lib.build_library) and its second gfx950 code object.  The
// code object of catan_abi.hip holds k_step and the learner's kernels, and must stay, byte for byte in .text, what it is without these
// players: placed inside catan_abi.hip, even behind every other kernel, the teacher's three kernels moved all of its code by a few KB, and
// with no teacher configured bench.py and the learner's step measured slower than the parent's spread.  Hence nothing of
// catan_kernels.hip is included.  What both units need comes from headers that emit no code of their own: the layout from catan_state.h,
// the views and helpers from catan_view.h, the topology from catan_topology.inc, and the builder's rule from catan_scripted.hip
// (CATAN_SCRIPTED_RULE_ONLY leaves its kernel, k_sample_scripted, in the first unit, where it has always been).  All catan_abi.hip sees of
// this file is catan_players.h.  profiles/players_unit.txt holds the comparison of both code objects with their predecessors.
//
// The discipline of every lane-per-row kernel here is the builder's: no LDS, no scratch (local arrays are read and written at
// compile-time indices only; tools/kernel_resources.py is where that is checked), a record and its mask words are read only for a valid
// game that is not busy, 8-byte row stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "catan_state.h"
#include "catan_view.h"
#include "catan_players.h"

#define CATAN_TABLE static __device__ __constant__ const
#define CATAN_FN static __device__ __forceinline__
#define CATAN_TOPOLOGY_CODE
#include "catan_topology.inc"

#define CATAN_SCRIPTED_RULE_ONLY
#include "catan_scripted.hip"

namespace catan {

constexpr int PLAYERS_BLOCK = 256;
static inline unsigned players_blocks(long n) { return (unsigned)((n + PLAYERS_BLOCK - 1) / PLAYERS_BLOCK); }

// ================================================================================================ teacher
// The three kernels that turn a player's actions into a training signal:
//   k_complete_action_rows  makes any legal action row teacher-forceable through the net's heads: the columns the row's type does
//                           NOT use (zero as the samplers leave them) become the lowest legal index of the mask the head would
//                           apply, so that no head evaluates log(0) on a row it then multiplies by 0 (-inf x 0 = NaN).  One lane per row.
//   k_collector_label       stores the teacher's row of a game at the slot k_collector_post stores the net's action in.  One lane per game.
//   k_imitation_loss        the imitation term -mean(lp) with its gradient and its read-out, one launch, conventions of k_ppo_diag.
//
// Which columns a row of type t uses is _ActionHeads.forward's table of head counts (policy.py): head 1 (column 1) Settlement / City,
// 2 Road, 3 MoveRobber, 4 PlayDev, 5 Respond, 6 Propose / Steal, 9 (column 15) Exchange or PlayDev with YoP / Monopoly, 10 (column 16)
// Exchange or PlayDev with YoP, 11 (column 17) Discard, 7 / 8 (columns 7..10, 11..14) Propose.  An unused column gets the lowest set
// bit of the mask row that forward() selects for the row (0 when that row is empty); used columns are never written.
// A row whose type is outside 0..12, whose game id is out of range or whose game waits inside a deferred sequence stays as it is.
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_complete_action_rows(const u32* __restrict__ records, long n, const u32* __restrict__ mpk, const i32* __restrict__ games, long rows,
                                                                       const u8* __restrict__ busy, i32* __restrict__ actions) {
    const long j = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    if (j >= rows) return;
    const long e = games != nullptr ? (long)games[j] : j;
    if (e < 0 || e >= n || (busy != nullptr && busy[e] != 0)) return;
    int a[ACTION_WORDS];
    load_action_row(actions, j, a);
    const int t = a[0];
    if (t < 0 || t > 12) return;
    u32 m[MASK_WORDS];
#pragma unroll
    for (int i = 0; i < MASK_WORDS; i++) m[i] = mpk[e * MPK_STRIDE + i];
    if (!(t == T_SETTLE || t == T_CITY)) a[1] = script_lowest(getr<M1 + 108, 54>(m));           // row 2 of (3, 54)
    if (t != T_ROAD) {
        const u64 lo = getr<M2, 64>(m), hi = getr<M2 + 64, 9>(m);
        a[2] = lo ? script_lowest(lo) : (hi ? 64 + script_lowest(hi) : 0);
    }
    if (t != T_ROBBER) a[3] = script_lowest(getr<M3, 19>(m));
    if (t != T_PLAYDEV) a[4] = script_lowest(getr<M4, 5>(m));
    if (t != T_RESPOND) a[5] = script_lowest(getr<M5, 2>(m));
    if (!(t == T_PROPOSE || t == T_STEAL)) a[6] = script_lowest(getr<M6 + 6, 3>(m));            // row 2 of (3, 3)
    const int card = a[4];
    const bool playdev = t == T_PLAYDEV;
    const bool use9 = t == T_EXCHANGE || (playdev && (card == C_YOP || card == C_MONO));
    const bool use10 = t == T_EXCHANGE || (playdev && card == C_YOP);
    if (!use9) {
        u64 m9 = getr<M9 + 5, 5>(m);                                                            // mask_t: row 1 (row 0 is Exchange's, which uses the head) ...
        if (playdev) m9 &= card == C_MONO ? getr<M9 + 10, 5>(m) : (card == C_YOP ? getr<M9 + 15, 5>(m) : getr<M9 + 5, 5>(m));   // ... AND mask_c
        a[15] = script_lowest(m9);
    }
    if (!use10) a[16] = script_lowest(getr<M10, 5>(m));
    if (t != T_DISCARD) a[17] = script_lowest(getr<M11, 5>(m));
    if (t != T_PROPOSE) {
        // the trade lists: step 0 of head 7 offers "stop" only with an empty hand, else the resources held (obs_f[12:18], the deciding
        // player's hand as k_obs_rows writes it: slot 0 empty, slot 1 + r = resource r); head 8 the same with every resource offered
        const StRead s(records, e);
        const int me = deciding(s) & 3;
        int first = 0;
#pragma unroll
        for (int r = 4; r >= 0; r--) first = s.res(me, r) > 0 ? r + 1 : first;
        a[7] = first; a[8] = 0; a[9] = 0; a[10] = 0;
        a[11] = first ? 1 : 0; a[12] = 0; a[13] = 0; a[14] = 0;
    }
    store_action_row(actions, j, a);
}

// The teacher's row of game g goes where k_collector_post stores the net's action of the same decision: slot t = min(n_act[g], T - 1),
// for a game whose action the env consumes in this iteration and whose deciding seat is the active one.  Launched IN FRONT OF
// k_collector_post (it reads n_act before the increment and `live` as k_collector_pre left it).  Opponent seats are never labelled.
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_collector_label(long n, int T, const long long* __restrict__ n_act, const u8* __restrict__ live,
                                                                  const long long* __restrict__ active_pid, const i32* __restrict__ deciding,
                                                                  const u8* __restrict__ waiting_before, const i32* __restrict__ labels,
                                                                  short* __restrict__ st_teacher) {
    const long g = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    if (g >= n) return;
    const bool consumed = live[g] != 0 && (waiting_before == nullptr || waiting_before[g] == 0);
    if (!consumed || deciding[g] != (int)active_pid[g]) return;
    const long long na = n_act[g];
    const long t = na < T - 1 ? na : T - 1;
    const i32* src = labels + g * ACTION_WORDS;
    u32* dst = reinterpret_cast<u32*>(st_teacher + (t * n + g) * ACTION_WORDS);   // 36 B rows: 4 B aligned
#pragma unroll
    for (int k = 0; k < ACTION_WORDS / 2; k++) dst[k] = ((u32)src[2 * k] & 0xFFFFu) | ((u32)src[2 * k + 1] << 16);
}

// The imitation term of an optimiser step and its read-out.  lp float [B]: the joint log-prob of the teacher's rows under the net;
// teacher int64 [B][18]: those rows (column 0, the type, is read).  nll_i = -(double)lp_i.  loss[0] = (float)(sum nll / B), dlp_i =
// (float)(-1.0 / B).  A row whose lp is not finite adds nothing, gets dlp 0 and is counted as skipped (expected: none).
// ACCUMULATED into block double [33]:
//    0 rows   1 calls   2 sum nll   3 max nll (>= 0)   4 rows with lp > -0.6931472f   5 skipped rows
//    6..18 rows per teacher type   19..31 sum nll per teacher type   32 spare
// As k_ppo_diag: fp64 sums, per-workgroup partials in `ws` (IMIT_PART * IMIT_BLOCKS + 1 doubles, the last the arrival counter; zero
// before the first call, left zero by every call) folded in index order by the workgroup that arrives last, the block's only writer -
// no atomic on the block, one stream for all calls into a block, the same bits on every repeat.
constexpr int IMIT_WAVES = IMIT_THREADS / 64;
__device__ __forceinline__ bool imit_is_max(int q) { return q == 1; }
__device__ __forceinline__ double imit_wave_fold(double v, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(v, o, 64);
        v = is_max ? fmax(v, y) : v + y;
    }
    return v;
}
__global__ __launch_bounds__(IMIT_THREADS) void k_imitation_loss(const float* __restrict__ lp, const long long* __restrict__ teacher, long B,
                                                                float* __restrict__ loss, float* __restrict__ dlp, double* __restrict__ block,
                                                                double* __restrict__ ws) {
    __shared__ double sh[IMIT_WAVES][IMIT_PART];
    __shared__ bool last;
    double sum = 0.0, mx = 0.0, tsum[13];
    unsigned half = 0, skipped = 0, tcnt[13];
#pragma unroll
    for (int k = 0; k < 13; k++) { tsum[k] = 0.0; tcnt[k] = 0; }
    const float g = (float)(-1.0 / (double)B);
    for (long i = (long)blockIdx.x * IMIT_THREADS + threadIdx.x; i < B; i += (long)gridDim.x * IMIT_THREADS) {
        const float l = lp[i];
        const bool finite = (__float_as_uint(l) & 0x7f800000u) != 0x7f800000u;
        const int t = (int)teacher[i * ACTION_WORDS];
        const double nll = finite ? -(double)l : 0.0;
        dlp[i] = finite ? g : 0.0f;
        sum += nll;
        mx = fmax(mx, nll);
        half += (finite && l > -0.6931472f) ? 1u : 0u;
        skipped += finite ? 0u : 1u;
#pragma unroll
        for (int k = 0; k < 13; k++) {                          // (selects over the unrolled index: the arrays stay in registers)
            const bool hit = finite && t == k;
            tcnt[k] += hit ? 1u : 0u;
            tsum[k] += hit ? nll : 0.0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto put = [&](int q, double v) {                       // the wave's partial q (a fixed butterfly: the same bits on every run)
        const double r = imit_wave_fold(v, imit_is_max(q));
        if (lane == 0) sh[wave][q] = r;
    };
    put(0, sum); put(1, mx); put(2, (double)half); put(3, (double)skipped);
#pragma unroll
    for (int k = 0; k < 13; k++) { put(4 + k, (double)tcnt[k]); put(17 + k, tsum[k]); }
    __syncthreads();
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(ws + IMIT_PART * IMIT_BLOCKS);
    if (threadIdx.x < IMIT_PART) {
        const int q = threadIdx.x;
        double v = sh[0][q];
#pragma unroll
        for (int w = 1; w < IMIT_WAVES; w++) v = imit_is_max(q) ? fmax(v, sh[w][q]) : v + sh[w][q];
        ws[q * IMIT_BLOCKS + blockIdx.x] = v;
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(counter, 1ull) == (unsigned long long)gridDim.x - 1;
    }
    __syncthreads();
    if (last) {                                             // the last workgroup: lane q adds partial q of workgroups 0, 1, ... in that order
        __threadfence();
        if (threadIdx.x < IMIT_PART) {
            const int q = threadIdx.x;
            double v = 0.0;                                 // (0 is neutral for the maximum too: nll >= 0 where it counts)
            for (unsigned k = 0; k < gridDim.x; k++) {
                double* p = ws + q * IMIT_BLOCKS + k;
                const double y = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *p = 0.0;
                v = imit_is_max(q) ? fmax(v, y) : v + y;
            }
            block[q + 2] = imit_is_max(q) ? fmax(block[q + 2], v) : block[q + 2] + v;
            if (q == 0) {
                loss[0] = (float)(v / (double)B);
                block[0] += (double)B; block[1] += 1.0;
                *counter = 0ull;
            }
        }
    }
}

hipError_t teacher_launch_complete(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                   int32_t* actions, hipStream_t stream) {
    hipLaunchKernelGGL(k_complete_action_rows, dim3(players_blocks(rows)), dim3(PLAYERS_BLOCK), 0, stream, records, n, mpk, games, rows, busy, actions);
    return hipGetLastError();
}
hipError_t teacher_launch_label(long n, int T, const long long* n_act, const uint8_t* live, const long long* active_pid, const int32_t* deciding,
                                const uint8_t* waiting_before, const int32_t* labels, short* st_teacher, hipStream_t stream) {
    hipLaunchKernelGGL(k_collector_label, dim3(players_blocks(n)), dim3(PLAYERS_BLOCK), 0, stream, n, T, n_act, live, active_pid, deciding, waiting_before,
                       labels, st_teacher);
    return hipGetLastError();
}
hipError_t teacher_launch_imitation(const float* lp, const long long* teacher, long B, float* loss, float* dlp, double* block, double* workspace,
                                    hipStream_t stream) {
    long nb = (B + IMIT_THREADS - 1) / IMIT_THREADS;
    if (nb > IMIT_BLOCKS) nb = IMIT_BLOCKS;
    hipLaunchKernelGGL(k_imitation_loss, dim3((unsigned)nb), dim3(IMIT_THREADS), 0, stream, lp, teacher, B, loss, dlp, block, workspace);
    return hipGetLastError();
}

// ================================================================================================ trader
// The builder's table (catan_scripted.hip) with its row 2 replaced and two rows put in front of its row 11:
//   2T   Respond: accept an offer that brings the hand closer to the player's goal, else reject
//   11P  Propose: one spare card for one needed card, to the weakest opponent that holds it and was not yet asked this turn
//   11E  Exchange: a spare resource for a needed one at the bank / harbour rate
// Wherever none of the three fires the action is sample_scripted's, bit for bit: that function is decided first and the new rows only
// look at what it returns.  The rule is restated in numpy by tests/trader_reference.py.  The eight counters fire on every pass, so they
// are reduced within the wave (__ballot + __popcll) and cost one atomic per wave and counter that has anything to add.
constexpr int TRADER_GOALS = 4;            // City, Settlement, Road, DevCard: the table of DESIGN.md 8.14, in its order
constexpr int TRADER_VP_CAP = 8;           // no deal with a player at this many victory points or more
constexpr int TRADER_MAX_ROADS = 15;

// cost of goal g in resource r (r0 order Brick, Wood, Ore, Sheep, Wheat); both indices are compile-time wherever it is called
DEVI constexpr int trader_cost(int g, int r) {
    return g == 0 ? (r == R_ORE ? 3 : (r == R_WHEAT ? 2 : 0))
         : g == 1 ? (r == R_ORE ? 0 : 1)
         : g == 2 ? ((r == R_BRICK || r == R_WOOD) ? 1 : 0)
                  : ((r == R_ORE || r == R_SHEEP || r == R_WHEAT) ? 1 : 0);
}
DEVI int trader_deficit(const int (&cost)[5], const int (&h)[5]) {
    int d = 0;
#pragma unroll
    for (int r = 0; r < 5; r++) d += max(0, cost[r] - h[r]);
    return d;
}
// the goal of player `me` holding h: the available row of the table with the smallest deficit, ties in table order -> its index, or -1
DEVI int trader_goal(const StRead& s, int me, const int (&h)[5], int (&cost)[5]) {
    Boards b;
    load_boards(s, me, b);
    const bool site = (~topo_blocked(b.occ) & ALL54 & topo_touched(b.own_rlo, b.own_rhi)) != 0;     // an open site, as row 10 of 8.8 defines it
    const int roads = __popcll(b.own_rlo) + __popc(b.own_rhi);
    const bool avail[TRADER_GOALS] = { b.own_set != 0 && s.pb(me, P_CLEFT) > 0, site && s.pb(me, P_SLEFT) > 0, !site && roads < TRADER_MAX_ROADS,
                                       s.b(B_PILE_LEN) > 0 };
    int goal = -1, best = 0x7fffffff;
#pragma unroll
    for (int g = 0; g < TRADER_GOALS; g++) {
        int d = 0;
#pragma unroll
        for (int r = 0; r < 5; r++) d += max(0, trader_cost(g, r) - h[r]);
        if (avail[g] && d < best) { goal = g; best = d; }
    }
#pragma unroll
    for (int r = 0; r < 5; r++) {
        int c = 0;
#pragma unroll
        for (int g = 0; g < TRADER_GOALS; g++) c = goal == g ? trader_cost(g, r) : c;
        cost[r] = c;
    }
    return goal;
}
// the r with the largest key[r] > 0 among the bits of `legal`; ties to the lowest r; -1 when there is none
DEVI int trader_pick(u32 legal, const int (&key)[5]) {
    int best = -1, bv = 0;
#pragma unroll
    for (int r = 0; r < 5; r++) if (((legal >> r) & 1u) && key[r] > bv) { best = r; bv = key[r]; }
    return best;
}

// -> the bits (1 << TC_*) this decision counts; a[] = the action
DEVI u32 sample_trader(const StRead& s, const u32 (&m)[MASK_WORDS], int (&a)[ACTION_WORDS]) {
    const int row = sample_scripted(s, m, a);
    u32 counts = 1u << TC_DECISIONS;
    if (row != 2 && row < 11) return counts;                               // rows 1, 3..10: the builder's
    const u32 types = (u32)getr<M0, 13>(m);
    const int me = deciding(s) & 3;
    int h[5], cost[5], need[5], spare[5];
#pragma unroll
    for (int r = 0; r < 5; r++) h[r] = s.res(me, r);
    const int goal = trader_goal(s, me, h, cost);
    const int deficit = trader_deficit(cost, h);
    if (row == 2) {                                                        // 2T
        const int ng = s.b(B_TRADE_NG), nr = s.b(B_TRADE_NR);
        int h2[5];
#pragma unroll
        for (int r = 0; r < 5; r++) h2[r] = h[r];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int g = s.b(B_TRADE_GIVE + i) - 1, rc = s.b(B_TRADE_RECV + i) - 1;
#pragma unroll
            for (int r = 0; r < 5; r++) h2[r] += ((i < ng && g == r) ? 1 : 0) - ((i < nr && rc == r) ? 1 : 0);
        }
        const bool legal = (getr<M5, 2>(m) & 1u) != 0;
        const bool accept = legal && nr <= ng && s.b(B_CURVP + (s.b(B_TRADE_PROP) & 3)) < TRADER_VP_CAP && goal >= 0 && trader_deficit(cost, h2) < deficit;
        a[5] = accept ? 0 : 1;
        return counts | (1u << TC_RESPONSES) | (1u << (accept ? TC_ACCEPTS : (legal ? TC_REJECT_OTHER : TC_REJECT_ILLEGAL)));
    }
    if (goal >= 0 && deficit >= 1) {
#pragma unroll
        for (int r = 0; r < 5; r++) { need[r] = max(0, cost[r] - h[r]); spare[r] = max(0, h[r] - cost[r]); }
        if (types & (1u << T_PROPOSE)) {                                   // 11P
            const int want = trader_pick(31u, need), give = trader_pick(31u, spare);
            if (give >= 0) {
                const int order = s.b(B_ORDER), seatof = s.b(B_SEATOF), k = s.b(B_TRADES);
                int key[3];                                                // (victory points, label) of a candidate, -1: not one
#pragma unroll
                for (int l = 0; l < 3; l++) {
                    const int p = player_at_label(order, seatof, me, l), vp = s.b(B_CURVP + p);
                    key[l] = (s.res(p, want) >= 1 && vp < TRADER_VP_CAP) ? vp * 4 + l : -1;
                }
                int target = -1;                                           // the candidate with exactly k candidates in front of it
#pragma unroll
                for (int l = 0; l < 3; l++) {
                    int before = 0;
#pragma unroll
                    for (int o = 0; o < 3; o++) before += (key[o] >= 0 && key[o] < key[l]) ? 1 : 0;
                    if (key[l] >= 0 && before == k) target = l;
                }
                if (target >= 0) {
#pragma unroll
                    for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
                    a[0] = T_PROPOSE; a[6] = target; a[7] = give + 1; a[11] = want + 1;
                    return counts | (1u << TC_PROPOSALS);
                }
            }
        }
        if (types & (1u << T_EXCHANGE)) {                                  // 11E
            const int hb = s.pb(me, P_HARB);
            u32 can = 0;
#pragma unroll
            for (int r = 0; r < 5; r++) {
                const int rate = ((hb >> (r + 1)) & 1) ? 2 : ((hb & 1) ? 3 : 4);
                if (spare[r] >= rate) can |= 1u << r;
            }
            const int give = trader_pick(can & (u32)getr<M9, 5>(m), spare), want = trader_pick((u32)getr<M10, 5>(m), need);
            if (give >= 0 && want >= 0) {
#pragma unroll
                for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
                a[0] = T_EXCHANGE; a[15] = give; a[16] = want;
                return counts | (1u << TC_EXCHANGES);
            }
        }
    }
    return counts | (row == SCRIPT_ROWS ? 1u << TC_FALLBACKS : 0u);         // the builder's 11, 12 or 13
}

// Row j of `actions` (int32 [rows][18]) = the trader's action for game games[j] (games == nullptr: game j).  A negative or out-of-range
// id, and a game that waits for its deferred step, gets EndTurn and counts nothing, exactly as in k_sample_scripted.
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_sample_trader(const u32* __restrict__ records, long n, const u32* __restrict__ mpk, const i32* __restrict__ games,
                                                                 long rows, const u8* __restrict__ busy, i32* __restrict__ actions,
                                                                 unsigned long long* __restrict__ counts) {
    const long j = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    const bool in = j < rows;
    const long e = !in ? -1 : (games != nullptr ? (long)games[j] : j);
    int a[ACTION_WORDS];
    u32 hit = 0;
    if (e < 0 || e >= n || (busy != nullptr && busy[e] != 0)) {
#pragma unroll
        for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
        a[0] = T_ENDTURN;
    } else {
        const StRead s(records, e);
        u32 m[MASK_WORDS];
#pragma unroll
        for (int i = 0; i < MASK_WORDS; i++) m[i] = mpk[e * MPK_STRIDE + i];
        hit = sample_trader(s, m, a);
    }
    if (in) store_action_row(actions, j, a);
    // every lane of the wave is here (no early return above): one ballot per counter, the wave's first lane adds the population
#pragma unroll
    for (int k = 0; k < TC_WORDS; k++) {
        const unsigned long long b = __ballot((hit >> k) & 1u);
        if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(counts + k, (unsigned long long)__popcll(b));
    }
}

hipError_t trader_launch_sample(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                int32_t* actions, unsigned long long* counts, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_trader, dim3(players_blocks(rows)), dim3(PLAYERS_BLOCK), 0, stream, records, n, mpk, games, rows, busy,
                       actions, counts);
    return hipGetLastError();
}

// ================================================================================================ playout player
// A call forks every root game into C*K slots of a scratch ("sim") handle - sim slot s = (j*C + c)*K + k holds playout k of candidate
// c of row j -, plays candidate c as the first action of its K slots, lets the rule-based player finish `depth` steps in every seat and
// picks, per row, the candidate whose K final positions score best for the root's deciding player.  The games themselves are stepped by
// the kernels that step every other game (catan_state_fork, the samplers, catan_randomise_uncertainty, catan_step); what stands here is
// the bookkeeping around them:
//   k_playout_slots    the fork's index arrays and the candidate samplers' `games` list
//   k_playout_expand   candidate rows, duplicates, every slot's first action, controlling player and latch
//   k_playout_hold     in front of every later step: a finished, duplicate or bad slot is frozen (action type -1), the others count a step
//   k_playout_score    integer score per slot, summed per (row, candidate) within one wave; the best candidate's row
// Everything is integer and nothing is accumulated with atomics: the result does not depend on the order in which waves arrive.
// The rule is restated over the CPU oracle by tests/playout_reference.py.
constexpr int PLAYOUT_WIN_SCORE = 1000, PLAYOUT_VP_SCORE = 10;

// One lane per slot in use.  src_idx[s]: the root game of row j (games[j], null: j), -1 where that id is outside the root handle (the
// fork copies nothing for it); draw_off[s] = (1 + k) << 22, the stride of forward_search.py; slot0[j*C + c] = the slot (j, c, 0).
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_playout_slots(PlayoutShape sh, const i32* __restrict__ games, long root_n, long long* __restrict__ src_idx,
                                                                 u32* __restrict__ draw_off, i32* __restrict__ slot0) {
    const long s = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    if (s >= sh.used) return;
    const long jc = s / sh.K;
    const int k = (int)(s - jc * sh.K);
    const long j = jc / sh.C;
    const long g = games != nullptr ? (long)games[j] : j;
    src_idx[s] = (g >= 0 && g < root_n) ? (long long)g : -1ll;
    draw_off[s] = (u32)(1 + k) << 22;
    if (k == 0) slot0[jc] = (i32)s;
}

// candidate c of row j as the samplers left it: word w of its 18
DEVI i32 playout_cand_word(const PlayoutShape& sh, const i32* __restrict__ by_builder, const i32* __restrict__ by_trader, const i32* __restrict__ by_random,
                           long j, int c, int w) {
    const long jc = j * sh.C + c;
    const i32* row = c < sh.n_builder ? by_builder + jc * ACTION_WORDS
                   : c < sh.n_builder + sh.n_trader ? by_trader + jc * ACTION_WORDS
                                                     : by_random + jc * sh.K * ACTION_WORDS;
    return row[w];
}

// One lane per slot of the sim handle (the slots behind the ones in use get a no-op row and a closed latch, so that the steps of this
// call leave them alone).  The slot's record is still the root's (the fork ran, nothing was stepped or re-dealt yet).
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_playout_expand(PlayoutShape sh, const u32* __restrict__ records, const long long* __restrict__ src_idx,
                                                                  const i32* __restrict__ by_builder, const i32* __restrict__ by_trader,
                                                                  const i32* __restrict__ by_random, i32* __restrict__ cand, u8* __restrict__ dup,
                                                                  i32* __restrict__ act, i32* __restrict__ ctrl, u8* __restrict__ held,
                                                                  i32* __restrict__ steps, i32* __restrict__ rpid) {
    const long s = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    if (s >= sh.sim_n) return;
    i32 a[ACTION_WORDS];
#pragma unroll
    for (int w = 0; w < ACTION_WORDS; w++) a[w] = 0;
    bool frozen = true;
    int pid = 0;
    if (s < sh.used) {
        const long jc = s / sh.K;
        const int k = (int)(s - jc * sh.K);
        const long j = jc / sh.C;
        const int c = (int)(jc - j * sh.C);
        const bool bad = src_idx[s] < 0;
        bool is_dup = false;
        if (!bad) {
            const StRead st(records, s);
            // (deciding_pid0 with all five bytes read up front, not catan_view.h's deciding(): this kernel's code is what it was)
            pid = deciding_pid0(st.b(B_NDISC), st.b(B_DISC), st.flags(), st.b(B_TRADE_TGT), st.b(B_GO)) + 1;
#pragma unroll
            for (int w = 0; w < ACTION_WORDS; w++) a[w] = playout_cand_word(sh, by_builder, by_trader, by_random, j, c, w);
            for (int o = 0; o < c; o++) {                       // bytewise equal to a lower-numbered candidate of the row: the samplers leave unused columns 0
                bool same = true;
#pragma unroll
                for (int w = 0; w < ACTION_WORDS; w++) same = same && playout_cand_word(sh, by_builder, by_trader, by_random, j, o, w) == a[w];
                is_dup = is_dup || same;
            }
        }
        if (k == 0) {
            store_action_row(cand, jc, a);
            dup[jc] = (bad || is_dup) ? 1 : 0;
            if (c == 0) rpid[j] = bad ? 0 : pid;
        }
        frozen = bad || is_dup;
    }
    if (frozen) a[0] = -1;
    store_action_row(act, s, a);
    ctrl[s] = (frozen || !sh.determinise) ? 0 : pid;
    held[s] = frozen ? 1 : 0;
    steps[s] = frozen ? 0 : 1;                                  // the candidate's own step
}

// One lane per slot in use, behind the sampler that wrote the rows of the next step and in front of that step.
__global__ __launch_bounds__(PLAYERS_BLOCK) void k_playout_hold(long used, const u8* __restrict__ done, u8* __restrict__ held, i32* __restrict__ act,
                                                                i32* __restrict__ steps) {
    const long s = (long)blockIdx.x * PLAYERS_BLOCK + threadIdx.x;
    if (s >= used) return;
    const bool h = held[s] != 0 || done[s] != 0;
    held[s] = h ? 1 : 0;
    if (h) act[s * ACTION_WORDS] = -1;
    else steps[s] += 1;
}

DEVI int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// One wave per row; lane l takes the sims l, l + 64, ... of the row's C*K.  The per-candidate sums are kept in registers at compile-time
// indices (a sim adds to the one candidate it belongs to through a select), summed over the wave with a butterfly, and every lane then
// holds every total: the pick is the same in all of them.
__global__ __launch_bounds__(64) void k_playout_score(PlayoutShape sh, const u32* __restrict__ records, const i32* __restrict__ cand, const u8* __restrict__ dup,
                                                      const i32* __restrict__ rpid, const i32* __restrict__ steps, i32* __restrict__ actions,
                                                      i32* __restrict__ chosen, long long* __restrict__ stats) {
    const long j = blockIdx.x;
    const int lane = threadIdx.x;
    if (j >= sh.rows) return;
    const int p = rpid[j];                                      // wave-uniform
    if (p < 1 || p > 4) {                                       // a bad row: EndTurn, nothing chosen, an all-zero block
        if (lane < ACTION_WORDS) actions[j * ACTION_WORDS + lane] = lane == 0 ? T_ENDTURN : 0;
        if (lane == 0 && chosen != nullptr) chosen[j] = -1;
        if (stats != nullptr) for (int i = lane; i < sh.C * PS_WORDS; i += 64) stats[j * sh.C * PS_WORDS + i] = 0;
        return;
    }
    int fin[PLAYOUT_MAX_CANDIDATES], win[PLAYOUT_MAX_CANDIDATES], sc[PLAYOUT_MAX_CANDIDATES], vps[PLAYOUT_MAX_CANDIDATES], stp[PLAYOUT_MAX_CANDIDATES];
#pragma unroll
    for (int c = 0; c < PLAYOUT_MAX_CANDIDATES; c++) { fin[c] = 0; win[c] = 0; sc[c] = 0; vps[c] = 0; stp[c] = 0; }
    const int per_row = sh.C * sh.K;
    for (int i = lane; i < per_row; i += 64) {
        const int c = i / sh.K;
        if (dup[j * sh.C + c]) continue;                        // its sims were never stepped
        const long s = j * per_row + i;
        const StRead st(records, s);
        const int winner = st.b(B_WINNER);
        int mine = 0, best_other = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int v = st.pb(q, P_VP);
            if (q == p - 1) mine = v;
            else best_other = v > best_other ? v : best_other;
        }
        const int f = winner != 0 ? 1 : 0, w = winner == p ? 1 : 0;
        const int score = PLAYOUT_WIN_SCORE * w + PLAYOUT_VP_SCORE * (mine - best_other);
        const int n = steps[s];
#pragma unroll
        for (int cc = 0; cc < PLAYOUT_MAX_CANDIDATES; cc++) {
            const bool here = cc == c;
            fin[cc] += here ? f : 0; win[cc] += here ? w : 0; sc[cc] += here ? score : 0; vps[cc] += here ? mine : 0; stp[cc] += here ? n : 0;
        }
    }
    int best = 0, best_score = 0;
    long long my[PS_WORDS];
#pragma unroll
    for (int f = 0; f < PS_WORDS; f++) my[f] = 0;
#pragma unroll
    for (int c = 0; c < PLAYOUT_MAX_CANDIDATES; c++) {
        if (c >= sh.C) break;                                   // (wave-uniform)
        const int t_fin = wave_sum(fin[c]), t_win = wave_sum(win[c]), t_sc = wave_sum(sc[c]), t_vp = wave_sum(vps[c]), t_stp = wave_sum(stp[c]);
        const bool valid = dup[j * sh.C + c] == 0;
        if (valid && (c == 0 || t_sc > best_score)) { best = c; best_score = t_sc; }      // ties stay with the lowest index; candidate 0 is never a duplicate
        if (lane == c) {
            my[PS_VALID] = valid ? 1 : 0; my[PS_SIMS] = valid ? sh.K : 0; my[PS_FINISHED] = t_fin; my[PS_WINS] = t_win;
            my[PS_SCORE_SUM] = t_sc; my[PS_VP_SUM] = t_vp; my[PS_STEPS_SUM] = t_stp;
        }
    }
    if (lane < ACTION_WORDS) actions[j * ACTION_WORDS + lane] = cand[(j * sh.C + best) * ACTION_WORDS + lane];
    if (lane == 0 && chosen != nullptr) chosen[j] = best;
    if (stats != nullptr && lane < sh.C) {
#pragma unroll
        for (int f = 0; f < PS_WORDS; f++) stats[(j * sh.C + lane) * PS_WORDS + f] = my[f];
    }
}

hipError_t playout_launch_slots(const PlayoutShape& sh, const int32_t* games, long root_n, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_slots, dim3(players_blocks(sh.used)), dim3(PLAYERS_BLOCK), 0, stream, sh, games, root_n, ws.src_idx, ws.draw_off, ws.slot0);
    return hipGetLastError();
}
hipError_t playout_launch_expand(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_expand, dim3(players_blocks(sh.sim_n)), dim3(PLAYERS_BLOCK), 0, stream, sh, sim_records, (const long long*)ws.src_idx,
                       (const i32*)ws.by_builder, (const i32*)ws.by_trader, (const i32*)ws.by_random, ws.cand, ws.dup, ws.act, ws.ctrl, ws.held, ws.steps, ws.rpid);
    return hipGetLastError();
}
hipError_t playout_launch_hold(const PlayoutShape& sh, const uint8_t* done, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_hold, dim3(players_blocks(sh.used)), dim3(PLAYERS_BLOCK), 0, stream, sh.used, done, ws.held, ws.act, ws.steps);
    return hipGetLastError();
}
hipError_t playout_launch_score(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, int32_t* actions, int32_t* chosen,
                                long long* stats, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_score, dim3((unsigned)sh.rows), dim3(64), 0, stream, sh, sim_records, (const i32*)ws.cand, (const u8*)ws.dup,
                       (const i32*)ws.rpid, (const i32*)ws.steps, actions, chosen, stats);
    return hipGetLastError();
}

}  // namespace catan
