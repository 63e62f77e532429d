// catan_trader.hip - the rule-based "trader" player on the device (catan_sample_scripted_actions_style, style 1).
//
// The builder's table (catan_scripted.hip) with its row 2 replaced and two rows put in front of its row 11:
//   2T   Respond: accept an offer that brings the hand closer to the player's goal, else reject
//   11P  Propose: one spare card for one needed card, to the weakest opponent that holds it and was not yet asked this turn
//   11E  Exchange: a spare resource for a needed one at the bank / harbour rate
// Wherever none of the three fires the action is sample_scripted's, bit for bit: that function is included from catan_scripted.hip
// as it stands (CATAN_SCRIPTED_RULE_ONLY leaves the builder's kernel out) and decided first; the new rows only look at what it returns.
// The rule is restated in numpy by tests/trader_reference.py.
//
// A translation unit of its own (compiled beside catan_abi.hip by _lib.build_library), for the reason catan_teacher.hip is one: the code
// object every other kernel lives in stays, byte for byte in .text, what it is without this file.  Hence nothing of catan_kernels.hip is
// included: the layout comes from catan_state.h, the topology from catan_topology.inc, and the few helpers the builder's rule calls (a
// read-only view of a record, getr, load_boards, player_at_label) are restated below.
//
// The builder's discipline: one lane per row of the call, no LDS, no scratch (local arrays are read and written at compile-time indices
// only; profiles/trader_kernel_resources.txt is where that is checked), a record and its mask words are read only for a valid game that
// is not busy, 8-byte row stores.  The eight counters fire on every pass, so they are reduced within the wave (__ballot + __popcll) and
// cost one atomic per wave and counter that has anything to add.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "catan_state.h"
#include "catan_trader.h"

#define CATAN_TABLE static __device__ __constant__ const
#define CATAN_FN static __device__ __forceinline__
#define CATAN_TOPOLOGY_CODE
#include "catan_topology.inc"

namespace catan {

#define DEVI __device__ __forceinline__
constexpr u64 ALL54 = (1ull << 54) - 1;

namespace {
// a game's record in HBM, read-only (view 1 of catan_kernels.hip without its writers; local to this translation unit)
struct St {
    const u32* P;
    DEVI St(const u32* R_, long e_) : P(R_ + e_ * REC) {}
    DEVI u32 w(int r) const { return P[r]; }
    DEVI int b(int f) const { return ((const u8*)(P + NW))[f]; }
    DEVI int pb(int p, int f) const { return b(B_PLAYER + p * PB + f); }
    DEVI int flags() const { return b(B_FLAGS); }
    DEVI int res(int p, int r0) const { return pb(p, P_RES + r0); }
    DEVI int total(int p) const { return res(p, 0) + res(p, 1) + res(p, 2) + res(p, 3) + res(p, 4); }
    DEVI u64 settle(int p) const { return (u64)w(W_SETTLE_LO + p) | ((u64)w(W_SETTLE_HI + p) << 32); }
    DEVI u64 city(int p) const { return (u64)w(W_CITY_LO + p) | ((u64)w(W_CITY_HI + p) << 32); }
    DEVI u64 road_lo(int p) const { return (u64)w(W_ROAD0 + p) | ((u64)w(W_ROAD1 + p) << 32); }
    DEVI u32 road_hi(int p) const { return w(W_ROAD2 + p); }
};
}  // namespace

// bit range [OFF, OFF + NBITS) of the 11 packed mask words (getr of catan_kernels.hip)
template <int OFF, int NBITS>
DEVI u64 getr(const u32 (&m)[MASK_WORDS]) {
    constexpr int w0 = OFF >> 5, sh = OFF & 31;
    constexpr u64 full = NBITS >= 64 ? ~0ull : ((1ull << NBITS) - 1);
    u64 v = (u64)m[w0] >> sh;
    if constexpr (sh + NBITS > 32) v |= (u64)m[w0 + 1] << (32 - sh);
    if constexpr (sh + NBITS > 64) v |= (u64)m[w0 + 2] << (64 - sh);
    return v & full;
}
struct Boards { u64 occ, own_bld, own_set, own_rlo, all_rlo; u32 own_rhi, all_rhi; };
DEVI void load_boards(const St& s, int pid, Boards& b) {
    b.occ = 0; b.own_bld = 0; b.own_set = 0; b.own_rlo = 0; b.all_rlo = 0; b.own_rhi = 0; b.all_rhi = 0;
    for (int p = 0; p < 4; p++) {
        u64 st = s.settle(p), ct = s.city(p), rl = s.road_lo(p);
        u32 rh = s.road_hi(p);
        b.occ |= st | ct; b.all_rlo |= rl; b.all_rhi |= rh;
        if (p == pid) { b.own_bld = st | ct; b.own_set = st; b.own_rlo = rl; b.own_rhi = rh; }
    }
}
DEVI int seat_of(int seatof, int p) { return (seatof >> (2 * p)) & 3; }
DEVI int pid_at(int order, int seat) { return (order >> (2 * (seat & 3))) & 3; }
DEVI int player_at_label(int order, int seatof, int me, int label) { return pid_at(order, seat_of(seatof, me) + 1 + label); }

}  // namespace catan

#define CATAN_SCRIPTED_RULE_ONLY
#include "catan_scripted.hip"

namespace catan {

constexpr int TRADER_BLOCK = 256;
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
DEVI int trader_goal(const St& s, int me, const int (&h)[5], int (&cost)[5]) {
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
DEVI u32 sample_trader(const St& s, const u32 (&m)[MASK_WORDS], int (&a)[ACTION_WORDS]) {
    const int row = sample_scripted(s, m, a);
    u32 counts = 1u << TC_DECISIONS;
    if (row != 2 && row < 11) return counts;                               // rows 1, 3..10: the builder's
    const u32 types = (u32)getr<M0, 13>(m);
    int me;                                                                // the deciding player, as sample_scripted finds it
    if (s.b(B_NDISC) > 0) me = s.b(B_DISC);
    else if (s.flags() & F_MUST_RESPOND) me = s.b(B_TRADE_TGT);
    else me = s.b(B_GO);
    me &= 3;
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
__global__ __launch_bounds__(TRADER_BLOCK) void k_sample_trader(const u32* __restrict__ records, long n, const u32* __restrict__ mpk, const i32* __restrict__ games,
                                                                 long rows, const u8* __restrict__ busy, i32* __restrict__ actions,
                                                                 unsigned long long* __restrict__ counts) {
    const long j = (long)blockIdx.x * TRADER_BLOCK + threadIdx.x;
    const bool in = j < rows;
    const long e = !in ? -1 : (games != nullptr ? (long)games[j] : j);
    int a[ACTION_WORDS];
    u32 hit = 0;
    if (e < 0 || e >= n || (busy != nullptr && busy[e] != 0)) {
#pragma unroll
        for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
        a[0] = T_ENDTURN;
    } else {
        const St s(records, e);
        u32 m[MASK_WORDS];
#pragma unroll
        for (int i = 0; i < MASK_WORDS; i++) m[i] = mpk[e * MPK_STRIDE + i];
        hit = sample_trader(s, m, a);
    }
    if (in) {
        uint2* row = reinterpret_cast<uint2*>(actions + j * ACTION_WORDS);    // 72 B rows: 8 B aligned
#pragma unroll
        for (int i = 0; i < ACTION_WORDS / 2; i++) row[i] = make_uint2((u32)a[2 * i], (u32)a[2 * i + 1]);
    }
    // every lane of the wave is here (no early return above): one ballot per counter, the wave's first lane adds the population
#pragma unroll
    for (int k = 0; k < TC_WORDS; k++) {
        const unsigned long long b = __ballot((hit >> k) & 1u);
        if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(counts + k, (unsigned long long)__popcll(b));
    }
}

hipError_t trader_launch_sample(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                int32_t* actions, unsigned long long* counts, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_trader, dim3((unsigned)((rows + TRADER_BLOCK - 1) / TRADER_BLOCK)), dim3(TRADER_BLOCK), 0, stream, records, n, mpk, games, rows, busy,
                       actions, counts);
    return hipGetLastError();
}

}  // namespace catan
