// catan_scripted.hip - the rule-based "builder" player on the device (catan_sample_scripted_actions, include/catan_hip_tuning.h).
//
// A fixed-strength opponent for evaluation games and for the collector's opponent slots: deterministic (the same state gives the same
// action; all randomness stays in the dice), always legal under the game's masks, one lane per game.  The rule is DESIGN.md 8.8, restated
// in numpy by tests/scripted_reference.py; the reference project has no such player.
//
// What a lane reads: the game's 11 packed mask words (side row) and, of its record (view 1), the bitboards (words 0..27), the tile bytes,
// the control block and the four players' hands - whichever of them the chosen row of the rule needs.  Topology comes from the constant
// tables of catan_topology.inc.  No LDS, no atomics except the counter of the fall-back row.  No scratch: every local array (the hand,
// the action words, the mask words) is read and written at compile-time indices only - in fully unrolled loops, a value chosen at run time
// picked by a chain of selects over the unrolled index, never by subscript - so the arrays live in registers; the resources table in
// profiles/scripted_policy_kernel_resources.txt is where that is checked (scratch 0).  The branches diverge by action type within a wave,
// as in k_sample_random.
//
// Included behind every other kernel file of catan_abi.hip: no existing kernel's code changes with it.  catan_players.hip includes it
// too, for the rule alone (CATAN_SCRIPTED_RULE_ONLY); the views and helpers it reads a game through are catan_view.h's.
#pragma once

namespace catan {

constexpr int SCRIPT_BLOCK = 256;
constexpr int SCRIPT_ROWS = 13;          // rows of the table in DESIGN.md 8.8 (1-based; 13 = the fall-back)

// the 19 tiles in two 64-bit words, 3 bits per tile: pips = 6 - |7 - value| (0 for the desert) and the resource (Terrain value, 0 = desert)
struct ScriptTiles { u64 pips, res; };
template <class S>
DEVI ScriptTiles script_tiles(const S& s) {
    u32 w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = s.w(NW + B_TILE / 4 + k);
    ScriptTiles t{ 0, 0 };
#pragma unroll
    for (int i = 0; i < 19; i++) {
        const int b = (int)((w[i >> 2] >> (8 * (i & 3))) & 255u), r = b & 15, v = b >> 4;
        const int d = v > 7 ? v - 7 : 7 - v;
        const int p = (r == 0 || d > 5) ? 0 : 6 - d;
        t.pips |= (u64)p << (3 * i);
        t.res |= (u64)(r & 7) << (3 * i);
    }
    return t;
}
DEVI int script_corner_value(const ScriptTiles& t, int c) {
    int v = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int tl = CORNER_TILE[c][k];
        if (tl < 19) v += (int)((t.pips >> (3 * tl)) & 7);
    }
    return v;
}
// distinct non-desert resources among the corner's tiles
DEVI int script_corner_kinds(const ScriptTiles& t, int c) {
    u32 seen = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int tl = CORNER_TILE[c][k];
        if (tl < 19) seen |= 1u << ((t.res >> (3 * tl)) & 7);
    }
    return __popc(seen & ~1u);
}
// the legal corner (bits of `legal`) with the largest corner value; kinds: ties go to more distinct resources; then to the lowest index
DEVI int script_best_corner(const ScriptTiles& t, u64 legal, bool kinds) {
    int best = 0, bv = -1, bk = -1;
    for (u64 m = legal; m; m &= m - 1) {
        const int c = __ffsll((unsigned long long)m) - 1;
        const int v = script_corner_value(t, c), k = kinds ? script_corner_kinds(t, c) : 0;
        if (v > bv || (v == bv && k > bk)) { best = c; bv = v; bk = k; }
    }
    return best;
}
// the set bit r of `legal` (5 bits) with the largest (most = true) or smallest key[r]; ties to the lowest r; 0 when nothing is legal
DEVI int script_pick_res(u32 legal, const int (&key)[5], bool most) {
    int best = 0, bv = 0;
    bool have = false;
#pragma unroll
    for (int r = 0; r < 5; r++) {
        if (!((legal >> r) & 1u)) continue;
        const int v = most ? key[r] : -key[r];
        if (!have || v > bv) { best = r; bv = v; have = true; }
    }
    return best;
}

// -> the row of the table that fired (1..13); a[] = the action.  S: a view of the game's record (catan_view.h)
template <class S>
DEVI int sample_scripted(const S& s, const u32 (&m)[MASK_WORDS], int (&a)[ACTION_WORDS]) {
#pragma unroll
    for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
    const u32 types = (u32)getr<M0, 13>(m);
    const int me = deciding(s) & 3;
    int hand[5];
#pragma unroll
    for (int r = 0; r < 5; r++) hand[r] = s.res(me, r);

    if (types & (1u << T_DISCARD)) {                                      // 1
        a[0] = T_DISCARD; a[17] = script_pick_res((u32)getr<M11, 5>(m), hand, true);
        return 1;
    }
    if (types & (1u << T_RESPOND)) {                                      // 2: reject (env/wrapper.py:159-160: action[5] == 1)
        a[0] = T_RESPOND; a[5] = 1;
        return 2;
    }
    if (types & (1u << T_STEAL)) {                                        // 3
        const u32 tg = (u32)getr<M6 + 3, 3>(m);
        const int order = s.b(B_ORDER), seatof = s.b(B_SEATOF);
        int best = 0, bc = -1, bv = -1;
#pragma unroll
        for (int l = 0; l < 3; l++) {
            if (!((tg >> l) & 1u)) continue;
            const int p = player_at_label(order, seatof, me, l);
            const int cards = s.total(p), vp = s.b(B_CURVP + p);
            if (cards > bc || (cards == bc && vp > bv)) { best = l; bc = cards; bv = vp; }
        }
        a[0] = T_STEAL; a[6] = best;
        return 3;
    }
    if (types & (1u << T_ROBBER)) {                                       // 4
        const ScriptTiles t = script_tiles(s);
        u64 st[4], ct[4];
#pragma unroll
        for (int p = 0; p < 4; p++) { st[p] = s.settle(p); ct[p] = s.city(p); }
        int best = 0, bs = -0x7fffffff;
        for (u32 lm = (u32)getr<M3, 19>(m); lm; lm &= lm - 1) {
            const int tl = __ffs(lm) - 1;
            const u64 tm = TILE_CORNER_MASK[tl];
            int others = 0, own = 0;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int n = __popcll(st[p] & tm) + 2 * __popcll(ct[p] & tm);
                if (p == me) own += n; else others += n;
            }
            const int sc = own ? -1000 : (int)((t.pips >> (3 * tl)) & 7) * others;
            if (sc > bs) { best = tl; bs = sc; }
        }
        a[0] = T_ROBBER; a[3] = best;
        return 4;
    }
    if (types & (1u << T_ROLL)) { a[0] = T_ROLL; return 5; }              // 5
    if (types & (1u << T_CITY)) {                                         // 6
        const ScriptTiles t = script_tiles(s);
        a[0] = T_CITY; a[1] = script_best_corner(t, getr<M1 + 54, 54>(m), false);
        return 6;
    }
    if (types & (1u << T_SETTLE)) {                                       // 7 (also the initial placements)
        const ScriptTiles t = script_tiles(s);
        a[0] = T_SETTLE; a[1] = script_best_corner(t, getr<M1, 54>(m), true);
        return 7;
    }
    if (types & (1u << T_PLAYDEV)) {                                      // 8
        const u32 cm = (u32)getr<M4, 5>(m);
        if (cm & ~(1u << C_VP)) {
            a[0] = T_PLAYDEV;
            if (cm & (1u << C_KNIGHT)) a[4] = C_KNIGHT;
            else if (cm & (1u << C_RB)) a[4] = C_RB;
            else if (cm & (1u << C_YOP)) {
                // the first resource where sample_random reads it (head 9, row 3), narrowed to what head 10 offers (the bank's stock)
                const u32 h9 = (u32)getr<M9 + 15, 5>(m), h10 = (u32)getr<M10, 5>(m);
                a[4] = C_YOP;
                a[15] = script_pick_res((h9 & h10) ? (h9 & h10) : h9, hand, false);
                int held[5];
#pragma unroll
                for (int r = 0; r < 5; r++) held[r] = hand[r] + (r == a[15] ? 1 : 0);
                a[16] = script_pick_res(h10, held, false);
            } else {
                int theirs[5];
#pragma unroll
                for (int r = 0; r < 5; r++) {
                    theirs[r] = 0;
#pragma unroll
                    for (int p = 0; p < 4; p++) theirs[r] += p == me ? 0 : s.res(p, r);
                }
                a[4] = C_MONO; a[15] = script_pick_res((u32)getr<M9 + 10, 5>(m), theirs, true);
            }
            return 8;
        }
    }
    if (types & (1u << T_BUYDEV)) { a[0] = T_BUYDEV; return 9; }          // 9
    if (types & (1u << T_ROAD)) {                                         // 10
        Boards b;
        load_boards(s, me, b);
        const u64 open = ~topo_blocked(b.occ) & ALL54;                    // empty corners with no building next to them
        const bool only = (types & ~(1u << T_ENDTURN)) == (1u << T_ROAD);
        if (only || (open & topo_touched(b.own_rlo, b.own_rhi)) == 0) {
            const ScriptTiles t = script_tiles(s);
            const u64 lo = getr<M2, 64>(m);
            const u32 hi = (u32)getr<M2 + 64, 9>(m);
            int best = 72, bs = -2;                                       // the dummy edge (bit 8 of hi) only when no real edge is legal
            for (u64 em = lo; em; em &= em - 1) {
                const int e = __ffsll((unsigned long long)em) - 1;
                int sc = -1;
                for (u64 cm = EDGE_CORNER_MASK[e] & open; cm; cm &= cm - 1) sc = max(sc, script_corner_value(t, __ffsll((unsigned long long)cm) - 1));
                if (sc > bs) { best = e; bs = sc; }
            }
            for (u32 em = hi & 0xFFu; em; em &= em - 1) {
                const int e = 64 + __ffs(em) - 1;
                int sc = -1;
                for (u64 cm = EDGE_CORNER_MASK[e] & open; cm; cm &= cm - 1) sc = max(sc, script_corner_value(t, __ffsll((unsigned long long)cm) - 1));
                if (sc > bs) { best = e; bs = sc; }
            }
            a[0] = T_ROAD; a[2] = best;
            return 10;
        }
    }
    if (types & (1u << T_EXCHANGE)) {                                     // 11
        const u32 give = (u32)getr<M9, 5>(m);
        const int g = script_pick_res(give, hand, true);
        int most = 0;                                                     // hand[g] without a runtime index into the local array
#pragma unroll
        for (int r = 0; r < 5; r++) most = r == g ? hand[r] : most;
        if (((give >> g) & 1u) && most >= 5) {
            a[0] = T_EXCHANGE; a[15] = g; a[16] = script_pick_res((u32)getr<M10, 5>(m), hand, false);
            return 11;
        }
    }
    if (types & (1u << T_ENDTURN)) { a[0] = T_ENDTURN; return 12; }       // 12
    // 13, the fall-back: the lowest legal type but ProposeTrade, every sub-head at its lowest legal index (sample_random with all-zero words)
    const int t = script_lowest(types & ~(1u << T_PROPOSE));
    a[0] = t;
    switch (t) {
    case T_SETTLE: a[1] = script_lowest(getr<M1, 54>(m)); break;
    case T_CITY: a[1] = script_lowest(getr<M1 + 54, 54>(m)); break;
    case T_ROAD: { const u64 lo = getr<M2, 64>(m), hi = getr<M2 + 64, 9>(m); a[2] = lo ? script_lowest(lo) : (hi ? 64 + script_lowest(hi) : 0); break; }
    case T_ROBBER: a[3] = script_lowest(getr<M3, 19>(m)); break;
    case T_PLAYDEV:
        a[4] = script_lowest(getr<M4, 5>(m));
        if (a[4] == C_MONO) a[15] = script_lowest(getr<M9 + 10, 5>(m));
        else if (a[4] == C_YOP) { a[15] = script_lowest(getr<M9 + 15, 5>(m)); a[16] = script_lowest(getr<M10, 5>(m)); }
        break;
    case T_EXCHANGE: a[15] = script_lowest(getr<M9, 5>(m)); a[16] = script_lowest(getr<M10, 5>(m)); break;
    case T_RESPOND: a[5] = script_lowest(getr<M5, 2>(m)); break;
    case T_STEAL: a[6] = script_lowest(getr<M6 + 3, 3>(m)); break;
    case T_DISCARD: a[17] = script_lowest(getr<M11, 5>(m)); break;
    default: break;
    }
    return 13;
}

#ifndef CATAN_SCRIPTED_RULE_ONLY    // catan_players.hip takes the rule above into its own code object, without the builder's kernel
// Row j of `actions` (int32 [rows][18]) = the bot's action for game games[j] (games == nullptr: game j).  A negative or out-of-range id,
// and a game that waits for its deferred step (busy != nullptr: an open catan_step_deferred sequence), gets EndTurn - the bot's answer
// to the placeholder mask row catan_masks_of hands out for such a game; neither the record nor the masks of such a game are read.
__global__ __launch_bounds__(SCRIPT_BLOCK) void k_sample_scripted(Ctx c, const u32* __restrict__ mpk, const i32* __restrict__ games, long rows,
                                                                   const u8* __restrict__ busy, i32* __restrict__ actions,
                                                                   unsigned long long* __restrict__ fallback) {
    const long j = (long)blockIdx.x * SCRIPT_BLOCK + threadIdx.x;
    if (j >= rows) return;
    const long e = games != nullptr ? (long)games[j] : j;
    int a[ACTION_WORDS];
    if (e < 0 || e >= c.n || (busy != nullptr && busy[e] != 0)) {
#pragma unroll
        for (int i = 0; i < ACTION_WORDS; i++) a[i] = 0;
        a[0] = T_ENDTURN;
    } else {
        const St s(c.R, c.N, e);
        u32 m[MASK_WORDS];
#pragma unroll
        for (int i = 0; i < MASK_WORDS; i++) m[i] = mpk[e * MPK_STRIDE + i];
        if (sample_scripted(s, m, a) == SCRIPT_ROWS) atomicAdd(fallback, 1ull);
    }
    store_action_row(actions, j, a);
}
#endif

}  // namespace catan
