// catan_state_check.h - the rules of the state check (spec.STATE_CHECK_RULES; include/catan_hip_tuning.h catan_state_check).
// Two parts.  The first is what catan_abi.hip sees through catan_hooks.h: the rules' bit numbers, no code.  The second, behind
// CATAN_STATE_CHECK_CODE, is state_check_blob - one blob in, its violation word out - for catan_hooks.hip's k_state_check and, compiled for
// the host, for tools/native/state_check_host.cpp.  It needs catan_topology.inc's generated helpers (CATAN_TOPOLOGY_CODE) included in
// front of it, DEVI, and __popcll / __popc.
#ifndef CATAN_STATE_CHECK_H
#define CATAN_STATE_CHECK_H
#include "catan_state.h"

namespace catan {
// The rules in bit order (restated in include/catan_hip_tuning.h and spec.py STATE_CHECK_RULES): bit r of a blob's word = rule r is broken.
enum { SC_RANGE_BOARD = 0, SC_RANGE_PLAYERS, SC_RANGE_TURN, SC_TERRAIN_MULTISET, SC_TOKEN_MULTISET, SC_HARBOUR_PERMUTATION, SC_BUILDING_OWNER,
       SC_DISTANCE_RULE, SC_PIECES_LEFT, SC_RESOURCE_CONSERVATION, SC_CARD_CONSERVATION, SC_ARMY, SC_LARGEST_ARMY, SC_LONGEST_ROAD,
       SC_VICTORY_POINTS, SC_WINNER, SC_TURN_ORDER, SC_ROADS_ATTACHED, SC_INITIAL_PHASE, SC_DICE, SC_DISCARD, SC_TRADE, SC_ESTIMATES, SC_BOUGHT,
       SC_ROAD_BUILDING, SC_HARBOUR_FLAGS, SC_RULES };
static_assert(SC_RULES == 26, "restate spec.STATE_CHECK_RULES and include/catan_hip_tuning.h when a rule is added");
}  // namespace catan
#endif /* CATAN_STATE_CHECK_H */

#if defined(CATAN_STATE_CHECK_CODE) && !defined(CATAN_STATE_CHECK_CODE_DONE)
#define CATAN_STATE_CHECK_CODE_DONE
namespace catan {

// Two masks the generated helpers do not carry, each a fact of the hexagonal grid that tests/test_state_check_reference_cpu.py checks
// against the topology fixture: the corners are two-colourable (no corner neighbours one of its own colour), so "two neighbouring
// corners built" is topo_blocked(built & A) & built & ~A; and the edges fall into three classes such that two edges that share a corner
// are never of one class, so the roads of class i are attached iff they lie in topo_edges_at(buildings | topo_touched(the owner's roads
// of the other two classes)).  The third: the two corners of each harbour slot (CORNER_HSLOT of catan_topology.inc, by slot).
constexpr u64 SC_CORNER_COLOUR_A = 0x2ad55554aa9555ull;
constexpr u64 SC_EDGE_CLASS_LO[3] = { 0x4922a490a9219499ull, 0x12904a4314862126ull, 0xa44d112c42584a40ull };
constexpr u32 SC_EDGE_CLASS_HI[3] = { 0x24u, 0x4bu, 0x90u };
constexpr u64 SC_HARBOUR_SLOT_CORNERS[9] = { 0x3ull, 0x240ull, 0x1001000ull, 0x3000000000ull, 0x600000000000ull, 0xc000000000000ull,
                                             0x1800000000000ull, 0x4008000000ull, 0xc000ull };
static_assert((SC_EDGE_CLASS_LO[0] ^ SC_EDGE_CLASS_LO[1] ^ SC_EDGE_CLASS_LO[2]) == ~0ull && (SC_EDGE_CLASS_LO[0] & SC_EDGE_CLASS_LO[1]) == 0ull &&
              (SC_EDGE_CLASS_LO[0] & SC_EDGE_CLASS_LO[2]) == 0ull && (SC_EDGE_CLASS_HI[0] ^ SC_EDGE_CLASS_HI[1] ^ SC_EDGE_CLASS_HI[2]) == 0xFFu &&
              (SC_EDGE_CLASS_HI[0] & SC_EDGE_CLASS_HI[1]) == 0u && (SC_EDGE_CLASS_HI[0] & SC_EDGE_CLASS_HI[2]) == 0u, "the three edge classes partition the 72 edges");

// word offsets of the blob (spec.STATE_FIELDS)
namespace sc {
constexpr int TILE_RES = 0, TILE_VAL = 19, ROBBER = 38, HARBOUR = 39, BLD = 48, OWNER = 102, EDGE = 156, PLAYER = 228, PLAYER_WORDS = 99,
              PL_RES = 0, PL_VIS = 5, PL_MIN = 10, PL_MAX = 25, PL_HARB = 40, PL_NHID = 46, PL_HID = 47, PL_NPLAYED = 72, PL_PLAYED = 73, PL_VP = 98,
              BANK = 624, SLEFT = 629, CLEFT = 633, PILE_LEN = 637, PILE = 638, ORDER = 663, ORDER_ID = 667, GO = 668, INITIAL = 669, ISET = 670,
              IROAD = 674, ISECOND = 678, ROLLED = 682, PLAYED_DEV = 683, MUST_USE = 684, MUST_RESPOND = 685, TRADE_PROP = 686, TRADE_TGT = 687,
              TRADE_NG = 688, TRADE_GIVE = 689, TRADE_NR = 693, TRADE_RECV = 694, RB_ACTIVE = 698, RB_COUNT = 699, CAN_ROBBER = 700,
              JUST_ROBBER = 701, NEED_DISCARD = 702, N_DISCARD = 703, DISCARD = 704, DIE1 = 708, DIE2 = 709, BOUGHT = 713, LR_PLAYER = 718,
              LR_COUNT = 719, LA_PLAYER = 720, LA_COUNT = 721, CURLP = 722, ARMY = 726, CURVP = 730, WINNER = 734, RNG = 735;
static_assert(PLAYER + 4 * PLAYER_WORDS == BANK && PL_VP == PLAYER_WORDS - 1 && RNG == STATE_WORDS - 1, "spec.STATE_FIELDS");
}

struct ScBlob {
    const i32* p; long cnt, i;
    DEVI int operator()(int k) const { return p[(long)k * cnt + i]; }
};
// the range rule of a loaded word: outside lo..hi it sets `bad` and becomes lo
DEVI int sc_range(int v, int lo, int hi, bool& bad) { const bool out = v < lo || v > hi; bad |= out; return out ? lo : v; }
DEVI int sc_min0(int v, bool& bad) { const bool out = v < 0; bad |= out; return out ? 0 : v; }
// x[sel] for a sel in 0..3 that is no compile-time constant
template <class T> DEVI T sc_pick(const T (&x)[4], int sel) { return sel == 0 ? x[0] : (sel == 1 ? x[1] : (sel == 2 ? x[2] : x[3])); }
// a dev-card list: `len` (range-checked) cards of 25 words at `at`; the card counts go to the byte fields of `cards`, those of card 0 and 1 to n0 / n1
DEVI void sc_card_list(const ScBlob& W, int at, int len, bool& bad, u64& cards, int& n0, int& n1) {
    for (int k = 0; k < 25; k++) {
        const int c = W(at + k);
        const bool in = k < len, out = in && (c < 0 || c > 4);
        bad |= out;
        const int card = (in && !out) ? c : 0;
        cards += (u64)(in ? 1 : 0) << (8 * card);
        n0 += (in && card == 0) ? 1 : 0; n1 += (in && card == 1) ? 1 : 0;
    }
}
// a holder rule: holder h (0: nobody), the count it holds the title with, the four players' sizes, the least size that earns the title
DEVI bool sc_holder_bad(int h, int count, const int (&size)[4], int least, bool none_below) {
    int mx = size[0];
#pragma unroll
    for (int p = 1; p < 4; p++) mx = size[p] > mx ? size[p] : mx;
    if (h != 0) return count != sc_pick(size, h - 1) || count < least || mx > count;
    return count != 0 || (none_below && mx >= least);
}

// one blob -> its violation word
DEVI u64 state_check_blob(const ScBlob& W) {
    u64 v = 0ull;
    bool rb = false, rp = false, rt = false;
    auto set = [&](int rule, bool broken) { v |= (u64)(broken ? 1 : 0) << rule; };

    // ---- board
    u32 terrain = 0u; u64 tokens = 0ull; bool desert_bad = false;
    for (int t = 0; t < 19; t++) {
        const int r = sc_range(W(sc::TILE_RES + t), 0, 5, rb), val = sc_range(W(sc::TILE_VAL + t), 2, 12, rb);
        terrain += 1u << (5 * r);
        if (r != 0) tokens += 1ull << (5 * (val - 2)); else desert_bad |= val != 7;
    }
    // five bits per count: terrains 0..5 = 1 3 4 3 4 4 (TERRAIN_TO_PLACE), tokens 2..12 = 1 2 2 2 2 0 2 2 2 2 1 (DEFAULT_NUMBER_ORDER)
    set(SC_TERRAIN_MULTISET, terrain != (1u | 3u << 5 | 4u << 10 | 3u << 15 | 4u << 20 | 4u << 25));
    set(SC_TOKEN_MULTISET, desert_bad || tokens != (1ull | 2ull << 5 | 2ull << 10 | 2ull << 15 | 2ull << 20 | 2ull << 30 | 2ull << 35 | 2ull << 40 | 2ull << 45 | 1ull << 50));
    sc_range(W(sc::ROBBER), 0, 18, rb);
    u32 hbit[9], hall = 0u;
#pragma unroll
    for (int s = 0; s < 9; s++) { hbit[s] = 1u << sc_range(W(sc::HARBOUR + s), 0, 8, rb); hall |= hbit[s]; }
    set(SC_HARBOUR_PERMUTATION, hall != 0x1FFu);
    u64 b1 = 0ull, b2 = 0ull, own[4] = { 0ull, 0ull, 0ull, 0ull };
    for (int cn = 0; cn < 54; cn++) {
        const int b = sc_range(W(sc::BLD + cn), 0, 2, rb), o = sc_range(W(sc::OWNER + cn), 0, 4, rb);
        b1 |= (u64)(b == 1 ? 1 : 0) << cn; b2 |= (u64)(b == 2 ? 1 : 0) << cn;
#pragma unroll
        for (int p = 0; p < 4; p++) own[p] |= (u64)(o == p + 1 ? 1 : 0) << cn;
    }
    const u64 built = b1 | b2;
    set(SC_BUILDING_OWNER, built != (own[0] | own[1] | own[2] | own[3]));
    set(SC_DISTANCE_RULE, (topo_blocked(built & SC_CORNER_COLOUR_A) & built & ~SC_CORNER_COLOUR_A) != 0ull);
    u64 rl[4] = { 0ull, 0ull, 0ull, 0ull }; u32 rh[4] = { 0u, 0u, 0u, 0u };
    for (int e = 0; e < 64; e++) {
        const int o = sc_range(W(sc::EDGE + e), 0, 4, rb);
#pragma unroll
        for (int p = 0; p < 4; p++) rl[p] |= (u64)(o == p + 1 ? 1 : 0) << e;
    }
    for (int e = 0; e < 8; e++) {
        const int o = sc_range(W(sc::EDGE + 64 + e), 0, 4, rb);
#pragma unroll
        for (int p = 0; p < 4; p++) rh[p] |= (u32)(o == p + 1 ? 1 : 0) << e;
    }

    // ---- whose turn, the phase, the holders (read in front of the players, who are judged against them)
    int order[4]; u32 seen = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) { order[k] = sc_range(W(sc::ORDER + k), 1, 4, rt); seen |= 1u << order[k]; }
    const int order_id = sc_range(W(sc::ORDER_ID), 0, 3, rt), go = sc_range(W(sc::GO), 1, 4, rt);
    set(SC_TURN_ORDER, seen != 0x1Eu || go != sc_pick(order, order_id));
    const bool initial = sc_range(W(sc::INITIAL), 0, 1, rt) != 0, rolled = sc_range(W(sc::ROLLED), 0, 1, rt) != 0;
    sc_range(W(sc::PLAYED_DEV), 0, 1, rt); sc_range(W(sc::MUST_USE), 0, 1, rt);
    sc_range(W(sc::CAN_ROBBER), 0, 1, rt); sc_range(W(sc::JUST_ROBBER), 0, 1, rt);
    const int lr_player = sc_range(W(sc::LR_PLAYER), 0, 4, rt), la_player = sc_range(W(sc::LA_PLAYER), 0, 4, rt);
    int curlp[4], army[4], curvp[4];
#pragma unroll
    for (int p = 0; p < 4; p++) { curlp[p] = W(sc::CURLP + p); army[p] = W(sc::ARMY + p); curvp[p] = W(sc::CURVP + p); }
    set(SC_LARGEST_ARMY, sc_holder_bad(la_player, W(sc::LA_COUNT), army, 3, true));
    set(SC_LONGEST_ROAD, sc_holder_bad(lr_player, W(sc::LR_COUNT), curlp, 5, false));
    const int winner = sc_range(W(sc::WINNER), 0, 4, rt);
    {
        int mx = curvp[0];
#pragma unroll
        for (int p = 1; p < 4; p++) mx = curvp[p] > mx ? curvp[p] : mx;
        set(SC_WINNER, winner == 0 ? mx >= 10 : sc_pick(curvp, winner - 1) < 10);
    }
    const int d1 = sc_range(W(sc::DIE1), 0, 6, rt), d2 = sc_range(W(sc::DIE2), 0, 6, rt);
    set(SC_DICE, rolled && (d1 < 1 || d2 < 1));
    const bool rb_active = sc_range(W(sc::RB_ACTIVE), 0, 1, rt) != 0;
    set(SC_ROAD_BUILDING, sc_range(W(sc::RB_COUNT), 0, 2, rt) > 0 && !rb_active);

    // ---- the players
    int hand[4][5], n_hidden[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int r = 0; r < 5; r++) hand[q][r] = 0;
    u64 cards = 0ull;
    bool pieces_bad = false, army_bad = false, vp_bad = false, roads_bad = false, initial_bad = initial && rolled, harbour_bad = false;
#pragma unroll 1
    for (int p = 0; p < 4; p++) {
        const int at = sc::PLAYER + p * sc::PLAYER_WORDS;
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int h = sc_min0(W(at + sc::PL_RES + r), rp);
            sc_min0(W(at + sc::PL_VIS + r), rp);
#pragma unroll
            for (int q = 0; q < 4; q++) hand[q][r] = q == p ? h : hand[q][r];
        }
        u32 flags = 0u;
#pragma unroll
        for (int k = 0; k < 6; k++) flags |= (u32)sc_range(W(at + sc::PL_HARB + k), 0, 1, rp) << k;
        const int nh = sc_range(W(at + sc::PL_NHID), 0, 25, rp), np = sc_range(W(at + sc::PL_NPLAYED), 0, 25, rp);
        int hid0 = 0, hid1 = 0, knights = 0, vp_cards = 0;
        sc_card_list(W, at + sc::PL_HID, nh, rp, cards, hid0, hid1);
        sc_card_list(W, at + sc::PL_PLAYED, np, rp, cards, knights, vp_cards);
#pragma unroll
        for (int q = 0; q < 4; q++) n_hidden[q] = q == p ? nh : n_hidden[q];
        const u64 mine = sc_pick(own, p), bld = built & mine, road_lo = sc_pick(rl, p);
        const u32 road_hi = sc_pick(rh, p);
        const int n_set = __popcll(b1 & mine), n_city = __popcll(b2 & mine);
        pieces_bad |= n_set != 5 - sc_range(W(sc::SLEFT + p), 0, 5, rp) || n_city != 4 - sc_range(W(sc::CLEFT + p), 0, 4, rp);
        army_bad |= sc_pick(army, p) != knights;
        const int vp = W(at + sc::PL_VP);
        vp_bad |= vp != n_set + 2 * n_city + (lr_player == p + 1 ? 2 : 0) + (la_player == p + 1 ? 2 : 0) + vp_cards || vp != sc_pick(curvp, p);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            u64 at_lo; u32 at_hi;
            topo_edges_at(bld | topo_touched(road_lo & ~SC_EDGE_CLASS_LO[k], road_hi & ~SC_EDGE_CLASS_HI[k]), at_lo, at_hi);
            roads_bad |= (road_lo & SC_EDGE_CLASS_LO[k] & ~at_lo) != 0ull || (road_hi & SC_EDGE_CLASS_HI[k] & ~at_hi) != 0u;
        }
        const int iset = sc_range(W(sc::ISET + p), 0, 2, rt), iroad = sc_range(W(sc::IROAD + p), 0, 2, rt);
        sc_range(W(sc::ISECOND + p), -1, 53, rt);
        initial_bad |= initial ? (iset != __popcll(bld) || iroad != __popcll(road_lo) + __popc(road_hi))
                               : (iset != 2 || iroad != 2 || (bld & ~topo_touched(road_lo, road_hi)) != 0ull);
        u32 ids = 0u;                                  // the harbour ids at the player's buildings
#pragma unroll
        for (int s = 0; s < 9; s++) ids |= (bld & SC_HARBOUR_SLOT_CORNERS[s]) != 0ull ? hbit[s] : 0u;
        // flag 0 the 3:1 harbours (ids 5..8), flag r the 2:1 harbour of Resource r: ids 4, 3, 0, 1, 2 (board.py:29-33; spec.HARBOUR_FLAG_OF_ID)
        const u32 want = ((ids & 0x1E0u) != 0u ? 1u : 0u) | ((ids >> 4) & 1u) << 1 | ((ids >> 3) & 1u) << 2 | (ids & 1u) << 3 | ((ids >> 1) & 1u) << 4 | ((ids >> 2) & 1u) << 5;
        harbour_bad |= want != flags;
    }
    set(SC_PIECES_LEFT, pieces_bad); set(SC_ARMY, army_bad); set(SC_VICTORY_POINTS, vp_bad); set(SC_ROADS_ATTACHED, roads_bad);
    set(SC_INITIAL_PHASE, initial_bad); set(SC_HARBOUR_FLAGS, harbour_bad);

    // ---- estimates: slot l of player p is the (l + 1)-th player behind p in player_order (p's seat: the last k with order[k] == p + 1, else 0)
    bool est_bad = false;
#pragma unroll 1
    for (int p = 0; p < 4; p++) {
        const int at = sc::PLAYER + p * sc::PLAYER_WORDS;
        int seat = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) seat = order[k] == p + 1 ? k : seat;
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const int q = sc_pick(order, (seat + l + 1) & 3) - 1;
#pragma unroll
            for (int r = 0; r < 5; r++) {
                const int held = q == 0 ? hand[0][r] : (q == 1 ? hand[1][r] : (q == 2 ? hand[2][r] : hand[3][r]));
                const int mn = sc_min0(W(at + sc::PL_MIN + 5 * l + r), rp), mx = sc_min0(W(at + sc::PL_MAX + 5 * l + r), rp);
                est_bad |= mn > held || held > mx;
            }
        }
    }
    set(SC_ESTIMATES, est_bad);

    // ---- bank, pile, conservation
    bool res_bad = false;
    long long total[4] = { 0ll, 0ll, 0ll, 0ll };
#pragma unroll
    for (int r = 0; r < 5; r++) {
        long long sum = (long long)sc_min0(W(sc::BANK + r), rp);
#pragma unroll
        for (int q = 0; q < 4; q++) { sum += hand[q][r]; total[q] += hand[q][r]; }
        res_bad |= sum != 19ll;
    }
    set(SC_RESOURCE_CONSERVATION, res_bad);
    { int unused0 = 0, unused1 = 0; sc_card_list(W, sc::PILE, sc_range(W(sc::PILE_LEN), 0, 25, rp), rp, cards, unused0, unused1); }
    set(SC_CARD_CONSERVATION, cards != (14ull | 5ull << 8 | 2ull << 16 | 2ull << 24 | 2ull << 32));
    {
        long long sum = 0ll;
#pragma unroll
        for (int k = 0; k < 5; k++) sum += (long long)W(sc::BOUGHT + k);
        set(SC_BOUGHT, sum > (long long)sc_pick(n_hidden, go - 1));
    }

    // ---- discard, trade
    {
        const bool need = sc_range(W(sc::NEED_DISCARD), 0, 1, rt) != 0;
        const int nd = sc_range(W(sc::N_DISCARD), 0, 4, rt);
        bool bad = need != (nd > 0);
        u32 few_of = 0u;                                // bit q: player q + 1 holds at most 7 cards
#pragma unroll
        for (int q = 0; q < 4; q++) few_of |= (total[q] <= 7ll ? 1u : 0u) << q;
        int id[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            id[k] = sc_range(W(sc::DISCARD + k), 0, 4, rt);
            bool again = false;
#pragma unroll
            for (int j = 0; j < k; j++) again |= id[j] == id[k];
            const bool few = ((few_of >> ((id[k] > 1 ? id[k] : 1) - 1)) & 1u) != 0u;
            bad |= k < nd ? (id[k] == 0 || few || again) : id[k] != 0;
        }
        set(SC_DISCARD, bad);
    }
    {
        const bool mr = sc_range(W(sc::MUST_RESPOND), 0, 1, rt) != 0;
        const int tp = sc_range(W(sc::TRADE_PROP), 0, 4, rt), tt = sc_range(W(sc::TRADE_TGT), 0, 4, rt);
        const int ng = sc_range(W(sc::TRADE_NG), 0, 4, rt), nr = sc_range(W(sc::TRADE_NR), 0, 4, rt);
        int give[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int g = W(sc::TRADE_GIVE + k), r = W(sc::TRADE_RECV + k);
            const bool gout = k < ng && (g < 1 || g > 5), rout = k < nr && (r < 1 || r > 5);
            rt |= gout || rout;
            give[k] = k < ng ? (gout ? 1 : g) : 0;            // 0: behind the count, matches no resource
        }
        bool short_of = false;
        const int ph = (tp > 1 ? tp : 1) - 1;
#pragma unroll
        for (int r = 0; r < 5; r++) {
            int n = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) n += give[k] == r + 1 ? 1 : 0;
            short_of |= n > (ph == 0 ? hand[0][r] : (ph == 1 ? hand[1][r] : (ph == 2 ? hand[2][r] : hand[3][r])));
        }
        set(SC_TRADE, mr ? (tp == 0 || tt == 0 || tp == tt || short_of) : (tp != 0 || tt != 0 || ng != 0 || nr != 0));
    }
    set(SC_RANGE_BOARD, rb); set(SC_RANGE_PLAYERS, rp); set(SC_RANGE_TURN, rt);
    return v;
}

}  // namespace catan
#endif /* CATAN_STATE_CHECK_CODE */
