// catan_view.h - the one place that knows how to read a game: the accessors derived from a record's layout (catan_state.h), a read-only
// view of a record in HBM, the packed mask words' bit ranges, the seat arithmetic, and the load and store of an action row.
// Device code, included behind catan_state.h by both translation units of the library (catan_kernels.hip, catan_players.hip).
// Everything here is inlined into its callers: no kernel, no table, nothing that takes a place in a code object.
#pragma once
#include "catan_state.h"

namespace catan {

#define DEVI __device__ __forceinline__

constexpr u64 ALL54 = (1ull << 54) - 1;

// Derived helpers shared by the state views (CRTP): a view supplies w / b / cold, and sw / sb / scold if it is written through.
template <class D>
struct StOps {
    DEVI const D& self() const { return *static_cast<const D*>(this); }
    DEVI int pb(int p, int f) const { return self().b(B_PLAYER + p * PB + f); }
    DEVI void spb(int p, int f, int v) const { self().sb(B_PLAYER + p * PB + f, v); }
    DEVI u64 settle(int p) const { return (u64)self().w(W_SETTLE_LO + p) | ((u64)self().w(W_SETTLE_HI + p) << 32); }
    DEVI u64 city(int p) const { return (u64)self().w(W_CITY_LO + p) | ((u64)self().w(W_CITY_HI + p) << 32); }
    DEVI void set_settle(int p, u64 v) const { self().sw(W_SETTLE_LO + p, (u32)v); self().sw(W_SETTLE_HI + p, (u32)(v >> 32)); }
    DEVI void set_city(int p, u64 v) const { self().sw(W_CITY_LO + p, (u32)v); self().sw(W_CITY_HI + p, (u32)(v >> 32)); }
    DEVI u64 road_lo(int p) const { return (u64)self().w(W_ROAD0 + p) | ((u64)self().w(W_ROAD1 + p) << 32); }
    DEVI u32 road_hi(int p) const { return self().w(W_ROAD2 + p); }
    DEVI int flags() const { return self().b(B_FLAGS); }
    DEVI int res(int p, int r0) const { return pb(p, P_RES + r0); }
    DEVI int total(int p) const { return res(p, 0) + res(p, 1) + res(p, 2) + res(p, 3) + res(p, 4); }
    // cold byte fields (always global): ordered card lists and the pile
    DEVI int hidden(int p, int i) const { return self().cold(B_CARDS + p * 50 + i); }
    DEVI void set_hidden(int p, int i, int v) const { self().scold(B_CARDS + p * 50 + i, v); }
    DEVI int played(int p, int i) const { return self().cold(B_CARDS + p * 50 + 25 + i); }
    DEVI void set_played(int p, int i, int v) const { self().scold(B_CARDS + p * 50 + 25 + i, v); }
    DEVI int pile(int i) const { return self().cold(B_PILE + i); }
    DEVI void set_pile(int i, int v) const { self().scold(B_PILE + i, v); }
};
// a game's record in HBM, read-only (the players' unit; StOps' writers are members of a template, never instantiated for it)
struct StRead : StOps<StRead> {
    const u32* P;
    DEVI StRead(const u32* R_, long e_) : P(R_ + e_ * REC) {}
    DEVI u32 w(int r) const { return P[r]; }
    DEVI int b(int f) const { return ((const u8*)(P + NW))[f]; }
    DEVI int cold(int f) const { return b(f); }
};

// The player who decides in a state, as pid0: the rule of catan_state.h's deciding_pid0 over a view, reading only the entries the answer
// needs - the form the samplers have always had (k_playout_expand reads all five up front and calls deciding_pid0 itself)
template <class S>
DEVI int deciding(const S& s) {
    const int flags = s.flags();
    int p;
    if (s.b(B_NDISC) > 0) p = s.b(B_DISC);
    else if (flags & F_MUST_RESPOND) p = s.b(B_TRADE_TGT);
    else p = s.b(B_GO);
    return p;
}

DEVI int seat_of(int seatof, int p) { return (seatof >> (2 * p)) & 3; }
DEVI int pid_at(int order, int seat) { return (order >> (2 * (seat & 3))) & 3; }
// ref: game/components/player.py:12-20
DEVI int label_of(int seatof, int me, int other) { return ((seat_of(seatof, other) - seat_of(seatof, me)) & 3) - 1; }
DEVI int player_at_label(int order, int seatof, int me, int label) { return pid_at(order, seat_of(seatof, me) + 1 + label); }

// bit range [OFF, OFF + NBITS) of the 11 packed mask words
template <int OFF, int NBITS>
DEVI u64 getr(const u32 (&m)[MASK_WORDS]) {
    constexpr int w0 = OFF >> 5, sh = OFF & 31;
    constexpr u64 full = NBITS >= 64 ? ~0ull : ((1ull << NBITS) - 1);
    u64 v = (u64)m[w0] >> sh;
    if constexpr (sh + NBITS > 32) v |= (u64)m[w0 + 1] << (32 - sh);
    if constexpr (sh + NBITS > 64) v |= (u64)m[w0 + 2] << (64 - sh);
    return v & full;
}
// the lowest set bit's index, 0 for an empty set
DEVI int script_lowest(u64 v) { return v ? __ffsll((unsigned long long)v) - 1 : 0; }

struct Boards { u64 occ, own_bld, own_set, own_rlo, all_rlo; u32 own_rhi, all_rhi; };
template <class S>
DEVI void load_boards(const S& s, int pid, Boards& b) {
    b.occ = 0; b.own_bld = 0; b.own_set = 0; b.own_rlo = 0; b.all_rlo = 0; b.own_rhi = 0; b.all_rhi = 0;
    for (int p = 0; p < 4; p++) {
        u64 st = s.settle(p), ct = s.city(p), rl = s.road_lo(p);
        u32 rh = s.road_hi(p);
        b.occ |= st | ct; b.all_rlo |= rl; b.all_rhi |= rh;
        if (p == pid) { b.own_bld = st | ct; b.own_set = st; b.own_rlo = rl; b.own_rhi = rh; }
    }
}

// ---- action rows of the lane-per-row kernels: int32 [rows][18], 72 B rows, 8 B aligned, moved as nine uint2
DEVI void load_action_row(const i32* actions, long j, int (&a)[ACTION_WORDS]) {
    const uint2* row = reinterpret_cast<const uint2*>(actions + j * ACTION_WORDS);
#pragma unroll
    for (int i = 0; i < ACTION_WORDS / 2; i++) { const uint2 v = row[i]; a[2 * i] = (int)v.x; a[2 * i + 1] = (int)v.y; }
}
DEVI void store_action_row(i32* actions, long j, const int (&a)[ACTION_WORDS]) {
    uint2* row = reinterpret_cast<uint2*>(actions + j * ACTION_WORDS);
#pragma unroll
    for (int i = 0; i < ACTION_WORDS / 2; i++) row[i] = make_uint2((u32)a[2 * i], (u32)a[2 * i + 1]);
}

}  // namespace catan
