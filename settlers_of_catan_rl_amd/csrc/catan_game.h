// catan_game.h - what catan_kernels.hip and catan_hooks.hip both need of a handle and of a game that is written or exported: the
// launch-invariant handle fields (Ctx), the written view of a record in HBM (St), the estimate words' unpacking, one game's canonical
// blob (export_game) and Philox.  A header of its own beside catan_view.h, which stays the read-only views and the helpers every unit
// shares: the players' unit needs nothing of this.  Like catan_view.h it is structs and inlined device functions only: no kernel, no
// table, nothing that takes a place in a code object.
#pragma once
#include "catan_state.h"
#include "catan_view.h"

namespace catan {

struct MtPair;        // catan_kernels.hip: contract (A)'s two MT19937 generators
struct BoardCfg;      // catan_kernels.hip: the device copy of catan_board_cfg_t
struct Ctx {          // launch-invariant handle fields
    u32* R;           // game records, REC words each
    long N;           // padded number of games (row pitch)
    long n;           // real number of games
    u32 key0, key1;   // philox key = seed
    u64 env_id0;      // global id of game 0 (multi-GPU shards keep their global ids)
    MtPair* mt;       // contract (A): the handle's two MT19937 generators (n == 1), or null = contract (B), per-game Philox streams
    const BoardCfg* bcfg;   // board layouts (<= MAX_BOARD_CFGS entries), or null = every deal fully random
    const u8* bcfg_idx;     // [N] layout of each game (read only when bcfg != null)
};

// (StOps, the accessors both views derive from the layout, is catan_view.h's)
// view 1: the game's record in HBM (k_masks, k_reset, k_sample_random, export/import, k_obs_rows, tier-2 longest road)
struct St : StOps<St> {
    u32* P;           // the game's record
    long e;
    DEVI St(u32* R_, long /*N*/, long e_) : P(R_ + e_ * REC), e(e_) {}
    DEVI u32 w(int r) const { return P[r]; }
    DEVI void sw(int r, u32 v) const { P[r] = v; }
    DEVI int cold(int f) const { return ((const u8*)(P + NW))[f]; }
    DEVI void scold(int f, int v) const { ((u8*)(P + NW))[f] = (u8)v; }
    DEVI int b(int f) const { return cold(f); }
    DEVI void sb(int f, int v) const { scold(f, v); }
};

constexpr int FORK_REC_CHUNKS = REC / 4;      // a record in 16-byte chunks: the lanes of a wave that copies one (k_fork, the pool's install)

// Philox4x32-10 (Salmon et al., SC'11).  Contract: SURVEY.md 8.4 / DESIGN.md "RNG".
DEVI void philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1, u32 (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        u32 n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct Est { int mn[5], mx[5]; };
template <class S>
DEVI void est_load(const S& s, int o, int l, Est& E) {
    int base = W_EST + (o * 3 + l) * 3;
    u32 a = s.w(base), b = s.w(base + 1), c = s.w(base + 2);
#pragma unroll
    for (int r = 0; r < 4; r++) { E.mn[r] = (a >> (8 * r)) & 255; E.mx[r] = (b >> (8 * r)) & 255; }
    E.mn[4] = c & 255; E.mx[4] = (c >> 8) & 255;
}

// canonical int32 blob, layout spec.py STATE_FIELDS; blob is [STATE_WORDS][cnt] (word-major); idx = game ids or null
struct BlobW {
    i32* p; long cnt, i; int k;
    DEVI void put(int v) { p[(long)k * cnt + i] = v; k++; }
};
// one game's blob (k_export; the recorder's snapshots, catan_hooks.hip, with cnt = 1)
DEVI void export_game(const St& s, BlobW o) {
    for (int t = 0; t < 19; t++) o.put(s.b(B_TILE + t) & 15);
    for (int t = 0; t < 19; t++) o.put(s.b(B_TILE + t) >> 4);
    o.put(s.b(B_ROBBER));
    for (int t = 0; t < 9; t++) o.put(s.b(B_HARB + t));
    u64 st[4], ct[4], rl[4]; u32 rh[4];
    for (int p = 0; p < 4; p++) { st[p] = s.settle(p); ct[p] = s.city(p); rl[p] = s.road_lo(p); rh[p] = s.road_hi(p); }
    for (int cn = 0; cn < 54; cn++) { int v = 0; for (int p = 0; p < 4; p++) { if ((st[p] >> cn) & 1) v = 1; if ((ct[p] >> cn) & 1) v = 2; } o.put(v); }
    for (int cn = 0; cn < 54; cn++) { int v = 0; for (int p = 0; p < 4; p++) if (((st[p] | ct[p]) >> cn) & 1) v = p + 1; o.put(v); }
    for (int e = 0; e < 72; e++) { int v = 0; for (int p = 0; p < 4; p++) if (e < 64 ? ((rl[p] >> e) & 1) : ((rh[p] >> (e - 64)) & 1)) v = p + 1; o.put(v); }
    for (int p = 0; p < 4; p++) {
        for (int r = 0; r < 5; r++) o.put(s.pb(p, P_RES + r));
        for (int r = 0; r < 5; r++) o.put(s.pb(p, P_VIS + r));
        Est E[3];
        for (int l = 0; l < 3; l++) est_load(s, p, l, E[l]);
        for (int l = 0; l < 3; l++) for (int r = 0; r < 5; r++) o.put(E[l].mn[r]);
        for (int l = 0; l < 3; l++) for (int r = 0; r < 5; r++) o.put(E[l].mx[r]);
        int hb = s.pb(p, P_HARB);
        for (int k = 0; k < 6; k++) o.put((hb >> k) & 1);
        int nh = s.pb(p, P_NHID);
        o.put(nh);
        for (int k = 0; k < 25; k++) o.put(k < nh ? s.hidden(p, k) : -1);
        int np = s.pb(p, P_NPLAYED);
        o.put(np);
        for (int k = 0; k < 25; k++) o.put(k < np ? s.played(p, k) : -1);
        o.put(s.pb(p, P_VP));
    }
    for (int r = 0; r < 5; r++) o.put(s.b(B_BANK + r));
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_SLEFT));
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_CLEFT));
    int pl = s.b(B_PILE_LEN);
    o.put(pl);
    for (int k = 0; k < 25; k++) o.put(k < pl ? s.pile(k) : -1);
    int order = s.b(B_ORDER);
    for (int k = 0; k < 4; k++) o.put(pid_at(order, k) + 1);
    o.put(s.b(B_ORDER_ID)); o.put(s.b(B_GO) + 1);
    int fl = s.flags();
    o.put((fl & F_INITIAL) ? 1 : 0);
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_ISET));
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_IROAD));
    for (int p = 0; p < 4; p++) { int v = s.pb(p, P_ISECOND); o.put(v == 255 ? -1 : v); }
    o.put((fl & F_ROLLED) ? 1 : 0); o.put((fl & F_PLAYED_DEV) ? 1 : 0); o.put((fl & F_MUST_USE_DEV) ? 1 : 0);
    int mr = (fl & F_MUST_RESPOND) ? 1 : 0;
    o.put(mr);
    o.put(mr ? s.b(B_TRADE_PROP) + 1 : 0); o.put(mr ? s.b(B_TRADE_TGT) + 1 : 0);
    o.put(s.b(B_TRADE_NG));
    for (int k = 0; k < 4; k++) o.put(s.b(B_TRADE_GIVE + k));
    o.put(s.b(B_TRADE_NR));
    for (int k = 0; k < 4; k++) o.put(s.b(B_TRADE_RECV + k));
    o.put((fl & F_RB_ACTIVE) ? 1 : 0); o.put(s.b(B_RB_COUNT));
    o.put((fl & F_CAN_ROBBER) ? 1 : 0); o.put((fl & F_JUST_ROBBER) ? 1 : 0);
    int nd = s.b(B_NDISC);
    o.put(nd > 0 ? 1 : 0); o.put(nd);
    for (int k = 0; k < 4; k++) o.put(k < nd ? s.b(B_DISC + k) + 1 : 0);
    o.put(s.b(B_DIE1)); o.put(s.b(B_DIE2));
    o.put(s.b(B_TRADES)); o.put((int)s.w(W_ACTIONS)); o.put((int)s.w(W_TURN));
    for (int k = 0; k < 5; k++) o.put(s.b(B_BOUGHT + k));
    o.put(s.b(B_LR_PLAYER)); o.put(s.b(B_LR_COUNT)); o.put(s.b(B_LA_PLAYER)); o.put(s.b(B_LA_COUNT));
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_CURLP));
    for (int p = 0; p < 4; p++) o.put(s.pb(p, P_ARMY));
    for (int p = 0; p < 4; p++) o.put(s.b(B_CURVP + p));
    o.put(s.b(B_WINNER));
    o.put((int)s.w(W_RNG));
}

}  // namespace catan
