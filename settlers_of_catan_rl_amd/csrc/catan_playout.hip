// catan_playout.hip - the kernels of the flat Monte-Carlo playout player (catan_playout_actions, include/catan_hip_tuning.h).
//
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
//
// A translation unit of its own (compiled beside catan_abi.hip by _lib.build_library), for the reason catan_teacher.hip and
// catan_trader.hip are: the code objects of the units before it stay, byte for byte in .text, what they are without this file
// (profiles/playout_kernel_resources.txt).  Nothing of catan_kernels.hip is included: the record's layout comes from catan_state.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "catan_state.h"
#include "catan_playout.h"

namespace catan {

#define DEVI __device__ __forceinline__

namespace {
// a game's record in HBM, read-only (the view catan_trader.hip has; local to this translation unit)
struct St {
    const u32* P;
    DEVI St(const u32* R_, long e_) : P(R_ + e_ * REC) {}
    DEVI int b(int f) const { return ((const u8*)(P + NW))[f]; }
    DEVI int pb(int p, int f) const { return b(B_PLAYER + p * PB + f); }
    DEVI int flags() const { return b(B_FLAGS); }
};
// the deciding PlayerId 1..4 (the rule is catan_state.h's deciding_pid0, which k_deciding of catan_kernels.hip states inline)
DEVI int deciding_pid(const St& s) { return deciding_pid0(s.b(B_NDISC), s.b(B_DISC), s.flags(), s.b(B_TRADE_TGT), s.b(B_GO)) + 1; }
}  // namespace

constexpr int PLAYOUT_BLOCK = 256;
constexpr int PLAYOUT_WIN_SCORE = 1000, PLAYOUT_VP_SCORE = 10;

// One lane per slot in use.  src_idx[s]: the root game of row j (games[j], null: j), -1 where that id is outside the root handle (the
// fork copies nothing for it); draw_off[s] = (1 + k) << 22, the stride of forward_search.py; slot0[j*C + c] = the slot (j, c, 0).
__global__ __launch_bounds__(PLAYOUT_BLOCK) void k_playout_slots(PlayoutShape sh, const i32* __restrict__ games, long root_n, long long* __restrict__ src_idx,
                                                                 u32* __restrict__ draw_off, i32* __restrict__ slot0) {
    const long s = (long)blockIdx.x * PLAYOUT_BLOCK + threadIdx.x;
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
__global__ __launch_bounds__(PLAYOUT_BLOCK) void k_playout_expand(PlayoutShape sh, const u32* __restrict__ records, const long long* __restrict__ src_idx,
                                                                  const i32* __restrict__ by_builder, const i32* __restrict__ by_trader,
                                                                  const i32* __restrict__ by_random, i32* __restrict__ cand, u8* __restrict__ dup,
                                                                  i32* __restrict__ act, i32* __restrict__ ctrl, u8* __restrict__ held,
                                                                  i32* __restrict__ steps, i32* __restrict__ rpid) {
    const long s = (long)blockIdx.x * PLAYOUT_BLOCK + threadIdx.x;
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
            pid = deciding_pid(St(records, s));
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
            uint2* row = reinterpret_cast<uint2*>(cand + jc * ACTION_WORDS);      // 72 B rows: 8 B aligned
#pragma unroll
            for (int w = 0; w < ACTION_WORDS / 2; w++) row[w] = make_uint2((u32)a[2 * w], (u32)a[2 * w + 1]);
            dup[jc] = (bad || is_dup) ? 1 : 0;
            if (c == 0) rpid[j] = bad ? 0 : pid;
        }
        frozen = bad || is_dup;
    }
    if (frozen) a[0] = -1;
    uint2* row = reinterpret_cast<uint2*>(act + s * ACTION_WORDS);
#pragma unroll
    for (int w = 0; w < ACTION_WORDS / 2; w++) row[w] = make_uint2((u32)a[2 * w], (u32)a[2 * w + 1]);
    ctrl[s] = (frozen || !sh.determinise) ? 0 : pid;
    held[s] = frozen ? 1 : 0;
    steps[s] = frozen ? 0 : 1;                                  // the candidate's own step
}

// One lane per slot in use, behind the sampler that wrote the rows of the next step and in front of that step.
__global__ __launch_bounds__(PLAYOUT_BLOCK) void k_playout_hold(long used, const u8* __restrict__ done, u8* __restrict__ held, i32* __restrict__ act,
                                                                i32* __restrict__ steps) {
    const long s = (long)blockIdx.x * PLAYOUT_BLOCK + threadIdx.x;
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
        const St st(records, s);
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

static inline unsigned playout_blocks(long n) { return (unsigned)((n + PLAYOUT_BLOCK - 1) / PLAYOUT_BLOCK); }

hipError_t playout_launch_slots(const PlayoutShape& sh, const int32_t* games, long root_n, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_slots, dim3(playout_blocks(sh.used)), dim3(PLAYOUT_BLOCK), 0, stream, sh, games, root_n, ws.src_idx, ws.draw_off, ws.slot0);
    return hipGetLastError();
}
hipError_t playout_launch_expand(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_expand, dim3(playout_blocks(sh.sim_n)), dim3(PLAYOUT_BLOCK), 0, stream, sh, sim_records, (const long long*)ws.src_idx,
                       (const i32*)ws.by_builder, (const i32*)ws.by_trader, (const i32*)ws.by_random, ws.cand, ws.dup, ws.act, ws.ctrl, ws.held, ws.steps, ws.rpid);
    return hipGetLastError();
}
hipError_t playout_launch_hold(const PlayoutShape& sh, const uint8_t* done, const PlayoutWs& ws, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_hold, dim3(playout_blocks(sh.used)), dim3(PLAYOUT_BLOCK), 0, stream, sh.used, done, ws.held, ws.act, ws.steps);
    return hipGetLastError();
}
hipError_t playout_launch_score(const PlayoutShape& sh, const uint32_t* sim_records, const PlayoutWs& ws, int32_t* actions, int32_t* chosen,
                                long long* stats, hipStream_t stream) {
    hipLaunchKernelGGL(k_playout_score, dim3((unsigned)sh.rows), dim3(64), 0, stream, sh, sim_records, (const i32*)ws.cand, (const u8*)ws.dup,
                       (const i32*)ws.rpid, (const i32*)ws.steps, actions, chosen, stats);
    return hipGetLastError();
}

}  // namespace catan
