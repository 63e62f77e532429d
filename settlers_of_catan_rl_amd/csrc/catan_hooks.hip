// catan_hooks.hip - the opt-in hooks of a finished game and of a re-deal: whole games recorded on the device, re-dealt
// games started from a pool of saved positions (8.11), the pool's weighted pick and its per-entry outcome tallies (8.12), round-robin
// tournaments seated and booked at the re-deal (8.16) - and, no hook but opt-in like them, the check of state blobs (8.17).  All opt-in: with no
// recorder enabled, no pool installed, no tournament enabled and no check asked for nothing here is launched.
//
// The library's THIRD translation unit and gfx950 code object, for the reason at the top of catan_players.hip: the first code object holds
// k_step and the learner's kernels and stays, byte for byte in .text, what it is without these hooks (profiles/hooks_unit.txt).  Nothing of
// catan_kernels.hip is included; what both units need comes from headers that emit no code (catan_state.h, catan_view.h, catan_game.h).
// All catan_abi.hip sees of this file is catan_hooks.h.
#include "catan_hooks.h"

namespace catan {

constexpr int HOOKS_BLOCK = 256;
static inline unsigned hooks_blocks(long n, int b) { return (unsigned)((n + b - 1) / b); }

// ================================================================================================ recorder
// A game's draws come from Philox keyed by (handle seed, global game id) and counted by the game's own draw counter, which sits in
// the state (W_RNG, blob word rng_draws).  So a start blob, the applied actions, the seed, the game id and catan_cfg_t reproduce the
// game bit for bit on a fresh one-game handle: nothing is added to k_step, the recorder only copies what the caller passes in.
//
// m slots (1..4096), each bound to one game (slot_of[game] = slot or -1: one lookup per listed game in the hooks).  A slot holds
//   header   4 x uint32: state (IDLE / WAIT_DEAL / RECORDING / SEALED), game, length (actions applied), flags (TRUNCATED, FROM_DEAL)
//   start    736 x int32: the blob export_game (k_export's routine) gives for the game when the recording starts
//   final    736 x int32: ... and when the game's last step is complete
//   log      capacity x 18 x int16 action words, then one uint32 guard word (RECORD_GUARD; checked by catan_record_status / _read)
// = 16 + 2 x 2 944 + 36 x capacity + 4 bytes of device memory per slot: 300 820 bytes (294 KiB) at the default capacity 8 192,
// 1.15 GiB for 4 096 such slots.
//
// int16 action words.  spec.MASK_SHAPES = (13,), (3, 54), (73,), (19,), (5,), (2,), (3, 3), (6,), (6,), (4, 5), (5,), (5,): every head of an
// action that the masks allow is an index into one of these, so every word of a legal action lies in [0, 72] (the type in [0, 12]; a
// negative type is the no-op and is never logged).  A mask-ILLEGAL action may carry any int32: its words are saturated to
// [-32 768, 32 767] (rec_sat16).  A saturated word is still outside [0, 72], so it indexes no head and the replay rejects the action as the
// live game did; words inside the int16 range, legal or not, are stored exactly.
// Where each kernel runs: the enqueue_* hooks of catan_abi_hooks.h, in the order enqueue_redeal (catan_abi.hip) states.
DEVI short rec_sat16(i32 v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }
DEVI void record_snapshot(const Ctx& c, long game, i32* blob) { export_game(St(c.R, c.N, game), BlobW{ blob, 1, 0, 0 }); }

// catan_record_enable: slot s takes games[s].  bad counts the ids outside [0, n) and the games listed twice (slot_of is all -1 before).
__global__ __launch_bounds__(HOOKS_BLOCK) void k_record_bind(long n, const i32* __restrict__ games, RecordBuf rb, u32* __restrict__ bad) {
    const int s = blockIdx.x * HOOKS_BLOCK + threadIdx.x;
    if (s >= rb.m) return;
    const long g = games[s];
    u32* h = rb.hdr + (long)s * RECORD_HDR_WORDS;
    h[REC_H_STATE] = REC_IDLE; h[REC_H_GAME] = (u32)g; h[REC_H_LENGTH] = 0u; h[REC_H_FLAGS] = 0u;
    *reinterpret_cast<u32*>(rb.log + (long)s * rb.log_stride + (long)rb.capacity * ACTION_WORDS) = RECORD_GUARD;
    if (g < 0 || g >= n) { atomicAdd(bad, 1u); return; }
    if (atomicCAS(&rb.slot_of[g], -1, s) != -1) atomicAdd(bad, 1u);
}
// catan_record_arm: slots[0..k-1] (null: slots 0..k-1).  now: the current state is the start and the slot records from the next applied
// action; else the slot waits for its game's next re-deal.
__global__ __launch_bounds__(64) void k_record_arm(Ctx c, RecordBuf rb, const i32* __restrict__ slots, int k, int now) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= k) return;
    const int s = slots ? slots[j] : j;
    if (s < 0 || s >= rb.m) return;
    u32* h = rb.hdr + (long)s * RECORD_HDR_WORDS;
    h[REC_H_LENGTH] = 0u; h[REC_H_FLAGS] = 0u;
    if (now) record_snapshot(c, (long)h[REC_H_GAME], rb.start + (long)s * STATE_WORDS);
    h[REC_H_STATE] = now ? REC_RECORDING : REC_WAIT_DEAL;
}
// One lane per slot, in front of the step's first kernel: a RECORDING slot appends its game's action row.  Not logged: the explicit no-op
// (negative type) and - busy != null, a deferred sequence - the action of a game that waits for its slow path, which k_classify_deferred
// ignores by the same test.  A waiting game's slot is not touched at all: a side stream may be sealing or opening it.
__global__ __launch_bounds__(64) void k_record_append(Ctx c, RecordBuf rb, const i32* __restrict__ actions, const u8* __restrict__ busy) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= rb.m) return;
    u32* h = rb.hdr + (long)s * RECORD_HDR_WORDS;
    const long g = (long)h[REC_H_GAME];                  // (written by k_record_bind only)
    if (g < 0 || g >= c.n) return;
    if (busy != nullptr && busy[g] != 0) return;
    if (h[REC_H_STATE] != REC_RECORDING) return;
    const i32* a = actions + g * ACTION_WORDS;
    if (a[0] < 0) return;
    const u32 len = h[REC_H_LENGTH];
    if (len < (u32)rb.capacity) {
        short* row = rb.log + (long)s * rb.log_stride + (long)len * ACTION_WORDS;
#pragma unroll
        for (int k = 0; k < ACTION_WORDS; k++) row[k] = rec_sat16(a[k]);
    } else h[REC_H_FLAGS] |= REC_F_TRUNCATED;
    h[REC_H_LENGTH] = len + 1u;
}
// list != null: one lane per game of a re-deal list (its length at *count_p), in front of the list's consumer - the records are still the
// final states.  list == null (handles without auto_reset): one lane per slot at the end of a stepping call; the game's step is complete
// with done = 1 (status != null, the deferred calls: and status 0; else: and the call's action was no no-op).
// A RECORDING slot writes its final blob and becomes SEALED.
__global__ __launch_bounds__(64) void k_record_seal(Ctx c, RecordBuf rb, const u32* __restrict__ count_p, const i32* __restrict__ list,
                                                    const u8* __restrict__ done, const u8* __restrict__ status, const i32* __restrict__ actions) {
    const u32 count = list ? *count_p : (u32)rb.m;
    for (u32 r = (u32)blockIdx.x * 64u + threadIdx.x; r < count; r += gridDim.x * 64u) {
        int s; long g;
        if (list) {
            g = list[r];
            if (g < 0 || g >= c.n) continue;
            s = rb.slot_of[g];
            if (s < 0 || s >= rb.m) continue;
        } else {
            s = (int)r;
            g = (long)rb.hdr[(long)s * RECORD_HDR_WORDS + REC_H_GAME];
            if (g < 0 || g >= c.n || done[g] == 0) continue;
            if (status != nullptr ? status[g] != 0 : actions[g * ACTION_WORDS] < 0) continue;
        }
        u32* h = rb.hdr + (long)s * RECORD_HDR_WORDS;
        if (h[REC_H_STATE] != REC_RECORDING) continue;
        record_snapshot(c, g, rb.fin + (long)s * STATE_WORDS);
        h[REC_H_STATE] = REC_SEALED;
    }
}
// Behind the consumer of a re-deal list, same list: a WAIT_DEAL slot takes the freshly dealt game as its start and records from here on.
__global__ __launch_bounds__(64) void k_record_open(Ctx c, RecordBuf rb, const u32* __restrict__ count_p, const i32* __restrict__ list) {
    const u32 count = *count_p;
    for (u32 r = (u32)blockIdx.x * 64u + threadIdx.x; r < count; r += gridDim.x * 64u) {
        const long g = list[r];
        if (g < 0 || g >= c.n) continue;
        const int s = rb.slot_of[g];
        if (s < 0 || s >= rb.m) continue;
        u32* h = rb.hdr + (long)s * RECORD_HDR_WORDS;
        if (h[REC_H_STATE] != REC_WAIT_DEAL) continue;
        record_snapshot(c, g, rb.start + (long)s * STATE_WORDS);
        h[REC_H_LENGTH] = 0u; h[REC_H_FLAGS] = REC_F_FROM_DEAL;
        h[REC_H_STATE] = REC_RECORDING;
    }
}

hipError_t record_launch_bind(long n, const i32* games, const RecordBuf& rb, u32* bad, hipStream_t stream) {
    hipLaunchKernelGGL(k_record_bind, dim3(hooks_blocks(rb.m, HOOKS_BLOCK)), dim3(HOOKS_BLOCK), 0, stream, n, games, rb, bad);
    return hipGetLastError();
}
hipError_t record_launch_arm(const Ctx& c, const RecordBuf& rb, const i32* slots, int k, int now, hipStream_t stream) {
    hipLaunchKernelGGL(k_record_arm, dim3(hooks_blocks(k, 64)), dim3(64), 0, stream, c, rb, slots, k, now);
    return hipGetLastError();
}
hipError_t record_launch_append(const Ctx& c, const RecordBuf& rb, const i32* actions, const u8* busy, hipStream_t stream) {
    hipLaunchKernelGGL(k_record_append, dim3(hooks_blocks(rb.m, 64)), dim3(64), 0, stream, c, rb, actions, busy);
    return hipPeekAtLastError();
}
hipError_t record_launch_seal(const Ctx& c, const RecordBuf& rb, const u32* count_p, const i32* list, const u8* done, const u8* status, const i32* actions, hipStream_t stream) {
    hipLaunchKernelGGL(k_record_seal, dim3(list ? RECORD_LIST_GRID : hooks_blocks(rb.m, 64)), dim3(64), 0, stream, c, rb, count_p, list, done, status, actions);
    return hipPeekAtLastError();
}
hipError_t record_launch_open(const Ctx& c, const RecordBuf& rb, const u32* count_p, const i32* list, hipStream_t stream) {
    hipLaunchKernelGGL(k_record_open, dim3(RECORD_LIST_GRID), dim3(64), 0, stream, c, rb, count_p, list);
    return hipPeekAtLastError();
}

// ================================================================================================ start pool
// A pool is m entries (1..65 536), each one position in the handle's own packed form: the record (REC words, hot and cold part, as
// k_import writes it) and the position's side row under the handle's limits (MPK_STRIDE words, as k_masks writes it: the mask words
// are its first MASK_WORDS).  = m x (704 + 128) bytes of device memory, plus (2 + m) x 8 bytes of counters.
//
// The install is a POST-PASS behind a re-deal: k_reset_list / k_install_list / k_reset have dealt the listed games exactly as they do
// without a pool (the deal consumes its draws), and then, on the same stream, for each listed game g:
//   d  = the game's draw counter as the deal left it (W_RNG);  id = env_id0 + g
//   o  = philox4x32_10(c0 = d, c1 = POOL_STREAM, c2 = lo32(id), c3 = hi32(id), k0 = lo32(seed), k1 = hi32(seed))
//        (the game's own stream has c1 = 0 and the random policy c1 = 1: this block is neither, and no draw is consumed)
//   (o[1] >> 16) < fresh_q16 : the fresh deal stays                                         -> counter [1]
//   else entry k             : the record becomes entry k's, EXCEPT W_RNG, which stays d;
//                              the side row's mask words become entry k's                    -> counters [0] and [2 + k]
// so that catan_state_export of the game equals pool blob k with rng_draws = d.  The pick depends on the seed, the global game id
// and d alone: every schedule makes the same picks.
//
// The pick, in integers.  Uniform: k = umulhi(o[0], m).  Weighted (catan_start_pool_set_weights): the weights are uint32 w[m] with sum
// W, 1 <= W <= 2^32 - 1; the handle keeps the inclusive prefix sums cum[k] = w[0] + ... + w[k] (k_pool_scan), t = umulhi(o[0], W) and the
// entry is the smallest k with cum[k] > t: an entry of weight 0 is never picked (cum[k] == cum[k - 1], so k - 1 already qualifies, and
// cum[0] == 0 is never above t), and with every weight 1 this is the uniform k.
//
// The search is a 64-ary search by ballot: the range [lo, lo + n) is cut into 64 chunks of ceil(n / 64) entries, lane l loads the LAST
// prefix sum of chunk l (the chunks behind the range's end collapse onto its last entry), and the first lane whose pivot is above t names
// the chunk that holds the answer.  cum[lo + n - 1] > t holds throughout (at the start it is W > t), so the ballot is never empty.  Three
// rounds - three dependent loads of a table of at most 256 KiB - cover 65 536 entries.  No LDS, no scratch.
//
// Copy shape: k_fork's.  A record is 44 chunks of 16 bytes and the masks are 2 chunks and 3 words; one wave takes one game, lane q < 44
// chunk q of the record, lanes 44 / 45 mask words 0..3 / 4..7, lane 46 mask words 8..10 (word 11 of a side row is not a mask word and
// everything from ROW_ACT on is the game's own, as in k_install_list).  The pick is wave-uniform: every lane computes it from the same
// d, once per game.  The counters are global atomics of lane 0 (a launch installs a handful of games).
//
// Outcomes.  origin[g] (int32 [n]) is the pool entry the game's current episode started from, -1 for a fresh deal; lane 0 of an install
// writes it.  k_pool_outcomes runs at the hook of k_episode_stats / k_league_stats (in front of a re-deal list's consumer, on its stream,
// while the listed records are the final states and origin[g] is still the finished episode's; the install that overwrites origin[g]
// follows on the same stream) and adds each finished game to a table of 2 + (m + 1) x PO_WORDS uint64 sums.

// catan_start_pool_set, behind k_import on the pool's own records: bad counts the finished positions
__global__ __launch_bounds__(HOOKS_BLOCK) void k_pool_count_finished(const u32* __restrict__ records, int m, u32* __restrict__ bad) {
    const long k = (long)blockIdx.x * HOOKS_BLOCK + threadIdx.x;
    if (k >= m) return;
    if (StRead(records, k).b(B_WINNER) != 0) atomicAdd(bad, 1u);
}

// catan_start_pool_set_weights: one workgroup.  Thread i owns the chunk [i * per, (i + 1) * per) of the weights: it sums the chunk, the
// workgroup scans the 1 024 chunk sums (a wave scan by shuffles, the 16 wave totals through LDS), and the thread writes its chunk's prefix
// sums.  Everything is summed in 64 bits, so that *total is exact (m x (2^32 - 1) < 2^48) and the host can refuse a sum above 2^32 - 1;
// cum holds the low words, which are the sums themselves wherever the total is accepted.
__global__ __launch_bounds__(POOL_SCAN_THREADS) void k_pool_scan(const u32* __restrict__ w, u32* __restrict__ cum, unsigned long long* __restrict__ total, int m) {
    __shared__ unsigned long long wave_sum[POOL_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (m + POOL_SCAN_THREADS - 1) / POOL_SCAN_THREADS;
    const int lo = tid * per < m ? tid * per : m, hi = lo + per < m ? lo + per : m;
    unsigned long long mine = 0ull;
    for (int i = lo; i < hi; i++) mine += w[i];
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long base = 0ull, all = 0ull;
#pragma unroll
    for (int i = 0; i < POOL_SCAN_THREADS / 64; i++) {
        const unsigned long long s = wave_sum[i];
        base += i < wave ? s : 0ull;
        all += s;
    }
    unsigned long long run = base + incl - mine;
    for (int i = lo; i < hi; i++) { run += w[i]; cum[i] = (u32)run; }
    if (tid == 0) *total = all;
}

// the entry for t < W = cum[m - 1]: the smallest k with cum[k] > t.  Wave-uniform: every lane gets the same t and returns the same k.
DEVI int pool_weighted_pick(const u32* __restrict__ cum, int m, u32 t, int lane) {
    int lo = 0, n = m;
    while (n > 1) {
        const int stride = (n + 63) >> 6;
        const int end = (lane + 1) * stride < n ? (lane + 1) * stride : n;      // one past chunk `lane`'s last entry (>= 1)
        const unsigned long long above = __ballot(cum[lo + end - 1] > t);
        if (above == 0ull) return lo + n - 1;                                    // (never: lane 63's pivot is the range's last entry, and that is above t)
        const int j = __ffsll(above) - 1;
        const int first = j * stride, stop = (j + 1) * stride < n ? (j + 1) * stride : n;
        lo += first; n = stop - first;
    }
    return lo;
}

// one wave, one freshly dealt game g (0 <= g < c.n); WEIGHTED: the weighted pick, ORIGIN: the origin word is written
template <bool WEIGHTED, bool ORIGIN>
DEVI void pool_install_game_x(const Ctx& c, u32* __restrict__ mpk, const StartPoolBuf& pb, const PoolPick& pp, long g, int lane) {
    const u32 d = c.R[g * REC + W_RNG];
    const u64 id = c.env_id0 + (u64)g;
    u32 o[4];
    philox4x32_10(d, POOL_STREAM, (u32)id, (u32)(id >> 32), c.key0, c.key1, o);
    if ((o[1] >> 16) < pb.fresh_q16) {
        if (lane == 0) {
            atomicAdd(pb.cnt + 1, 1ull);
            if (ORIGIN) pp.origin[g] = -1;
        }
        return;
    }
    const long k = WEIGHTED ? (long)pool_weighted_pick(pp.cum, pb.m, __umulhi(o[0], pp.W), lane) : (long)__umulhi(o[0], (u32)pb.m);
    if (lane < FORK_REC_CHUNKS) {
        const uint4 v = reinterpret_cast<const uint4*>(pb.rec + k * REC)[lane];
        reinterpret_cast<uint4*>(c.R + g * REC)[lane] = make_uint4(lane == W_RNG / 4 ? d : v.x, v.y, v.z, v.w);
    } else if (lane < FORK_REC_CHUNKS + 2) {
        reinterpret_cast<uint4*>(mpk + g * MPK_STRIDE)[lane - FORK_REC_CHUNKS] = reinterpret_cast<const uint4*>(pb.mask + k * MPK_STRIDE)[lane - FORK_REC_CHUNKS];
    } else if (lane == FORK_REC_CHUNKS + 2) {
        const u32* i3 = pb.mask + k * MPK_STRIDE + 8;
        u32* o3 = mpk + g * MPK_STRIDE + 8;
        const u32 a = i3[0], b = i3[1], w = i3[2];
        o3[0] = a; o3[1] = b; o3[2] = w;
    }
    if (lane == 0) {
        atomicAdd(pb.cnt, 1ull); atomicAdd(pb.cnt + 2 + k, 1ull);
        if (ORIGIN) pp.origin[g] = (i32)k;
    }
}

// behind the consumer of a re-deal list (k_reset_list / k_install_list), same stream, same list (its length at *count_p)
template <bool WEIGHTED, bool ORIGIN>
__global__ __launch_bounds__(64) void k_pool_install_list_x(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, PoolPick pp, const u32* __restrict__ count_p, const i32* __restrict__ list) {
    const u32 count = *count_p;
    for (u32 r = blockIdx.x; r < count; r += gridDim.x) {
        const long g = list[r];
        if (g < 0 || g >= c.n) continue;
        pool_install_game_x<WEIGHTED, ORIGIN>(c, mpk, pb, pp, g, (int)threadIdx.x);
    }
}
// behind catan_reset's k_reset and masks: the games with sel[g] != 0, or every game (sel == nullptr)
template <bool WEIGHTED, bool ORIGIN>
__global__ __launch_bounds__(64) void k_pool_install_sel_x(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, PoolPick pp, const u8* __restrict__ sel) {
    for (long g = blockIdx.x; g < c.n; g += gridDim.x) {
        if (sel != nullptr && sel[g] == 0) continue;
        pool_install_game_x<WEIGHTED, ORIGIN>(c, mpk, pb, pp, g, (int)threadIdx.x);
    }
}

// catan_state_import / catan_state_fork while outcomes are on: the games they overwrite did not come from the pick
__global__ __launch_bounds__(HOOKS_BLOCK) void k_pool_origin_clear(i32* __restrict__ origin, long n, const long* __restrict__ idx, long cnt) {
    const long i = (long)blockIdx.x * HOOKS_BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const long g = idx != nullptr ? idx[i] : i;
    if (g >= 0 && g < n) origin[g] = -1;
}

// One lane per finished game of `list` (its length at *count_p: the arguments of k_reset_list / k_install_list).  Plain global atomics: a
// pass finishes tens of games and up to 65 537 rows do not fit in LDS.  All counters are integer sums, independent of the order of arrival.
// focus: int32 [n] PlayerId per game (0: none), or null.
__global__ __launch_bounds__(64) void k_pool_outcomes(Ctx c, const u32* __restrict__ count_p, const i32* __restrict__ list, const i32* __restrict__ origin,
                                                      const i32* __restrict__ focus, unsigned long long* __restrict__ table, int m) {
    const u32 count = *count_p;
    if ((u32)blockIdx.x * 64u >= count) return;          // (wave-uniform: nothing listed for this wave)
    for (u32 r = (u32)blockIdx.x * 64u + threadIdx.x; r < count; r += gridDim.x * 64u) {
        const long e = list[r];
        if (e < 0 || e >= c.N) continue;
        atomicAdd(&table[PO_HEAD_SEEN], 1ull);
        int winner = 0, from = -2;
        unsigned long long turn = 0ull;
        if (e < c.n) {                                    // (origin has n rows; a padding game has none)
            const St s(c.R, c.N, e);
            winner = s.b(B_WINNER);
            turn = s.w(W_TURN);
            from = origin[e];
        }
        if (winner < 1 || winner > 4 || from < -1 || from >= m) { atomicAdd(&table[PO_HEAD_SKIPPED], 1ull); continue; }
        unsigned long long* const row = table + PO_HEAD + (size_t)(from < 0 ? m : from) * PO_WORDS;
        atomicAdd(&row[PO_GAMES], 1ull);
        atomicAdd(&row[PO_WINS_PLAYER + winner - 1], 1ull);
        const int f = focus != nullptr ? focus[e] : 0;
        if (f >= 1 && f <= 4) {
            atomicAdd(&row[PO_FOCUS_GAMES], 1ull);
            if (f == winner) atomicAdd(&row[PO_FOCUS_WINS], 1ull);
        }
        if (turn) atomicAdd(&row[PO_TURNS_SUM], turn);
    }
}

hipError_t pool_launch_count_finished(const u32* records, int m, u32* bad, hipStream_t stream) {
    hipLaunchKernelGGL(k_pool_count_finished, dim3(hooks_blocks(m, HOOKS_BLOCK)), dim3(HOOKS_BLOCK), 0, stream, records, m, bad);
    return hipGetLastError();
}
hipError_t pool_launch_scan(const u32* w, u32* cum, unsigned long long* total, int m, hipStream_t stream) {
    hipLaunchKernelGGL(k_pool_scan, dim3(1), dim3(POOL_SCAN_THREADS), 0, stream, w, cum, total, m);
    return hipGetLastError();
}
template <bool WEIGHTED, bool ORIGIN>
static void pool_install(const Ctx& c, u32* mpk, const StartPoolBuf& pb, const PoolPick& pp, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream) {
    if (count_p != nullptr)
        hipLaunchKernelGGL((k_pool_install_list_x<WEIGHTED, ORIGIN>), dim3(POOL_LIST_GRID), dim3(64), 0, stream, c, mpk, pb, pp, count_p, list);
    else
        hipLaunchKernelGGL((k_pool_install_sel_x<WEIGHTED, ORIGIN>), dim3((unsigned)(c.n < POOL_SEL_GRID_MAX ? c.n : POOL_SEL_GRID_MAX)), dim3(64), 0, stream, c, mpk, pb, pp, sel);
}
hipError_t pool_launch_install(const Ctx& c, u32* mpk, const StartPoolBuf& pb, const PoolPick& pp, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream) {
    const bool weighted = pp.cum != nullptr, origin = pp.origin != nullptr;
    if (weighted && origin) pool_install<true, true>(c, mpk, pb, pp, count_p, list, sel, stream);
    else if (weighted) pool_install<true, false>(c, mpk, pb, pp, count_p, list, sel, stream);
    else if (origin) pool_install<false, true>(c, mpk, pb, pp, count_p, list, sel, stream);
    else pool_install<false, false>(c, mpk, pb, pp, count_p, list, sel, stream);
    return hipPeekAtLastError();
}
hipError_t pool_launch_origin_clear(i32* origin, long n, const long* idx, long cnt, hipStream_t stream) {
    hipLaunchKernelGGL(k_pool_origin_clear, dim3(hooks_blocks(cnt, HOOKS_BLOCK)), dim3(HOOKS_BLOCK), 0, stream, origin, n, idx, cnt);
    return hipPeekAtLastError();
}
hipError_t pool_launch_outcomes(const Ctx& c, const u32* count_p, const i32* list, const i32* origin, const i32* focus, unsigned long long* table, int m, hipStream_t stream) {
    hipLaunchKernelGGL(k_pool_outcomes, dim3(POOL_OUTCOMES_GRID), dim3(64), 0, stream, c, count_p, list, origin, focus, table, m);
    return hipPeekAtLastError();
}

// ================================================================================================ tournament
// A table of L lineups, each four player ids; per game the handle keeps its lineup (-1: unseated), the lineup position that each
// PlayerId plays, and the number of episodes it has opened.  Both hooks take one lane per game and read or write nothing of the game's
// state but - the tally - the final record's winner, points, turn and order.
//
// The seating, in integers and without a draw.  Game g opens its k-th episode (k = episode[g], counted from 0) with
//   s = (env_id0 + g) * E + k          (E > 0: every game slot plays E episodes, so the s of all games and episodes are 0, 1, 2, ...)
//   s = (env_id0 + g) + k * 2^32       (E == 0: unlimited)
// both modulo 2^64; the lineup is s mod L and the seat permutation the ((s div L) mod 24)-th permutation of (0, 1, 2, 3) in
// lexicographic order: entry p of it is the lineup position PlayerId p+1 plays.  Any 24 L consecutive s meet every (lineup, permutation)
// pair once.  s depends on the global game id and the episode number alone: every schedule and every sharding seats alike.
// k == E > 0: the game becomes unseated - retired -, is counted once, and stays so.
//
// The permutation by its factorial digits: digit j picks among the positions still free, in ascending order (2 bits each in `avail`).
DEVI u32 tourney_perm(u32 idx) {
    const u32 d[3] = { idx / 6u, (idx % 6u) / 2u, idx & 1u };
    u32 avail = 0xE4u, out = 0u;                       // positions 3, 2, 1, 0
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const u32 sh = 2u * d[j];
        out |= ((avail >> sh) & 3u) << (2 * j);
        avail = (avail & ((1u << sh) - 1u)) | ((avail >> (sh + 2u)) << sh);
    }
    return out | ((avail & 3u) << 6);                  // 2 bits per PlayerId-1
}

// one lane, one freshly dealt game g (0 <= g < c.n)
DEVI void tourney_seat_game(const Ctx& c, const TourneyBuf& tb, long g) {
    unsigned long long* const tot = tb.table + (size_t)tb.L * TY_WORDS;
    const u32 k = tb.episode[g];
    if (tb.E != 0u && k >= tb.E) {
        tb.lineup_of[g] = -1;
        reinterpret_cast<int4*>(tb.pos_of_pid)[g] = make_int4(-1, -1, -1, -1);
        if (k == tb.E) { tb.episode[g] = tb.E + 1u; atomicAdd(&tot[TT_RETIRED], 1ull); }
        return;
    }
    const u64 id = c.env_id0 + (u64)g;
    const u64 s = tb.E != 0u ? id * (u64)tb.E + (u64)k : id + ((u64)k << 32);
    const u32 perm = tourney_perm((u32)((s / (u64)tb.L) % 24ull));
    tb.lineup_of[g] = (i32)(s % (u64)tb.L);
    reinterpret_cast<int4*>(tb.pos_of_pid)[g] = make_int4((int)(perm & 3u), (int)((perm >> 2) & 3u), (int)((perm >> 4) & 3u), (int)(perm >> 6));
    tb.episode[g] = k + 1u;
    atomicAdd(&tot[TT_SEATED], 1ull);
}
// Behind the consumer of a re-deal list, same stream, same list (count_p != null: its length at *count_p), and behind catan_reset's deal
// (count_p == null): the games with sel[g] != 0, or every game (sel == null).  One lane per game.
__global__ __launch_bounds__(64) void k_tourney_seat(Ctx c, TourneyBuf tb, const u32* __restrict__ count_p, const i32* __restrict__ list, const u8* __restrict__ sel) {
    const u32 count = count_p != nullptr ? *count_p : (u32)c.n;
    for (u32 r = (u32)blockIdx.x * 64u + threadIdx.x; r < count; r += gridDim.x * 64u) {
        const long g = count_p != nullptr ? (long)list[r] : (long)r;
        if (g < 0 || g >= c.n) continue;
        if (count_p == nullptr && sel != nullptr && sel[g] == 0) continue;
        tourney_seat_game(c, tb, g);
    }
}

// one finished game e into `acc` (the table or its LDS copy; `tot` its totals row).  skip_unseated: catan_reset's forms
DEVI void tourney_tally_game(const Ctx& c, const TourneyBuf& tb, unsigned long long* acc, unsigned long long* tot, long e, bool skip_unseated) {
    int lineup = -1, pos[4] = { -1, -1, -1, -1 }, used = 0;
    if (e < c.n) {                                        // (the arrays have n rows; a padding game has none)
        lineup = tb.lineup_of[e];
        const int4 v = reinterpret_cast<const int4*>(tb.pos_of_pid)[e];
        pos[0] = v.x; pos[1] = v.y; pos[2] = v.z; pos[3] = v.w;
#pragma unroll
        for (int p = 0; p < 4; p++) used |= (pos[p] >= 0 && pos[p] <= 3) ? 1 << pos[p] : 0;
    }
    const bool seated = lineup >= 0 && lineup < tb.L && used == 15;
    if (!seated && skip_unseated) return;
    atomicAdd(&tot[TT_SEEN], 1ull);
    if (!seated) { atomicAdd(&tot[TT_SKIPPED_UNSEATED], 1ull); return; }
    const St s(c.R, c.N, e);
    const int winner = s.b(B_WINNER);
    unsigned long long* const row = acc + (size_t)lineup * TY_WORDS;
    atomicAdd(&row[TY_GAMES], 1ull);
    if (winner < 1 || winner > 4) { atomicAdd(&row[TY_DRAWS], 1ull); atomicAdd(&tot[TT_DRAWS], 1ull); return; }
    atomicAdd(&tot[TT_TALLIED], 1ull);
    const int w0 = winner - 1;
    int wpos = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        wpos = w0 == p ? pos[p] : wpos;
        const int vp = s.pb(p, P_VP);
        if (vp) atomicAdd(&row[TY_VP + pos[p]], (unsigned long long)vp);
    }
    atomicAdd(&row[TY_WINS + wpos], 1ull);
    atomicAdd(&row[TY_WINS_BY_TURN + ((s.b(B_SEATOF) >> (2 * w0)) & 3)], 1ull);
    const unsigned long long turn = s.w(W_TURN);
    if (turn) atomicAdd(&row[TY_TURNS], turn);
}
// In front of the consumer of a re-deal list, beside k_league_stats and by its scheme: one lane per listed game; LDS_TABLE: the
// workgroup (one wave) accumulates in an LDS copy of the table and then issues ONE global atomic per non-zero entry; otherwise
// (L > TOURNEY_LDS_MAX_LINEUPS) every contribution is a global atomic of its own.  All sums are integer sums: the result does not
// depend on the order of arrival.
// count_p == null: in front of catan_reset's deal, the games with sel[g] != 0 (sel == null: every game).  The seated ones among them
// are booked - as draws, unless they just ended, and a handle with auto_reset re-deals those itself -; an unseated one is no finished
// game (its reset is what seats it) and is passed over.
template <bool LDS_TABLE>
__global__ __launch_bounds__(64) void k_tourney_tally(Ctx c, TourneyBuf tb, const u32* __restrict__ count_p, const i32* __restrict__ list, const u8* __restrict__ sel) {
    __shared__ unsigned long long lds[LDS_TABLE ? TOURNEY_LDS_ROWS * TY_WORDS : 1];
    const int lane = threadIdx.x;
    const u32 count = count_p != nullptr ? *count_p : (u32)c.n;
    if ((u32)blockIdx.x * 64u >= count) return;          // (wave-uniform: nothing listed for this wave)
    const int words = (tb.L + 1) * TY_WORDS;             // (the host launches LDS_TABLE only where this fits)
    unsigned long long* const acc = LDS_TABLE ? lds : tb.table;
    if (LDS_TABLE) {
        for (int i = lane; i < words; i += 64) lds[i] = 0ull;
        __syncthreads();
    }
    for (u32 r = (u32)blockIdx.x * 64u + (u32)lane; r < count; r += gridDim.x * 64u) {
        const long e = count_p != nullptr ? (long)list[r] : (long)r;
        if (e < 0 || e >= c.N) continue;
        if (count_p == nullptr && sel != nullptr && sel[e] == 0) continue;
        tourney_tally_game(c, tb, acc, acc + (size_t)tb.L * TY_WORDS, e, count_p == nullptr);
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int i = lane; i < words; i += 64) {
            const unsigned long long v = lds[i];
            if (v != 0ull) atomicAdd(&tb.table[i], v);
        }
    }
}

// catan_reset's forms: one lane per game of the handle, up to TOURNEY_SEL_GRID_MAX waves, grid-stride beyond
static unsigned tourney_grid(const Ctx& c, const u32* count_p) {
    if (count_p != nullptr) return TOURNEY_GRID;
    const unsigned b = hooks_blocks(c.n, 64);
    return b < (unsigned)TOURNEY_SEL_GRID_MAX ? b : (unsigned)TOURNEY_SEL_GRID_MAX;
}
hipError_t tourney_launch_tally(const Ctx& c, const TourneyBuf& tb, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream) {
    if (tb.L <= TOURNEY_LDS_MAX_LINEUPS)
        hipLaunchKernelGGL(k_tourney_tally<true>, dim3(tourney_grid(c, count_p)), dim3(64), 0, stream, c, tb, count_p, list, sel);
    else
        hipLaunchKernelGGL(k_tourney_tally<false>, dim3(tourney_grid(c, count_p)), dim3(64), 0, stream, c, tb, count_p, list, sel);
    return hipPeekAtLastError();
}
hipError_t tourney_launch_seat(const Ctx& c, const TourneyBuf& tb, const u32* count_p, const i32* list, const u8* sel, hipStream_t stream) {
    hipLaunchKernelGGL(k_tourney_seat, dim3(tourney_grid(c, count_p)), dim3(64), 0, stream, c, tb, count_p, list, sel);
    return hipPeekAtLastError();
}

// ================================================================================================ state check
// k_state_check: the rules of spec.STATE_CHECK_RULES (restated in include/catan_hip_tuning.h) over blobs in catan_state_import's
// orientation, int32 [736][cnt].  One lane per blob: word k of the wave's 64 blobs is 256 contiguous bytes, every load is coalesced, and
// a blob is 2 944 bytes in and 8 bytes out.  No handle, no record, no LDS, no scratch: boards are bitboards as in catan_state.h, the
// neighbour tests are catan_topology.inc's generated helpers, and the players' loop is NOT unrolled - what it keeps per player (hands,
// hidden-card counts) is written by the predicated assignment k_import uses for cnt5, `x[q] = q == p ? v : x[q]`, and read by sc_pick.
//
// TOTAL ON EVERY INPUT.  A word that has a range rule goes through sc_range the moment it is loaded: outside the range it sets the range
// bit and becomes THE LOWEST VALUE OF ITS RANGE for all that follows, so a shift count, a selector or a length is always inside its
// range.  Cards behind a length and trade resources behind a count are loaded and ignored.  The words without a range rule (the four
// counts of turns / actions / trades / draws, bought_this_turn, lr_count, la_count, cur_longest_path, cur_army_size, curr_vps, pP_vp) are
// only compared, or summed in 64 bits.  No loop bound and no address depends on a blob word.
//
// The rules themselves, state_check_blob, stand in catan_state_check.h: one blob in, its violation word out, nothing of the device in it,
// so that tools/native/state_check_host.cpp compiles the very same lines for the host (tests/test_state_check_host_cpu.py runs them
// under the undefined-behaviour sanitizer over every single-word corruption).
#define CATAN_TABLE static __device__ __constant__ const
#define CATAN_FN static __device__ __forceinline__
#define CATAN_TOPOLOGY_CODE
}  // namespace catan
#include "catan_topology.inc"
#define CATAN_STATE_CHECK_CODE
#include "catan_state_check.h"
namespace catan {

__global__ __launch_bounds__(64) void k_state_check(const i32* __restrict__ blob, long cnt, u64* __restrict__ viol, unsigned long long* __restrict__ n_bad) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    u64 v = 0ull;
    if (i < cnt) {
        v = state_check_blob(ScBlob{ blob, cnt, i });
        viol[i] = v;
    }
    if (n_bad != nullptr) {                               // one atomic per wave that saw a bad blob
        const unsigned long long bad_lanes = __ballot(v != 0ull);
        if (bad_lanes != 0ull && threadIdx.x == (unsigned)(__ffsll(bad_lanes) - 1)) atomicAdd(n_bad, (unsigned long long)__popcll(bad_lanes));
    }
}

hipError_t state_check_launch(const i32* blob, long cnt, u64* viol, unsigned long long* n_bad, hipStream_t stream) {
    hipLaunchKernelGGL(k_state_check, dim3(hooks_blocks(cnt, 64)), dim3(64), 0, stream, blob, cnt, viol, n_bad);
    return hipGetLastError();
}

}  // namespace catan
