// catan_teacher.hip - kickstarting from the rule-based player: the three kernels that turn k_sample_scripted's actions
// into a training signal.  All opt-in; nothing here is launched unless a teacher is configured.
//
//   k_complete_action_rows  makes any legal action row teacher-forceable through the net's heads: the columns the row's type does
//                           NOT use (zero as the samplers leave them) become the lowest legal index of the mask the head would
//                           apply, so that no head evaluates log(0) on a row it then multiplies by 0 (-inf x 0 = NaN).  One lane per row.
//   k_collector_label       stores the teacher's row of a game at the slot k_collector_post stores the net's action in.  One lane per game.
//   k_imitation_loss        the imitation term -mean(lp) with its gradient and its read-out, one launch, conventions of k_ppo_diag.
//
// A translation unit of its own (compiled beside catan_abi.hip by _lib.build_library): these kernels are a second gfx950 code object of
// the library, and the code object every other kernel lives in is, byte for byte in .text, the one it is without them - placed inside
// catan_abi.hip, even behind every other kernel, they moved all of its code by a few KB, and with no teacher configured bench.py and the
// learner's step measured slower than the parent's spread.  Hence nothing of catan_kernels.hip is included: the layout
// constants come from catan_state.h, and the record's byte fields are read directly (view 1 of catan_kernels.hip, St).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "catan_state.h"
#include "catan_teacher.h"

namespace catan {

#define DEVI __device__ __forceinline__
constexpr int TEACH_BLOCK = 256;

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
DEVI int script_lowest(u64 v) { return v ? __ffsll((unsigned long long)v) - 1 : 0; }

// Which columns a row of type t uses is _ActionHeads.forward's table of head counts (policy.py): head 1 (column 1) Settlement / City,
// 2 Road, 3 MoveRobber, 4 PlayDev, 5 Respond, 6 Propose / Steal, 9 (column 15) Exchange or PlayDev with YoP / Monopoly, 10 (column 16)
// Exchange or PlayDev with YoP, 11 (column 17) Discard, 7 / 8 (columns 7..10, 11..14) Propose.  An unused column gets the lowest set
// bit of the mask row that forward() selects for the row (0 when that row is empty); used columns are never written.
// A row whose type is outside 0..12, whose game id is out of range or whose game waits inside a deferred sequence stays as it is.
__global__ __launch_bounds__(TEACH_BLOCK) void k_complete_action_rows(const u32* __restrict__ records, long n, const u32* __restrict__ mpk, const i32* __restrict__ games, long rows,
                                                                       const u8* __restrict__ busy, i32* __restrict__ actions) {
    const long j = (long)blockIdx.x * TEACH_BLOCK + threadIdx.x;
    if (j >= rows) return;
    const long e = games != nullptr ? (long)games[j] : j;
    if (e < 0 || e >= n || (busy != nullptr && busy[e] != 0)) return;
    uint2* row = reinterpret_cast<uint2*>(actions + j * ACTION_WORDS);    // 72 B rows: 8 B aligned
    int a[ACTION_WORDS];
#pragma unroll
    for (int i = 0; i < ACTION_WORDS / 2; i++) { const uint2 v = row[i]; a[2 * i] = (int)v.x; a[2 * i + 1] = (int)v.y; }
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
        const u8* b = reinterpret_cast<const u8*>(records + e * REC + NW);                      // the record's byte fields
        int me;                                                                                 // the deciding player (k_deciding)
        if (b[B_NDISC] > 0) me = b[B_DISC];
        else if (b[B_FLAGS] & F_MUST_RESPOND) me = b[B_TRADE_TGT];
        else me = b[B_GO];
        me &= 3;
        int first = 0;
#pragma unroll
        for (int r = 4; r >= 0; r--) first = b[B_PLAYER + me * PB + P_RES + r] > 0 ? r + 1 : first;
        a[7] = first; a[8] = 0; a[9] = 0; a[10] = 0;
        a[11] = first ? 1 : 0; a[12] = 0; a[13] = 0; a[14] = 0;
    }
#pragma unroll
    for (int i = 0; i < ACTION_WORDS / 2; i++) row[i] = make_uint2((u32)a[2 * i], (u32)a[2 * i + 1]);
}

// The teacher's row of game g goes where k_collector_post stores the net's action of the same decision: slot t = min(n_act[g], T - 1),
// for a game whose action the env consumes in this iteration and whose deciding seat is the active one.  Launched IN FRONT OF
// k_collector_post (it reads n_act before the increment and `live` as k_collector_pre left it).  Opponent seats are never labelled.
__global__ __launch_bounds__(TEACH_BLOCK) void k_collector_label(long n, int T, const long long* __restrict__ n_act, const u8* __restrict__ live,
                                                                  const long long* __restrict__ active_pid, const i32* __restrict__ deciding,
                                                                  const u8* __restrict__ waiting_before, const i32* __restrict__ labels,
                                                                  short* __restrict__ st_teacher) {
    const long g = (long)blockIdx.x * TEACH_BLOCK + threadIdx.x;
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

static inline unsigned teach_blocks(long n, int b) { return (unsigned)((n + b - 1) / b); }

hipError_t teacher_launch_complete(const uint32_t* records, long n, const uint32_t* mpk, const int32_t* games, long rows, const uint8_t* busy,
                                   int32_t* actions, hipStream_t stream) {
    hipLaunchKernelGGL(k_complete_action_rows, dim3(teach_blocks(rows, TEACH_BLOCK)), dim3(TEACH_BLOCK), 0, stream, records, n, mpk, games, rows, busy, actions);
    return hipGetLastError();
}
hipError_t teacher_launch_label(long n, int T, const long long* n_act, const uint8_t* live, const long long* active_pid, const int32_t* deciding,
                                const uint8_t* waiting_before, const int32_t* labels, short* st_teacher, hipStream_t stream) {
    hipLaunchKernelGGL(k_collector_label, dim3(teach_blocks(n, TEACH_BLOCK)), dim3(TEACH_BLOCK), 0, stream, n, T, n_act, live, active_pid, deciding, waiting_before,
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

}  // namespace catan
