// catan_start_pool_weighted.hip - the start pool's weighted pick and its per-entry outcome tallies (catan_start_pool_set_weights,
// catan_start_pool_outcomes_*, include/catan_hip_tuning.h).  Built beside catan_start_pool.hip, whose kernels keep their
// code: a handle with no weights set and outcomes off launches none of the kernels below.
//
// Weighted pick, in integers.  Weights are uint32 w[m] with sum W, 1 <= W <= 2^32 - 1; the handle keeps the inclusive prefix sums
// cum[k] = w[0] + ... + w[k] (k_pool_scan).  The Philox block o, its counter words, its key and the freshness test on o[1] are 8.11's.
// Where the deal does not stay fresh, t = umulhi(o[0], W) and the entry is the smallest k with cum[k] > t: an entry of weight 0 is never
// picked (cum[k] == cum[k - 1], so k - 1 already qualifies, and cum[0] == 0 is never above t), and with every weight 1 this is 8.11's
// k = umulhi(o[0], m).  The pick depends on (seed, global game id, d) alone.
//
// The search is a 64-ary search by ballot: the range [lo, lo + n) is cut into 64 chunks of ceil(n / 64) entries, lane l loads the LAST
// prefix sum of chunk l (the chunks behind the range's end collapse onto its last entry), and the first lane whose pivot is above t names
// the chunk that holds the answer.  cum[lo + n - 1] > t holds throughout (at the start it is W > t), so the ballot is never empty.  Three
// rounds - three dependent loads of a table of at most 256 KiB - cover 65 536 entries.  No LDS, no scratch.
//
// Outcomes.  origin[g] (int32 [n]) is the pool entry the game's current episode started from, -1 for a fresh deal; lane 0 of an install
// writes it.  k_pool_outcomes runs at the hook of k_episode_stats / k_league_stats (in front of a re-deal list's consumer, on its stream,
// while the listed records are the final states and origin[g] is still the finished episode's; the install that overwrites origin[g]
// follows on the same stream) and adds each finished game to a table of 2 + (m + 1) x PO_WORDS uint64 sums.
//
// Included behind every other kernel file, and every kernel here is a template first used at the very end of catan_abi.hip.
#pragma once

namespace catan {

// Columns of an entry's row of the outcome table (restated in include/catan_hip_tuning.h and spec.py START_POOL_OUTCOME_FIELDS); row m is
// the fresh deals', and two head words stand in front of the rows
constexpr int PO_GAMES = 0;              // games finished
constexpr int PO_WINS_PLAYER = 1;        // +PlayerId-1 (4)
constexpr int PO_FOCUS_GAMES = 5;        // games with a focus PlayerId in 1..4
constexpr int PO_FOCUS_WINS = 6;         // ... that the focus player won
constexpr int PO_TURNS_SUM = 7;          // sum of the final W_TURN (k_episode_stats' game length)
constexpr int PO_WORDS = 8;
constexpr int PO_HEAD_SEEN = 0, PO_HEAD_SKIPPED = 1, PO_HEAD = 2;
constexpr int POOL_OUTCOMES_GRID = LEAGUE_STATS_GRID;
constexpr int POOL_SCAN_THREADS = 1024;
static_assert(POOL_MAX_ENTRIES <= POOL_SCAN_THREADS * 64, "one workgroup scans the weights: at most 64 per thread");

struct PoolPick {
    const u32* cum;              // [m] inclusive prefix sums of the weights, or nullptr (uniform)
    u32 W;                       // their sum, cum[m - 1]
    i32* origin;                 // [n] or nullptr (outcomes off)
};

// catan_start_pool_set_weights: one workgroup.  Thread i owns the chunk [i * per, (i + 1) * per) of the weights: it sums the chunk, the
// workgroup scans the 1 024 chunk sums (a wave scan by shuffles, the 16 wave totals through LDS), and the thread writes its chunk's prefix
// sums.  Everything is summed in 64 bits, so that *total is exact (m x (2^32 - 1) < 2^48) and the host can refuse a sum above 2^32 - 1;
// cum holds the low words, which are the sums themselves wherever the total is accepted.
template <int AT_THE_END = 0>
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

// pool_install_game with the weighted rule (WEIGHTED) and the origin word (ORIGIN); the copy is its copy
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
        reinterpret_cast<uint4*>(mpk + g * MPK_STRIDE)[lane - FORK_REC_CHUNKS] = reinterpret_cast<const uint4*>(pb.mask + k * POOL_MASK_STRIDE)[lane - FORK_REC_CHUNKS];
    } else if (lane == FORK_REC_CHUNKS + 2) {
        const u32* i3 = pb.mask + k * POOL_MASK_STRIDE + 8;
        u32* o3 = mpk + g * MPK_STRIDE + 8;
        const u32 a = i3[0], b = i3[1], w = i3[2];
        o3[0] = a; o3[1] = b; o3[2] = w;
    }
    if (lane == 0) {
        atomicAdd(pb.cnt, 1ull); atomicAdd(pb.cnt + 2 + k, 1ull);
        if (ORIGIN) pp.origin[g] = (i32)k;
    }
}

// k_pool_install_list / k_pool_install_sel for a handle with weights set, outcomes on, or both
template <bool WEIGHTED, bool ORIGIN>
__global__ __launch_bounds__(64) void k_pool_install_list_x(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, PoolPick pp, const u32* __restrict__ count_p, const i32* __restrict__ list) {
    const u32 count = *count_p;
    for (u32 r = blockIdx.x; r < count; r += gridDim.x) {
        const long g = list[r];
        if (g < 0 || g >= c.n) continue;
        pool_install_game_x<WEIGHTED, ORIGIN>(c, mpk, pb, pp, g, (int)threadIdx.x);
    }
}
template <bool WEIGHTED, bool ORIGIN>
__global__ __launch_bounds__(64) void k_pool_install_sel_x(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, PoolPick pp, const u8* __restrict__ sel) {
    for (long g = blockIdx.x; g < c.n; g += gridDim.x) {
        if (sel != nullptr && sel[g] == 0) continue;
        pool_install_game_x<WEIGHTED, ORIGIN>(c, mpk, pb, pp, g, (int)threadIdx.x);
    }
}

// catan_state_import / catan_state_fork while outcomes are on: the games they overwrite did not come from the pick
template <int AT_THE_END = 0>
__global__ __launch_bounds__(BLOCK) void k_pool_origin_clear(i32* __restrict__ origin, long n, const long* __restrict__ idx, long cnt) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    const long g = idx != nullptr ? idx[i] : i;
    if (g >= 0 && g < n) origin[g] = -1;
}

// One lane per finished game of `list` (its length at *count_p: the arguments of k_reset_list / k_install_list).  Plain global atomics: a
// pass finishes tens of games and up to 65 537 rows do not fit in LDS.  All counters are integer sums, independent of the order of arrival.
// focus: int32 [n] PlayerId per game (0: none), or null.
template <int AT_THE_END = 0>
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

}  // namespace catan
