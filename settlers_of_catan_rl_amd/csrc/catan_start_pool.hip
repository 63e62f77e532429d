// catan_start_pool.hip - re-dealt games started from a pool of saved positions (catan_start_pool_*, include/catan_hip_tuning.h;
// DESIGN.md 8.11).
//
// A pool is m entries (1..65 536), each one position in the handle's own packed form: the record (REC words, hot and cold part, as
// k_import writes it) and the position's mask words under the handle's limits (MASK_WORDS, in a row of POOL_MASK_STRIDE words).
// = m x (704 + 48) bytes of device memory, plus (2 + m) x 8 bytes of counters.
//
// The install is a POST-PASS behind a re-deal: k_reset_list / k_install_list / k_reset have dealt the listed games exactly as they do
// without a pool (the deal consumes its draws), and then, on the same stream, for each listed game g:
//   d  = the game's draw counter as the deal left it (W_RNG);  id = env_id0 + g
//   o  = philox4x32_10(c0 = d, c1 = POOL_STREAM, c2 = lo32(id), c3 = hi32(id), k0 = lo32(seed), k1 = hi32(seed))
//        (the game's own stream has c1 = 0 and the random policy c1 = 1: this block is neither, and no draw is consumed)
//   (o[1] >> 16) < fresh_q16 : the fresh deal stays                                         -> counter [1]
//   else k = umulhi(o[0], m) : the record becomes entry k's, EXCEPT W_RNG, which stays d;
//                              the side row's mask words become entry k's                    -> counters [0] and [2 + k]
// so that catan_state_export of the game equals pool blob k with rng_draws = d.  The pick depends on the seed, the global game id
// and d alone: every schedule makes the same picks.
//
// Copy shape: k_fork's.  A record is 44 chunks of 16 bytes and the masks are 2 chunks and 3 words; one wave takes one game, lane q < 44
// chunk q of the record, lanes 44 / 45 mask words 0..3 / 4..7, lane 46 mask words 8..10 (word 11 of a side row is not a mask word and
// everything from ROW_ACT on is the game's own, as in k_install_list).  The pick is wave-uniform: every lane computes it from the same
// d, once per game.  No LDS; the counters are global atomics of lane 0 (a launch installs a handful of games).
//
// Included behind every other kernel file, and every kernel here is a template (AT_THE_END, never anything but 0) first used at the end
// of catan_abi.hip, so that their code follows every other kernel's in the code object.
#pragma once

namespace catan {

constexpr u32 POOL_STREAM = 0x504F4F4Cu;          // "POOL": the c1 word of the pick's Philox block
constexpr int POOL_MAX_ENTRIES = 65536, POOL_MASK_STRIDE = 12;
constexpr u32 POOL_Q16_ONE = 65536u;
constexpr int POOL_LIST_GRID = 64;                // one wave per listed game, grid-stride beyond
constexpr int POOL_COPY_LANES = FORK_REC_CHUNKS + 3;
static_assert(POOL_MASK_STRIDE % 4 == 0 && POOL_MASK_STRIDE >= MASK_WORDS && POOL_MASK_STRIDE <= ROW_ACT && POOL_COPY_LANES <= 64,
              "a pool mask row is three 16-byte chunks that fit in front of a side row's action words; a wave copies one game");

struct StartPoolBuf {
    u32* rec;                    // [m][REC]
    u32* mask;                   // [m][POOL_MASK_STRIDE]
    unsigned long long* cnt;     // [2 + m]: pool deals, fresh deals, installs per entry
    int m;
    u32 fresh_q16;               // 0..65 536
};

// catan_start_pool_set, behind k_import on the pool's own records: entry k's masks under the handle's limits; bad counts finished positions
template <int AT_THE_END = 0>
__global__ __launch_bounds__(BLOCK) void k_pool_masks(StartPoolBuf pb, Limits lim, u32* __restrict__ bad) {
    const long k = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= pb.m) return;
    St s(pb.rec, (long)pb.m, k);
    if (s.b(B_WINNER) != 0) atomicAdd(bad, 1u);
    u32 m[MASK_WORDS];
    compute_masks(s, m, lim);
    u32* row = pb.mask + k * POOL_MASK_STRIDE;
#pragma unroll
    for (int i = 0; i < MASK_WORDS; i++) row[i] = m[i];
    for (int i = MASK_WORDS; i < POOL_MASK_STRIDE; i++) row[i] = 0u;
}

// one wave, one freshly dealt game g (0 <= g < c.n)
DEVI void pool_install_game(const Ctx& c, u32* __restrict__ mpk, const StartPoolBuf& pb, long g, int lane) {
    const u32 d = c.R[g * REC + W_RNG];
    const u64 id = c.env_id0 + (u64)g;
    u32 o[4];
    philox4x32_10(d, POOL_STREAM, (u32)id, (u32)(id >> 32), c.key0, c.key1, o);
    if ((o[1] >> 16) < pb.fresh_q16) {
        if (lane == 0) atomicAdd(pb.cnt + 1, 1ull);
        return;
    }
    const long k = (long)__umulhi(o[0], (u32)pb.m);              // < m
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
    if (lane == 0) { atomicAdd(pb.cnt, 1ull); atomicAdd(pb.cnt + 2 + k, 1ull); }
}

// behind the consumer of a re-deal list (k_reset_list / k_install_list), same stream, same list (its length at *count_p)
template <int AT_THE_END = 0>
__global__ __launch_bounds__(64) void k_pool_install_list(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, const u32* __restrict__ count_p, const i32* __restrict__ list) {
    const u32 count = *count_p;
    for (u32 r = blockIdx.x; r < count; r += gridDim.x) {
        const long g = list[r];
        if (g < 0 || g >= c.n) continue;
        pool_install_game(c, mpk, pb, g, (int)threadIdx.x);
    }
}
// behind catan_reset's k_reset and masks: the games with sel[g] != 0, or every game (sel == nullptr)
template <int AT_THE_END = 0>
__global__ __launch_bounds__(64) void k_pool_install_sel(Ctx c, u32* __restrict__ mpk, StartPoolBuf pb, const u8* __restrict__ sel) {
    for (long g = blockIdx.x; g < c.n; g += gridDim.x) {
        if (sel != nullptr && sel[g] == 0) continue;
        pool_install_game(c, mpk, pb, g, (int)threadIdx.x);
    }
}

}  // namespace catan
