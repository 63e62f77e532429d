// catan_record.hip - whole games recorded on the device (catan_record_*, include/catan_hip_tuning.h).
//
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
//
// Hooks (catan_abi.hip).  k_record_append runs on the call's stream in front of the step's first kernel that reads the actions.
// k_record_seal runs beside k_episode_stats in front of every consumer of a re-deal list (k_reset_list / k_install_list), on the
// consumer's stream, and - handles without auto_reset - at the end of the stepping calls over their done flags.  k_record_open runs
// behind the same consumers with the same list.  Off (the default) nothing is launched.
//
// Included behind every other kernel file, and every kernel here is a template (AT_THE_END, never anything but 0) that is first used at the
// end of catan_abi.hip: that puts their code behind every other kernel's in the code object (see there).  k_export's body moved into export_game (catan_kernels.hip) so that a snapshot IS an export;
// its compiled code is unchanged (profiles/record_kernel_resources.txt).
#pragma once

namespace catan {

constexpr u32 REC_IDLE = 0, REC_WAIT_DEAL = 1, REC_RECORDING = 2, REC_SEALED = 3;
constexpr u32 REC_F_TRUNCATED = 1, REC_F_FROM_DEAL = 2, REC_F_GUARD_BROKEN = 4;   // (the last one is set by the host reads only)
constexpr u32 RECORD_GUARD = 0x5EA1C0DEu;
constexpr int RECORD_MAX_SLOTS = 4096, RECORD_MAX_CAPACITY = 65535, RECORD_HDR_WORDS = 4;
constexpr int RECORD_LIST_GRID = 8;      // one lane per listed game, 512 per round, grid-stride beyond (as EPISODE_STATS_GRID)
enum { REC_H_STATE = 0, REC_H_GAME = 1, REC_H_LENGTH = 2, REC_H_FLAGS = 3 };

struct RecordBuf {
    u32* hdr;          // [m][RECORD_HDR_WORDS]
    i32* slot_of;      // [N] game -> slot, -1: none
    i32* start;        // [m][STATE_WORDS]
    i32* fin;          // [m][STATE_WORDS]
    short* log;        // [m][log_stride]: capacity rows of ACTION_WORDS int16, then the guard word
    i32* arm_list;     // [m] scratch: the slots of a catan_record_arm call
    int m, capacity;
    long log_stride;   // int16 elements per slot = capacity * ACTION_WORDS + 2
};
DEVI short rec_sat16(i32 v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }
DEVI void record_snapshot(const Ctx& c, long game, i32* blob) { export_game(St(c.R, c.N, game), BlobW{ blob, 1, 0, 0 }); }

// catan_record_enable: slot s takes games[s].  bad counts the ids outside [0, n) and the games listed twice (slot_of is all -1 before).
template <int AT_THE_END = 0>
__global__ __launch_bounds__(BLOCK) void k_record_bind(long n, const i32* __restrict__ games, RecordBuf rb, u32* __restrict__ bad) {
    const int s = blockIdx.x * BLOCK + threadIdx.x;
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
template <int AT_THE_END = 0>
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
template <int AT_THE_END = 0>
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
template <int AT_THE_END = 0>
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
template <int AT_THE_END = 0>
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

}  // namespace catan
