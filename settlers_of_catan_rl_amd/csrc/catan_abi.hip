// catan_abi.hip - host side of libcatan_hip.so: the kernel files of the first code object, then the host code of the C ABI in five files
// included below them.  This file itself keeps the handle and everything that schedules (include/catan_hip.h, and the tuning and
// profiling entry points of include/catan_hip_tuning.h); catan_abi_base.h: what every host file needs; catan_abi_nn_launch.h and
// catan_abi_nn.h: the net's launch templates and entry points (include/catan_hip_nn.h); catan_abi_hooks.h: what hangs on a re-deal;
// catan_abi_players.h: the players.  Where each is included is part of the build: the order in which the unit first uses its kernel
// templates is the order of the kernels in the code object (catan_abi_nn_launch.h).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/catan_hip.h"
#include "../../include/catan_hip_nn.h"
#include "../../include/catan_hip_tuning.h"
#include "catan_kernels.hip"
#include "catan_obs.hip"
#include "catan_ppo.hip"
#include "catan_nn.hip"
#include "catan_tile_encoder.hip"
#include "catan_heads.hip"
#include "catan_collector.hip"
#include "catan_rows.hip"
#include "catan_te_bwd.hip"
#include "catan_optim.hip"
#include "catan_wgrad_big.hip"
#include "catan_stats.hip"
#include "catan_scripted.hip"
#include "catan_league_stats.hip"
#include "catan_players.h"
#include "catan_hooks.h"

using namespace catan;
#include "catan_abi_base.h"
#include "catan_abi_nn_launch.h"

// Every scheduling knob of a handle (results never depend on any of them).  Filled once, by sched_from_env at catan_create: the defaults below, then
// the environment switches listed in include/catan_hip_tuning.h; the catan_set_* entry points write the same fields afterwards.
struct Sched {
    int step_games;       // games per k_step wave: 64, 32 or 16 (catan_set_step_wave_games, CATAN_STEP_WAVE_GAMES)
    int step_bin_order;   // k_step: longest-lasting bins first (StepCfg::bin_order; CATAN_STEP_BIN_ORDER)
    int deferred_fused;   // the library's own deferred loop in its fused-sampling form (catan_set_deferred_fused, CATAN_DEFERRED_FUSED)
    int fused_subs;       // ... its sub-lists per bin (CATAN_FUSED_SUBS: 1, 2, 4, 8 or 16; Pending::nsub while that loop runs)
    int t1_group;         // the sampler form of that loop: passes per tier-1 launch, 2 or 1 (CATAN_T1_GROUP)
    int t1_delay_us;      // the fused-sampling loop: tier 1 staggered this many microseconds behind the group's last k_step (CATAN_T1_DELAY_US; <= 0: not staggered)
    int lr_split;         // tier 1 as search (k_lr_finish<LRF_SPLIT>) + lane-per-game completion (k_lr_complete): 0 never, 1 where a launch has two passes, 2 everywhere (CATAN_LR_SPLIT)
    int lr_grid;          // workgroups of k_lr_finish in every schedule (CATAN_LR_GRID, >= 64), or 0: each schedule's own (LR_GRID, LR_GRID_DEFERRED, LR_GRID_FUSED)
    int lr_mid_budget;    // deferred windows: the middle tier's budget (0: off), and k_lr_heavy's workgroups behind it (CATAN_LR_MID_BUDGET, CATAN_LR_MID_HEAVY_GRID)
    int lr_mid_heavy_grid;
    int lr_budget[3];     // tier-1 longest-road iteration budget: [0] lock-step, [1] deferred (tails are amortised there), [2] the fused-sampling loop (catan_set_lr_budgets)
    int lr_round[2];      // tier-2 iterations per bulk-synchronous round: [0] lock-step, [1] deferred (catan_set_lr_rounds)
};

struct catan_env {
    int device;
    long n, N;
    Ctx ctx;
    catan_cfg_t cfg;
    Sched sched;
    std::vector<void*> owned;   // every device allocation of catan_create (dev_alloc), freed by catan_destroy
    void* state;          // W rows then B rows
    u32* mpk;             // packed masks [N][16]
    u32* spec_state;      // shadow records / masks for speculative re-deals inside a lock-step step (enqueue_slow)
    u32* spec_mpk;
    u32 spec_epoch;       // lock-step step counter: tags the shadows of a step
    int ctr_clean;        // lock-step: the counters are maintained by the kernels themselves (no memset per step) once set
    int lock_parity;      // ... and the sort alternates between its two count sets
    u32* err;             // invalid-action counter
    double* reward64;     // caller-owned [n][4] unrounded rewards of catan_step (catan_set_reward_f64_buffer), or NULL
    // scratch for catan_random_rollout
    i32* scratch_actions; // [n][18]
    float* scratch_reward;// [n][4]
    u8* scratch_done;     // [n]
    Pending pend;         // tier-2 longest-road hand-off (device arrays)
    unsigned long long* prof; // device [12] phase profile of k_step, enabled by catan_profile_enable
    int prof_on;
    int g_open, g_slot, g_passes; int64_t g_count;   // the sampler form of the library's own deferred loop: its running tier-1 group
    u32* prof_wave;       // [N/64][8] per-wave phase ticks of the last k_step (catan_profile_enable(env, 2))
    u32* pctr;            // [N] per-game decision counters of the random policy (deferred rollouts)
    hipStream_t side;     // re-deals run here, concurrently with the longest-road kernels on the caller's stream
    hipEvent_t ev_fork, ev_join;
    hipStream_t fstream;  // deferred rollouts: tier-1 longest road + completion run here during the passes that follow
    hipEvent_t ev_fready[3], ev_fdone[3];   // per tier-1 slot (the sampler loop with a tier-1 launch per pass rotates three)
    float* f_reward;      // [n][4] / [n]: outputs of the completions that run on fstream (scratch)
    u8* f_done;
    hipStream_t sstream;  // deferred rollouts: tier 2 + re-deals of window w run here during window w+1
    hipEvent_t ev_sdone[2];
    float* s_reward;      // outputs of the completions that run on sstream (scratch)
    u8* s_done;
    // catan_step_deferred / catan_step_flush: the deferred schedule for caller-supplied actions
    int64_t d_it;         // calls since the last flush (0: no deferred sequence is open)
    int d_window;         // its window length
    hipStream_t d_stream; // ... and the caller's stream (one stream per sequence)
    MtPair* mt_dev;       // RNG contract (A): the handle's two MT19937 generators on the device (catan_seed_mt19937), else NULL
    BoardCfg* bcfg_dev;   // catan_set_board_configs: the layout table and the games' indices into it (ctx.bcfg / ctx.bcfg_idx), else NULL
    u8* bcfg_idx_dev;
    unsigned long long* stats;   // catan_episode_stats_enable: the block of ES_WORDS counters (catan_stats.hip), allocated at the first enable
    const i32* stats_focus;      // ... the caller's focus array (device int32 [n]) or NULL
    int stats_on;
    unsigned long long* lstats;  // catan_league_stats_enable: the table of (lstats_nets + 1) x LS_WORDS counters (catan_league_stats.hip); not in `owned`: it grows
    const i32* lstats_slot;      // ... the caller's maps (device int32 [n][4] and [n][3])
    const i32* lstats_net;
    int lstats_nets, lstats_cap; // rows in use (without the totals row), and allocated
    int lstats_on;               // 0 off, else the mode bits of catan_league_stats_enable
    unsigned long long* script_fallback;   // catan_sample_scripted_actions: decisions taken by the fall-back row (catan_scripted.hip), allocated at the first call
    unsigned long long* trade_counts;      // catan_sample_scripted_actions_style, style 1: the trader's TC_WORDS counters (catan_players.h), allocated at its first call
    void* playout_mem;           // catan_playout_actions with this handle as `sim`: the workspace (catan_players.h PlayoutWs, carved from one allocation), allocated at its first call
    RecordBuf rec;               // catan_record_enable: the recorder's slots (catan_hooks.h); not in `owned`: freed and re-made by every enable
    int rec_on;
    StartPoolBuf pool;           // catan_start_pool_set: the saved positions (catan_hooks.h); not in `owned`: freed and re-made by every set
    int pool_on;
    u32* pool_cum;               // catan_start_pool_set_weights: the inclusive prefix sums of the weights [pool.m], or NULL: the uniform pick
    u32 pool_W;                  // ... and their sum
    i32* pool_origin;            // catan_start_pool_outcomes_enable: per game the entry its episode started from, -1 fresh [n]
    unsigned long long* pool_out;   // ... the table of PO_HEAD + (pool.m + 1) x PO_WORDS sums
    const i32* pool_out_focus;   // ... the caller's focus array (device int32 [n]) or NULL
    int pool_out_on;
    TourneyBuf tourney;          // catan_tourney_enable: the lineups, the per-game seating and the table (catan_hooks.h); not in `owned`: freed and re-made by every enable
    int tourney_on;
};
static_assert(sizeof(BoardCfg) == sizeof(catan_board_cfg_t) && sizeof(catan_board_cfg_t) == 56 &&
              offsetof(BoardCfg, terrain) == offsetof(catan_board_cfg_t, terrain) &&
              offsetof(BoardCfg, numbers) == offsetof(catan_board_cfg_t, numbers), "board layout: device and C ABI layouts differ");

// games per k_step wave (catan_set_step_wave_games).  32 since the end of round 5: two waves per SIMD, so that one wave's gather overlaps the other's
// rules code - 41.4 -> 40.9 us per pass, lock-step 180.8 -> 178 us (profiles/r05_s5_pass_experiments.txt, run 20; 16: 43.2 us).  In round 3 the
// same switch bought nothing (28.3 -> 27.6 us of k_step): the launch was then bound by the CUs tier 2 held, not by its waves.
constexpr int DEFAULT_STEP_WAVE_GAMES = 32;
// sub-lists per sort bin in the fused-sampling deferred loop (Pending::bctr): one counter per bin serialises the launch's range reservations
constexpr int DEFAULT_FUSED_SUBS = 8;
constexpr int LR_BUDGET_DEFERRED = 12;   // (swept together with the window length: tools/deferred_sweep.py)
// The fused-sampling loop (round 6; profiles/r06_t1_stagger_ab.txt): tier 1's launch is STAGGERED - a one-wave kernel that idles T1_STAGGER_US in front of
// it on the side stream - so that the next pass's k_step, which becomes eligible at the same moment, gets its workgroups dispatched first (with both
// kernels' workgroups interleaved, tier 1's 3 072-4 096 one-wave workgroups held the LDS and registers k_step's second wave per SIMD needs: its waves
// started over ~20 us, 9 % of them in a second round; staggered: within 5-7 us, 2 %).  Any delay from 1 to 6 us gives the same 38.9 -> 36.9 us per pass:
// it is the ORDER of dispatch that matters, not the time.  With it, 4 096 tier-1 workgroups and budget 10 measure best (36.0 us).
constexpr int T1_STAGGER_US = 4, LR_GRID_FUSED = 4096, LR_BUDGET_FUSED = 10;
// cross-stream ordering inside one device: no timing, no system-scope release (which would flush L2 at every record)
constexpr unsigned EV_SYNC = hipEventDisableTiming | hipEventDisableSystemFence;

// ---- what the hooks' file and the rest of this one need of the handle: its limits, its allocations, the guards of the entry points
static inline Limits limits_of(const catan_env_t* e) { return Limits{ e->cfg.max_proposed_trades_per_turn, e->cfg.max_actions_per_turn }; }
// one device allocation of catan_create, owned by the handle until catan_destroy; nothing is tried after the first failure (rc)
template <class T>
static void dev_alloc(catan_env* e, hipError_t& rc, T*& p, size_t bytes) {
    if (rc != hipSuccess) return;
    rc = hipMalloc((void**)&p, bytes);
    if (rc == hipSuccess) e->owned.push_back(p);
}
// (catan_step_deferred / catan_step_flush: most entry points are refused between the two)
static int deferred_open_error(const catan_env_t* e, const char* what) {
    if (e && e->d_it > 0) return fail(CATAN_EINVAL, std::string(what) + ": a deferred step sequence is open (call catan_step_flush first)");
    return CATAN_OK;
}
#define NOT_DEFERRED(e, what) do { int r_ = deferred_open_error(e, what); if (r_ != CATAN_OK) return r_; } while (0)
#define NOT_MT(e, what) do { if ((e)->ctx.mt != nullptr) return fail(CATAN_EINVAL, std::string(what) + ": not available for a handle under the MT19937 contract (catan_seed_mt19937)"); } while (0)
// the fused deferred rollout draws a fresh game's first action inside the re-deal kernel, from the state an install would then replace
#define NO_START_POOL(e, what) do { if ((e)->pool_on) return fail(CATAN_EINVAL, std::string(what) + ": a start pool is installed (catan_start_pool_clear first)"); } while (0)
// Hooks in flight on any of the handle's streams may still read or write what a call is about to free or replace (the recorder's slots, a
// pool in use and its counters, the table of weights): all four streams are waited for
static int sync_hook_streams(catan_env_t* e, hipStream_t st) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(e->side));
    HIPCHK(hipStreamSynchronize(e->fstream));
    HIPCHK(hipStreamSynchronize(e->sstream));
    return CATAN_OK;
}

#include "catan_abi_hooks.h"

// The handle's scheduling knobs at creation: the measured defaults, then the environment (the ONLY place the library reads it: a switch set after a
// handle's creation does not reach that handle; A/B diagnostics of the schedules, listed in include/catan_hip_tuning.h).
static Sched sched_from_env() {
    Sched k;
    auto env_int = [](const char* name, int& v) { const char* t = getenv(name); if (t) v = atoi(t); return t != nullptr; };
    int v = 0;
    k.step_games = DEFAULT_STEP_WAVE_GAMES;
    if (env_int("CATAN_STEP_WAVE_GAMES", v) && (v == 64 || v == 32 || v == 16)) k.step_games = v;
    k.step_bin_order = 1;   // on since round 5 (54.5 -> 52.3-53.4 us per pass: profiles/r05_s5_pass_experiments.txt); CATAN_STEP_BIN_ORDER=0: bins in index order
    if (env_int("CATAN_STEP_BIN_ORDER", v)) k.step_bin_order = v != 0;
    // the fused-sampling loop is the library's own deferred loop since round 6 (one kernel per pass on the main stream; with per-bin sub-lists,
    // 32-game waves and the middle tier: 38.9 us per pass against 41.4 for sampler + k_step, profiles/r06_fused_loop_ab.txt); CATAN_DEFERRED_FUSED=0: the sampler form
    k.deferred_fused = 1;
    if (env_int("CATAN_DEFERRED_FUSED", v)) k.deferred_fused = v != 0;
    k.fused_subs = DEFAULT_FUSED_SUBS;
    static_assert(DEFAULT_FUSED_SUBS <= MAX_SUBS, "sub-lists per bin");
    if (env_int("CATAN_FUSED_SUBS", v) && (v == 1 || v == 2 || v == 4 || v == 8 || v == 16)) k.fused_subs = v;
    k.t1_group = 2;       // on since round 5 (47.8 -> 45.5 us per pass at 88.9 instead of 90.0 % active games: +3.6 % env-steps/s, profiles/r05_s5_pass_experiments.txt);
    if (env_int("CATAN_T1_GROUP", v)) k.t1_group = v == 1 ? 1 : 2;   // CATAN_T1_GROUP=1: a tier-1 launch per pass, three rotating slots (deferred_iter_sampler)
    k.t1_delay_us = T1_STAGGER_US;
    env_int("CATAN_T1_DELAY_US", k.t1_delay_us);
    // tier 1 as search + lane-per-game completion: in the library's own deferred loop since round 5 (a tier-1 launch there has two passes to finish and its
    // waves share the SIMDs with the sampler and k_step: 44.7 -> 43.8 us per pass), not inside a lock-step step (one more kernel on its critical path:
    // 184 -> 197 us) nor in catan_step_deferred (a launch per call: 64.0 -> 65.3 us per call).
    // CATAN_LR_SPLIT=0: never, 2: everywhere
    k.lr_split = 1;
    if (env_int("CATAN_LR_SPLIT", v)) k.lr_split = v == 0 ? 0 : (v == 2 ? 2 : 1);
    k.lr_grid = 0;
    if (env_int("CATAN_LR_GRID", v) && v >= 64) k.lr_grid = v;
    // the middle tier of a deferred window: on since round 5 (budget 256, 32 tier-2 workgroups behind it: 53.9 -> 51.2-51.6 us per pass,
    // same file); CATAN_LR_MID_BUDGET=0: every tier-2 request straight to k_lr_heavy on 128 workgroups
    k.lr_mid_budget = 256; k.lr_mid_heavy_grid = 32;
    if (env_int("CATAN_LR_MID_BUDGET", v)) { k.lr_mid_budget = v > 0 ? v : 0; if (k.lr_mid_budget == 0) k.lr_mid_heavy_grid = 128; }
    if (env_int("CATAN_LR_MID_HEAVY_GRID", v) && v >= 8 && v <= 256) k.lr_mid_heavy_grid = v;
    k.lr_budget[0] = LR_BUDGET; k.lr_budget[1] = LR_BUDGET_DEFERRED; k.lr_budget[2] = LR_BUDGET_FUSED;
    k.lr_round[0] = LR_ROUND_LOCKSTEP; k.lr_round[1] = LR_ROUND;
    return k;
}
// Pending as a lock-step step wants it, and as every deferred schedule leaves it behind
static void pend_lockstep(catan_env* e) {
    e->pend.fa = 0; e->pend.ftag = 1; e->pend.sa = 0; e->pend.stag = 1; e->pend.sample = 0; e->pend.brel = -1; e->pend.nsub = 1;
}
// ... and for one pass of a deferred schedule: tier-1 slot fa (request list, busy tag), window slot sa (tag 4 + sa), the sort's sets
static void pend_pass(catan_env* e, int fa, int ftag, int sa, int bsel, int bclear) {
    e->pend.fa = fa; e->pend.ftag = ftag; e->pend.sa = sa; e->pend.stag = 4 + sa; e->pend.bsel = bsel; e->pend.bclear = bclear;
    e->pend.sample = 0; e->pend.brel = -1; e->pend.nsub = 1;
}
// k_step with G games per wave in one-wave workgroups; pend.sample (fused-sampling rollouts): actions from / to the side rows
template <int G>
static void launch_step(catan_env_t* e, const int32_t* actions, float* reward, uint8_t* done, hipStream_t st, const StepCfg& sc, const u32* bins) {
    const dim3 grid(blocks(e->N, G) + SORT_PAD_WAVES);
    if (e->pend.sample) hipLaunchKernelGGL((k_step<G, true>), grid, dim3(64), 0, st, e->ctx, actions, e->mpk, reward, done, e->err, sc, e->pend, bins);
    else hipLaunchKernelGGL((k_step<G, false>), grid, dim3(64), 0, st, e->ctx, actions, e->mpk, reward, done, e->err, sc, e->pend, bins);
}

extern "C" {

void catan_cfg_default(catan_cfg_t* c) {
    c->max_proposed_trades_per_turn = 4; c->win_reward = 500.0; c->dense_reward = 0;
    c->reward_annealing_factor = 1.0; c->validate_actions = 1; c->auto_reset = 1; c->max_actions_per_turn = -1;
}
int32_t catan_state_words(void) { return STATE_WORDS; }
int32_t catan_mask_words(void) { return MASK_BITS; }
int32_t catan_action_words(void) { return ACTION_WORDS; }
int32_t catan_obs_floats(void) { return OBS_FLOATS; }
int32_t catan_state_bytes_per_game(void) { return STATE_BYTES_PER_GAME; }
int64_t catan_num_envs(const catan_env_t* e) { return e ? e->n : 0; }

static int launch_masks(catan_env_t* e, hipStream_t st) {
    hipLaunchKernelGGL(k_masks, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, e->mpk, limits_of(e));
    return launched();
}

int catan_create(catan_env_t** out, int device, int64_t n_envs, uint64_t seed, uint64_t env_id0, const catan_cfg_t* cfg) {
    if (!out || n_envs <= 0) return fail(CATAN_EINVAL, "catan_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(CATAN_ENODEV, "catan_create: no HIP device (the HIP path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(CATAN_EINVAL, "catan_create: bad device index");
    HIPCHK(hipSetDevice(device));
    // whichever way the call fails from here on, the handle and all it holds by then go through catan_destroy
    std::unique_ptr<catan_env, decltype(&catan_destroy)> guard(new (std::nothrow) catan_env(), &catan_destroy);
    catan_env* const e = guard.get();
    if (!e) return fail(CATAN_ENOMEM, "catan_create: host allocation failed");
    e->device = device;
    e->n = n_envs;
    e->N = (n_envs + BLOCK - 1) / BLOCK * BLOCK;
    if (cfg) e->cfg = *cfg; else catan_cfg_default(&e->cfg);
    e->sched = sched_from_env();
    const size_t bytes = (size_t)e->N * STATE_BYTES_PER_GAME, games = (size_t)e->N, envs = (size_t)e->n;
    hipError_t rc = hipSuccess;
    dev_alloc(e, rc, e->state, bytes);
    dev_alloc(e, rc, e->mpk, games * MPK_STRIDE * sizeof(u32));
    dev_alloc(e, rc, e->spec_state, games * REC * sizeof(u32));
    dev_alloc(e, rc, e->spec_mpk, games * MPK_STRIDE * sizeof(u32));
    dev_alloc(e, rc, e->err, 64);
    dev_alloc(e, rc, e->scratch_actions, envs * ACTION_WORDS * sizeof(i32));
    dev_alloc(e, rc, e->scratch_reward, envs * 4 * sizeof(float));
    dev_alloc(e, rc, e->scratch_done, envs);
    dev_alloc(e, rc, e->pend.ctr, CTR_WORDS * sizeof(u32));
    for (int i = 0; i < 3; i++) dev_alloc(e, rc, e->pend.req[i], games * sizeof(u64));
    dev_alloc(e, rc, e->f_reward, envs * 4 * sizeof(float));
    dev_alloc(e, rc, e->f_done, envs);
    // HIP multiplexes streams onto 4 hardware queues; streams that share a queue serialise.  Caller's stream + side +
    // fstream + sstream = 4, so the tier-1 slots share one stream (tier 1 of an iteration must fit in one iteration).
    // (A second tier-1 stream was measured with GPU_MAX_HW_QUEUES=4 and 8: 883 M and 447 M env-steps/s against 1 015 M -
    // two tier-1 launches in flight take the SIMDs from k_step.)
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&e->fstream, hipStreamNonBlocking);
    for (int i = 0; i < 3 && rc == hipSuccess; i++) {
        rc = hipEventCreateWithFlags(&e->ev_fready[i], EV_SYNC);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&e->ev_fdone[i], EV_SYNC);
    }
    for (int i = 0; i < 2; i++) {
        dev_alloc(e, rc, e->pend.heavy[i], games * sizeof(u64));
        for (int k = 0; k < 3; k++) dev_alloc(e, rc, e->pend.resets[i][k], games * sizeof(i32));
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&e->ev_sdone[i], EV_SYNC);
    }
    dev_alloc(e, rc, e->pend.heavy2, games * sizeof(u64));
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&e->sstream, hipStreamNonBlocking);
    dev_alloc(e, rc, e->s_reward, envs * 4 * sizeof(float));
    dev_alloc(e, rc, e->s_done, envs);
    // the sort's lists: BIN_SETS sets x NBINS bins x (fused-sampling rollouts) fused_subs sub-lists of up to N game ids each - a game is in at most
    // one list, so no sub-list can overflow whatever the split; only what is used is ever touched (65 536 games, 8 sub-lists: 151 MB of address space)
    dev_alloc(e, rc, e->pend.lists, (size_t)BIN_SETS * NBINS * e->sched.fused_subs * games * sizeof(i32));
    dev_alloc(e, rc, e->pend.bctr, (size_t)BIN_SETS * NBINS * MAX_SUBS * BCTR_PAD * sizeof(u32));
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking);
    if (rc == hipSuccess) rc = hipEventCreateWithFlags(&e->ev_fork, EV_SYNC);
    if (rc == hipSuccess) rc = hipEventCreateWithFlags(&e->ev_join, EV_SYNC);
    dev_alloc(e, rc, e->pend.type, games);
    dev_alloc(e, rc, e->pend.who, games);
    dev_alloc(e, rc, e->pend.len, games * sizeof(u64));
    dev_alloc(e, rc, e->pend.arrive, games * sizeof(u32));
    dev_alloc(e, rc, e->pend.spec, games * sizeof(u64));
    dev_alloc(e, rc, e->pend.busy, games);
    dev_alloc(e, rc, e->pctr, games * sizeof(u32));
    dev_alloc(e, rc, e->prof_wave, (size_t)prof_wave_rows(e->N) * 8 * sizeof(u32));
    dev_alloc(e, rc, e->prof, PROF_WORDS * sizeof(unsigned long long));
    if (rc != hipSuccess) return fail(CATAN_ENOMEM, std::string("catan_create: hipMalloc: ") + hipGetErrorString(rc));
    HIPCHK(hipMemset(e->state, 0, bytes));
    HIPCHK(hipMemset(e->err, 0, 64));
    HIPCHK(hipMemset(e->spec_mpk, 0, games * MPK_STRIDE * sizeof(u32)));   // no shadow carries the tag of a step yet (epochs start at 1)
    HIPCHK(hipMemset(e->pend.ctr, 0, CTR_WORDS * sizeof(u32)));
    HIPCHK(hipMemset(e->pend.type, 0, games));
    HIPCHK(hipMemset(e->pend.busy, 0, games));
    HIPCHK(hipMemset(e->pend.len, 0, games * sizeof(u64)));      // (bit 63 of a game's word is k_lr_finish<LRF_SPLIT>'s mark for k_lr_complete)
    HIPCHK(hipMemset(e->pctr, 0, games * sizeof(u32)));
    pend_lockstep(e);
    e->pend.bnext = 0; e->pend.bclear = 1; e->pend.lrq_clear = -1;
    HIPCHK(hipMemset(e->pend.bctr, 0, (size_t)BIN_SETS * NBINS * MAX_SUBS * BCTR_PAD * sizeof(u32)));
    HIPCHK(hipMemset(e->mpk, 0, (size_t)e->N * MPK_STRIDE * sizeof(u32)));
    e->ctx.R = (u32*)e->state;
    e->ctx.N = e->N; e->ctx.n = e->n;
    e->ctx.key0 = (u32)seed; e->ctx.key1 = (u32)(seed >> 32);
    e->ctx.env_id0 = env_id0;
    OK_OR_RETURN(catan_reset(e, nullptr, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    *out = guard.release();
    return CATAN_OK;
}

void catan_destroy(catan_env_t* e) {
    if (!e) return;
    hipSetDevice(e->device);
    for (void* p : e->owned) hipFree(p);
    if (e->mt_dev) hipFree(e->mt_dev);
    if (e->bcfg_dev) hipFree(e->bcfg_dev);
    if (e->bcfg_idx_dev) hipFree(e->bcfg_idx_dev);
    hooks_free(e);
    for (hipStream_t st : { e->fstream, e->sstream, e->side }) if (st) hipStreamDestroy(st);
    for (hipEvent_t ev : { e->ev_fready[0], e->ev_fready[1], e->ev_fready[2], e->ev_fdone[0], e->ev_fdone[1], e->ev_fdone[2], e->ev_sdone[0], e->ev_sdone[1],
                           e->ev_fork, e->ev_join })
        if (ev) hipEventDestroy(ev);
    delete e;
}

// contract (A): the generators' output rings topped up in front of a kernel that may draw
static int mt_refill(catan_env_t* e, hipStream_t st) {
    if (e->ctx.mt == nullptr) return CATAN_OK;
    hipLaunchKernelGGL(k_mt_refill, dim3(1), dim3(64), 0, st, e->ctx);
    return launched();
}
int catan_reset(catan_env_t* e, const uint8_t* reset_mask, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_reset: null handle");
    NOT_DEFERRED(e, "catan_reset");
    int r = mt_refill(e, S(stream));
    if (r != CATAN_OK) return r;
    enqueue_tourney_tally(e, nullptr, nullptr, reset_mask, S(stream));   // (in front of the deal: the selected games' records are still what they ended as)
    hipLaunchKernelGGL(k_reset, dim3((unsigned)(e->N < 16384 ? e->N : 16384)), dim3(64), 0, S(stream), e->ctx, reset_mask, 0);
    HIPCHK(hipGetLastError());
    r = launch_masks(e, S(stream));
    if (r != CATAN_OK) return r;
    enqueue_start_pool_sel(e, reset_mask, S(stream));            // (behind the masks of the fresh deals: an installed game takes its entry's)
    enqueue_tourney_seat(e, nullptr, nullptr, reset_mask, S(stream));
    return launched();
}
int catan_reset_board_only(catan_env_t* e, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_reset_board_only: null handle");
    NOT_DEFERRED(e, "catan_reset_board_only");
    int r = mt_refill(e, S(stream));
    if (r != CATAN_OK) return r;
    hipLaunchKernelGGL(k_reset, dim3((unsigned)(e->N < 16384 ? e->N : 16384)), dim3(64), 0, S(stream), e->ctx, (const u8*)nullptr, 1);
    return launched();
}

// ---- RNG contract (A): MT19937 as numpy (init_genrand) and CPython (init_by_array with a one-word key) seed it; the outputs are generated on the
// device (k_mt_refill), here only the 624-word start states
static void mt_host_init_genrand(uint32_t* mt, uint32_t s) {
    mt[0] = s;
    for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}
static void mt_host_init_by_array(uint32_t* mt, const uint32_t* key, int klen) {
    mt_host_init_genrand(mt, 19650218u);
    int i = 1, j = 0;
    for (int k = 624 > klen ? 624 : klen; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        i++; j++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
        if (j >= klen) j = 0;
    }
    for (int k = 623; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        i++;
        if (i >= 624) { mt[0] = mt[623]; i = 1; }
    }
    mt[0] = 0x80000000u;
}
// installs generator `which` (its 624 state words and position) with an empty output ring; the consumers' positions restart at 0
static int mt_install(catan_env_t* e, int which, const uint32_t* key, int pos, hipStream_t st) {
    if (e->n != 1) return fail(CATAN_EINVAL, "MT19937 contract: a single-game handle only (the reference's generators are process-global: SURVEY.md 8.4)");
    if (e->d_it > 0) return fail(CATAN_EINVAL, "MT19937 contract: a deferred step sequence is open");
    if (!e->mt_dev) {
        HIPCHK(hipMalloc((void**)&e->mt_dev, sizeof(MtPair)));
        HIPCHK(hipMemset(e->mt_dev, 0, sizeof(MtPair)));
        // (an uninstalled generator: position 624 of an all-zero state; both are installed by catan_seed_mt19937)
    }
    HIPCHK(hipStreamSynchronize(st));
    MtGen* g = which == 0 ? &e->mt_dev->np : &e->mt_dev->py;
    uint32_t head[626];
    memcpy(head, key, 624 * sizeof(uint32_t));
    head[624] = (uint32_t)pos; head[625] = 0u;                 // idx, produced
    HIPCHK(hipMemcpy(g, head, sizeof head, hipMemcpyHostToDevice));
    if (which == 0) HIPCHK(hipMemset(e->ctx.R + W_RNG, 0, sizeof(u32)));           // the numpy stream's position = the game's draw counter
    else HIPCHK(hipMemset(&e->mt_dev->cons_py, 0, sizeof(u32)));
    e->ctx.mt = e->mt_dev;
    return CATAN_OK;
}
int catan_seed_mt19937(catan_env_t* e, uint32_t numpy_seed, uint32_t python_seed, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_seed_mt19937: null handle");
    uint32_t mt[624];
    mt_host_init_genrand(mt, numpy_seed);                      // np.random.seed(int)
    int r = mt_install(e, 0, mt, 624, S(stream));
    if (r != CATAN_OK) return r;
    mt_host_init_by_array(mt, &python_seed, 1);                // random.seed(int), int < 2**32
    return mt_install(e, 1, mt, 624, S(stream));
}
int catan_mt19937_set_state(catan_env_t* e, int32_t which, const uint32_t* key624, int32_t pos, catan_stream_t stream) {
    if (!e || !key624 || (which != 0 && which != 1) || pos < 0 || pos > 624) return fail(CATAN_EINVAL, "catan_mt19937_set_state: bad arguments");
    return mt_install(e, which, key624, pos, S(stream));
}

// ---- board layouts (include/catan_hip.h)
static const char* board_cfg_error(const catan_board_cfg_t& c) {
    if (c.has_fixed_terrain) {
        static const int want[6] = { 1, 3, 4, 3, 4, 4 };       // TERRAIN_TO_PLACE: Desert, Hills, Forest, Mountains, Pastures, Fields
        int cnt[6] = { 0, 0, 0, 0, 0, 0 };
        for (int t = 0; t < 19; t++) {
            if (c.terrain[t] < 0 || c.terrain[t] > 5) return "a terrain value outside 0..5";
            cnt[c.terrain[t]]++;
        }
        for (int k = 0; k < 6; k++) if (cnt[k] != want[k]) return "the fixed terrain is not the multiset of TERRAIN_TO_PLACE";
    }
    if (c.has_fixed_numbers) {
        static const int want[13] = { 0, 0, 1, 2, 2, 2, 2, 0, 2, 2, 2, 2, 1 };   // DEFAULT_NUMBER_ORDER: one 2 and one 12, two of 3..6 and 8..11
        int cnt[13] = { 0 };
        for (int i = 0; i < 18; i++) {
            if (c.numbers[i] < 2 || c.numbers[i] > 12) return "a number token outside 2..12";
            cnt[c.numbers[i]]++;
        }
        for (int k = 0; k < 13; k++) if (cnt[k] != want[k]) return "the fixed number order is not the multiset of DEFAULT_NUMBER_ORDER";
    }
    return nullptr;
}
int catan_set_board_configs(catan_env_t* e, const catan_board_cfg_t* cfgs, int32_t n_cfgs, const uint8_t* game_cfg, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_set_board_configs: null handle");
    NOT_DEFERRED(e, "catan_set_board_configs");
    if (n_cfgs < 0 || n_cfgs > MAX_BOARD_CFGS) return fail(CATAN_EINVAL, "catan_set_board_configs: n_cfgs must be 0..16");
    if (n_cfgs > 0 && !cfgs) return fail(CATAN_EINVAL, "catan_set_board_configs: null cfgs");
    for (int i = 0; i < n_cfgs; i++)
        if (const char* why = board_cfg_error(cfgs[i])) return fail(CATAN_EINVAL, "catan_set_board_configs: layout " + std::to_string(i) + ": " + why);
    const hipStream_t st = S(stream);
    // the old table may still be read by re-deals in flight on any of the handle's streams
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(e->side));
    HIPCHK(hipStreamSynchronize(e->fstream));
    HIPCHK(hipStreamSynchronize(e->sstream));
    BoardCfg* tab = nullptr;
    u8* idx = nullptr;
    Staged stage;
    if (n_cfgs > 0) {
        u32* bad = nullptr;
        stage.alloc(tab, (size_t)n_cfgs * sizeof(BoardCfg));
        stage.alloc(idx, (size_t)e->N);
        stage.alloc(bad, sizeof(u32));
        hipError_t rc = stage.rc;                          // (this call reports a failed allocation as any other HIP error)
        if (rc == hipSuccess) rc = hipMemcpyAsync(tab, cfgs, (size_t)n_cfgs * sizeof(BoardCfg), hipMemcpyHostToDevice, st);
        if (rc == hipSuccess) rc = hipMemsetAsync(bad, 0, sizeof(u32), st);
        if (rc == hipSuccess) {
            hipLaunchKernelGGL(k_board_cfg_index, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, (long)e->n, (long)e->N, game_cfg, (int)n_cfgs, idx, bad);
            rc = hipGetLastError();
        }
        u32 nbad = 0;
        if (rc == hipSuccess) rc = hipMemcpyAsync(&nbad, bad, sizeof(u32), hipMemcpyDeviceToHost, st);
        if (rc == hipSuccess) rc = hipStreamSynchronize(st);
        stage.free_now(bad);
        if (rc != hipSuccess) return fail(CATAN_EHIP, std::string("catan_set_board_configs: ") + hipGetErrorString(rc));
        if (nbad != 0) return fail(CATAN_EINVAL, "catan_set_board_configs: " + std::to_string(nbad) + " game_cfg entries >= n_cfgs");
    }
    stage.commit();
    if (e->bcfg_dev) hipFree(e->bcfg_dev);
    if (e->bcfg_idx_dev) hipFree(e->bcfg_idx_dev);
    e->bcfg_dev = tab; e->bcfg_idx_dev = idx;
    e->ctx.bcfg = tab; e->ctx.bcfg_idx = idx;
    return CATAN_OK;
}

static StepCfg step_cfg(const catan_env_t* e) {
    StepCfg sc;
    sc.validate = e->cfg.validate_actions; sc.dense_reward = e->cfg.dense_reward; sc.win_reward = e->cfg.win_reward;
    sc.annealing = e->cfg.reward_annealing_factor; sc.lim = limits_of(e); sc.auto_reset = e->cfg.auto_reset;
    sc.reward64 = e->reward64;
    sc.prof = e->prof_on ? e->prof : nullptr;
    sc.prof_wave = e->prof_on >= 2 ? e->prof_wave : nullptr;
    sc.prof_timeline = e->prof_on == 3;
    sc.bin_order = e->sched.step_bin_order;
    return sc;
}
// One env step = the games listed by action type (k_sample_random / k_classify), then k_step (fused: apply + done/reward +
// next masks for every game that needs no longest-road update) - the FAST path.  The few games that placed a road /
// settlement or ended take the SLOW path: k_lr_finish (tier-1 path search + completion, one game per wave), k_lr_heavy
// (tier 2 + completion), k_reset_list (re-deal, one wave per finished game).  Its launch times are the latency tails of a
// handful of serial searches / re-deals.
//   lock-step (catan_step, catan_random_rollout): the slow path runs inside every step; the re-deals (real ones and
//     speculative successors of the games the step may still end) run on a side stream right behind k_step.
//   deferred (catan_random_rollout_deferred): a game on the slow path is BUSY (no action, no policy draw).  Tier 1 of
//     iteration t runs on a side stream during iteration t+1 and its games play again at t+2; tier 2 and the re-deals of
//     window w (W iterations) run on another stream during window w+1 and their games play again in window w+2.  Every
//     game's own trajectory is unchanged because its policy stream is indexed by its own decision counter; the release
//     points are fixed by this schedule (the main stream waits for the side work there), never by kernel timing.
constexpr int LR_HEAVY_GRID = 256;   // one 1024-thread workgroup per CU; requests x split parts are strided over them
constexpr int LR_HEAVY_GRID_DEFERRED = 128;  // next to the fast path: leave most CUs (and their LDS) to k_step
constexpr int LR_GRID = 4096;
constexpr int LR_GRID_DEFERRED = 3072;
constexpr int LR_MID_GRID = 2048;          // the middle tier: one request per one-wave workgroup (a window leaves ~640)
constexpr int LR_COMPLETE_GRID = 128;   // k_lr_complete: 64 requests per one-wave workgroup, grid-stride beyond 8 192 requests
constexpr int RESET_GRID = 2048;
// ev (optional): [0] before the sort, [1] after it, [2] after k_step
static int enqueue_fast(catan_env_t* e, const int32_t* actions, float* reward, uint8_t* done, hipStream_t st, hipEvent_t* ev,
                        bool have_hist = false) {
    StepCfg sc = step_cfg(e);
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    u32* bins = e->pend.ctr + 16 + NBINS * e->pend.bsel;
    if (!have_hist) {                                     // (the rollout loops sort inside k_sample_random)
        hipLaunchKernelGGL(k_classify, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, actions, bins, e->pend.lists + (size_t)e->pend.bsel * NBINS * e->N,
                           e->pend.ctr + 4, 12, sc.validate ? e->err : (u32*)nullptr);
        if (ev) HIPCHK(hipEventRecord(ev[1], st));
    }
    switch (e->sched.step_games) {
    case 16: launch_step<16>(e, actions, reward, done, st, sc, bins); break;
    case 32: launch_step<32>(e, actions, reward, done, st, sc, bins); break;
    default: launch_step<64>(e, actions, reward, done, st, sc, bins); break;
    }
    if (ev) HIPCHK(hipEventRecord(ev[2], st));
    return launched();
}
// tier 1 + completion of request list `fl` on stream `st`.  ev (optional): recorded on st: [8] before, [6] after
// workgroups of k_lr_finish: `grid` (the fused-sampling loop's), else by the schedule (Sched::lr_grid overrides all three: diagnostics, tools/pass_experiments.py).
// Deferred schedules (tags >= 2): 3 072 - three tier-1 waves
// per SIMD leave registers for a sampler / k_step wave beside them (4 x 120 of a SIMD's 512 do not), and the launch - one per two passes - has the
// time to take its ~4 000 requests in two rounds: 45.6 -> 44.9 us per pass (profiles/r05_s5_pass_experiments.txt, run 9)
static int enqueue_tier1(catan_env_t* e, float* reward, uint8_t* done, hipStream_t st, hipEvent_t* ev, int fl, int lr_budget, bool two_passes = false, int grid = 0) {
    if (grid <= 0) grid = e->pend.ftag >= 2 ? LR_GRID_DEFERRED : LR_GRID;
    if (e->sched.lr_grid) grid = e->sched.lr_grid;
    StepCfg sc = step_cfg(e);
    if (ev) HIPCHK(hipEventRecord(ev[8], st));
    if (e->sched.lr_split == 2 || (e->sched.lr_split == 1 && two_passes)) {     // (1: only where a launch has two passes to finish - the library's own deferred loops)
        hipLaunchKernelGGL(k_lr_finish<LRF_SPLIT>, dim3(grid), dim3(64), 0, st, e->ctx, e->mpk, reward, done, sc, e->pend, fl, lr_budget,
                           sc.prof && e->prof_on < 2 ? sc.prof + 2 * PROF_PHASES : nullptr, reinterpret_cast<unsigned long long*>(e->err + 4));
        hipLaunchKernelGGL(k_lr_complete, dim3(LR_COMPLETE_GRID), dim3(64), 0, st, e->ctx, e->mpk, reward, done, sc, e->pend, fl);
    } else
    hipLaunchKernelGGL(k_lr_finish<LRF_TIER1>, dim3(grid), dim3(64), 0, st, e->ctx, e->mpk, reward, done, sc, e->pend, fl, lr_budget,
                       sc.prof && e->prof_on < 2 ? sc.prof + 2 * PROF_PHASES : nullptr, reinterpret_cast<unsigned long long*>(e->err + 4));
    if (ev) HIPCHK(hipEventRecord(ev[6], st));
    return launched();
}
// One re-deal list (its length at *count_p) and everything that hangs on the moment it is consumed, on stream st.  The order is a correctness
// condition, and this is the one place that states it:
//   in front of the consumer, the hooks that READ the listed games' final states, which the consumer overwrites: the finished-game
//     statistics, the league results, the start pool's per-entry outcomes (they also read the origins the pool install rewrites), the
//     tournament's tally (it reads the seating the seat hook rewrites) and the recorder's seal;
//   the consumer: a fresh deal (k_reset_list), a fresh deal that also deals step_impl's speculative successors into the shadow arrays
//     (pend.spec; they are no episodes, so the hooks see the real list only), or the install of those shadows (k_install_list);
//   behind it, the hooks that WRITE the fresh games: the start pool's install, then the recorder's opening, whose start blob is the state
//     the install left; and the tournament's seat, which writes the games' next seating and nothing of the games.
// All of it stands in front of whatever the caller records or waits for on st to publish the re-deal.  Every hook that is off launches nothing.
enum Redeal { REDEAL_FRESH, REDEAL_FRESH_AND_SPEC, REDEAL_INSTALL };
static void enqueue_redeal(catan_env_t* e, Redeal how, const u32* count_p, const i32* list, u8* busy, hipStream_t st) {
    enqueue_episode_stats(e, count_p, list, st);
    enqueue_league_stats(e, count_p, list, st);
    enqueue_start_pool_outcomes(e, count_p, list, st);
    enqueue_tourney_tally(e, count_p, list, nullptr, st);
    enqueue_record_seal(e, count_p, list, st);
    if (how == REDEAL_INSTALL)
        hipLaunchKernelGGL(k_install_list, dim3(256), dim3(64), 0, st, e->ctx, e->mpk, limits_of(e), count_p, list, busy,
                           (const u32*)e->spec_state, (const u32*)e->spec_mpk, e->spec_epoch, e->err);
    else if (how == REDEAL_FRESH_AND_SPEC)
        hipLaunchKernelGGL(k_reset_list, dim3(RESET_GRID), dim3(64), 0, st, e->ctx, e->mpk, limits_of(e), count_p, list, busy, step_cfg(e).prof,
                           (const u32*)(e->pend.ctr + 6), (const u64*)e->pend.spec, e->spec_state, e->spec_mpk, e->spec_epoch, e->pend);
    else
        hipLaunchKernelGGL(k_reset_list, dim3(RESET_GRID), dim3(64), 0, st, e->ctx, e->mpk, limits_of(e), count_p, list, busy, step_cfg(e).prof,
                           (const u32*)nullptr, (const u64*)nullptr, (u32*)nullptr, (u32*)nullptr, 0u, e->pend);
    enqueue_start_pool(e, count_p, list, st);
    enqueue_record_open(e, count_p, list, st);
    enqueue_tourney_seat(e, count_p, list, nullptr, st);
}
// tier 2 (+ the completion of its games) and the re-deals of window slot pend.sa on stream st.
//   deferred window: the games that ended in k_step / k_lr_finish (list 0) are re-dealt on the side stream while tier 2 runs,
//     those that end in the tier-2 completion (list 1) afterwards.
//   lock-step step: no re-deal is left on the critical path - step_impl started, right behind k_step and on the side stream,
//     the re-deals of the games that ended in k_step AND a speculative successor (shadow records) for every game on the
//     longest-road path; the games that then end in k_lr_finish (list 2) or in the tier-2 completion (list 1) only take
//     their shadow (k_install_list).
// ev (optional): [9] before k_lr_heavy, [3] / [7] after it, [4] at the end
static int enqueue_slow(catan_env_t* e, float* reward, uint8_t* done, hipStream_t st, hipEvent_t* ev, int heavy_grid) {
    StepCfg sc = step_cfg(e);
    const int sa = e->pend.sa;
    const bool lockstep = heavy_grid == LR_HEAVY_GRID;
    u32* sctr = e->pend.ctr + 8 + 4 * sa;
    u8* busy = e->pend.stag < 2 ? e->pend.busy : nullptr;       // tagged games are released by the sampler, not here
    if (e->cfg.auto_reset) {
        if (!lockstep) {
            HIPCHK(hipEventRecord(e->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
            enqueue_redeal(e, REDEAL_FRESH, sctr + 1, e->pend.resets[sa][0], busy, e->side);
            HIPCHK(hipEventRecord(e->ev_join, e->side));
        }
    }
    if (ev) HIPCHK(hipEventRecord(ev[9], st));
    if (!lockstep && e->sched.lr_mid_budget > 0) {     // (both forms of the deferred loop since round 6: the fused loop's failures with it were its own window-close race, deferred_iter)
        // the middle tier: one wave per tier-2 request with a large budget; k_lr_heavy - fewer workgroups: few requests are left - takes the rest
        HIPCHK(hipMemsetAsync(e->pend.ctr + CTR_HEAVY2, 0, sizeof(u32), st));
        hipLaunchKernelGGL(k_lr_finish<LRF_MID>, dim3(LR_MID_GRID), dim3(64), 0, st, e->ctx, e->mpk, reward, done, sc, e->pend, 0, e->sched.lr_mid_budget,
                           (unsigned long long*)nullptr, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(k_lr_heavy, dim3(e->sched.lr_mid_heavy_grid), dim3(LR_HEAVY_THREADS), 0, st, e->ctx, (const u32*)(e->pend.ctr + CTR_HEAVY2), (const u64*)e->pend.heavy2,
                           e->pend.len, e->sched.lr_round[1], e->mpk, reward, done, sc, e->pend);
    } else
    hipLaunchKernelGGL(k_lr_heavy, dim3(heavy_grid), dim3(LR_HEAVY_THREADS), 0, st, e->ctx, (const u32*)sctr, (const u64*)e->pend.heavy[sa], e->pend.len,
                       e->sched.lr_round[lockstep ? 0 : 1], e->mpk, reward, done, sc, e->pend);   // search + completion
    if (ev) HIPCHK(hipEventRecord(ev[3], st));
    if (ev) HIPCHK(hipEventRecord(ev[7], st));
    if (e->cfg.auto_reset) {
        if (lockstep) {
            HIPCHK(hipStreamWaitEvent(st, e->ev_join, 0));      // the side stream's launch of step_impl: it had the whole slow path to finish
            enqueue_redeal(e, REDEAL_INSTALL, sctr + 3, e->pend.resets[sa][2], busy, st);
            enqueue_redeal(e, REDEAL_INSTALL, sctr + 2, e->pend.resets[sa][1], busy, st);
        } else {
            HIPCHK(hipStreamWaitEvent(st, e->ev_join, 0));
            enqueue_redeal(e, REDEAL_FRESH, sctr + 2, e->pend.resets[sa][1], busy, st);
        }
    }
    if (ev) HIPCHK(hipEventRecord(ev[4], st));
    return launched();
}
constexpr int EV_PER_STEP = 10;
// sample_step != nullptr: the random policy draws the actions first (into `actions`), fused with the sort's histogram
static int step_impl(catan_env_t* e, int32_t* actions, float* reward, uint8_t* done, hipStream_t st, hipEvent_t* ev = nullptr,
                     const uint32_t* sample_step = nullptr) {
    pend_lockstep(e);
    { int rr = mt_refill(e, st); if (rr != CATAN_OK) return rr; }
    if (ev) HIPCHK(hipEventRecord(ev[5], st));
    // the step's first kernel zeroes the slow-path list counters (ctr[4..15]) and k_step the count set of the NEXT sort, so a
    // memset is only needed after anything else used the counters (creation, a deferred rollout)
    if (!e->ctr_clean) { HIPCHK(hipMemsetAsync(e->pend.ctr, 0, CTR_WORDS * sizeof(u32), st)); e->ctr_clean = 1; e->lock_parity = 0; }
    e->pend.bsel = e->lock_parity; e->pend.bclear = e->lock_parity ^ 1; e->lock_parity ^= 1;
    if (sample_step)
        hipLaunchKernelGGL(k_sample_random<BLOCK>, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, st, e->ctx, (const u32*)e->mpk, *sample_step, actions,
                           (u32*)nullptr, (u8*)nullptr, 0, 0, e->pend.ctr + 4, 12, e->pend.ctr + 16 + NBINS * e->pend.bsel,
                           e->pend.lists + (size_t)e->pend.bsel * NBINS * e->N);
    enqueue_record_append(e, actions, nullptr, st);              // (behind the sampler where it is the one that writes `actions`)
    int r = enqueue_fast(e, actions, reward, done, st, ev, sample_step != nullptr);
    if (r == CATAN_OK && e->cfg.auto_reset) {                    // the games that ended in k_step: re-dealt on the side stream from here on
        HIPCHK(hipEventRecord(e->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
        // ... and every game on the longest-road path that this step may end (k_step's list pend.spec) gets a speculative successor
        e->spec_epoch++;
        enqueue_redeal(e, REDEAL_FRESH_AND_SPEC, e->pend.ctr + 8 + 1, e->pend.resets[0][0], e->pend.busy, e->side);
        HIPCHK(hipEventRecord(e->ev_join, e->side));
    }
    if (r == CATAN_OK) r = enqueue_tier1(e, reward, done, st, ev, 0, e->sched.lr_budget[0]);
    if (r == CATAN_OK) r = enqueue_slow(e, reward, done, st, ev, LR_HEAVY_GRID);
    if (r == CATAN_OK) enqueue_record_seal_done(e, done, nullptr, actions, st);
    return r;
}

int catan_step(catan_env_t* e, const int32_t* actions, float* reward, uint8_t* done, catan_stream_t stream) {
    if (!e || !actions || !reward || !done) return fail(CATAN_EINVAL, "catan_step: null argument");
    NOT_DEFERRED(e, "catan_step");
    return step_impl(e, const_cast<int32_t*>(actions), reward, done, S(stream));
}

int catan_masks(catan_env_t* e, float* out, catan_stream_t stream) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_masks: null argument");
    long total = e->n * MASK_BITS;
    if (e->d_it > 0)                     // an open deferred sequence: a waiting game's row is the placeholder (only EndTurn), never a half-written mask
        hipLaunchKernelGGL(k_expand_masks_of, dim3(blocks(total, BLOCK)), dim3(BLOCK), 0, S(stream), (const u32*)e->mpk, (const i32*)nullptr, (long)e->n, (long)e->n, (const u8*)e->pend.busy, out);
    else
        hipLaunchKernelGGL(k_expand_masks, dim3(blocks(total, BLOCK)), dim3(BLOCK), 0, S(stream), e->mpk, e->N, e->n, out);
    return launched();
}

int catan_masks_packed_copy(catan_env_t* e, uint32_t* out, catan_stream_t stream) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_masks_packed_copy: null argument");
    hipLaunchKernelGGL(k_copy_masks11, dim3(blocks(e->n * 11, BLOCK)), dim3(BLOCK), 0, S(stream), (const u32*)e->mpk, (long)e->n, out);
    return launched();
}

int catan_masked_row_store(void* dst, const void* src, const int64_t* t, const uint8_t* sel, int64_t rows, int64_t row_bytes,
                           int64_t step_stride_bytes, catan_stream_t stream) {
    if (!dst || !src || !t || !sel || rows <= 0 || row_bytes <= 0 || step_stride_bytes < rows * row_bytes)
        return fail(CATAN_EINVAL, "catan_masked_row_store: bad arguments");
    hipLaunchKernelGGL(k_masked_row_store, dim3((unsigned)rows), dim3(256), 0, S(stream), (unsigned char*)dst, (const unsigned char*)src,
                       (const long long*)t, sel, (long)row_bytes, (long)step_stride_bytes);
    return launched();
}

int catan_expand_masks(const uint32_t* packed, int64_t rows, int32_t pitch_words, float* out, catan_stream_t stream) {
    if (!packed || !out || rows <= 0 || pitch_words < (MASK_BITS + 31) / 32) return fail(CATAN_EINVAL, "catan_expand_masks: bad arguments");
    hipLaunchKernelGGL(k_expand_masks, dim3(blocks(rows * MASK_BITS, BLOCK)), dim3(BLOCK), 0, S(stream), packed, (long)rows, (long)rows, out, (int)pitch_words);
    return launched();
}

int catan_masks_packed(catan_env_t* e, const uint32_t** out_ptr, int64_t* out_pitch) {
    if (!e || !out_ptr || !out_pitch) return fail(CATAN_EINVAL, "catan_masks_packed: null argument");
    *out_ptr = e->mpk; *out_pitch = MPK_STRIDE;
    return CATAN_OK;
}

int catan_deciding_seat(catan_env_t* e, int32_t* out, catan_stream_t stream) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_deciding_seat: null argument");
    hipLaunchKernelGGL(k_deciding, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, S(stream), e->ctx, out, 0);
    return launched();
}

int catan_players_turn_sim(catan_env_t* e, int32_t* out, catan_stream_t stream) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_players_turn_sim: null argument");
    hipLaunchKernelGGL(k_deciding, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, S(stream), e->ctx, out, 1);
    return launched();
}

int catan_sample_random_actions(catan_env_t* e, uint32_t step_idx, int32_t* actions, catan_stream_t stream) {
    if (!e || !actions) return fail(CATAN_EINVAL, "catan_sample_random_actions: null argument");
    hipLaunchKernelGGL(k_sample_random<BLOCK>, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, S(stream), e->ctx, e->mpk, step_idx, actions,
                       (u32*)nullptr, (u8*)nullptr, 0, 0, (u32*)nullptr, 0, (u32*)nullptr, (i32*)nullptr);
    return launched();
}

int catan_state_export(catan_env_t* e, int32_t* blob, const int64_t* env_idx, int64_t cnt, catan_stream_t stream) {
    if (!e || !blob || cnt <= 0 || (!env_idx && cnt > e->n)) return fail(CATAN_EINVAL, "catan_state_export: bad arguments");
    NOT_DEFERRED(e, "catan_state_export");
    hipLaunchKernelGGL(k_export, dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, S(stream), e->ctx, (const long*)env_idx, (long)cnt, blob);
    return launched();
}

int catan_state_import(catan_env_t* e, const int32_t* blob, const int64_t* env_idx, int64_t cnt, catan_stream_t stream) {
    if (!e || !blob || cnt <= 0 || (!env_idx && cnt > e->n)) return fail(CATAN_EINVAL, "catan_state_import: bad arguments");
    NOT_DEFERRED(e, "catan_state_import");
    hipLaunchKernelGGL(k_import, dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, S(stream), e->ctx, (const long*)env_idx, (long)cnt, blob);
    enqueue_start_pool_origin_clear(e, (const long*)env_idx, (long)cnt, S(stream));
    HIPCHK(hipGetLastError());
    return launch_masks(e, S(stream));
}

int catan_state_fork(catan_env_t* dst, const catan_env_t* src, const int64_t* src_idx, const int64_t* dst_idx, const uint32_t* draw_offset,
                     int64_t cnt, catan_stream_t stream) {
    if (!dst || !src || !src_idx || cnt <= 0 || (!dst_idx && cnt > dst->n)) return fail(CATAN_EINVAL, "catan_state_fork: bad arguments");
    if (dst == src) return fail(CATAN_EINVAL, "catan_state_fork: the two handles are the same (a fork inside one handle is not supported)");
    if (dst->device != src->device) return fail(CATAN_EINVAL, "catan_state_fork: the handles live on different devices");
    NOT_DEFERRED(dst, "catan_state_fork");
    NOT_DEFERRED(src, "catan_state_fork");
    NOT_MT(dst, "catan_state_fork");
    NOT_MT(src, "catan_state_fork");
    // the packed masks depend on the state and on two limits of the handle's configuration: equal limits -> the source's words are the destination's
    const Limits ls = limits_of(src), ld = limits_of(dst);
    const int copy_masks = ls.max_trades == ld.max_trades && ls.max_actions == ld.max_actions;
    hipLaunchKernelGGL(k_fork, dim3(blocks(cnt * FORK_SLOTS, BLOCK)), dim3(BLOCK), 0, S(stream), dst->ctx, dst->mpk, src->ctx, (const u32*)src->mpk,
                       (const long*)src_idx, (const long*)dst_idx, (const u32*)draw_offset, (long)cnt, copy_masks);
    enqueue_start_pool_origin_clear(dst, (const long*)dst_idx, (long)cnt, S(stream));
    HIPCHK(hipGetLastError());
    if (!copy_masks) {
        hipLaunchKernelGGL(k_masks_of_list, dim3(blocks(cnt, BLOCK)), dim3(BLOCK), 0, S(stream), dst->ctx, dst->mpk, ld, (const long*)dst_idx, (long)cnt);
        HIPCHK(hipGetLastError());
    }
    return CATAN_OK;
}

int catan_set_reward_f64_buffer(catan_env_t* e, double* reward64) {
    if (!e) return fail(CATAN_EINVAL, "catan_set_reward_f64_buffer: null handle");
    e->reward64 = reward64;
    return CATAN_OK;
}

int catan_set_reward_annealing(catan_env_t* e, double f) {
    if (!e) return fail(CATAN_EINVAL, "catan_set_reward_annealing: null handle");
    e->cfg.reward_annealing_factor = f;
    return CATAN_OK;
}

// one word of the handle's error block (err[0] invalid actions, [1] inconsistent deals, [2] missed speculations), or -1
static int64_t err_word(catan_env_t* e, int k, catan_stream_t stream) {
    if (!e) return -1;
    u32 v = 0;
    if (hipMemcpyAsync(&v, e->err + k, sizeof v, hipMemcpyDeviceToHost, S(stream)) != hipSuccess) return -1;
    if (hipStreamSynchronize(S(stream)) != hipSuccess) return -1;
    return (int64_t)v;
}
int64_t catan_invalid_action_count(catan_env_t* e, catan_stream_t stream) { return err_word(e, 0, stream); }
int64_t catan_inconsistent_deal_count(catan_env_t* e, catan_stream_t stream) { return err_word(e, 1, stream); }
int64_t catan_missed_speculation_count(catan_env_t* e, catan_stream_t stream) { return err_word(e, 2, stream); }

int catan_randomise_uncertainty(catan_env_t* e, const int32_t* controlling_player, catan_stream_t stream) {
    if (!e || !controlling_player) return fail(CATAN_EINVAL, "catan_randomise_uncertainty: null argument");
    NOT_DEFERRED(e, "catan_randomise_uncertainty");
    NOT_MT(e, "catan_randomise_uncertainty");
    hipLaunchKernelGGL(k_randomise_uncertainty, dim3(blocks(e->n, 64)), dim3(64), 0, S(stream), e->ctx, controlling_player, e->mpk, e->err,
                       100000, limits_of(e));
    return launched();
}

int catan_random_rollout(catan_env_t* e, uint32_t step_idx0, int64_t steps, catan_stream_t stream) {
    if (!e || steps < 0) return fail(CATAN_EINVAL, "catan_random_rollout: bad arguments");
    NOT_DEFERRED(e, "catan_random_rollout");
    for (int64_t s = 0; s < steps; s++) {
        const uint32_t step_idx = step_idx0 + (uint32_t)s;
        int r = step_impl(e, e->scratch_actions, e->scratch_reward, e->scratch_done, S(stream), nullptr, &step_idx);
        if (r != CATAN_OK) return r;
    }
    return CATAN_OK;
}

// ---- the deferred schedules' windows.  Pass (or call) `it` belongs to window w = it / window, which uses slot sa = w & 1 (busy tag 4 + sa, the four
// counters ctr[8 + 4 sa ..], its tier-2 / re-deal lists).  The window's slow path runs on the window stream (sstream) during window w + 1 and its
// games play again when window w + 2 opens - on the same slot, which is why that pass first waits for ev_sdone[sa].
struct Win {
    int64_t w; int sa;
    bool opens;           // the window's first pass
    bool back;            // ... which takes the slot over from window w - 2: that window's games come back
    bool closes, last;    // the window's last pass (the call's last pass closes its window early); the call's last pass
};
// iters < 0: a sequence of unknown length (catan_step_deferred; catan_step_flush closes the window that is still open)
static Win win_of(int64_t it, int64_t iters, int window) {
    Win x;
    x.w = it / window; x.sa = (int)(x.w & 1);
    x.opens = it % window == 0; x.back = x.opens && x.w >= 2;
    x.last = it + 1 == iters; x.closes = (it + 1) % window == 0 || x.last;
    return x;
}
// the slow path of window w-2 is complete (the fused-sampling loop then enqueues its games: k_release_window)
static int window_wait(catan_env_t* e, const Win& win, hipStream_t st) {
    if (win.back) HIPCHK(hipStreamWaitEvent(st, e->ev_sdone[win.sa], 0));
    return CATAN_OK;
}
// a sequence's first pass zeroes every counter, a pass that opens a later window the four of the window's slot
static int window_clear(catan_env_t* e, const Win& win, int64_t it, hipStream_t st) {
    if (it == 0) HIPCHK(hipMemsetAsync(e->pend.ctr, 0, CTR_WORDS * sizeof(u32), st));
    else if (win.opens) HIPCHK(hipMemsetAsync(e->pend.ctr + 8 + 4 * win.sa, 0, 4 * sizeof(u32), st));
    return CATAN_OK;
}
// The window's slow path (enqueue_slow for pend.sa == win.sa) on the window stream.  Its tier-2 / re-deal lists are complete once the outstanding
// tier-1 launches are (t1_cnt of them, slots t1_first ^ 0, ^ 1, ..: two slots from either, or all three from slot 0; one side stream: the latest
// implies the others) AND the closing pass's k_step has
// appended the games it ends.  A tier-1 launch behind that k_step orders the two; where there is none, the caller passes an event recorded behind
// the k_step (step_done).  reward / done: the result rows of the completions.
static int window_close(catan_env_t* e, const Win& win, hipEvent_t* ev, float* reward, uint8_t* done, int t1_first, int t1_cnt, hipEvent_t step_done = nullptr) {
    if (t1_cnt > (t1_first == 0 ? 3 : 2)) return fail(CATAN_EINVAL, "window_close: three tier-1 slots are waited for from slot 0 only");
    for (int k = 0; k < t1_cnt; k++) HIPCHK(hipStreamWaitEvent(e->sstream, e->ev_fdone[t1_first ^ k], 0));
    if (step_done) HIPCHK(hipStreamWaitEvent(e->sstream, step_done, 0));
    int r = enqueue_slow(e, reward, done, e->sstream, ev, LR_HEAVY_GRID_DEFERRED);
    if (r != CATAN_OK) return r;
    HIPCHK(hipEventRecord(e->ev_sdone[win.sa], e->sstream));
    return CATAN_OK;
}
// the end of a sequence: the main stream joins the slow paths of its last window and of the one before (the caller then releases every game)
static int window_join(catan_env_t* e, const Win& win, hipStream_t st) {
    HIPCHK(hipStreamWaitEvent(st, e->ev_sdone[win.sa], 0));
    if (win.w >= 1) HIPCHK(hipStreamWaitEvent(st, e->ev_sdone[win.sa ^ 1], 0));
    return CATAN_OK;
}

// The deferred iteration in its sampler form (rounds 1-5; catan_set_deferred_fused(env, 0)): a sampling + sorting kernel in front of every
// k_step, busy tags cleared by it; the sort's bin sets alternate.
// Tier 1 is forked once per GROUP of P = Sched::t1_group passes (2 since round 5): both passes push their longest-road requests to the group's list
// under the group's tag, tier 1 runs on the side stream behind the group's last k_step, and the group's games play again when the slot (request
// list, busy tag 2 / 3 / 6, event pair; D of them rotate) is used next: two groups later - the games of the first pass sit out three passes, those
// of the second two.  The event record behind k_step and the event wait in front of the sampler - ~3.3 us of drained main stream each - are
// then paid once per two passes.  A window's last pass (and a call's last) closes its group early, so the window's slow path still sees every
// tier-1 launch that can hand it work.
// P = 1 (CATAN_T1_GROUP=1, diagnostics): a group per pass.  With D = 2 slots the loop's period would be tied to a dependency cycle:
// k_step(it) -> [event hand-over to the side stream, ~11 us] -> k_lr_finish (~40 us: its slowest search) -> [hand-over back, ~11 us] ->
// sampler(it + 2), i.e. 2 P >= 62 us + sampler + k_step (profiles/r05_k_step_pass_experiments.txt).  D = 3 frees the cycle (P >= 36 us) -
// measured (same file, session 12): 54.3 -> 52.8 us per pass, but the longest-road games sit out one more pass (92.6 -> 90.0 % of the games
// active): 1.118 G env-steps/s either way.  What keeps the pass above the main stream's own 45 us is then the event record / wait packets
// around every pass (~7 us of gaps) and the side work's share of the CUs.
static int deferred_iter_sampler(catan_env_t* e, int64_t it, int64_t iters, int window, hipStream_t st, hipEvent_t* ev) {
    const int P = e->sched.t1_group, D = P == 1 ? 3 : 2;       // passes per group, group slots
    const int ba = (int)(it & 1);                              // bin-count / list set of this pass
    e->ctr_clean = 0;                                          // (the lock-step path re-initialises the counters after this)
    const Win win = win_of(it, iters, window);
    if (it == 0) { e->g_open = 0; e->g_count = 0; }
    const bool g_opens = !e->g_open;
    if (g_opens) { e->g_slot = (int)(e->g_count % D); e->g_passes = 0; e->g_open = 1; }
    const int fa = e->g_slot, ftag = fa < 2 ? 2 + fa : 6;      // (4, 5 are the window slots' tags)
    u32* const req_ctr = e->pend.ctr + (fa < 2 ? 4 + fa : 7);  // the length of the slot's request list (lrq_ctr)
    if (g_opens && e->g_count >= D) HIPCHK(hipStreamWaitEvent(st, e->ev_fdone[fa], 0));   // tier 1 of the group that used this slot last is complete
    OK_OR_RETURN(window_wait(e, win, st));
    OK_OR_RETURN(window_clear(e, win, it, st));
    pend_pass(e, fa, ftag, win.sa, ba, ba ^ 1);
    if (ev) HIPCHK(hipEventRecord(ev[5], st));
    // the group's first pass releases the slot's previous games (tag) and empties its request list; the second touches neither
    hipLaunchKernelGGL(k_sample_random<512>, dim3(blocks(e->n, 512)), dim3(512), 0, st, e->ctx, (const u32*)e->mpk, 0u, e->scratch_actions,
                       e->pctr, e->pend.busy, g_opens ? ftag : 0, win.back ? 4 + win.sa : 0,
                       (g_opens && it != 0) ? req_ctr : (u32*)nullptr, 1,
                       e->pend.ctr + 16 + NBINS * ba, e->pend.lists + (size_t)ba * NBINS * e->N);
    OK_OR_RETURN(enqueue_fast(e, e->scratch_actions, e->scratch_reward, e->scratch_done, st, ev, true));
    e->g_passes++;
    if (e->g_passes == P || win.closes) {                      // close the group: its tier 1 on the side stream
        HIPCHK(hipEventRecord(e->ev_fready[fa], st));
        HIPCHK(hipStreamWaitEvent(e->fstream, e->ev_fready[fa], 0));
        OK_OR_RETURN(enqueue_tier1(e, e->f_reward, e->f_done, e->fstream, ev, fa, e->sched.lr_budget[1], P == 2));
        HIPCHK(hipEventRecord(e->ev_fdone[fa], e->fstream));
        e->g_open = 0; e->g_count++;
    }
    if (win.closes) {
        OK_OR_RETURN(window_close(e, win, ev, e->s_reward, e->s_done, 0, (int)(e->g_count < D ? e->g_count : D)));
        if (win.last) {                               // the call returns with every step complete and no busy game
            OK_OR_RETURN(window_join(e, win, st));
            hipLaunchKernelGGL(k_release_tags, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, e->pend.busy);
            pend_lockstep(e);
        }
    }
    return CATAN_OK;
}

// One iteration of the deferred rollout (schedule above), fused-sampling form (round 4; the default since round 6): the main stream runs ONE
// kernel per pass.  k_step takes each game's action from the game's side row, and for every game it completes it draws the next action
// from the new masks and appends the game to the next pass's lists; a game on the slow path is simply in no list until the
// kernel that completes its step (k_lr_finish: the group after next; tier 2 / re-deal: the window after next, through the
// window's release list) has drawn its next action and enqueued it.  Every draw is a pure function of (game, decision index,
// state), so the games' trajectories are the lock-step ones whoever draws.
static int deferred_iter(catan_env_t* e, int64_t it, int64_t iters, int window, hipStream_t st, hipEvent_t* ev) {
    if (!e->sched.deferred_fused) return deferred_iter_sampler(e, it, iters, window, st, ev);
    // Tier 1 is forked once per GROUP of P passes (P = 2): a k_lr_finish launch lasts as long as its slowest search (~45 us next
    // to k_step) whatever the number of requests, the launches of consecutive groups serialise on one side stream, and the games
    // of group g return in the first pass of group g + 2 - with P = 1 the chain k_step -> k_lr_finish -> k_step two passes later
    // and the side stream's throughput bound the pass at ~(k_step + k_lr_finish) / 2; with P = 2 neither does.
    // S = P + 2 sets of bin counts / lists rotate: k_step(t) reads set t % S, appends to set (t + 1) % S and empties set
    // (t - 1) % S (its reader is done), which k_lr_finish(g) - launched behind the last pass of group g - and the k_steps before
    // pass (g + 2) P then fill.  Three tier-1 request lists rotate by group.
    constexpr int P = 2, S = P + 2;
    const int64_t g = it / P;
    const int ga = (int)(g & 1), gl = (int)(g % 3), rs = (int)(it % S);
    const bool gfirst = it % P == 0, glast = (it + 1) % P == 0;
    e->ctr_clean = 0;                                          // (the lock-step path re-initialises the counters after this)
    const Win win = win_of(it, iters, window);
    if (gfirst && g >= 2) HIPCHK(hipStreamWaitEvent(st, e->ev_fdone[ga], 0));   // tier 1 of group g-2 is complete (its games are in this pass's lists)
    if (ev) HIPCHK(hipEventRecord(ev[5], st));
    pend_pass(e, gl, 2 + ga, win.sa, rs, (rs + S - 1) % S);
    e->pend.bnext = (rs + 1) % S; e->pend.sample = 1; e->pend.nsub = e->sched.fused_subs;
    OK_OR_RETURN(window_wait(e, win, st));
    if (win.back)                                              // ... its games play again
        hipLaunchKernelGGL(k_release_window, dim3(64), dim3(BLOCK), 0, st, e->ctx, (const u32*)e->mpk, (const u32*)(e->pend.ctr + 11 + 4 * win.sa),
                           (const i32*)e->pend.resets[win.sa][2], e->pend, rs);
    OK_OR_RETURN(window_clear(e, win, it, st));
    if (it == 0) {
        HIPCHK(hipMemsetAsync(e->pend.bctr, 0, (size_t)BIN_SETS * NBINS * MAX_SUBS * BCTR_PAD * sizeof(u32), st));
        hipLaunchKernelGGL(k_sample_first, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, e->mpk, (const u32*)e->pctr, e->pend, rs);
    }
    e->pend.lrq_clear = glast ? (gl + 1) % 3 : -1;             // the next group's request list (read last by tier 1 of group g-2: complete)
    e->pend.brel = (int)(((g + 2) * P) % S);                   // tier 1 of this group: its games return in the first pass of group g + 2
    OK_OR_RETURN(enqueue_fast(e, e->scratch_actions, e->scratch_reward, e->scratch_done, st, ev, true));
    const bool forks = glast || win.last;                      // the group's tier 1 on the side stream
    if (forks) {
        HIPCHK(hipEventRecord(e->ev_fready[ga], st));
        HIPCHK(hipStreamWaitEvent(e->fstream, e->ev_fready[ga], 0));
        // (search + lane-per-game completion only with CATAN_LR_SPLIT=2: measured 41.0 us per pass with the split against 38.9 without - here the
        // completion kernel samples and enqueues lane per game with one atomic each, and tier 1's launches are not what bounds this loop)
        // tier 1 staggered behind the next pass's dispatch (T1_STAGGER_US above; Sched::t1_delay_us)
        // (the instrumented loop - catan_random_rollout_timed - has an event record in front of every k_step, which holds that launch back by ~3 us: the
        // stagger is lengthened by 4 us there, so that the ORDER of dispatch - and with it k_step's duration by the events - is the uninstrumented
        // loop's: 30.2 us by the events against 30.1 us by rocprofv3 over the plain loop; without the compensation the events read 33 us)
        const int t1_us = e->sched.t1_delay_us > 0 && ev != nullptr ? e->sched.t1_delay_us + 4 : e->sched.t1_delay_us;
        if (t1_us > 0) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, e->fstream, (long long)t1_us * 100);
        OK_OR_RETURN(enqueue_tier1(e, e->f_reward, e->f_done, e->fstream, ev, gl, e->sched.lr_budget[2], false, LR_GRID_FUSED));
        HIPCHK(hipEventRecord(e->ev_fdone[ga], e->fstream));
    }
    if (win.closes) {
        // When the pass is its group's last, the tier-1 launch behind it orders its k_step before the window's slow path.  A window of an ODD number
        // of passes closes in the MIDDLE of a group, and until round 6 nothing did: the re-deal kernel could read the re-deal list's length while k_step
        // was still appending, a game that ended in that pass was then never re-dealt and dropped out of every list (its counter is zeroed when the
        // slot opens again) - the intermittent trajectory-parity failures of the windows of 1 and 5 passes (HISTORY.md round 5,
        // DESIGN.md 4.0; guard: test_deferred_small_windows_repeated_with_the_middle_tier).
        if (!forks) HIPCHK(hipEventRecord(e->ev_fready[2], st));
        e->pend.brel = -1;                                     // tier 2 / re-deals: into the window's release list
        OK_OR_RETURN(window_close(e, win, ev, e->s_reward, e->s_done, ga, g >= 1 ? 2 : 1, forks ? nullptr : e->ev_fready[2]));
        if (win.last) {                               // the call returns with every step complete and no game left waiting
            OK_OR_RETURN(window_join(e, win, st));
            hipLaunchKernelGGL(k_finish_rollout, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, (const u32*)e->mpk, e->pctr, e->pend.busy);
            pend_lockstep(e);
        }
    }
    return CATAN_OK;
}

int catan_random_rollout_deferred(catan_env_t* e, int64_t iters, int32_t window, catan_stream_t stream) {
    if (!e || iters < 0 || window <= 0) return fail(CATAN_EINVAL, "catan_random_rollout_deferred: bad arguments");
    NOT_DEFERRED(e, "catan_random_rollout_deferred");
    NOT_MT(e, "catan_random_rollout_deferred");
    OK_OR_RETURN(record_not_armed(e, "catan_random_rollout_deferred", S(stream)));
    NO_START_POOL(e, "catan_random_rollout_deferred");
    for (int64_t it = 0; it < iters; it++) {
        int r = deferred_iter(e, it, iters, window, S(stream), nullptr);
        if (r != CATAN_OK) return r;
    }
    return CATAN_OK;
}

// ---- the deferred schedule for caller-supplied actions.  Call `it` of a sequence is iteration `it` of deferred_iter_sampler with a tier-1 launch per
// call on two slots and k_classify_deferred in the sampler's place; what differs is WHEN the waiting games are released: at the end of the call before
// the one they play in again (k_deliver), not at its start - the caller needs their completed state (observation, masks) to choose
// the action it passes to that call.  Every kernel writes a step's reward / done into the handle's result rows (f_reward /
// f_done: one row per game, written by whichever kernel completes the game's step); k_deliver hands them over.
int catan_step_deferred(catan_env_t* e, const int32_t* actions, int32_t window, float* reward, uint8_t* done, uint8_t* status, catan_stream_t stream) {
    if (!e || !actions || !reward || !done || !status || window <= 0) return fail(CATAN_EINVAL, "catan_step_deferred: bad arguments");
    NOT_MT(e, "catan_step_deferred");
    hipStream_t st = S(stream);
    if (e->d_it > 0 && (window != e->d_window || st != e->d_stream))
        return fail(CATAN_EINVAL, "catan_step_deferred: window and stream must stay the same between two flushes");
    const int64_t it = e->d_it;
    const int fa = (int)(it & 1);
    const Win win = win_of(it, -1, window);
    e->ctr_clean = 0;                                          // (the lock-step path re-initialises the counters after this)
    e->d_window = window; e->d_stream = st;
    // (tier 1 of call it-2 and, when this call opens window w, the slow path of window w-2 were joined at the end of call it-1)
    OK_OR_RETURN(window_clear(e, win, it, st));
    pend_pass(e, fa, 2 + fa, win.sa, fa, fa ^ 1);
    enqueue_record_append(e, actions, e->pend.busy, st);
    hipLaunchKernelGGL(k_classify_deferred, dim3(blocks(e->N, BLOCK)), dim3(BLOCK), 0, st, e->ctx, actions, (const u8*)e->pend.busy, e->pend.ctr + 16 + NBINS * fa,
                       e->pend.lists + (size_t)fa * NBINS * e->N, it == 0 ? (u32*)nullptr : e->pend.ctr + 4 + fa, 1, e->cfg.validate_actions ? e->err : (u32*)nullptr);
    OK_OR_RETURN(enqueue_fast(e, actions, e->f_reward, e->f_done, st, nullptr, true));
    HIPCHK(hipEventRecord(e->ev_fready[fa], st));
    HIPCHK(hipStreamWaitEvent(e->fstream, e->ev_fready[fa], 0));
    OK_OR_RETURN(enqueue_tier1(e, e->f_reward, e->f_done, e->fstream, nullptr, fa, e->sched.lr_budget[1]));
    HIPCHK(hipEventRecord(e->ev_fdone[fa], e->fstream));
    if (win.closes) OK_OR_RETURN(window_close(e, win, nullptr, e->f_reward, e->f_done, fa, it >= 1 ? 2 : 1));
    // what call it+1 needs: tier 1 of call it-1 complete (its games play again), and - if it opens window w' >= 2 - the slow path of w'-2
    const int64_t nit = it + 1;
    const Win next = win_of(nit, -1, window);
    if (nit >= 2) HIPCHK(hipStreamWaitEvent(st, e->ev_fdone[nit & 1], 0));
    OK_OR_RETURN(window_wait(e, next, st));
    hipLaunchKernelGGL(k_deliver, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, st, e->ctx, e->pend.busy, nit >= 2 ? 2 + (int)(nit & 1) : 0, next.back ? 4 + next.sa : 0, 0,
                       (const float*)e->f_reward, (const u8*)e->f_done, reward, done, status);
    enqueue_record_seal_done(e, done, status, nullptr, st);
    HIPCHK(hipGetLastError());
    e->d_it = nit;
    return CATAN_OK;
}

int catan_step_flush(catan_env_t* e, float* reward, uint8_t* done, uint8_t* status, catan_stream_t stream) {
    if (!e || !reward || !done || !status) return fail(CATAN_EINVAL, "catan_step_flush: null argument");
    hipStream_t st = S(stream);
    const int64_t it = e->d_it;
    if (it > 0) {
        if (st != e->d_stream) return fail(CATAN_EINVAL, "catan_step_flush: not the stream of the open sequence");
        const Win win = win_of(it - 1, -1, e->d_window);        // the window of the last call
        // ... is still open: close it (its pend.sa / stag are still set)
        if (!win.closes) OK_OR_RETURN(window_close(e, win, nullptr, e->f_reward, e->f_done, 0, it >= 2 ? 2 : 1));
        HIPCHK(hipStreamWaitEvent(st, e->ev_fdone[0], 0));
        if (it >= 2) HIPCHK(hipStreamWaitEvent(st, e->ev_fdone[1], 0));
        OK_OR_RETURN(window_join(e, win, st));
    }
    hipLaunchKernelGGL(k_deliver, dim3(blocks(e->n, BLOCK)), dim3(BLOCK), 0, st, e->ctx, e->pend.busy, 0, 0, 1, (const float*)e->f_reward, (const u8*)e->f_done, reward, done, status);
    enqueue_record_seal_done(e, done, status, nullptr, st);
    HIPCHK(hipGetLastError());
    pend_lockstep(e);
    e->d_it = 0;
    return CATAN_OK;
}

int catan_policy_counters(catan_env_t* e, uint32_t* out, catan_stream_t stream) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_policy_counters: null argument");
    HIPCHK(hipMemcpyAsync(out, e->pctr, (size_t)e->n * sizeof(u32), hipMemcpyDeviceToDevice, S(stream)));
    return CATAN_OK;
}

int catan_set_policy_counters(catan_env_t* e, const uint32_t* in, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_set_policy_counters: null handle");
    if (in) HIPCHK(hipMemcpyAsync(e->pctr, in, (size_t)e->n * sizeof(u32), hipMemcpyDeviceToDevice, S(stream)));
    else HIPCHK(hipMemsetAsync(e->pctr, 0, (size_t)e->N * sizeof(u32), S(stream)));
    return CATAN_OK;
}

int catan_set_step_wave_games(catan_env_t* e, int32_t games) {
    if (!e || (games != 64 && games != 32 && games != 16)) return fail(CATAN_EINVAL, "catan_set_step_wave_games: 64, 32 or 16");
    e->sched.step_games = games;
    return CATAN_OK;
}

int32_t catan_hip_runtime_version(void) { int v = 0; return hipRuntimeGetVersion(&v) == hipSuccess ? (int32_t)v : -1; }
int32_t catan_step_algorithmic_bytes(void) { return STEP_ALGO_BYTES; }
int32_t catan_step_fused_algorithmic_bytes(void) { return STEP_FUSED_ALGO_BYTES; }
int32_t catan_deferred_fused(const catan_env_t* e) { return e ? e->sched.deferred_fused : -1; }
int catan_set_deferred_fused(catan_env_t* e, int32_t on) {
    if (!e) return fail(CATAN_EINVAL, "catan_set_deferred_fused: null handle");
    e->sched.deferred_fused = on != 0;
    return CATAN_OK;
}
int catan_set_lr_budgets(catan_env_t* e, int32_t lockstep, int32_t deferred) {
    if (!e || lockstep < 1 || deferred < 1) return fail(CATAN_EINVAL, "catan_set_lr_budgets: bad arguments");
    e->sched.lr_budget[0] = lockstep; e->sched.lr_budget[1] = deferred; e->sched.lr_budget[2] = deferred;
    return CATAN_OK;
}

int catan_slow_path_counts(catan_env_t* e, catan_stream_t stream, uint64_t* out3) {
    if (!e || !out3) return fail(CATAN_EINVAL, "catan_slow_path_counts: null argument");
    HIPCHK(hipMemcpyAsync(out3, e->err + 4, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, S(stream)));
    HIPCHK(hipStreamSynchronize(S(stream)));
    return CATAN_OK;
}

int catan_set_lr_rounds(catan_env_t* e, int32_t lockstep, int32_t deferred) {
    if (!e || lockstep < 1 || deferred < 1) return fail(CATAN_EINVAL, "catan_set_lr_rounds: bad arguments");
    e->sched.lr_round[0] = lockstep; e->sched.lr_round[1] = deferred;
    return CATAN_OK;
}

int catan_calib_copy(void* dst, const void* src, int64_t bytes, catan_stream_t stream) {
    if (!dst || !src || bytes <= 0 || bytes % 16) return fail(CATAN_EINVAL, "catan_calib_copy: bad arguments");
    hipLaunchKernelGGL(k_calib_copy, dim3(4096), dim3(BLOCK), 0, S(stream), (const uint4*)src, (uint4*)dst, (long)(bytes / 16));
    return launched();
}

// k_step phase profile (100 MHz wall_clock64 ticks): enable/zero, then read [8] sums over waves + [8] maxima.
// phases: stage-in, validate+apply, tier-1 longest road, holder logic (+cut), done/reward, reset, masks, write-back.
int catan_profile_enable(catan_env_t* e, int on) {
    if (!e) return fail(CATAN_EINVAL, "catan_profile_enable: null handle");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(e->prof, 0, PROF_WORDS * sizeof(unsigned long long)));
    HIPCHK(hipMemset(e->prof_wave, 0, (size_t)(e->N / 16 + SORT_PAD_WAVES) * 8 * sizeof(u32)));
    e->prof_on = on;
    return CATAN_OK;
}
int catan_profile_read_waves(catan_env_t* e, uint32_t* out) {
    if (!e || !out) return fail(CATAN_EINVAL, "catan_profile_read_waves: bad arguments");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, e->prof_wave, (size_t)prof_wave_rows(e->N) * 8 * sizeof(u32), hipMemcpyDeviceToHost));
    return CATAN_OK;
}
int catan_profile_read(catan_env_t* e, uint64_t* out16) {
    if (!e || !out16) return fail(CATAN_EINVAL, "catan_profile_read: bad arguments");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out16, e->prof, PROF_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CATAN_OK;
}

// The rollout loops with a hipEvent around every kernel launch (recorded on the stream the kernel runs on).
// window <= 0: the lock-step loop of catan_random_rollout; window > 0: the deferred loop.  kernel_ms (host, float[5])
// receives the summed elapsed milliseconds of:
// [0] k_sample_random (incl. the sort by action type)  [1] k_step  [2] k_lr_finish  [3] k_lr_heavy (incl. the completion of
// its games)  [4] re-deals / installs (k_reset_list, k_install_list).
int catan_random_rollout_timed(catan_env_t* e, uint32_t step_idx0, int64_t steps, int32_t window, catan_stream_t stream, float* kernel_ms) {
    if (!e || steps <= 0 || !kernel_ms) return fail(CATAN_EINVAL, "catan_random_rollout_timed: bad arguments");
    if (window > 0) NOT_MT(e, "catan_random_rollout_timed (deferred)");
    if (window > 0) OK_OR_RETURN(record_not_armed(e, "catan_random_rollout_timed (deferred)", S(stream)));
    if (window > 0) NO_START_POOL(e, "catan_random_rollout_timed (deferred)");
    hipStream_t st = S(stream);
    const int K = EV_PER_STEP;             // see enqueue_fast / enqueue_tier1 / enqueue_slow; [5] = before the sampler
    struct Events {                        // destroyed however the call returns
        std::vector<hipEvent_t> v;
        ~Events() { for (hipEvent_t x : v) if (x) hipEventDestroy(x); }
        hipEvent_t& operator[](size_t i) { return v[i]; }
    } ev{ std::vector<hipEvent_t>((size_t)steps * K, nullptr) };
    for (auto& x : ev.v) HIPCHK(hipEventCreateWithFlags(&x, hipEventDisableSystemFence));   // no L2 flush between kernels
    std::vector<char> slow((size_t)steps, 0);
    for (int64_t s = 0; s < steps; s++) {
        hipEvent_t* v = &ev[(size_t)s * K];
        int r;
        if (window > 0) {
            r = deferred_iter(e, s, steps, window, st, v);
            slow[s] = ((s + 1) % window == 0 || s + 1 == steps);
        } else {
            const uint32_t step_idx = step_idx0 + (uint32_t)s;
            r = step_impl(e, e->scratch_actions, e->scratch_reward, e->scratch_done, st, v, &step_idx);
            slow[s] = 1;
        }
        if (r != CATAN_OK) return r;
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(e->fstream));
    HIPCHK(hipStreamSynchronize(e->sstream));
    for (int k = 0; k < 5; k++) kernel_ms[k] = 0.0f;
    for (int64_t s = 0; s < steps; s++) {
        hipEvent_t* v = &ev[(size_t)s * K];
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, v[5], v[0])); kernel_ms[0] += ms;      // k_sample_random (sampling + sort lists)
        HIPCHK(hipEventElapsedTime(&ms, v[0], v[2])); kernel_ms[1] += ms;      // k_step
        if (hipEventElapsedTime(&ms, v[8], v[6]) == hipSuccess) kernel_ms[2] += ms;   // k_lr_finish (deferred loop: launched once per group of passes)
        else (void)hipGetLastError();
        if (!slow[s]) continue;
        HIPCHK(hipEventElapsedTime(&ms, v[9], v[3])); kernel_ms[3] += ms;      // k_lr_heavy
        HIPCHK(hipEventElapsedTime(&ms, v[7], v[4])); kernel_ms[4] += ms;      // k_reset_list / k_install_list (wait for the side stream + second pass)
    }
    return CATAN_OK;
}

int catan_obs(catan_env_t* e, float* out_f, int32_t* out_lists, int32_t* out_lens, catan_stream_t stream) {
    if (!e || !out_f || !out_lists || !out_lens) return fail(CATAN_EINVAL, "catan_obs: null argument");
    hipLaunchKernelGGL((k_obs_rows<ObsF32, OBS_OG>), dim3(blocks(e->n, OBS_OG)), dim3(64), 0, S(stream), e->ctx, out_f, out_lists, out_lens,
                       (float*)nullptr, (signed char*)nullptr, (signed char*)nullptr, (const long long*)nullptr, (const u8*)nullptr, (const i32*)nullptr, (long)e->n);
    return launched();
}

static int obs_rows_impl(catan_env_t* e, int32_t bf16, void* dense_f, int32_t* dense_lists, int32_t* dense_lens, void* rows_f, int8_t* rows_lists,
                         int8_t* rows_lens, const int64_t* t_idx, const uint8_t* sel, const int32_t* games, int64_t n_rows, catan_stream_t stream) {
    if (!e || (!dense_f && !rows_f)) return fail(CATAN_EINVAL, "catan_obs_rows: no output");
    if ((dense_lists == nullptr) != (dense_lens == nullptr) || (rows_lists == nullptr) != (rows_lens == nullptr))
        return fail(CATAN_EINVAL, "catan_obs_rows: lists and lens come together");
    if (rows_f && (!t_idx || !sel)) return fail(CATAN_EINVAL, "catan_obs_rows: row stores need t_idx and sel");
    if ((rows_lists && !rows_f) || (dense_lists && !dense_f)) return fail(CATAN_EINVAL, "catan_obs_rows: lists without their observation rows");
    const dim3 grid(blocks(n_rows, OBS_OG));
    if (bf16) hipLaunchKernelGGL((k_obs_rows<ObsBF16, OBS_OG>), grid, dim3(64), 0, S(stream), e->ctx, (unsigned short*)dense_f, dense_lists, dense_lens, (unsigned short*)rows_f,
                                 (signed char*)rows_lists, (signed char*)rows_lens, (const long long*)t_idx, sel, games, (long)n_rows);
    else hipLaunchKernelGGL((k_obs_rows<ObsF32, OBS_OG>), grid, dim3(64), 0, S(stream), e->ctx, (float*)dense_f, dense_lists, dense_lens, (float*)rows_f,
                            (signed char*)rows_lists, (signed char*)rows_lens, (const long long*)t_idx, sel, games, (long)n_rows);
    return launched();
}
int catan_obs_rows(catan_env_t* e, int32_t bf16, void* dense_f, int32_t* dense_lists, int32_t* dense_lens, void* rows_f, int8_t* rows_lists,
                   int8_t* rows_lens, const int64_t* t_idx, const uint8_t* sel, catan_stream_t stream) {
    return obs_rows_impl(e, bf16, dense_f, dense_lists, dense_lens, rows_f, rows_lists, rows_lens, t_idx, sel, nullptr, e ? e->n : 0, stream);
}
int catan_obs_rows_of(catan_env_t* e, int32_t bf16, void* dense_f, int32_t* dense_lists, int32_t* dense_lens, void* rows_f, int8_t* rows_lists,
                      int8_t* rows_lens, const int64_t* t_idx, const uint8_t* sel, const int32_t* games, int64_t n_rows, catan_stream_t stream) {
    if (!e || !games || n_rows <= 0 || n_rows > e->n) return fail(CATAN_EINVAL, "catan_obs_rows_of: bad game list");
    return obs_rows_impl(e, bf16, dense_f, dense_lists, dense_lens, rows_f, rows_lists, rows_lens, t_idx, sel, games, n_rows, stream);
}
int catan_masks_of(catan_env_t* e, float* out, const int32_t* games, int64_t n_rows, catan_stream_t stream) {
    if (!e || !out || !games || n_rows <= 0 || n_rows > e->n) return fail(CATAN_EINVAL, "catan_masks_of: bad arguments");
    hipLaunchKernelGGL(k_expand_masks_of, dim3(blocks(n_rows * MASK_BITS, BLOCK)), dim3(BLOCK), 0, S(stream), (const u32*)e->mpk, games, (long)n_rows, (long)e->n,
                       e->d_it > 0 ? (const u8*)e->pend.busy : (const u8*)nullptr, out);
    return launched();
}

int catan_longest_path(catan_env_t* e, const int32_t* players, int32_t* out, catan_stream_t stream) {
    if (!e || !players || !out) return fail(CATAN_EINVAL, "catan_longest_path: null argument");
    hipLaunchKernelGGL(k_longest_path, dim3(blocks(e->N, 64)), dim3(64), 0, S(stream), e->ctx, players, out);
    return launched();
}

}  // extern "C"

#include "catan_abi_nn.h"
#include "catan_abi_players.h"
