// catan_abi_hooks.h - what hangs on a re-deal (include/catan_hip_tuning.h), feature by feature: the enqueue_* hook that enqueue_redeal and the
// stepping calls of catan_abi.hip run, then the feature's entry points.  Finished-game statistics, league results, game records, the start
// pool with its weights and outcomes, the tournament; the state check, which has no hook, stands last.  Included behind struct catan_env and
// its guards, in front of the stepping code.
#pragma once

extern "C" {

// ---- finished-game statistics (catan_stats.hip; catan_episode_stats_enable): the games of a re-deal list are counted on the stream of the kernel that consumes the
// list, immediately in front of it - their records are still the final states.  Off (the default): nothing is launched.
static void enqueue_episode_stats(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!e->stats_on) return;
    hipLaunchKernelGGL(k_episode_stats, dim3(EPISODE_STATS_GRID), dim3(64), 0, st, e->ctx, count_p, list, e->stats_focus, e->stats);
}
constexpr size_t EPISODE_STATS_BYTES = ES_WORDS * sizeof(unsigned long long);
int32_t catan_episode_stats_words(void) { return ES_WORDS; }
int catan_episode_stats_enable(catan_env_t* e, int on, const int32_t* focus_pid, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_episode_stats_enable: null handle");
    if (!e->cfg.auto_reset) return fail(CATAN_EINVAL, "catan_episode_stats_enable: the handle has auto_reset = 0 (no game is re-dealt: read the final states themselves)");
    NOT_DEFERRED(e, "catan_episode_stats_enable");
    NOT_MT(e, "catan_episode_stats_enable");
    if (!on) { e->stats_on = 0; e->stats_focus = nullptr; return CATAN_OK; }
    if (!e->stats) {
        hipError_t rc = hipSuccess;
        dev_alloc(e, rc, e->stats, EPISODE_STATS_BYTES);
        if (rc != hipSuccess) return fail(CATAN_ENOMEM, std::string("catan_episode_stats_enable: hipMalloc: ") + hipGetErrorString(rc));
    }
    HIPCHK(hipMemsetAsync(e->stats, 0, EPISODE_STATS_BYTES, S(stream)));
    e->stats_focus = focus_pid; e->stats_on = 1;
    return CATAN_OK;
}
int catan_episode_stats_read(catan_env_t* e, uint64_t* out_host, int reset, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_episode_stats_read: null argument");
    if (!e->stats_on) return fail(CATAN_EINVAL, "catan_episode_stats_read: statistics are not enabled on this handle (catan_episode_stats_enable)");
    NOT_DEFERRED(e, "catan_episode_stats_read");      // (the side streams of an open sequence are joined by catan_step_flush)
    return read_counters(out_host, e->stats, EPISODE_STATS_BYTES, reset, S(stream));
}

// ---- per-opponent results of a league rollout (catan_league_stats.hip; catan_league_stats_enable): count_p / list as above, or count_p == nullptr and `count` games (list == nullptr: games 0..count-1)
static void launch_league_stats(catan_env_t* e, const u32* count_p, u32 count, const i32* list, unsigned grid, hipStream_t st) {
    if (e->lstats_nets <= LEAGUE_STATS_LDS_MAX_NETS)
        hipLaunchKernelGGL(k_league_stats<true>, dim3(grid), dim3(64), 0, st, e->ctx, count_p, count, list, e->lstats_slot, e->lstats_net, e->lstats_nets, e->lstats);
    else
        hipLaunchKernelGGL(k_league_stats<false>, dim3(grid), dim3(64), 0, st, e->ctx, count_p, count, list, e->lstats_slot, e->lstats_net, e->lstats_nets, e->lstats);
}
// ... at the same hook as the finished-game statistics, and as independent of them.  Off (the default): nothing is launched.
static void enqueue_league_stats(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!(e->lstats_on & CATAN_LEAGUE_STATS_REDEALS)) return;
    launch_league_stats(e, count_p, 0u, list, LEAGUE_STATS_GRID, st);
}
static size_t league_table_bytes(int nets) { return ((size_t)nets + 1) * LS_WORDS * sizeof(unsigned long long); }   // (the last row: the totals)
int32_t catan_league_stats_words(void) { return LS_WORDS; }
int catan_league_stats_enable(catan_env_t* e, int on, const int32_t* slot_of_pid, const int32_t* net_of_slot, int32_t num_nets, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_league_stats_enable: null handle");
    if ((on & CATAN_LEAGUE_STATS_REDEALS) && !e->cfg.auto_reset)
        return fail(CATAN_EINVAL, "catan_league_stats_enable: the handle has auto_reset = 0 (no game is re-dealt: enable with CATAN_LEAGUE_STATS_COUNT_ONLY and use catan_league_stats_count)");
    NOT_DEFERRED(e, "catan_league_stats_enable");
    NOT_MT(e, "catan_league_stats_enable");
    if (!on) { e->lstats_on = 0; e->lstats_slot = e->lstats_net = nullptr; return CATAN_OK; }
    if (on & ~(CATAN_LEAGUE_STATS_REDEALS | CATAN_LEAGUE_STATS_COUNT_ONLY)) return fail(CATAN_EINVAL, "catan_league_stats_enable: unknown mode bits in `on`");
    if (num_nets < 1 || num_nets > LEAGUE_STATS_MAX_NETS) return fail(CATAN_EINVAL, "catan_league_stats_enable: num_nets must be in 1..65536");
    if (!slot_of_pid || !net_of_slot) return fail(CATAN_EINVAL, "catan_league_stats_enable: null map (slot_of_pid and net_of_slot are device int32 [n][4] and [n][3])");
    if (num_nets > e->lstats_cap) {                    // the table grows only
        // (hipFree waits for the device: no tally of the old table is in flight behind it)
        e->lstats_on = 0;
        if (e->lstats) { HIPCHK(hipFree(e->lstats)); e->lstats = nullptr; e->lstats_cap = 0; }
        Staged stage;
        stage.alloc(e->lstats, league_table_bytes(num_nets));
        if (!stage.ok()) return stage.enomem("catan_league_stats_enable");
        stage.commit();
        e->lstats_cap = num_nets;
    }
    HIPCHK(hipMemsetAsync(e->lstats, 0, league_table_bytes(num_nets), S(stream)));
    e->lstats_slot = slot_of_pid; e->lstats_net = net_of_slot; e->lstats_nets = num_nets; e->lstats_on = on;
    return CATAN_OK;
}
int catan_league_stats_read(catan_env_t* e, uint64_t* out_host, int reset, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_league_stats_read: null argument");
    if (!e->lstats_on) return fail(CATAN_EINVAL, "catan_league_stats_read: league results are not enabled on this handle (catan_league_stats_enable)");
    NOT_DEFERRED(e, "catan_league_stats_read");       // (the side streams of an open sequence are joined by catan_step_flush)
    return read_counters(out_host, e->lstats, league_table_bytes(e->lstats_nets), reset, S(stream));
}
int catan_league_stats_count(catan_env_t* e, const int32_t* games, int64_t m, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_league_stats_count: null handle");
    if (!e->lstats_on) return fail(CATAN_EINVAL, "catan_league_stats_count: league results are not enabled on this handle (catan_league_stats_enable)");
    NOT_DEFERRED(e, "catan_league_stats_count");
    NOT_MT(e, "catan_league_stats_count");
    if (m <= 0 || m > 0x7fffffffll) return fail(CATAN_EINVAL, "catan_league_stats_count: m must be in 1..2^31-1");
    if (!games && m > e->n) return fail(CATAN_EINVAL, "catan_league_stats_count: m exceeds the handle's games (games == NULL)");
    launch_league_stats(e, nullptr, (u32)m, games, grid_for(m, 64, 256), S(stream));
    return launched();
}

// ---- game records (catan_record_enable; the kernels of this and the next hooks are catan_hooks.hip's, and a launch's status stays pending for the
// hipGetLastError at the end of the caller's sequence: catan_hooks.h).  Seal: at the hook of the finished-game statistics, the listed games'
// records are still the final states.  Open: behind the list's consumer, on the same stream, the listed games are freshly dealt.  Off (the
// default): nothing is launched.
static void enqueue_record_seal(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!e->rec_on) return;
    (void)record_launch_seal(e->ctx, e->rec, count_p, list, nullptr, nullptr, nullptr, st);
}
static void enqueue_record_open(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!e->rec_on) return;
    (void)record_launch_open(e->ctx, e->rec, count_p, list, st);
}
// ... the append in front of the step's first kernel that reads `actions` (busy: the deferred calls' waiting games)
static void enqueue_record_append(catan_env_t* e, const i32* actions, const u8* busy, hipStream_t st) {
    if (!e->rec_on) return;
    (void)record_launch_append(e->ctx, e->rec, actions, busy, st);
}
// ... and, on a handle without auto_reset (no re-deal list is ever consumed), the seal at the end of a stepping call over its done flags
static void enqueue_record_seal_done(catan_env_t* e, const u8* done, const u8* status, const i32* actions, hipStream_t st) {
    if (!e->rec_on || e->cfg.auto_reset) return;
    (void)record_launch_seal(e->ctx, e->rec, nullptr, nullptr, done, status, actions, st);
}
static void record_free(catan_env_t* e) {
    for (void* p : { (void*)e->rec.hdr, (void*)e->rec.slot_of, (void*)e->rec.start, (void*)e->rec.fin, (void*)e->rec.log, (void*)e->rec.arm_list })
        if (p) hipFree(p);
    e->rec = RecordBuf{};
    e->rec_on = 0;
}
// every slot's header (and guard word) on the host; synchronises st
static int record_headers(catan_env_t* e, std::vector<u32>& hdr, hipStream_t st) {
    const int m = e->rec.m;
    hdr.assign((size_t)m * RECORD_HDR_WORDS, 0u);
    std::vector<u32> guard((size_t)m, 0u);
    HIPCHK(hipMemcpyAsync(hdr.data(), e->rec.hdr, hdr.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(guard.data(), sizeof(u32), e->rec.log + (size_t)e->rec.capacity * ACTION_WORDS, (size_t)e->rec.log_stride * sizeof(short),
                            sizeof(u32), (size_t)m, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < m; s++) if (guard[s] != RECORD_GUARD) hdr[(size_t)s * RECORD_HDR_WORDS + REC_H_FLAGS] |= REC_F_GUARD_BROKEN;
    return CATAN_OK;
}
// the library's own deferred loops draw their actions inside k_step: there is no action row to log
static int record_not_armed(catan_env_t* e, const char* what, hipStream_t st) {
    if (!e->rec_on) return CATAN_OK;
    std::vector<u32> hdr;
    OK_OR_RETURN(record_headers(e, hdr, st));
    for (int s = 0; s < e->rec.m; s++) {
        const u32 state = hdr[(size_t)s * RECORD_HDR_WORDS + REC_H_STATE];
        if (state == REC_WAIT_DEAL || state == REC_RECORDING)
            return fail(CATAN_EINVAL, std::string(what) + ": record slot " + std::to_string(s) + " is armed (the deferred rollout's actions never exist outside k_step)");
    }
    return CATAN_OK;
}
int catan_record_enable(catan_env_t* e, const int32_t* games, int32_t m, int32_t capacity, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_record_enable: null handle");
    NOT_DEFERRED(e, "catan_record_enable");
    NOT_MT(e, "catan_record_enable");
    if (m < 0 || m > RECORD_MAX_SLOTS) return fail(CATAN_EINVAL, "catan_record_enable: m must be in 0..4096");
    if (m > 0 && (capacity < 1 || capacity > RECORD_MAX_CAPACITY)) return fail(CATAN_EINVAL, "catan_record_enable: capacity must be in 1..65535");
    if (m > 0 && !games) return fail(CATAN_EINVAL, "catan_record_enable: null games");
    const hipStream_t st = S(stream);
    OK_OR_RETURN(sync_hook_streams(e, st));                       // the old slots may still be written
    record_free(e);                                               // the old slots are gone whether the new ones come to stand or not
    if (m == 0) return CATAN_OK;
    RecordBuf rb{};
    rb.m = m; rb.capacity = capacity; rb.log_stride = (long)capacity * ACTION_WORDS + 2;
    u32* bad = nullptr;
    Staged stage;
    stage.alloc(rb.hdr, (size_t)m * RECORD_HDR_WORDS * sizeof(u32));
    stage.alloc(rb.slot_of, (size_t)e->N * sizeof(i32));
    stage.alloc(rb.start, (size_t)m * STATE_WORDS * sizeof(i32));
    stage.alloc(rb.fin, (size_t)m * STATE_WORDS * sizeof(i32));
    stage.alloc(rb.log, (size_t)m * rb.log_stride * sizeof(short));
    stage.alloc(rb.arm_list, (size_t)m * sizeof(i32));
    stage.alloc(bad, sizeof(u32));
    if (!stage.ok()) return stage.enomem("catan_record_enable");
    hipError_t rc = hipMemsetAsync(rb.slot_of, 0xFF, (size_t)e->N * sizeof(i32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(rb.start, 0, (size_t)m * STATE_WORDS * sizeof(i32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(rb.fin, 0, (size_t)m * STATE_WORDS * sizeof(i32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(bad, 0, sizeof(u32), st);
    if (rc == hipSuccess) rc = record_launch_bind((long)e->n, games, rb, bad, st);
    u32 nbad = 0;
    if (rc == hipSuccess) rc = hipMemcpyAsync(&nbad, bad, sizeof(u32), hipMemcpyDeviceToHost, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    stage.free_now(bad);
    if (rc != hipSuccess) return fail(CATAN_EHIP, std::string("catan_record_enable: ") + hipGetErrorString(rc));
    if (nbad != 0) return fail(CATAN_EINVAL, "catan_record_enable: " + std::to_string(nbad) + " entries of games are outside [0, n) or list a game twice");
    stage.commit();
    e->rec = rb;
    e->rec_on = 1;
    return CATAN_OK;
}
int catan_record_arm(catan_env_t* e, const int32_t* slots, int32_t k, int32_t mode, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_record_arm: null handle");
    if (!e->rec_on) return fail(CATAN_EINVAL, "catan_record_arm: recording is not enabled on this handle (catan_record_enable)");
    NOT_DEFERRED(e, "catan_record_arm");
    if (mode != CATAN_RECORD_NOW && mode != CATAN_RECORD_AT_DEAL) return fail(CATAN_EINVAL, "catan_record_arm: mode is CATAN_RECORD_NOW or CATAN_RECORD_AT_DEAL");
    if (mode == CATAN_RECORD_AT_DEAL && !e->cfg.auto_reset) return fail(CATAN_EINVAL, "catan_record_arm: CATAN_RECORD_AT_DEAL on a handle with auto_reset = 0 (no game is re-dealt)");
    if (!slots) k = e->rec.m;
    if (k < 1 || k > e->rec.m) return fail(CATAN_EINVAL, "catan_record_arm: k must be in 1..m");
    if (slots) {
        for (int j = 0; j < k; j++)
            if (slots[j] < 0 || slots[j] >= e->rec.m) return fail(CATAN_EINVAL, "catan_record_arm: slot " + std::to_string(slots[j]) + " is outside [0, m)");
        // (a pageable source: the copy has left the caller's array when the call returns)
        HIPCHK(hipMemcpyAsync(e->rec.arm_list, slots, (size_t)k * sizeof(i32), hipMemcpyHostToDevice, S(stream)));
    }
    HIPCHK(record_launch_arm(e->ctx, e->rec, slots ? (const i32*)e->rec.arm_list : (const i32*)nullptr, (int)k, mode == CATAN_RECORD_NOW ? 1 : 0, S(stream)));
    return CATAN_OK;
}
int catan_record_status(catan_env_t* e, uint32_t* out_host, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_record_status: null argument");
    if (!e->rec_on) return fail(CATAN_EINVAL, "catan_record_status: recording is not enabled on this handle (catan_record_enable)");
    NOT_DEFERRED(e, "catan_record_status");           // (the side streams of an open sequence are joined by catan_step_flush)
    std::vector<u32> hdr;
    OK_OR_RETURN(record_headers(e, hdr, S(stream)));
    memcpy(out_host, hdr.data(), hdr.size() * sizeof(u32));
    return CATAN_OK;
}
int catan_record_read(catan_env_t* e, int32_t slot, int32_t* start_blob, int32_t* final_blob, int32_t* actions, uint32_t* out_host_header, catan_stream_t stream) {
    if (!e || !out_host_header) return fail(CATAN_EINVAL, "catan_record_read: null argument");
    if (!e->rec_on) return fail(CATAN_EINVAL, "catan_record_read: recording is not enabled on this handle (catan_record_enable)");
    NOT_DEFERRED(e, "catan_record_read");
    if (slot < 0 || slot >= e->rec.m) return fail(CATAN_EINVAL, "catan_record_read: slot is outside [0, m)");
    const hipStream_t st = S(stream);
    std::vector<u32> hdr;
    OK_OR_RETURN(record_headers(e, hdr, st));
    const u32* h = hdr.data() + (size_t)slot * RECORD_HDR_WORDS;
    memcpy(out_host_header, h, RECORD_HDR_WORDS * sizeof(u32));
    if (h[REC_H_STATE] != REC_SEALED && h[REC_H_STATE] != REC_RECORDING)
        return fail(CATAN_EINVAL, "catan_record_read: slot " + std::to_string(slot) + " is neither SEALED nor RECORDING");
    const size_t rows = h[REC_H_LENGTH] < (u32)e->rec.capacity ? h[REC_H_LENGTH] : (u32)e->rec.capacity;
    std::vector<short> log(rows * ACTION_WORDS);
    if (start_blob) HIPCHK(hipMemcpyAsync(start_blob, e->rec.start + (size_t)slot * STATE_WORDS, STATE_WORDS * sizeof(i32), hipMemcpyDeviceToHost, st));
    if (final_blob && h[REC_H_STATE] == REC_SEALED)
        HIPCHK(hipMemcpyAsync(final_blob, e->rec.fin + (size_t)slot * STATE_WORDS, STATE_WORDS * sizeof(i32), hipMemcpyDeviceToHost, st));
    if (actions && rows) HIPCHK(hipMemcpyAsync(log.data(), e->rec.log + (size_t)slot * e->rec.log_stride, log.size() * sizeof(short), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (actions) for (size_t i = 0; i < log.size(); i++) actions[i] = (int32_t)log[i];
    return CATAN_OK;
}

// ---- start pool (catan_start_pool_set; the kernels are catan_hooks.hip's but for k_import and k_masks): directly behind the consumer of a re-deal list (enqueue_redeal has the order and its reasons), or
// behind catan_reset's deal over the games with sel[g] != 0 (sel == nullptr: every game).  Weights set: the weighted pick; outcomes on:
// the origin word is written.  No pool installed (the default): nothing is launched.
static PoolPick pool_pick_of(const catan_env_t* e) { return PoolPick{ e->pool_cum, e->pool_W, e->pool_out_on ? e->pool_origin : nullptr }; }
static void enqueue_start_pool(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!e->pool_on) return;
    (void)pool_launch_install(e->ctx, e->mpk, e->pool, pool_pick_of(e), count_p, list, nullptr, st);
}
static void enqueue_start_pool_sel(catan_env_t* e, const u8* sel, hipStream_t st) {
    if (!e->pool_on) return;
    (void)pool_launch_install(e->ctx, e->mpk, e->pool, pool_pick_of(e), nullptr, nullptr, sel, st);
}
// ... its per-entry outcomes (catan_start_pool_outcomes_enable) at the hook of the league results, directly beside them, and the origins of the games
// that catan_state_import / catan_state_fork overwrite.  Outcomes off (the default): nothing is launched.
static void enqueue_start_pool_outcomes(catan_env_t* e, const u32* count_p, const i32* list, hipStream_t st) {
    if (!e->pool_out_on) return;
    (void)pool_launch_outcomes(e->ctx, count_p, list, e->pool_origin, e->pool_out_focus, e->pool_out, e->pool.m, st);
}
static void enqueue_start_pool_origin_clear(catan_env_t* e, const long* idx, long cnt, hipStream_t st) {
    if (!e->pool_out_on) return;
    (void)pool_launch_origin_clear(e->pool_origin, e->n, idx, cnt, st);
}
static void start_pool_free(catan_env_t* e) {
    for (void* p : { (void*)e->pool.rec, (void*)e->pool.mask, (void*)e->pool.cnt, (void*)e->pool_cum, (void*)e->pool_origin, (void*)e->pool_out })
        if (p) hipFree(p);
    e->pool = StartPoolBuf{};
    e->pool_on = 0;
    // weights and outcomes belong to the pool they were set on (catan_start_pool_set carries the outcomes over itself)
    e->pool_cum = nullptr; e->pool_W = 0u;
    e->pool_origin = nullptr; e->pool_out = nullptr; e->pool_out_focus = nullptr; e->pool_out_on = 0;
}
static size_t start_pool_count_bytes(int m) { return ((size_t)m + 2) * sizeof(unsigned long long); }               // pool, fresh, then per entry
static size_t start_pool_outcome_bytes(int m) { return ((size_t)PO_HEAD + ((size_t)m + 1) * PO_WORDS) * sizeof(unsigned long long); }
int catan_start_pool_set(catan_env_t* e, const int32_t* blobs, int32_t m, int32_t fresh_q16, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_start_pool_set: null handle");
    NOT_DEFERRED(e, "catan_start_pool_set");
    NOT_MT(e, "catan_start_pool_set");
    if (m < 1 || m > POOL_MAX_ENTRIES) return fail(CATAN_EINVAL, "catan_start_pool_set: m must be in 1..65536");
    if (fresh_q16 < 0 || fresh_q16 > (int32_t)POOL_Q16_ONE) return fail(CATAN_EINVAL, "catan_start_pool_set: fresh_q16 must be in 0..65536");
    if (!blobs) return fail(CATAN_EINVAL, "catan_start_pool_set: null blobs");
    const hipStream_t st = S(stream);
    // the new pool is built beside the one in use, which stays installed if this call fails
    StartPoolBuf pb{};
    pb.m = m; pb.fresh_q16 = (u32)fresh_q16;
    u32* bad = nullptr;
    unsigned long long* out = nullptr;                // outcomes on: they stay on, with a fresh zeroed table of the new size
    Staged stage;
    stage.alloc(pb.rec, (size_t)m * REC * sizeof(u32));
    if (e->pool_out_on) stage.alloc(out, start_pool_outcome_bytes(m));
    stage.alloc(pb.mask, (size_t)m * MPK_STRIDE * sizeof(u32));
    stage.alloc(pb.cnt, start_pool_count_bytes(m));
    stage.alloc(bad, sizeof(u32));
    if (!stage.ok()) return stage.enomem("catan_start_pool_set");
    hipError_t rc = hipMemsetAsync(pb.rec, 0, (size_t)m * REC * sizeof(u32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(pb.cnt, 0, start_pool_count_bytes(m), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(bad, 0, sizeof(u32), st);
    if (rc == hipSuccess && out) rc = hipMemsetAsync(out, 0, start_pool_outcome_bytes(m), st);
    if (rc == hipSuccess) {
        // k_import and k_masks themselves, on the pool's records as a handle of m games: an entry's record is what catan_state_import makes of
        // its blob, and its mask row what catan_reset's masks would be under the handle's limits
        Ctx pc = e->ctx;
        pc.R = pb.rec; pc.N = m; pc.n = m; pc.mt = nullptr; pc.bcfg = nullptr; pc.bcfg_idx = nullptr;
        hipLaunchKernelGGL(k_import, dim3(blocks(m, BLOCK)), dim3(BLOCK), 0, st, pc, (const long*)nullptr, (long)m, blobs);
        hipLaunchKernelGGL(k_masks, dim3(blocks(m, BLOCK)), dim3(BLOCK), 0, st, pc, pb.mask, limits_of(e));
        rc = pool_launch_count_finished(pb.rec, m, bad, st);
    }
    u32 nbad = 0;
    if (rc == hipSuccess) rc = hipMemcpyAsync(&nbad, bad, sizeof(u32), hipMemcpyDeviceToHost, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    if (rc != hipSuccess) return fail(CATAN_EHIP, std::string("catan_start_pool_set: ") + hipGetErrorString(rc));
    if (nbad != 0) return fail(CATAN_EINVAL, "catan_start_pool_set: " + std::to_string(nbad) + " blobs are positions of finished games (winner != 0)");
    stage.free_now(bad);
    if (e->pool_on) OK_OR_RETURN(sync_hook_streams(e, st));
    // the origins are reset: the games in flight started from the old pool and are not booked to the new one.  The weights go: a new pool is uniform.
    i32* const origin = e->pool_origin; const i32* const focus = e->pool_out_focus;
    e->pool_origin = nullptr;
    start_pool_free(e);
    stage.commit();
    e->pool = pb;
    e->pool_on = 1;
    if (out) {
        e->pool_out = out; e->pool_origin = origin; e->pool_out_focus = focus; e->pool_out_on = 1;
        // (a failure here is reported with the new pool installed, and the origins may then still name entries of the old one: kept as it has always been)
        HIPCHK(hipMemsetAsync(origin, 0xFF, (size_t)e->n * sizeof(i32), st));
    } else if (origin) hipFree(origin);
    return CATAN_OK;
}
int catan_start_pool_clear(catan_env_t* e, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_start_pool_clear: null handle");
    NOT_DEFERRED(e, "catan_start_pool_clear");
    if (!e->pool_on) return CATAN_OK;
    OK_OR_RETURN(sync_hook_streams(e, S(stream)));
    start_pool_free(e);
    return CATAN_OK;
}
int32_t catan_start_pool_size(const catan_env_t* e) { return e ? (e->pool_on ? e->pool.m : 0) : -1; }
int catan_start_pool_read(catan_env_t* e, uint64_t* out_host, int32_t reset, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_start_pool_read: null argument");
    if (!e->pool_on) return fail(CATAN_EINVAL, "catan_start_pool_read: no start pool is installed on this handle (catan_start_pool_set)");
    NOT_DEFERRED(e, "catan_start_pool_read");          // (the side streams of an open sequence are joined by catan_step_flush)
    return read_counters(out_host, e->pool.cnt, start_pool_count_bytes(e->pool.m), reset, S(stream));
}

// the weighted pick and the per-entry outcomes
int catan_start_pool_set_weights(catan_env_t* e, const uint32_t* weights_dev, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_start_pool_set_weights: null handle");
    NOT_DEFERRED(e, "catan_start_pool_set_weights");
    NOT_MT(e, "catan_start_pool_set_weights");
    if (!e->pool_on) return fail(CATAN_EINVAL, "catan_start_pool_set_weights: no start pool is installed on this handle (catan_start_pool_set)");
    const hipStream_t st = S(stream);
    if (!weights_dev) {                                // back to the uniform pick
        if (!e->pool_cum) return CATAN_OK;
        OK_OR_RETURN(sync_hook_streams(e, st));
        hipFree(e->pool_cum);
        e->pool_cum = nullptr; e->pool_W = 0u;
        return CATAN_OK;
    }
    // the new table is built beside the one in force, which stays if this call fails
    const int m = e->pool.m;
    u32* cum = nullptr;
    unsigned long long* total = nullptr;
    Staged stage;
    stage.alloc(cum, (size_t)m * sizeof(u32));
    stage.alloc(total, sizeof(unsigned long long));
    if (!stage.ok()) return stage.enomem("catan_start_pool_set_weights");
    hipError_t rc = pool_launch_scan((const u32*)weights_dev, cum, total, m, st);
    unsigned long long W = 0ull;
    if (rc == hipSuccess) rc = hipMemcpyAsync(&W, total, sizeof W, hipMemcpyDeviceToHost, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    if (rc != hipSuccess) return fail(CATAN_EHIP, std::string("catan_start_pool_set_weights: ") + hipGetErrorString(rc));
    if (W == 0ull || W > 0xFFFFFFFFull)
        return fail(CATAN_EINVAL, "catan_start_pool_set_weights: the weights sum to " + std::to_string(W) + " (the sum must be in 1..2^32-1)");
    stage.free_now(total);
    OK_OR_RETURN(sync_hook_streams(e, st));            // installs in flight read the old table
    if (e->pool_cum) hipFree(e->pool_cum);
    stage.commit();
    e->pool_cum = cum; e->pool_W = (u32)W;
    return CATAN_OK;
}

int32_t catan_start_pool_outcomes_words(void) { return PO_WORDS; }
int catan_start_pool_outcomes_enable(catan_env_t* e, int on, const int32_t* focus_pid_dev, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_enable: null handle");
    NOT_DEFERRED(e, "catan_start_pool_outcomes_enable");
    NOT_MT(e, "catan_start_pool_outcomes_enable");
    if (!e->pool_on) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_enable: no start pool is installed on this handle (catan_start_pool_set)");
    // off: the arrays stay (installs in flight may still write the origins) until the pool goes
    if (!on) { e->pool_out_on = 0; e->pool_out_focus = nullptr; return CATAN_OK; }
    if (!e->cfg.auto_reset) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_enable: the handle has auto_reset = 0 (no game is re-dealt, so none would be tallied)");
    const hipStream_t st = S(stream);
    const size_t bytes = start_pool_outcome_bytes(e->pool.m);
    i32* origin = e->pool_origin;                      // the arrays of an earlier enable are kept: only what is missing is allocated
    unsigned long long* out = e->pool_out;
    Staged stage;
    if (!origin) stage.alloc(origin, (size_t)e->n * sizeof(i32));
    if (!out) stage.alloc(out, bytes);
    if (!stage.ok()) return stage.enomem("catan_start_pool_outcomes_enable");
    stage.commit();
    e->pool_origin = origin; e->pool_out = out;
    // where the origins were kept by an earlier enable they are stale by now: every game counts as freshly dealt until its next deal
    if (!e->pool_out_on) HIPCHK(hipMemsetAsync(e->pool_origin, 0xFF, (size_t)e->n * sizeof(i32), st));
    HIPCHK(hipMemsetAsync(e->pool_out, 0, bytes, st));
    e->pool_out_focus = focus_pid_dev; e->pool_out_on = 1;
    return CATAN_OK;
}
int catan_start_pool_outcomes_read(catan_env_t* e, uint64_t* out_host, int32_t reset, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_read: null argument");
    if (!e->pool_on) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_read: no start pool is installed on this handle (catan_start_pool_set)");
    if (!e->pool_out_on) return fail(CATAN_EINVAL, "catan_start_pool_outcomes_read: outcomes are not enabled on this handle (catan_start_pool_outcomes_enable)");
    NOT_DEFERRED(e, "catan_start_pool_outcomes_read");          // (the side streams of an open sequence are joined by catan_step_flush)
    return read_counters(out_host, e->pool_out, start_pool_outcome_bytes(e->pool.m), reset, S(stream));
}

// ---- tournament (catan_tourney_enable; the kernels are catan_hooks.hip's).  The tally: at the hook of the league results, in front of the consumer of a re-deal
// list, or (count_p == nullptr) in front of catan_reset's deal over the games with sel[g] != 0 (sel == nullptr: every game).  The seat:
// behind the consumer or that deal, at the sites of the start pool's install; it writes the handle's three per-game arrays and nothing of
// a game.  Off (the default): nothing is launched.
static void enqueue_tourney_tally(catan_env_t* e, const u32* count_p, const i32* list, const u8* sel, hipStream_t st) {
    if (!e->tourney_on) return;
    (void)tourney_launch_tally(e->ctx, e->tourney, count_p, list, sel, st);
}
static void enqueue_tourney_seat(catan_env_t* e, const u32* count_p, const i32* list, const u8* sel, hipStream_t st) {
    if (!e->tourney_on) return;
    (void)tourney_launch_seat(e->ctx, e->tourney, count_p, list, sel, st);
}
static void tourney_free(catan_env_t* e) {
    for (void* p : { (void*)e->tourney.lineups, (void*)e->tourney.lineup_of, (void*)e->tourney.pos_of_pid, (void*)e->tourney.episode, (void*)e->tourney.table })
        if (p) hipFree(p);
    e->tourney = TourneyBuf{};
    e->tourney_on = 0;
}
static size_t tourney_table_bytes(int L) { return ((size_t)L + 1) * TY_WORDS * sizeof(unsigned long long); }
int32_t catan_tourney_words(void) { return TY_WORDS; }
int catan_tourney_enable(catan_env_t* e, const int32_t* lineups_host, int32_t L, int32_t M, int32_t E, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_tourney_enable: null handle");
    if (!e->cfg.auto_reset) return fail(CATAN_EINVAL, "catan_tourney_enable: the handle has auto_reset = 0 (no game is re-dealt, so none would be booked or seated anew)");
    NOT_DEFERRED(e, "catan_tourney_enable");
    NOT_MT(e, "catan_tourney_enable");
    if (L < 1 || L > TOURNEY_MAX_LINEUPS) return fail(CATAN_EINVAL, "catan_tourney_enable: L must be in 1..65536");
    if (M < 1) return fail(CATAN_EINVAL, "catan_tourney_enable: M must be at least 1");
    if (E < 0) return fail(CATAN_EINVAL, "catan_tourney_enable: E must be 0 (unlimited) or positive");
    if (!lineups_host) return fail(CATAN_EINVAL, "catan_tourney_enable: null lineups");
    for (long i = 0; i < 4l * L; i++)
        if (lineups_host[i] < 0 || lineups_host[i] >= M)
            return fail(CATAN_EINVAL, "catan_tourney_enable: lineup " + std::to_string(i / 4) + " names player " + std::to_string(lineups_host[i]) + ", outside 0.." + std::to_string(M - 1));
    const hipStream_t st = S(stream);
    if (e->tourney_on) OK_OR_RETURN(sync_hook_streams(e, st));   // hooks in flight read and write the old arrays
    tourney_free(e);                                             // an earlier tournament is gone whether the new one comes to stand or not
    TourneyBuf tb{};
    tb.L = L; tb.E = (u32)E;
    i32* lineups = nullptr;
    Staged stage;
    stage.alloc(lineups, (size_t)L * 4 * sizeof(i32));
    stage.alloc(tb.lineup_of, (size_t)e->n * sizeof(i32));
    stage.alloc(tb.pos_of_pid, (size_t)e->n * 4 * sizeof(i32));
    stage.alloc(tb.episode, (size_t)e->n * sizeof(u32));
    stage.alloc(tb.table, tourney_table_bytes(L));
    if (!stage.ok()) return stage.enomem("catan_tourney_enable");
    tb.lineups = lineups;
    // every game unseated, no episode opened: the caller's catan_reset seats them
    hipError_t rc = hipMemcpyAsync(lineups, lineups_host, (size_t)L * 4 * sizeof(i32), hipMemcpyHostToDevice, st);
    if (rc == hipSuccess) rc = hipMemsetAsync(tb.lineup_of, 0xFF, (size_t)e->n * sizeof(i32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(tb.pos_of_pid, 0xFF, (size_t)e->n * 4 * sizeof(i32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(tb.episode, 0, (size_t)e->n * sizeof(u32), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(tb.table, 0, tourney_table_bytes(L), st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);         // (the lineups are the caller's host memory)
    if (rc != hipSuccess) return fail(CATAN_EHIP, std::string("catan_tourney_enable: ") + hipGetErrorString(rc));
    stage.commit();
    e->tourney = tb;
    e->tourney_on = 1;
    return CATAN_OK;
}
int catan_tourney_disable(catan_env_t* e, catan_stream_t stream) {
    if (!e) return fail(CATAN_EINVAL, "catan_tourney_disable: null handle");
    NOT_DEFERRED(e, "catan_tourney_disable");
    if (!e->tourney_on) return CATAN_OK;
    OK_OR_RETURN(sync_hook_streams(e, S(stream)));
    tourney_free(e);
    return CATAN_OK;
}
int catan_tourney_read(catan_env_t* e, uint64_t* out_host, int32_t reset, catan_stream_t stream) {
    if (!e || !out_host) return fail(CATAN_EINVAL, "catan_tourney_read: null argument");
    if (!e->tourney_on) return fail(CATAN_EINVAL, "catan_tourney_read: no tournament is enabled on this handle (catan_tourney_enable)");
    NOT_DEFERRED(e, "catan_tourney_read");             // (the side streams of an open sequence are joined by catan_step_flush)
    return read_counters(out_host, e->tourney.table, tourney_table_bytes(e->tourney.L), reset, S(stream));
}
int catan_tourney_seating(catan_env_t* e, int32_t** lineup_of_dev, int32_t** pos_of_pid_dev) {
    if (!e || !lineup_of_dev || !pos_of_pid_dev) return fail(CATAN_EINVAL, "catan_tourney_seating: null argument");
    if (!e->tourney_on) return fail(CATAN_EINVAL, "catan_tourney_seating: no tournament is enabled on this handle (catan_tourney_enable)");
    *lineup_of_dev = e->tourney.lineup_of; *pos_of_pid_dev = e->tourney.pos_of_pid;
    return CATAN_OK;
}

// ---- state check (the kernel is catan_hooks.hip's.  No handle: no rule depends on catan_cfg_t)
static_assert(SC_RULES == CATAN_STATE_CHECK_RULES, "include/catan_hip_tuning.h restates the rules of catan_hooks.h");
int32_t catan_state_check_rules(void) { return SC_RULES; }
int catan_state_check(const int32_t* blob, int64_t cnt, uint64_t* viol, uint64_t* n_bad, catan_stream_t stream) {
    if (!blob || !viol || cnt <= 0) return fail(CATAN_EINVAL, "catan_state_check: null blob or viol, or cnt <= 0");
    HIPCHK(state_check_launch(blob, (long)cnt, (u64*)viol, (unsigned long long*)n_bad, S(stream)));
    return CATAN_OK;
}

// what catan_destroy frees of all this (the statistics' blocks are in the handle's `owned`)
static void hooks_free(catan_env_t* e) {
    if (e->lstats) hipFree(e->lstats);
    record_free(e);
    start_pool_free(e);
    tourney_free(e);
}

}  // extern "C"
