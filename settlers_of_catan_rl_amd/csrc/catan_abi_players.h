// catan_abi_players.h - the entry points of the players that read the games themselves, the last host file of
// catan_abi.hip: they call the env's entry points.  Host code only, but for k_sample_scripted (catan_scripted.hip, catan_abi.hip's code
// object): every other kernel is catan_players.hip's, the library's second translation unit and code object (catan_players.h).
#pragma once

extern "C" {

// What every call over rows of games checks first; `whose`: whose games the rows are, as the message says it
static int check_row_call(const char* what, const catan_env_t* e, const int32_t* games, int64_t n_rows, const int32_t* actions, const char* whose = "handle's") {
    const std::string w(what);
    if (!e) return fail(CATAN_EINVAL, w + ": null handle");
    if (!actions) return fail(CATAN_EINVAL, w + ": null actions");
    if (n_rows <= 0) return fail(CATAN_EINVAL, w + ": n_rows <= 0");
    if (!games && n_rows > e->n) return fail(CATAN_EINVAL, w + ": n_rows exceeds the " + whose + " games (games == NULL)");
    return CATAN_OK;
}
// A block of device counters owned by the handle, allocated and zeroed at its first use.  Zeroed synchronously (once per handle): in place before
// a call on ANY stream can count into it
static int counter_block(catan_env_t* e, const char* what, unsigned long long*& block, size_t words) {
    if (block) return CATAN_OK;
    hipError_t rc = hipSuccess;
    dev_alloc(e, rc, block, words * sizeof(unsigned long long));
    if (rc != hipSuccess) return fail(CATAN_ENOMEM, std::string(what) + ": hipMalloc: " + hipGetErrorString(rc));
    HIPCHK(hipMemset(block, 0, words * sizeof(unsigned long long)));
    HIPCHK(hipStreamSynchronize(nullptr));
    return CATAN_OK;
}
static const u8* busy_of(const catan_env_t* e) { return e->d_it > 0 ? (const u8*)e->pend.busy : (const u8*)nullptr; }

// the rule-based player, style 0: the builder (catan_scripted.hip)
int catan_sample_scripted_actions(catan_env_t* e, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream) {
    OK_OR_RETURN(check_row_call("catan_sample_scripted_actions", e, games, n_rows, actions));
    OK_OR_RETURN(counter_block(e, "catan_sample_scripted_actions", e->script_fallback, 1));
    hipLaunchKernelGGL(k_sample_scripted, dim3(blocks(n_rows, SCRIPT_BLOCK)), dim3(SCRIPT_BLOCK), 0, S(stream), e->ctx, (const u32*)e->mpk, games, (long)n_rows,
                       busy_of(e), actions, e->script_fallback);
    return launched();
}
int64_t catan_scripted_fallback_count(catan_env_t* e, catan_stream_t stream) {
    if (!e) return -1;
    if (!e->script_fallback) return 0;
    unsigned long long v = 0;
    if (hipMemcpyAsync(&v, e->script_fallback, sizeof v, hipMemcpyDeviceToHost, S(stream)) != hipSuccess) return -1;
    if (hipStreamSynchronize(S(stream)) != hipSuccess) return -1;
    return (int64_t)v;
}

// its styles: style 0 is the call above, style 1 the trader
int catan_sample_scripted_actions_style(catan_env_t* e, int32_t style, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream) {
    if (style == CATAN_SCRIPTED_BUILDER) return catan_sample_scripted_actions(e, games, n_rows, actions, stream);
    if (style != CATAN_SCRIPTED_TRADER) return fail(CATAN_EINVAL, "catan_sample_scripted_actions_style: unknown style (0 builder, 1 trader)");
    OK_OR_RETURN(check_row_call("catan_sample_scripted_actions_style", e, games, n_rows, actions));
    OK_OR_RETURN(counter_block(e, "catan_sample_scripted_actions_style", e->trade_counts, TC_WORDS));
    HIPCHK(trader_launch_sample(e->ctx.R, e->ctx.n, (const u32*)e->mpk, games, (long)n_rows, busy_of(e), actions, e->trade_counts, S(stream)));
    return CATAN_OK;
}
int catan_scripted_trade_counts(catan_env_t* e, uint64_t out[8], int32_t reset, catan_stream_t stream) {
    static_assert(TC_WORDS == 8, "catan_scripted_trade_counts: the block is 8 words (include/catan_hip_tuning.h)");
    if (!e || !out) return fail(CATAN_EINVAL, "catan_scripted_trade_counts: null argument");
    if (!e->trade_counts) {                                 // no trader call yet: nothing was counted
        for (int k = 0; k < TC_WORDS; k++) out[k] = 0;
        return CATAN_OK;
    }
    return read_counters(out, e->trade_counts, TC_WORDS * sizeof(unsigned long long), reset, S(stream));
}

// kickstarting from a player: its rows made teacher-forceable, stored beside the net's, and the imitation term
int catan_complete_action_rows(catan_env_t* e, const int32_t* games, int64_t n_rows, int32_t* actions, catan_stream_t stream) {
    OK_OR_RETURN(check_row_call("catan_complete_action_rows", e, games, n_rows, actions));
    HIPCHK(teacher_launch_complete(e->ctx.R, e->ctx.n, (const u32*)e->mpk, games, (long)n_rows, busy_of(e), actions, S(stream)));
    return CATAN_OK;
}
int catan_collector_label(int64_t n, int32_t T, const int64_t* counters4, const uint8_t* flags4, const int64_t* active_pid, const int32_t* deciding,
                          const int32_t* labels, int16_t* st_teacher, const uint8_t* waiting_before, catan_stream_t stream) {
    if (n <= 0 || T <= 0 || !counters4 || !flags4 || !active_pid || !deciding || !labels || !st_teacher)
        return fail(CATAN_EINVAL, "catan_collector_label: null argument");
    HIPCHK(teacher_launch_label((long)n, (int)T, (const long long*)counters4 + 2 * n, flags4 + 2 * n, (const long long*)active_pid, deciding, waiting_before, labels,
                                (short*)st_teacher, S(stream)));
    return CATAN_OK;
}
int64_t catan_imitation_loss_words(void) { return IMIT_WORDS; }
int64_t catan_imitation_loss_workspace_doubles(void) { return IMIT_PART * IMIT_BLOCKS + 1; }
int catan_imitation_loss(const float* lp, const int64_t* teacher, int64_t B, float* loss, float* dlp, double* block, double* workspace, catan_stream_t stream) {
    if (B < 1) return fail(CATAN_EINVAL, "catan_imitation_loss: B must be at least 1");
    if (!lp || !teacher) return fail(CATAN_EINVAL, "catan_imitation_loss: a NULL input array");
    if (!loss || !dlp) return fail(CATAN_EINVAL, "catan_imitation_loss: a NULL output array");
    if (!block || !workspace) return fail(CATAN_EINVAL, "catan_imitation_loss: a NULL block or workspace");
    HIPCHK(teacher_launch_imitation(lp, (const long long*)teacher, (long)B, loss, dlp, block, workspace, S(stream)));
    return CATAN_OK;
}

// the playout player: the order of the launches.  The games are forked, sampled, re-dealt and stepped by the entry points above.
// The workspace of a sim handle of n games, carved from one device allocation (8-byte arrays first, then the 72-byte rows, words, bytes)
static PlayoutWs playout_carve(void* mem, size_t n) {
    PlayoutWs w;
    char* p = (char*)mem;
    const size_t rows = n * ACTION_WORDS * sizeof(i32);
    w.src_idx = (long long*)p; p += n * sizeof(long long);
    w.by_builder = (i32*)p; p += rows;
    w.by_trader = (i32*)p; p += rows;
    w.by_random = (i32*)p; p += rows;
    w.act = (i32*)p; p += rows;
    w.cand = (i32*)p; p += rows;
    w.draw_off = (u32*)p; p += n * sizeof(u32);
    w.slot0 = (i32*)p; p += n * sizeof(i32);
    w.ctrl = (i32*)p; p += n * sizeof(i32);
    w.steps = (i32*)p; p += n * sizeof(i32);
    w.rpid = (i32*)p; p += n * sizeof(i32);
    w.held = (u8*)p; p += n;
    w.dup = (u8*)p;
    return w;
}
constexpr size_t PLAYOUT_WS_BYTES_PER_GAME = sizeof(long long) + 5 * ACTION_WORDS * sizeof(i32) + 5 * sizeof(u32) + 2;

int catan_playout_actions(catan_env_t* root, catan_env_t* sim, const int32_t* games, int64_t n_rows, const catan_playout_cfg_t* cfg, int32_t* actions,
                          int32_t* chosen, int64_t* stats, catan_stream_t stream) {
    static_assert(PS_WORDS == CATAN_PLAYOUT_STAT_WORDS, "catan_playout_actions: the stats row (include/catan_hip_tuning.h)");
    if (!root || !sim) return fail(CATAN_EINVAL, "catan_playout_actions: null handle");
    if (!cfg) return fail(CATAN_EINVAL, "catan_playout_actions: null cfg");
    if (!actions) return fail(CATAN_EINVAL, "catan_playout_actions: null actions");
    if (root == sim) return fail(CATAN_EINVAL, "catan_playout_actions: root and sim are the same handle (the playouts overwrite the sim handle's games)");
    if (root->device != sim->device) return fail(CATAN_EINVAL, "catan_playout_actions: the handles live on different devices");
    if (sim->cfg.auto_reset) return fail(CATAN_EINVAL, "catan_playout_actions: the sim handle has auto_reset = 1 (a finished playout must keep its final state)");
    const Limits lr = limits_of(root), ls = limits_of(sim);
    if (lr.max_trades != ls.max_trades || lr.max_actions != ls.max_actions)
        return fail(CATAN_EINVAL, "catan_playout_actions: max_proposed_trades_per_turn / max_actions_per_turn of the sim handle differ from the root's");
    if ((cfg->builder != 0 && cfg->builder != 1) || (cfg->trader != 0 && cfg->trader != 1) || cfg->randoms < 0 || cfg->randoms > PLAYOUT_MAX_CANDIDATES)
        return fail(CATAN_EINVAL, "catan_playout_actions: builder and trader are 0 or 1, randoms 0..8");
    const int Cn = cfg->builder + cfg->trader + cfg->randoms, K = cfg->playouts;
    if (Cn < 1 || Cn > PLAYOUT_MAX_CANDIDATES) return fail(CATAN_EINVAL, "catan_playout_actions: builder + trader + randoms must be in 1..8");
    if (K < 1 || K > PLAYOUT_MAX_PLAYOUTS) return fail(CATAN_EINVAL, "catan_playout_actions: playouts must be in 1..64");
    if (cfg->depth < 1) return fail(CATAN_EINVAL, "catan_playout_actions: depth must be at least 1");
    if (cfg->playout_style != CATAN_SCRIPTED_BUILDER && cfg->playout_style != CATAN_SCRIPTED_TRADER)
        return fail(CATAN_EINVAL, "catan_playout_actions: unknown playout_style (0 builder, 1 trader)");
    // (the two checks above it found root and actions set: what it still tests are the rows, where this call has always tested them)
    OK_OR_RETURN(check_row_call("catan_playout_actions", root, games, n_rows, actions, "root handle's"));
    if (n_rows > sim->n / ((int64_t)Cn * K)) return fail(CATAN_EINVAL, "catan_playout_actions: n_rows * candidates * playouts exceeds the sim handle's games");
    NOT_MT(root, "catan_playout_actions");
    NOT_MT(sim, "catan_playout_actions");
    NOT_DEFERRED(root, "catan_playout_actions");
    NOT_DEFERRED(sim, "catan_playout_actions");
    if (!sim->playout_mem) {
        hipError_t rc = hipSuccess;
        dev_alloc(sim, rc, sim->playout_mem, (size_t)sim->n * PLAYOUT_WS_BYTES_PER_GAME);
        if (rc != hipSuccess) { sim->playout_mem = nullptr; return fail(CATAN_ENOMEM, std::string("catan_playout_actions: hipMalloc: ") + hipGetErrorString(rc)); }
    }
    const PlayoutWs ws = playout_carve(sim->playout_mem, (size_t)sim->n);
    PlayoutShape sh;
    sh.rows = (long)n_rows; sh.used = (long)n_rows * Cn * K; sh.sim_n = sim->n; sh.C = Cn; sh.K = K;
    sh.n_builder = cfg->builder; sh.n_trader = cfg->trader; sh.determinise = cfg->determinise != 0;
    const hipStream_t st = S(stream);
    const long cand_rows = (long)n_rows * Cn;
    // 1. the fork: slot s = a copy of its row's root game, its draw counter moved on by (1 + k) << 22
    HIPCHK(playout_launch_slots(sh, games, (long)root->n, ws, st));
    OK_OR_RETURN(catan_state_fork(sim, root, (const int64_t*)ws.src_idx, nullptr, ws.draw_off, sh.used, stream));
    // 2. the candidates, sampled on the sim handle in the slots (j, c, 0): builder, trader, random
    if (cfg->builder) OK_OR_RETURN(catan_sample_scripted_actions_style(sim, CATAN_SCRIPTED_BUILDER, ws.slot0, cand_rows, ws.by_builder, stream));
    if (cfg->trader) OK_OR_RETURN(catan_sample_scripted_actions_style(sim, CATAN_SCRIPTED_TRADER, ws.slot0, cand_rows, ws.by_trader, stream));
    if (cfg->randoms) OK_OR_RETURN(catan_sample_random_actions(sim, cfg->step_idx, ws.by_random, stream));
    // 3 - 5. candidate rows, duplicates, first actions; the re-deal of what the deciding player cannot see; the candidates' own step
    HIPCHK(playout_launch_expand(sh, sim->ctx.R, ws, st));
    if (sh.determinise) OK_OR_RETURN(catan_randomise_uncertainty(sim, ws.ctrl, stream));
    OK_OR_RETURN(catan_step(sim, ws.act, sim->scratch_reward, sim->scratch_done, stream));
    // 6. the playouts: the rule-based player in every seat, finished / duplicate / bad slots frozen
    for (int d = 1; d < cfg->depth; d++) {
        OK_OR_RETURN(catan_sample_scripted_actions_style(sim, cfg->playout_style, nullptr, sh.used, ws.act, stream));
        HIPCHK(playout_launch_hold(sh, sim->scratch_done, ws, st));
        OK_OR_RETURN(catan_step(sim, ws.act, sim->scratch_reward, sim->scratch_done, stream));
    }
    // 7. the scores and the pick
    HIPCHK(playout_launch_score(sh, sim->ctx.R, ws, actions, chosen, (long long*)stats, st));
    return CATAN_OK;
}

}  // extern "C"
