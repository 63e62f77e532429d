// catan_abi_nn.h - the learner's stateless entry points (include/catan_hip_nn.h; none takes a catan_env_t), a section per kernel file.  They
// launch through the templates of catan_abi_nn_launch.h, and stand behind the env's code for the reason given there; for the same reason
// catan_nn.hip has two sections: k_recurrent_given of catan_rows.hip is first used between the weight gradients and the row-split linear.
#pragma once

extern "C" {

// ---- catan_ppo.hip
int64_t catan_gae_workspace_doubles(int64_t N) { return 2 * ((N + GAE_BLOCK - 1) / GAE_BLOCK) + 4; }

int catan_gae(const float* rewards, const float* values, const float* masks, int64_t T, int64_t N, double gamma, double lam,
              float* returns, float* adv_raw, double* workspace, double* stats3, catan_stream_t stream) {
    if (!rewards || !values || !masks || !returns || !adv_raw || !workspace || !stats3 || T <= 0 || N <= 0)
        return fail(CATAN_EINVAL, "catan_gae: bad arguments");
    const int nb = (int)((N + GAE_BLOCK - 1) / GAE_BLOCK);
    // python-scalar semantics of the reference: gamma and gamma*lambda are doubles, cast to fp32 where they meet a tensor
    const float gl = (float)(gamma * lam);
    hipLaunchKernelGGL(k_gae, dim3(nb), dim3(GAE_BLOCK), 0, S(stream), rewards, values, masks, (long)T, (long)N, (float)gamma, gl, returns, adv_raw, workspace);
    hipLaunchKernelGGL(k_adv_stats, dim3(1), dim3(GAE_BLOCK), 0, S(stream), (const double*)workspace, nb, (double)T * (double)N, stats3);
    return launched();
}

int catan_adv_normalise(float* adv, int64_t total, const double* stats3, catan_stream_t stream) {
    if (!adv || !stats3 || total <= 0) return fail(CATAN_EINVAL, "catan_adv_normalise: bad arguments");
    hipLaunchKernelGGL(k_adv_normalise, dim3(grid_for(total, GAE_BLOCK, 4096)), dim3(GAE_BLOCK), 0, S(stream), adv, (long)total, stats3);
    return launched();
}

int64_t catan_ppo_loss_workspace_doubles(void) { return 2 * PPO_BLOCKS + 1; }

int catan_ppo_loss(const float* logp, const float* old_logp, const float* adv, const float* values, const float* old_values,
                   const float* returns, int64_t B, float clip, float value_coef, int use_norm, float norm_mean, float norm_std,
                   float* losses2, float* d_logp, float* d_values, double* workspace, catan_stream_t stream) {
    if (!logp || !old_logp || !adv || !values || !old_values || !returns || !losses2 || !d_logp || !d_values || !workspace || B <= 0)
        return fail(CATAN_EINVAL, "catan_ppo_loss: bad arguments");
    PpoArgs a{ clip, value_coef, norm_mean, norm_std, use_norm };
    hipLaunchKernelGGL(k_ppo_loss, dim3(grid_for(B, PPO_THREADS * 4, PPO_BLOCKS)), dim3(PPO_THREADS), 0, S(stream), logp, old_logp, adv, values, old_values, returns, (long)B, a, losses2, d_logp,
                       d_values, workspace);
    return launched();
}

int64_t catan_ppo_diag_words(void) { return PPO_DIAG_WORDS; }
int64_t catan_ppo_diag_workspace_doubles(void) { return PPO_DIAG_PART * PPO_BLOCKS + 1; }

int catan_ppo_diag(const float* logp, const float* old_logp, const float* adv, const float* values, const float* old_values,
                   const float* returns, int64_t B, float clip, int use_norm, float norm_mean, float norm_std, const float* entropy,
                   const float* grad_norm, float max_grad_norm, double* block, double* workspace, catan_stream_t stream) {
    if (B < 1) return fail(CATAN_EINVAL, "catan_ppo_diag: B must be at least 1");
    if (!logp || !old_logp || !adv || !values || !old_values || !returns) return fail(CATAN_EINVAL, "catan_ppo_diag: a NULL input array");
    if (!block || !workspace) return fail(CATAN_EINVAL, "catan_ppo_diag: a NULL block or workspace");
    PpoDiagArgs a{ clip, norm_mean, norm_std, max_grad_norm, use_norm };
    hipLaunchKernelGGL(k_ppo_diag, dim3(grid_for(B, PPO_THREADS, PPO_BLOCKS)), dim3(PPO_THREADS), 0, S(stream), logp, old_logp, adv, values, old_values, returns, (long)B, a,
                       entropy, grad_norm, block, workspace);
    return launched();
}

// ---- catan_collector.hip
int catan_collector_pre(int64_t n, int32_t T, const int64_t* n_obs, const int64_t* actions, int32_t* a_env, uint8_t* live, catan_stream_t stream) {
    if (n <= 0 || T <= 0 || !n_obs || !actions || !a_env || !live) return fail(CATAN_EINVAL, "catan_collector_pre: bad arguments");
    CollectorArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.T = T; a.n_obs = (long long*)n_obs; a.actions = (const long long*)actions; a.a_env = a_env; a.live = live;
    hipLaunchKernelGGL(k_collector_pre, dim3(blocks(n, 256)), dim3(256), 0, S(stream), a);
    return launched();
}
int catan_collector_post(int64_t n, int32_t T, int64_t* counters4, double* racc, uint8_t* flags4, float* term, int64_t* t_obs, const int64_t* active_pid,
                         const int32_t* deciding, const int32_t* n_deciding, const int64_t* actions, const float* logp, const int32_t* pmasks,
                         const float* reward, const double* reward64, const uint8_t* done, int64_t* st_actions, float* st_logp, int32_t* st_amasks,
                         float* st_rewards, float* st_masks, int64_t* n_complete, const uint8_t* waiting_before, const uint8_t* status, catan_stream_t stream) {
    if (n <= 0 || T <= 0 || !counters4 || !racc || !flags4 || !term || !t_obs || !active_pid || !deciding || !n_deciding || !actions || !logp || !pmasks ||
        !reward || !done || !st_actions || !st_logp || !st_amasks || !st_rewards || !st_masks || !n_complete)
        return fail(CATAN_EINVAL, "catan_collector_post: null argument");
    CollectorArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.T = T;
    a.n_obs = (long long*)counters4; a.n_msk = a.n_obs + n; a.n_act = a.n_obs + 2 * n; a.n_rew = a.n_obs + 3 * n;
    a.racc = racc; a.done_since = flags4; a.pending_obs = flags4 + n; a.live = flags4 + 2 * n; a.sel = flags4 + 3 * n;
    a.term = term; a.t_obs = (long long*)t_obs; a.active_pid = (const long long*)active_pid;
    a.deciding = deciding; a.n_deciding = n_deciding; a.actions = (const long long*)actions; a.logp = logp; a.pmasks = pmasks;
    a.reward = reward; a.reward64 = reward64; a.done = done;
    a.st_actions = (long long*)st_actions; a.st_logp = st_logp; a.st_amasks = st_amasks; a.st_rewards = st_rewards; a.st_masks = st_masks;
    a.n_complete = (long long*)n_complete;
    if ((waiting_before == nullptr) != (status == nullptr)) return fail(CATAN_EINVAL, "catan_collector_post: waiting_before and status come together");
    a.waiting_before = waiting_before; a.status = status;
    hipLaunchKernelGGL(k_collector_post, dim3(blocks(n, 256)), dim3(256), 0, S(stream), a);
    return launched();
}

// ---- catan_nn.hip: attention, LayerNorm, weight gradients
int catan_attention_fwd(const void* qkv, const int32_t* lens, void* out, int64_t B, int L, int H, int HD, int is_bf16, catan_stream_t stream) {
    if (!qkv || !out || B <= 0) return fail(CATAN_EINVAL, "catan_attention_fwd: bad arguments");
    return BY_DTYPE(is_bf16, attn_dispatch, false, qkv, lens, nullptr, out, B, L, H, HD, S(stream));
}
int catan_attention_bwd(const void* qkv, const int32_t* lens, const void* dout, void* dqkv, int64_t B, int L, int H, int HD, int is_bf16, catan_stream_t stream) {
    if (!qkv || !dout || !dqkv || B <= 0) return fail(CATAN_EINVAL, "catan_attention_bwd: bad arguments");
    return BY_DTYPE(is_bf16, attn_dispatch, true, qkv, lens, dout, dqkv, B, L, H, HD, S(stream));
}

int catan_layer_norm_fwd(const void* x, const float* w, const float* b, void* y, int64_t rows, int D, float eps, int relu, int is_bf16, catan_stream_t stream) {
    if (!x || !w || !b || !y || rows <= 0) return fail(CATAN_EINVAL, "catan_layer_norm_fwd: bad arguments");
    if (D >= 128 && (((uintptr_t)x | (uintptr_t)y) & 15)) return fail(CATAN_EINVAL, "catan_layer_norm_fwd: x and y must be 16-byte aligned for D >= 128");
    return BY_DTYPE(is_bf16, ln_dispatch, false, x, w, b, nullptr, y, nullptr, nullptr, rows, D, eps, relu, S(stream));
}
int catan_layer_norm_bwd_res(const void* x, const float* w, const float* b, const void* dy, const void* dres, void* dx, float* dw, float* db,
                             int64_t rows, int D, float eps, int relu, int is_bf16, catan_stream_t stream) {
    if (!x || !w || !b || !dy || !dres || !dx || !dw || !db || rows <= 0) return fail(CATAN_EINVAL, "catan_layer_norm_bwd_res: bad arguments");
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dres | (uintptr_t)dx) & 15) return fail(CATAN_EINVAL, "catan_layer_norm_bwd_res: buffers must be 16-byte aligned");
    return BY_DTYPE(is_bf16, lnw_res_dispatch, x, w, b, dy, dres, dx, dw, db, rows, D, eps, relu, S(stream));
}
int catan_layer_norm_bwd(const void* x, const float* w, const float* b, const void* dy, void* dx, float* dw, float* db, int64_t rows, int D,
                         float eps, int relu, int is_bf16, catan_stream_t stream) {
    if (!x || !w || !b || !dy || !dx || !dw || !db || rows <= 0) return fail(CATAN_EINVAL, "catan_layer_norm_bwd: bad arguments");
    if (D >= 128 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15)) return fail(CATAN_EINVAL, "catan_layer_norm_bwd: x, dy and dx must be 16-byte aligned for D >= 128");
    return BY_DTYPE(is_bf16, ln_dispatch, true, x, w, b, dy, dx, dw, db, rows, D, eps, relu, S(stream));
}
static bool wgrad_sliced(int in_features, int out_features) {      // wide inputs: column slices of <= 128 (k_wgrad_tr on strided rows)
    return in_features + 1 > 160 && in_features <= 1024 && (in_features & 7) == 0 && (out_features & 7) == 0 && out_features <= 256;
}
int catan_linear_wgrad_supported(int64_t rows, int in_features, int out_features) {
    if (rows >= 1 && wgrad_sliced(in_features, out_features)) return 1;
    return rows >= 1 && in_features >= 1 && out_features >= 1 && in_features + 1 <= 160 && out_features <= 256;
}

int catan_linear_wgrad(const void* x, const void* dy, float* dw, float* db, int64_t rows, int in_features, int out_features,
                       catan_stream_t stream) {
    if (!x || !dy || !dw || !catan_linear_wgrad_supported(rows, in_features, out_features))
        return fail(CATAN_EINVAL, "catan_linear_wgrad: bad arguments / unsupported widths (in + 1 <= 160 or in a multiple of 8 up to 1024; out <= 256)");
    if (((uintptr_t)x | (uintptr_t)dy) & 15) return fail(CATAN_EINVAL, "catan_linear_wgrad: x and dy must be 16-byte aligned");
    if (wgrad_sliced(in_features, out_features)) {
        const int otw = ((out_features + 15) / 16 + 3) / 4;
        for (int c0 = 0; c0 < in_features; c0 += 128) {
            const int W = in_features - c0 < 128 ? in_features - c0 : 128;
            float* b = c0 == 0 ? db : nullptr;                // the bias gradient comes with the first slice
            int r;
            switch (otw) {
            case 1: r = wgrad_launch_slice<1>(x, dy, dw, b, rows, in_features, c0, W, out_features, S(stream)); break;
            case 2: r = wgrad_launch_slice<2>(x, dy, dw, b, rows, in_features, c0, W, out_features, S(stream)); break;
            case 3: r = wgrad_launch_slice<3>(x, dy, dw, b, rows, in_features, c0, W, out_features, S(stream)); break;
            default: r = wgrad_launch_slice<4>(x, dy, dw, b, rows, in_features, c0, W, out_features, S(stream)); break;
            }
            if (r != CATAN_OK) return r;
        }
        return CATAN_OK;
    }
    const int it = (in_features + 1 + 15) / 16, otw = ((out_features + 15) / 16 + 3) / 4;
    switch (otw) {
    case 1: return wgrad_dispatch_it<1>(it, x, dy, dw, db, rows, in_features, out_features, S(stream));
    case 2: return wgrad_dispatch_it<2>(it, x, dy, dw, db, rows, in_features, out_features, S(stream));
    case 3: return wgrad_dispatch_it<3>(it, x, dy, dw, db, rows, in_features, out_features, S(stream));
    default: return wgrad_dispatch_it<4>(it, x, dy, dw, db, rows, in_features, out_features, S(stream));
    }
}

// catan_linear_wgrad for a list of problems (host array) with as few launches as their tile shapes allow: units of the same
// (output tile, input tile) template share launches of up to WG_MAX_UNITS units; a problem the transposing-read kernel does not take
// (widths that are not multiples of 8) is launched on its own as before.
int catan_linear_wgrad_grouped(const catan_wgrad_problem_t* problems, int32_t n, catan_stream_t stream) {
    if (!problems || n <= 0) return fail(CATAN_EINVAL, "catan_linear_wgrad_grouped: bad arguments");
    struct Unit { WgUnit u; int otw, itc; bool tr; long nb; };
    std::vector<Unit> units;
    for (int p = 0; p < n; p++) {
        const catan_wgrad_problem_t& q = problems[p];
        if (!q.x || !q.dy || !q.dw || !catan_linear_wgrad_supported(q.rows, q.in_features, q.out_features))
            return fail(CATAN_EINVAL, "catan_linear_wgrad_grouped: bad problem / unsupported widths");
        if (((uintptr_t)q.x | (uintptr_t)q.dy) & 15) return fail(CATAN_EINVAL, "catan_linear_wgrad_grouped: x and dy must be 16-byte aligned");
        const int I = q.in_features, O = q.out_features;
        if (q.dw_ld < 0 || q.dw_col0 < 0 || (q.dw_ld != 0 && q.dw_col0 + I > q.dw_ld) || (q.dw_ld == 0 && q.dw_col0 != 0))
            return fail(CATAN_EINVAL, "catan_linear_wgrad_grouped: bad dw window (a column offset needs the leading dimension of dw)");
        const long ldw = q.dw_ld ? q.dw_ld : I;
        const int otw = ((O + 15) / 16 + 3) / 4;
        Unit t; long per;
        t.otw = otw;
        if (wgrad_sliced(I, O)) {
            for (int c0 = 0; c0 < I; c0 += 128) {
                const int W = I - c0 < 128 ? I - c0 : 128;
                wgrad_grid(q.rows, W, O, t.nb, per);
                t.u = WgUnit{ (const unsigned short*)q.x, (const unsigned short*)q.dy, q.dw, c0 == 0 ? q.db : nullptr, (long)q.rows, per, (long)I, ldw, W, O, c0, q.dw_col0 + c0, 0, 0 };
                t.itc = 10; t.tr = true;
                units.push_back(t);
            }
            continue;
        }
        const int it = (I + 1 + 15) / 16;
        wgrad_grid(q.rows, I, O, t.nb, per);
        t.u = WgUnit{ (const unsigned short*)q.x, (const unsigned short*)q.dy, q.dw, q.db, (long)q.rows, per, 0L, ldw, I, O, 0, q.dw_col0, 0, 0 };
        t.itc = it <= 2 ? 2 : (it <= 5 ? 5 : 10);
        t.tr = (I & 7) == 0 && (O & 7) == 0;               // 16 B vectors never straddle a row: the transposing-read kernel
        units.push_back(t);
    }
    std::vector<char> done(units.size(), 0);
    for (size_t a = 0; a < units.size(); a++) {
        if (done[a]) continue;
        WgBatch b; b.n = 0; long blocks = 0;
        for (size_t c = a; c < units.size(); c++) {
            if (done[c] || units[c].otw != units[a].otw || units[c].itc != units[a].itc || units[c].tr != units[a].tr) continue;
            if (b.n == WG_MAX_UNITS) break;
            b.u[b.n] = units[c].u; b.u[b.n].block0 = (int)blocks; blocks += units[c].nb; b.n++; done[c] = 1;
        }
        int r = wgrad_launch_grouped_dispatch(units[a].tr, units[a].otw, units[a].itc, b, blocks, S(stream));
        if (r != CATAN_OK) return r;
    }
    return CATAN_OK;
}

// ---- catan_wgrad_big.hip
int64_t catan_wgrad_big_workspace_floats(int64_t rows, int in_features, int out_features) {
    if (rows <= 0 || in_features <= 0 || out_features <= 0) return 0;
    const int tiles_i = (in_features + 1 + WB_T - 1) / WB_T;
    const int groups = 8 * (rows >= 8 * 2 * 4096 ? 2 : 1);
    return (int64_t)groups * out_features * tiles_i * WB_T;
}
int catan_linear_wgrad_big(const void* x, const void* dy, float* dw, int64_t dw_ld, float* db, float* workspace, int64_t rows, int in_features,
                           int out_features, int accumulate, catan_stream_t stream) {
    if (!x || !dy || !dw || !workspace || rows <= 0 || in_features < 8 || (in_features & 7) || out_features < WB_T || (out_features % WB_T) || dw_ld < in_features ||
        (((uintptr_t)x | (uintptr_t)dy) & 15))
        return fail(CATAN_EINVAL, "catan_linear_wgrad_big: bad arguments (in a multiple of 8, out a multiple of 128, 16-byte aligned operands)");
    const int tiles_o = out_features / WB_T, tiles_i = (in_features + 1 + WB_T - 1) / WB_T;
    const int groups = 8 * (rows >= 8 * 2 * 4096 ? 2 : 1);                 // row groups: one per XCD, two when every group still has >= 4 096 rows
    long per = (rows + groups - 1) / groups;
    per = (per + WG_KT - 1) / WG_KT * WG_KT;
    const long nblocks = (long)groups * tiles_o * tiles_i;
    hipLaunchKernelGGL(k_wgrad_big, dim3((unsigned)nblocks), dim3(256), 0, S(stream), (const unsigned short*)x, (const unsigned short*)dy, workspace, (long)rows,
                       in_features, out_features, per, tiles_o, tiles_i);
    const long n = (long)out_features * (in_features + 1);
    hipLaunchKernelGGL(k_wgrad_big_reduce, dim3(blocks(n, 256)), dim3(256), 0, S(stream), (const float*)workspace, groups, out_features, in_features, tiles_i * WB_T,
                       dw, (long)dw_ld, db, accumulate);
    return launched();
}

// ---- catan_optim.hip
int32_t catan_adam_chunk_elements(void) { return OPT_CHUNK; }
int catan_adam_step(const void* tensors, const void* chunks, int32_t n_chunks, const void* grads, int32_t n_tensors, int32_t none_is_zero, void* partial,
                    float max_norm, float lr, float beta1, float beta2, float eps, float* norm_out, catan_stream_t stream) {
    static_assert(sizeof(AdamTensor) == sizeof(catan_adam_tensor_t) && sizeof(AdamChunk) == sizeof(catan_adam_chunk_t), "the header's structs are the kernels'");
    if (!tensors || !chunks || !grads || !partial || n_chunks <= 0 || n_tensors <= 0)
        return fail(CATAN_EINVAL, "catan_adam_step: bad arguments");
    AdamHyper h = { max_norm, lr, beta1, beta2, eps, max_norm > 0.f ? 1 : 0, none_is_zero ? 1 : 0, (int)n_tensors };
    hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)n_chunks), dim3(OPT_BLOCK), 0, S(stream), (const AdamChunk*)chunks, (const float* const*)grads, (double*)partial);
    hipLaunchKernelGGL(k_adam_step, dim3((unsigned)n_chunks), dim3(OPT_BLOCK), 0, S(stream), (const AdamTensor*)tensors, (const AdamChunk*)chunks, (int)n_chunks,
                       (const float* const*)grads, (const double*)partial, h, norm_out);
    return launched();
}

// ---- catan_rows.hip
int catan_gather_rows(const void* src, int64_t src_pitch_bytes, const int64_t* idx, int64_t n, void* dst, int64_t dst_pitch_bytes, int64_t row_bytes,
                      catan_stream_t stream) {
    if (!src || !idx || !dst || n <= 0 || row_bytes <= 0 || (row_bytes & 1) || row_bytes > (1 << 30) || (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)src_pitch_bytes | (uintptr_t)dst_pitch_bytes) & 1))
        return fail(CATAN_EINVAL, "catan_gather_rows: rows are an even number of bytes at even addresses");
    const unsigned nb = grid_for(n, 1, 16384);
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)nb), dim3(256), 0, S(stream), (const unsigned char*)src, (long)src_pitch_bytes, (const long long*)idx, (long)n,
                       (unsigned char*)dst, (long)dst_pitch_bytes, (int)row_bytes);
    return launched();
}
int catan_expand_rows(const void* src, const int64_t* inv, int64_t n, void* out, int64_t row_bytes, catan_stream_t stream) {
    if (!src || !inv || !out || n <= 0 || row_bytes <= 0 || (row_bytes & 15) || (((uintptr_t)src | (uintptr_t)out) & 15))
        return fail(CATAN_EINVAL, "catan_expand_rows: rows are whole 16-byte pieces at 16-byte aligned addresses");
    const int chunks = (int)(row_bytes / 16);
    const unsigned nb = grid_for(n * chunks, 256, 65536);
    hipLaunchKernelGGL(k_expand_rows16, dim3((unsigned)nb), dim3(256), 0, S(stream), (const uint4*)src, (const long long*)inv, (long)n, (uint4*)out, chunks);
    return launched();
}
int catan_segment_sum_rows(const void* dy, int64_t dy_pitch_bytes, const int64_t* order, const int64_t* start, int64_t segments, void* out, int64_t row_bytes,
                           catan_stream_t stream) {
    if (!dy || !order || !start || !out || segments <= 0 || row_bytes <= 0 || (row_bytes & 15) || (((uintptr_t)dy | (uintptr_t)out | (uintptr_t)dy_pitch_bytes) & 15) ||
        dy_pitch_bytes < row_bytes)
        return fail(CATAN_EINVAL, "catan_segment_sum_rows: rows are whole 16-byte pieces at 16-byte aligned addresses");
    const int chunks = (int)(row_bytes / 16);
    const unsigned nb = grid_for(segments * chunks, 256, 65536);
    hipLaunchKernelGGL(k_segment_sum16, dim3((unsigned)nb), dim3(256), 0, S(stream), (const uint4*)dy, (const long long*)order, (const long long*)start, (long)segments,
                       (uint4*)out, chunks, (long)(dy_pitch_bytes / 16));
    return launched();
}
int catan_concat_rows(const void* const* srcs, const int64_t* row_bytes, int n, void* out, int64_t out_pitch_bytes, int64_t rows, catan_stream_t stream) {
    if (!srcs || !row_bytes || !out || n < 1 || n > CC_MAX || rows <= 0 || (((uintptr_t)out | (uintptr_t)out_pitch_bytes) & 15))
        return fail(CATAN_EINVAL, "catan_concat_rows: 1..4 sources; rows are whole 16-byte pieces at 16-byte aligned addresses");
    ConcatSrc cs;
    cs.n = n;
    int total = 0;
    for (int k = 0; k < CC_MAX; k++) { cs.src[k] = nullptr; cs.chunks[k] = 0; cs.first[k] = 0; }
    for (int k = 0; k < n; k++) {
        if (!srcs[k] || row_bytes[k] <= 0 || (row_bytes[k] & 15) || ((uintptr_t)srcs[k] & 15))
            return fail(CATAN_EINVAL, "catan_concat_rows: 1..4 sources; rows are whole 16-byte pieces at 16-byte aligned addresses");
        cs.src[k] = (const uint4*)srcs[k]; cs.chunks[k] = (int)(row_bytes[k] / 16); cs.first[k] = total; total += cs.chunks[k];
    }
    if ((long)total * 16 > out_pitch_bytes) return fail(CATAN_EINVAL, "catan_concat_rows: the sources' rows exceed the output pitch");
    const unsigned nb = grid_for(rows * total, 256, 65536);
    hipLaunchKernelGGL(k_concat_rows16, dim3((unsigned)nb), dim3(256), 0, S(stream), cs, (uint4*)out, (long)rows, total, (int)(out_pitch_bytes / 16));
    return launched();
}
int catan_recurrent_given(const int64_t* acts, int64_t acts_ld, const float* cur_res, const float* fixed, int32_t kf, int32_t from_hand, int64_t rows, int32_t cond_bf16,
                          void* cond, float* mask, int64_t* given, float* keep, float* out_final, catan_stream_t stream) {
    if (!acts || !cur_res || !cond || !mask || !given || !keep || !out_final || rows <= 0 || acts_ld < 4 || kf < 0 || kf > 32 || (kf > 0 && !fixed))
        return fail(CATAN_EINVAL, "catan_recurrent_given: bad arguments");
    const unsigned nb = (unsigned)((rows + 255) / 256);
    if (cond_bf16) hipLaunchKernelGGL(k_recurrent_given<true>, dim3(nb), dim3(256), 0, S(stream), (const long long*)acts, (long)acts_ld, cur_res, fixed, (int)kf, (int)from_hand, (long)rows,
                                      cond, mask, (long long*)given, keep, out_final);
    else hipLaunchKernelGGL(k_recurrent_given<false>, dim3(nb), dim3(256), 0, S(stream), (const long long*)acts, (long)acts_ld, cur_res, fixed, (int)kf, (int)from_hand, (long)rows,
                            cond, mask, (long long*)given, keep, out_final);
    return launched();
}
int catan_scatter_rows_ranges(const void* dy, int64_t dy_pitch_bytes, const int64_t* perm, int64_t n_perm, const int64_t* ranges, int n_ranges,
                              const void* add0, const void* add1, void* out, int64_t row_bytes, catan_stream_t stream) {
    if (!dy || !perm || !ranges || !out || n_perm <= 0 || n_ranges < 0 || n_ranges > SR_MAX || row_bytes <= 0 || (row_bytes & 15) ||
        (((uintptr_t)dy | (uintptr_t)out | (uintptr_t)dy_pitch_bytes | (uintptr_t)add0 | (uintptr_t)add1) & 15) || dy_pitch_bytes < row_bytes)
        return fail(CATAN_EINVAL, "catan_scatter_rows_ranges: at most 16 ranges; rows are whole 16-byte pieces at 16-byte aligned addresses");
    ScatterRanges rg;
    rg.n = n_ranges;
    for (int k = 0; k < SR_MAX; k++) { rg.a[k] = 0; rg.b[k] = 0; rg.off[k] = 0; }
    for (int k = 0; k < n_ranges; k++) {
        rg.a[k] = ranges[3 * k]; rg.b[k] = ranges[3 * k + 1]; rg.off[k] = ranges[3 * k + 2];
        if (rg.a[k] < 0 || rg.b[k] < rg.a[k] || rg.b[k] > n_perm || rg.off[k] < 0) return fail(CATAN_EINVAL, "catan_scatter_rows_ranges: a range outside the permutation");
        // the ranges' rows of dy follow each other (nn_kernels.gather_ranges lays them out that way): range k starts where range k - 1 ended, so
        // dy holds exactly the sum of the range lengths rows and no offset can point past it
        if (rg.off[k] != (k ? rg.off[k - 1] + (rg.b[k - 1] - rg.a[k - 1]) : 0)) return fail(CATAN_EINVAL, "catan_scatter_rows_ranges: the ranges' rows of dy must be consecutive from row 0");
    }
    const int chunks = (int)(row_bytes / 16);
    const unsigned nb = grid_for(n_perm * chunks, 256, 65536);
    hipLaunchKernelGGL(k_scatter_ranges16, dim3((unsigned)nb), dim3(256), 0, S(stream), (const uint4*)dy, (long)(dy_pitch_bytes / 16), (const long long*)perm, (long)n_perm, rg,
                       (const uint4*)add0, (const uint4*)add1, (uint4*)out, chunks);
    return launched();
}
int32_t catan_weight_image_bytes(void) { return (int32_t)sizeof(WeightImage); }
int catan_weight_images(const void* table, int32_t n, catan_stream_t stream) {
    if (!table || n <= 0) return fail(CATAN_EINVAL, "catan_weight_images: bad arguments");
    static_assert(sizeof(WeightImage) == 64 && sizeof(catan_weight_image_t) == sizeof(WeightImage), "the header's struct is the kernel's");
    hipLaunchKernelGGL(k_weight_images, dim3((unsigned)n, 8), dim3(256), 0, S(stream), (const WeightImage*)table, (int)n);
    return launched();
}

// ---- catan_te_bwd.hip
int catan_ffn_outproj_bwd(const void* dx, const void* h, const void* x, const void* w2t, const void* w1t, const float* ln_w, const float* ln_b, float eps,
                          void* dx_out, float* dw2, float* db2, float* dw1, float* db1, float* dln_w, float* dln_b,
                          const void* o, const void* wot, void* d_o, float* dwo, float* dbo, int64_t rows, catan_stream_t stream) {
    if (!dx || !h || !x || !w2t || !w1t || !ln_w || !ln_b || !dx_out || !dw2 || !db2 || !dw1 || !db1 || !dln_w || !dln_b || !o || !wot || !d_o || !dwo || !dbo || rows <= 0 ||
        (((uintptr_t)dx | (uintptr_t)h | (uintptr_t)x | (uintptr_t)w2t | (uintptr_t)w1t | (uintptr_t)dx_out | (uintptr_t)o | (uintptr_t)wot | (uintptr_t)d_o) & 15))
        return fail(CATAN_EINVAL, "catan_ffn_outproj_bwd: null or misaligned argument");
    long nb, per;
    te_bwd_grid(rows, nb, per);
    FfnOutProj op = { (const unsigned short*)o, (const unsigned short*)wot, (unsigned short*)d_o, dwo, dbo };
    hipLaunchKernelGGL(k_ffn_bwd_w, dim3((unsigned)nb), dim3(256), 0, S(stream), (const unsigned short*)dx, (const unsigned short*)h, (const unsigned short*)x,
                       (const unsigned short*)w2t, (const unsigned short*)w1t, ln_w, ln_b, eps, (unsigned short*)dx_out, dw2, db2, dw1, db1,
                       dln_w, dln_b, (long)rows, per, op);
    return launched();
}
int catan_qkv_bwd(const void* dqkv, const void* x, const void* dres, const void* wt, const float* ln_w, const float* ln_b, float eps, void* dx_out,
                  float* dw, float* db, float* dln_w, float* dln_b, int64_t rows, catan_stream_t stream) {
    if (!dqkv || !x || !dres || !wt || !ln_w || !ln_b || !dx_out || !dw || !db || !dln_w || !dln_b || rows <= 0 ||
        (((uintptr_t)dqkv | (uintptr_t)x | (uintptr_t)dres | (uintptr_t)wt | (uintptr_t)dx_out) & 15))
        return fail(CATAN_EINVAL, "catan_qkv_bwd: null or misaligned argument");
    long nb, per;
    te_bwd_grid(rows, nb, per);
    hipLaunchKernelGGL(k_qkv_bwd_w, dim3((unsigned)nb), dim3(256), 0, S(stream), (const unsigned short*)dqkv, (const unsigned short*)x, (const unsigned short*)dres,
                       (const unsigned short*)nullptr, (const unsigned short*)wt, ln_w, ln_b, eps, (unsigned short*)dx_out, dw, db, dln_w, dln_b, (long)rows, per);
    return launched();
}

// ---- catan_heads.hip
int32_t catan_head_weight_elems(void) { return HD_WELEMS; }
int32_t catan_head_vec_elems(void) { return HD_VELEMS; }
static int head_fwd(const char* fn, const void* pre, int64_t pre_ld, const float* cond, int64_t cond_ld, int32_t ncond, const void* wts, const float* vec,
                    float eps, int32_t K, const float* mask, int64_t mask_ld, const float* u, int64_t* action, float* logp, float* entropy, int64_t B,
                    catan_stream_t stream) {
    if (!pre || !wts || !vec || !mask || !action || !logp || B <= 0 || K < 1 || K > HD_KP || ncond < 0 || ncond > HD_NCP || (ncond > 0 && !cond) ||
        pre_ld % 8 != 0 || ((uintptr_t)pre & 15) != 0)
        return fail(CATAN_EINVAL, std::string(fn) + ": bad arguments (K <= 80, ncond <= 32, pre 16-byte aligned with a row pitch that is a multiple of 8)");
    HeadArgs a;
    a.pre = (const unsigned short*)pre; a.pre_ld = pre_ld; a.cond = cond; a.cond_ld = cond_ld; a.ncond = ncond;
    a.wts = (const unsigned short*)wts; a.vec = vec; a.eps = eps; a.K = K; a.mask = mask; a.mask_ld = mask_ld; a.u = u;
    a.action = (long long*)action; a.logp = logp; a.B = B; a.ent = entropy;
    a.state = nullptr; a.head_id = 0; a.step = 0; a.maskmat = nullptr; a.cur_res = nullptr; a.trade = nullptr; a.custom = nullptr;
    a.forced = nullptr; a.actions = nullptr; a.logp_out = nullptr;
    return head_launch(a, S(stream), entropy != nullptr);
}
int catan_head_fwd(const void* pre, int64_t pre_ld, const float* cond, int64_t cond_ld, int32_t ncond, const void* wts, const float* vec, float eps,
                   int32_t K, const float* mask, int64_t mask_ld, const float* u, int64_t* action, float* logp, int64_t B, catan_stream_t stream) {
    return head_fwd("catan_head_fwd", pre, pre_ld, cond, cond_ld, ncond, wts, vec, eps, K, mask, mask_ld, u, action, logp, nullptr, B, stream);
}
int catan_head_fwd_entropy(const void* pre, int64_t pre_ld, const float* cond, int64_t cond_ld, int32_t ncond, const void* wts, const float* vec, float eps,
                           int32_t K, const float* mask, int64_t mask_ld, const float* u, int64_t* action, float* logp, float* entropy, int64_t B,
                           catan_stream_t stream) {
    if (!entropy) return fail(CATAN_EINVAL, "catan_head_fwd_entropy: bad arguments (entropy is NULL)");
    return head_fwd("catan_head_fwd_entropy", pre, pre_ld, cond, cond_ld, ncond, wts, vec, eps, K, mask, mask_ld, u, action, logp, entropy, B, stream);
}

int32_t catan_head_state_floats(void) { return HD_STATE; }
static int head_chain(const char* fn, const void* pre, int64_t pre_ld, const void* wts, const float* vec, float eps, int32_t head_id, int32_t step,
                      float* state, const float* maskmat, const float* cur_res, const float* trade, const float* custom, const int64_t* forced,
                      const float* u, int64_t* actions, float* logp_out, bool stats, int64_t B, catan_stream_t stream) {
    static const int KS[12] = { 13, 54, 73, 19, 5, 2, 3, 6, 6, 5, 5, 5 }, NC[12] = { 0, 2, 0, 0, 0, 32, 2, 6, 12, 4, 9, 0 };
    if (!pre || !wts || !vec || !state || !maskmat || !cur_res || !actions || !logp_out || B <= 0 || head_id < 0 || head_id > 11 || step < 0 || step > 3 ||
        ((head_id != 7 && head_id != 8) && step != 0) || (head_id == 5 && (!trade || !custom)) || pre_ld % 8 != 0 || ((uintptr_t)pre & 15) != 0 ||
        ((uintptr_t)state & 15) != 0)
        return fail(CATAN_EINVAL, std::string(fn) + ": bad arguments");
    HeadArgs a;
    a.pre = (const unsigned short*)pre; a.pre_ld = pre_ld; a.cond = nullptr; a.cond_ld = 0; a.ncond = NC[head_id];
    a.wts = (const unsigned short*)wts; a.vec = vec; a.eps = eps; a.K = KS[head_id]; a.mask = nullptr; a.mask_ld = 0; a.u = u;
    a.action = nullptr; a.logp = nullptr; a.B = B; a.ent = nullptr;
    a.state = state; a.head_id = head_id; a.step = step; a.maskmat = maskmat; a.cur_res = cur_res; a.trade = trade; a.custom = custom;
    a.forced = (const long long*)forced; a.actions = (long long*)actions; a.logp_out = logp_out;
    return head_launch(a, S(stream), stats);
}
int catan_head_chain(const void* pre, int64_t pre_ld, const void* wts, const float* vec, float eps, int32_t head_id, int32_t step, float* state,
                     const float* maskmat, const float* cur_res, const float* trade, const float* custom, const int64_t* forced, const float* u,
                     int64_t* actions, float* logp_out, int64_t B, catan_stream_t stream) {
    return head_chain("catan_head_chain", pre, pre_ld, wts, vec, eps, head_id, step, state, maskmat, cur_res, trade, custom, forced, u, actions, logp_out,
                      false, B, stream);
}
int catan_head_chain_ex(const void* pre, int64_t pre_ld, const void* wts, const float* vec, float eps, int32_t head_id, int32_t step, float* state,
                        const float* maskmat, const float* cur_res, const float* trade, const float* custom, const int64_t* forced, const float* u,
                        int64_t* actions, float* logp_out, int32_t flags, int64_t B, catan_stream_t stream) {
    if ((flags & ~CATAN_HEAD_STATS) != 0) return fail(CATAN_EINVAL, "catan_head_chain_ex: bad arguments (unknown flags)");
    return head_chain("catan_head_chain_ex", pre, pre_ld, wts, vec, eps, head_id, step, state, maskmat, cur_res, trade, custom, forced, u, actions, logp_out,
                      (flags & CATAN_HEAD_STATS) != 0, B, stream);
}

// ---- catan_nn.hip, its second section: row-split linear, LSTM cell, masked categorical, card-list summary
int catan_linear_rows_supported(int64_t rows, int in_features, int out_features) {
    if (!(rows >= 1 && in_features >= 8 && in_features <= 192 && (in_features & 7) == 0 && out_features >= 1 && out_features <= 192)) return 0;
    const int ks = (in_features + 31) / 32, nt = (out_features + 15) / 16;
    const int ks_i = ks <= 4 ? ks : 6, nt_i = nt <= 1 ? 1 : (nt <= 2 ? 2 : (nt <= 4 ? 4 : (nt <= 8 ? 8 : 12)));   // instantiated sizes
    return ks_i * nt_i <= 32;                                // W fragments (4 VGPRs each) must fit the register file
}

int catan_linear_rows_fused(const void* x, const void* w, const void* bias, void* y, int64_t rows, int in_features, int out_features,
                            const void* aux, int mode, catan_stream_t stream) {
    if (!x || !w || !y || !catan_linear_rows_supported(rows, in_features, out_features))
        return fail(CATAN_EINVAL, "catan_linear_rows: bad arguments / unsupported widths (in multiple of 8 and <= 192, out <= 192, instantiated k-steps (1, 2, 3, 4, 6) x n-tiles (1, 2, 4, 8, 12) <= 32)");
    if (mode < 0 || mode > 3 || (mode >= 2 && !aux) || (mode != 0 && (out_features & 7)))
        return fail(CATAN_EINVAL, "catan_linear_rows_fused: mode 0..3; modes 2, 3 need aux; a fused epilogue needs out_features % 8 == 0");
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)aux) & 15) return fail(CATAN_EINVAL, "catan_linear_rows: x, w, y, aux must be 16-byte aligned");
    const int ks = (in_features + 31) / 32, nt = (out_features + 15) / 16;
    switch (ks) {
    case 1: return linrows_dispatch_nt<1>(nt, x, w, bias, y, rows, in_features, out_features, aux, mode, S(stream));
    case 2: return linrows_dispatch_nt<2>(nt, x, w, bias, y, rows, in_features, out_features, aux, mode, S(stream));
    case 3: return linrows_dispatch_nt<3>(nt, x, w, bias, y, rows, in_features, out_features, aux, mode, S(stream));
    case 4: return linrows_dispatch_nt<4>(nt, x, w, bias, y, rows, in_features, out_features, aux, mode, S(stream));
    default: return linrows_dispatch_nt<6>(nt, x, w, bias, y, rows, in_features, out_features, aux, mode, S(stream));
    }
}

int catan_linear_rows(const void* x, const void* w, const void* bias, void* y, int64_t rows, int in_features, int out_features,
                      catan_stream_t stream) {
    return catan_linear_rows_fused(x, w, bias, y, rows, in_features, out_features, nullptr, 0, stream);
}

int catan_lstm_cell_fwd(const void* gx, const void* gh, const float* c_prev, const float* mask, float* h_out, float* c_out, int64_t rows,
                        int hidden, int is_bf16, catan_stream_t stream) {
    if (!gx || !gh || !c_prev || !h_out || !c_out || rows <= 0 || hidden <= 0 || (hidden & 3))
        return fail(CATAN_EINVAL, "catan_lstm_cell_fwd: bad arguments (hidden must be a multiple of 4)");
    if (((uintptr_t)gx | (uintptr_t)gh | (uintptr_t)c_prev | (uintptr_t)h_out | (uintptr_t)c_out) & 15)
        return fail(CATAN_EINVAL, "catan_lstm_cell_fwd: buffers must be 16-byte aligned");
    return BY_DTYPE(is_bf16, lstm_cell_launch, false, gx, gh, c_prev, mask, nullptr, nullptr, h_out, c_out, rows, hidden, S(stream));
}

int catan_lstm_cell_bwd(const void* gx, const void* gh, const float* c_prev, const float* mask, const float* dh, const float* dc, void* dgates,
                        float* dc_prev, int64_t rows, int hidden, int is_bf16, catan_stream_t stream) {
    if (!gx || !gh || !c_prev || !dh || !dc || !dgates || !dc_prev || rows <= 0 || hidden <= 0 || (hidden & 3))
        return fail(CATAN_EINVAL, "catan_lstm_cell_bwd: bad arguments (hidden must be a multiple of 4)");
    if (((uintptr_t)gx | (uintptr_t)gh | (uintptr_t)c_prev | (uintptr_t)dh | (uintptr_t)dc | (uintptr_t)dgates | (uintptr_t)dc_prev) & 15)
        return fail(CATAN_EINVAL, "catan_lstm_cell_bwd: buffers must be 16-byte aligned");
    return BY_DTYPE(is_bf16, lstm_cell_launch, true, gx, gh, c_prev, mask, dh, dc, dgates, dc_prev, rows, hidden, S(stream));
}

int catan_categorical_fwd(const float* logits, const float* mask, int64_t mask_ld, const int64_t* given, const float* u, int64_t* action,
                          float* logp, float* entropy, float* lse, int64_t rows, int K, catan_stream_t stream) {
    if (!logits || !mask || !action || !logp || !entropy || !lse || rows <= 0 || K <= 0 || mask_ld < K)
        return fail(CATAN_EINVAL, "catan_categorical_fwd: bad arguments");
    hipLaunchKernelGGL(k_categorical_fwd, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), logits, mask, (long)mask_ld,
                       (const long long*)given, u, (long long*)action, logp, entropy, lse, (long)rows, K);
    return launched();
}

int catan_categorical_bwd(const float* logits, const float* mask, int64_t mask_ld, const int64_t* action, const float* lse, const float* entropy,
                          const float* dlogp, const float* dent, float* dlogits, int64_t rows, int K, catan_stream_t stream) {
    if (!logits || !mask || !action || !lse || !entropy || !dlogp || !dent || !dlogits || rows <= 0 || K <= 0 || mask_ld < K)
        return fail(CATAN_EINVAL, "catan_categorical_bwd: bad arguments");
    hipLaunchKernelGGL(k_categorical_bwd, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), logits, mask, (long)mask_ld,
                       (const long long*)action, lse, entropy, dlogp, dent, dlogits, (long)rows, K);
    return launched();
}

static int cat_bits_args(CatBits& mb, const uint32_t* packed, int64_t pitch_words, const int64_t* rows_idx, const int32_t* segs, int64_t rows, int K) {
    if (!packed || !segs || pitch_words < 1 || rows <= 0 || K <= 0) return 1;
    mb.pm = packed; mb.pitch = (long)pitch_words; mb.rows = (const long long*)rows_idx;
    mb.n0 = segs[0]; mb.n1 = segs[1];
    for (int k = 0; k < 3; k++) {
        mb.off[k] = segs[2 + 2 * k]; mb.aoff[k] = segs[3 + 2 * k];
        if (mb.off[k] < 0 || mb.off[k] + K > pitch_words * 32 || mb.aoff[k] + K > pitch_words * 32) return 1;
    }
    return mb.n0 < 0 || mb.n1 < mb.n0;
}
int catan_categorical_bits_fwd(const float* logits, const uint32_t* packed, int64_t pitch_words, const int64_t* rows_idx, const int32_t* segs, const int64_t* given,
                               int64_t given_ld, int64_t* action, float* logp, float* entropy, float* lse, int64_t rows, int K, catan_stream_t stream) {
    CatBits mb;
    if (!logits || !action || !logp || !entropy || !lse || cat_bits_args(mb, packed, pitch_words, rows_idx, segs, rows, K) || (given && given_ld < 1))
        return fail(CATAN_EINVAL, "catan_categorical_bits_fwd: bad arguments (segs: n0, n1, then (bit offset, AND offset or -1) x 3, inside the packed row)");
    hipLaunchKernelGGL(k_categorical_bits_fwd, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), logits, mb, (const long long*)given, (long)given_ld,
                       (long long*)action, logp, entropy, lse, (long)rows, K);
    return launched();
}
int catan_categorical_bits_bwd(const float* logits, const uint32_t* packed, int64_t pitch_words, const int64_t* rows_idx, const int32_t* segs, const int64_t* action,
                               const float* lse, const float* entropy, const float* dlogp, const float* dent, float* dlogits, int64_t rows, int K, catan_stream_t stream) {
    CatBits mb;
    if (!logits || !action || !lse || !entropy || !dlogp || !dent || !dlogits || cat_bits_args(mb, packed, pitch_words, rows_idx, segs, rows, K))
        return fail(CATAN_EINVAL, "catan_categorical_bits_bwd: bad arguments");
    hipLaunchKernelGGL(k_categorical_bits_bwd, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), logits, mb, (const long long*)action, lse, entropy, dlogp, dent,
                       dlogits, (long)rows, K);
    return launched();
}

int32_t catan_card_summary_params(void) { return CS_NPAR; }

static int card_summary_check(const void* ids, int esz, int64_t pitch, const int32_t* lens, const float* params, int64_t rows) {
    if (!ids || !lens || !params || rows <= 0 || pitch < 1 || (esz != 1 && esz != 4 && esz != 8)) return fail(CATAN_EINVAL, "catan_card_summary: bad arguments");
    return CATAN_OK;
}
int catan_card_summary_fwd(const void* ids, int id_bytes, int64_t pitch, const int32_t* lens, const float* params, float eps, float* out,
                           int32_t* keys, int64_t rows, catan_stream_t stream) {
    if (card_summary_check(ids, id_bytes, pitch, lens, params, rows) || !out) return fail(CATAN_EINVAL, "catan_card_summary_fwd: bad arguments");
    hipLaunchKernelGGL(k_card_summary_fwd, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), ids, id_bytes, (long)pitch, lens, params, eps, out, (long)rows, keys);
    return launched();
}
int catan_card_summary_lookup(const void* ids, int id_bytes, int64_t pitch, const int32_t* lens, const float* table, const float* params, float eps,
                              float* out, int64_t rows, catan_stream_t stream) {
    if (card_summary_check(ids, id_bytes, pitch, lens, params, rows) || !out || !table) return fail(CATAN_EINVAL, "catan_card_summary_lookup: bad arguments");
    hipLaunchKernelGGL(k_card_summary_lookup, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S(stream), ids, id_bytes, (long)pitch, lens, table, params, eps, out, (long)rows);
    return launched();
}
int catan_card_summary_bwd(const void* ids, int id_bytes, int64_t pitch, const int32_t* lens, const float* params, float eps, const float* dout,
                           float* dparams, const int32_t* only_unkeyed, const int32_t* n_unkeyed, int64_t rows, catan_stream_t stream) {
    if (card_summary_check(ids, id_bytes, pitch, lens, params, rows) || !dout || !dparams || (n_unkeyed && !only_unkeyed))
        return fail(CATAN_EINVAL, "catan_card_summary_bwd: bad arguments");
    const int rpl = rows >= 65536 ? 4 : 1;                 // lists per lane: few rows (the pattern table) want all the lanes they can get
    const int nb = (int)((rows + 256 * rpl - 1) / (256 * rpl));
    const int row_blocks = rows < 65536 ? nb : 0;          // ... and one query class per workgroup (CS_V x nb workgroups per slice)
    const dim3 grid((unsigned)(row_blocks > 0 ? CS_V * nb : nb), 7);
    hipLaunchKernelGGL(k_card_summary_bwd, grid, dim3(256), 0, S(stream), ids, id_bytes, (long)pitch, lens, params, eps, dout, dparams, (long)rows, only_unkeyed, rpl, n_unkeyed,
                       row_blocks);
    return launched();
}
int32_t catan_card_summary_patterns(void) { return CS_PATTERNS; }
int catan_card_pattern_sum(const int32_t* keys, const float* dout, float* dpat, int replicas, int32_t* n_unkeyed, int64_t rows, catan_stream_t stream) {
    if (!keys || !dout || !dpat || rows <= 0 || replicas < 1) return fail(CATAN_EINVAL, "catan_card_pattern_sum: bad arguments");
    hipLaunchKernelGGL(k_card_pattern_sum, dim3((unsigned)((rows + CPS_ROWS - 1) / CPS_ROWS)), dim3(256), 0, S(stream), keys, dout, dpat, (long)rows, replicas, n_unkeyed);
    return launched();
}

// ---- catan_tile_encoder.hip
int32_t catan_tile_encoder_weight_elems(void) { return TE_WTOTAL; }
int32_t catan_tile_encoder_vec_elems(void) { return TE_VTOTAL; }
int catan_tile_encoder_fwd(const void* tiles, const void* weights, const float* vecs, void* out, int64_t boards, catan_stream_t stream) {
    if (!tiles || !weights || !vecs || !out || boards <= 0) return fail(CATAN_EINVAL, "catan_tile_encoder_fwd: bad arguments");
    long nb = (boards + TE_G - 1) / TE_G;
    TeSaves sv;
    memset(&sv, 0, sizeof sv);
    hipLaunchKernelGGL(k_tile_encoder_fwd<0>, dim3((unsigned)nb), dim3(TE_THREADS), 0, S(stream), (const unsigned short*)tiles, (const unsigned short*)weights, vecs,
                       (unsigned short*)out, (long)boards, sv, (long)(TE_L * TE_OUT));
    return launched();
}
int catan_tile_encoder_fwd_train(const void* tiles, const void* weights, const float* vecs, void* out, int64_t out_pitch, const catan_te_saves_t* saves,
                                 int64_t boards, catan_stream_t stream) {
    if (!tiles || !weights || !vecs || !out || !saves || boards <= 0 || out_pitch < TE_L * TE_OUT) return fail(CATAN_EINVAL, "catan_tile_encoder_fwd_train: bad arguments");
    static_assert(sizeof(catan_te_saves_t) == sizeof(TeSaves), "the header's struct is the kernel's");
    const void* const* ptrs = reinterpret_cast<const void* const*>(saves);
    for (size_t i = 0; i < sizeof(TeSaves) / sizeof(void*); i++) {
        const bool optional = (i >= offsetof(TeSaves, n1) / sizeof(void*) && i < offsetof(TeSaves, n1) / sizeof(void*) + 2) ||
                              (i >= offsetof(TeSaves, n2) / sizeof(void*) && i < offsetof(TeSaves, n2) / sizeof(void*) + 2) ||
                              (i >= offsetof(TeSaves, h) / sizeof(void*) && i < offsetof(TeSaves, h) / sizeof(void*) + 2);
        if ((!ptrs[i] && !optional) || ((uintptr_t)ptrs[i] & 15))
            return fail(CATAN_EINVAL, "catan_tile_encoder_fwd_train: every save buffer but n1 / n2 / h must be set, all 16-byte aligned");
    }
    TeSaves sv;
    memcpy(&sv, saves, sizeof sv);
    long nb = (boards + TE_G - 1) / TE_G;
    hipLaunchKernelGGL(k_tile_encoder_fwd<1>, dim3((unsigned)nb), dim3(TE_THREADS), 0, S(stream), (const unsigned short*)tiles, (const unsigned short*)weights, vecs,
                       (unsigned short*)out, (long)boards, sv, (long)out_pitch);
    return launched();
}

}  // extern "C"
