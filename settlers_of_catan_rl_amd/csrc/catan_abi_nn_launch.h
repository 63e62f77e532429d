// catan_abi_nn_launch.h - the launch and dispatch templates of the net's kernels, which serve the entry points of catan_abi_nn.h and nothing
// else.  They stand apart from those, in front of the handle, for one reason: head_launch and wgrad_launch_grouped_dispatch instantiate their
// kernels where they are defined, and the order in which a unit first uses its kernel templates is the order of the kernels in its code
// object - these, then the env's (k_league_stats, k_step, .. k_obs_rows), then what the entry points instantiate (profiles/abi_split.txt).
#pragma once

template <class T>
static int attn_dispatch(bool bwd, const void* qkv, const int* lens, const void* dout, void* out, long B, int L, int H, int HD, hipStream_t st) {
    const T* q = (const T*)qkv;
    // bf16: the MFMA kernels (one wave per sequence); fp32 and unaligned buffers: the VALU kernels
    const bool mfma = sizeof(T) == 2 && (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout) & 15) == 0;
    const unsigned nb4 = (unsigned)((B + 3) / 4);
    const unsigned short* q16 = (const unsigned short*)qkv;
    if (L == 19 && H == 4 && HD == 16) {
        unsigned nb = (unsigned)((B + 2) / 3);
        if (mfma && !bwd) hipLaunchKernelGGL((k_attn_mfma_fwd<19, 4, 16>), dim3(nb4), dim3(256), 0, st, q16, lens, (unsigned short*)out, B);
        else if (mfma && lens) hipLaunchKernelGGL((k_attn_mfma_bwd<19, 4, 16, true>), dim3(nb4), dim3(256), 0, st, q16, lens, (const unsigned short*)dout, (unsigned short*)out, B);
        else if (mfma) hipLaunchKernelGGL((k_attn_mfma_bwd<19, 4, 16, false>), dim3(nb4), dim3(256), 0, st, q16, lens, (const unsigned short*)dout, (unsigned short*)out, B);
        else if (!bwd) hipLaunchKernelGGL((k_attn_fwd<T, 19, 4, 16>), dim3(nb), dim3(64), 0, st, q, lens, (T*)out, B);
        else hipLaunchKernelGGL((k_attn_bwd<T, 19, 4, 16>), dim3(nb), dim3(64), 0, st, q, lens, (const T*)dout, (T*)out, B);
    } else if (L == 25 && H == 4 && HD == 4) {
        unsigned nb = (unsigned)((B + 1) / 2);
        if (mfma && !bwd) hipLaunchKernelGGL((k_attn_mfma_fwd<25, 4, 4>), dim3(nb4), dim3(256), 0, st, q16, lens, (unsigned short*)out, B);
        else if (mfma && lens) hipLaunchKernelGGL((k_attn_mfma_bwd<25, 4, 4, true>), dim3(nb4), dim3(256), 0, st, q16, lens, (const unsigned short*)dout, (unsigned short*)out, B);
        else if (mfma) hipLaunchKernelGGL((k_attn_mfma_bwd<25, 4, 4, false>), dim3(nb4), dim3(256), 0, st, q16, lens, (const unsigned short*)dout, (unsigned short*)out, B);
        else if (!bwd) hipLaunchKernelGGL((k_attn_fwd<T, 25, 4, 4>), dim3(nb), dim3(64), 0, st, q, lens, (T*)out, B);
        else hipLaunchKernelGGL((k_attn_bwd<T, 25, 4, 4>), dim3(nb), dim3(64), 0, st, q, lens, (const T*)dout, (T*)out, B);
    } else return fail(CATAN_EINVAL, "catan_attention: unsupported (L, heads, head_dim); built for (19,4,16) and (25,4,4)");
    return launched();
}
template <class T, int D, int GL>
static int ln_launch(bool bwd, const void* x, const float* w, const float* b, const void* dy, void* out, float* dw, float* db,
                     long rows, float eps, int relu, hipStream_t st) {
    const unsigned nb = grid_for(rows, 256 / GL, bwd ? 2048 : 8192);   // bwd ends with 2*D atomics per block: keep the grid moderate
    if (!bwd) hipLaunchKernelGGL((k_ln_fwd<T, D, GL>), dim3(nb), dim3(256), 0, st, (const T*)x, w, b, (T*)out, rows, eps, relu);
    else hipLaunchKernelGGL((k_ln_bwd<T, D, GL>), dim3(nb), dim3(256), 0, st, (const T*)x, w, b, (const T*)dy, (T*)out, dw, db, rows, eps, relu);
    return launched();
}
template <class T, int EPL, int GL>
static int lnw_launch(bool bwd, const void* x, const float* w, const float* b, const void* dy, void* out, float* dw, float* db,
                      long rows, float eps, int relu, hipStream_t st) {
    const unsigned nb = grid_for(rows, 256 / GL, bwd ? 1024 : 8192);   // bwd ends with 2*D atomics per block
    if (!bwd) hipLaunchKernelGGL((k_lnw_fwd<T, EPL, GL>), dim3(nb), dim3(256), 0, st, (const T*)x, w, b, (T*)out, rows, eps, relu);
    else hipLaunchKernelGGL((k_lnw_bwd<T, EPL, GL>), dim3(nb), dim3(256), 0, st, (const T*)x, w, b, (const T*)dy, (T*)out, dw, db, rows, eps, relu);
    return launched();
}
template <class T>
static int ln_dispatch(bool bwd, const void* x, const float* w, const float* b, const void* dy, void* out, float* dw, float* db,
                       long rows, int D, float eps, int relu, hipStream_t st) {
    switch (D) {
    case 16: return ln_launch<T, 16, 16>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    case 25:
        if constexpr (sizeof(T) == 2) {      // bf16, enough rows, 16-byte aligned tensors: a lane per row through LDS (k_lnr_*)
            if (rows >= 4096 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)dy) & 15) == 0) {
                const unsigned nb = grid_for(rows, 256, 2048);
                if (!bwd) hipLaunchKernelGGL((k_lnr_fwd<25>), dim3(nb), dim3(256), 0, st, (const unsigned short*)x, w, b, (unsigned short*)out, rows, eps, relu);
                else hipLaunchKernelGGL((k_lnr_bwd<25>), dim3(nb), dim3(256), 0, st, (const unsigned short*)x, w, b, (const unsigned short*)dy,
                                        (unsigned short*)out, dw, db, rows, eps, relu);
                return launched();
            }
        }
        return ln_launch<T, 25, 32>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    case 32: return ln_launch<T, 32, 32>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    case 64:
        if ((((uintptr_t)x | (uintptr_t)out | (uintptr_t)dy) & 15) == 0) return lnw_launch<T, 8, 8>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
        return ln_launch<T, 64, 64>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    // 128 / 256 wide: 8 elements per lane (16-byte accesses for bf16), 16 / 32 lanes per row - with one wave per row a lane moved 4 or 8
    // bytes per access and the kernels ran at 1.6 TB/s (204 800 x 128: 100 us backward; 16-byte lanes: see profiles/r03_*)
    // (16-byte aligned: catan_layer_norm_fwd / _bwd refuse anything else at these widths)
    case 128: return lnw_launch<T, 8, 16>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    case 256: return lnw_launch<T, 8, 32>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    case 512: return lnw_launch<T, 8, 64>(bwd, x, w, b, dy, out, dw, db, rows, eps, relu, st);
    default: return fail(CATAN_EINVAL, "catan_layer_norm: unsupported width (built for 16, 25, 32, 64, 128, 256, 512)");
    }
}

template <class T>
static int lstm_cell_launch(bool bwd, const void* gx, const void* gh, const float* c_prev, const float* mask, const float* dh, const float* dc,
                            void* o0, float* o1, long n, int L, hipStream_t st) {
    const unsigned nb = grid_for(n * (L / 4), 256, 16384);
    if (!bwd) hipLaunchKernelGGL((k_lstm_cell_fwd<T>), dim3(nb), dim3(256), 0, st, (const T*)gx, (const T*)gh, c_prev, mask, (float*)o0, o1, n, L);
    else hipLaunchKernelGGL((k_lstm_cell_bwd<T>), dim3(nb), dim3(256), 0, st, (const T*)gx, (const T*)gh, c_prev, mask, dh, dc, (T*)o0, o1, n, L);
    return launched();
}

// How the rows of a weight gradient are split over the grid.  Every block ends with one atomic per element of its O x (I + 1)
// accumulator tile, so the grid is a balance between streaming parallelism and atomics (measured on MI355X, tools/bench_wgrad_shapes.py:
// 614 400 x (160 -> 256): 456 us with up to 1 024 blocks, 307 us with 256; 3.4 M x (64 -> 128): 340 / 288 / 395 us with 1 024 / 512 /
// 256; 3.4 M x (64 -> 32): 158 / 184 / 290 us): the wider the tile, the fewer blocks; long inputs take 16 stages per block, short ones 8.
static void wgrad_grid(long R, int I, int O, long& nb, long& per) {
    const long stages = (R + WG_KT - 1) / WG_KT;
    const long tile = (long)((O + 15) / 16 * 16) * ((I + 1 + 15) / 16 * 16);
    const long cap = tile >= 24576 ? 256 : (tile >= 3072 ? 512 : 1024);
    const long spb = R >= 131072 ? 16 : 8;
    nb = stages / spb < 1 ? 1 : (stages / spb < cap ? stages / spb : cap);
    per = (stages + nb - 1) / nb * WG_KT;
    nb = (R + per - 1) / per;
}
// ... and the rows of the tile encoder's one-pass backward kernels (k_ffn_bwd_w, k_qkv_bwd_w): every block ends with up to 20 864
// atomics, so several stages of FW_ROWS rows per block and at most 512 blocks
static void te_bwd_grid(long R, long& nb, long& per) {
    const long stages = (R + FW_ROWS - 1) / FW_ROWS;
    nb = stages / 16 < 1 ? 1 : (stages / 16 < 512 ? stages / 16 : 512);
    per = (stages + nb - 1) / nb * FW_ROWS;
    nb = (R + per - 1) / per;
}
// the column slice [col0, col0 + W) of a layer whose input is `ld` wide (W, col0, ld multiples of 8; W + 1 <= 160): X rows are strided
template <int OTW>
static int wgrad_launch_slice(const void* x, const void* dy, float* dw, float* db, long R, int ld, int col0, int W, int O, hipStream_t st) {
    long nb, per;
    wgrad_grid(R, W, O, nb, per);
    hipLaunchKernelGGL((k_wgrad_tr<OTW, 10>), dim3((unsigned)nb), dim3(256), 0, st, (const unsigned short*)x, (const unsigned short*)dy, dw, db, R, W, O, per,
                       (long)ld, col0);
    return launched();
}
template <int OTW, int IT>
static int wgrad_launch(const void* x, const void* dy, float* dw, float* db, long R, int I, int O, hipStream_t st) {
    long nb, per;
    wgrad_grid(R, I, O, nb, per);
    if ((I & 7) == 0 && (O & 7) == 0)      // 16 B vectors never straddle a row: row-major LDS image + transposing LDS reads
        hipLaunchKernelGGL((k_wgrad_tr<OTW, IT>), dim3((unsigned)nb), dim3(256), 0, st, (const unsigned short*)x, (const unsigned short*)dy, dw, db, R, I, O, per);
    else
        hipLaunchKernelGGL((k_wgrad<OTW, IT>), dim3((unsigned)nb), dim3(256), 0, st, (const unsigned short*)x, (const unsigned short*)dy, dw, db, R, I, O, per);
    return launched();
}
template <int OTW>
static int wgrad_dispatch_it(int it, const void* x, const void* dy, float* dw, float* db, long R, int I, int O, hipStream_t st) {
    if (it <= 2) return wgrad_launch<OTW, 2>(x, dy, dw, db, R, I, O, st);
    if (it <= 5) return wgrad_launch<OTW, 5>(x, dy, dw, db, R, I, O, st);
    if (it <= 10) return wgrad_launch<OTW, 10>(x, dy, dw, db, R, I, O, st);
    return fail(CATAN_EINVAL, "catan_linear_wgrad: in_features + 1 > 160");
}

template <int OTW, int IT>
static int wgrad_launch_grouped(bool tr, const WgBatch& b, long blocks, hipStream_t st) {
    if (tr) hipLaunchKernelGGL((k_wgrad_tr_grouped<OTW, IT>), dim3((unsigned)blocks), dim3(256), 0, st, b);
    else hipLaunchKernelGGL((k_wgrad_grouped<OTW, IT>), dim3((unsigned)blocks), dim3(256), 0, st, b);
    return launched();
}
static int wgrad_launch_grouped_dispatch(bool tr, int otw, int itc, const WgBatch& b, long blocks, hipStream_t st) {
#define CATAN_WG_CASE(A, B) if (otw == A && itc == B) return wgrad_launch_grouped<A, B>(tr, b, blocks, st)
    CATAN_WG_CASE(1, 2); CATAN_WG_CASE(1, 5); CATAN_WG_CASE(1, 10);
    CATAN_WG_CASE(2, 2); CATAN_WG_CASE(2, 5); CATAN_WG_CASE(2, 10);
    CATAN_WG_CASE(3, 2); CATAN_WG_CASE(3, 5); CATAN_WG_CASE(3, 10);
    CATAN_WG_CASE(4, 2); CATAN_WG_CASE(4, 5); CATAN_WG_CASE(4, 10);
#undef CATAN_WG_CASE
    return fail(CATAN_EINVAL, "catan_linear_wgrad_grouped: no kernel for this tile shape");
}

template <int RT, int WAVES, bool STATS>
static int head_launch_cfg(const HeadArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.B + WAVES * RT * 16 - 1) / (WAVES * RT * 16))), block(WAVES * 64);
    switch ((a.K + 15) / 16) {
    case 1: hipLaunchKernelGGL((k_head_fwd<1, RT, WAVES, STATS>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_head_fwd<2, RT, WAVES, STATS>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_head_fwd<3, RT, WAVES, STATS>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_head_fwd<4, RT, WAVES, STATS>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_head_fwd<5, RT, WAVES, STATS>), grid, block, 0, st, a); break;
    }
    return launched();
}
static int head_launch(const HeadArgs& a, hipStream_t st, bool stats = false) {
    if (stats)
        return a.B <= HD_NARROW_MAX_ROWS ? head_launch_cfg<HD_RT_NARROW, HD_WAVES_NARROW, true>(a, st) : head_launch_cfg<HD_RT_WIDE, HD_WAVES_WIDE, true>(a, st);
    return a.B <= HD_NARROW_MAX_ROWS ? head_launch_cfg<HD_RT_NARROW, HD_WAVES_NARROW, false>(a, st) : head_launch_cfg<HD_RT_WIDE, HD_WAVES_WIDE, false>(a, st);
}

template <int KS>
static int linrows_dispatch_nt(int nt, const void* x, const void* w, const void* b, void* y, long R, int K, int N, const void* aux, int mode, hipStream_t st) {
    const unsigned nb = grid_for((R + 15) / 16, 4, 2048);
#define CATAN_LINROWS(NT) hipLaunchKernelGGL((k_linear_rows<KS, NT>), dim3(nb), dim3(256), 0, st, (const unsigned short*)x, \
                                             (const unsigned short*)w, (const unsigned short*)b, (unsigned short*)y, R, K, N, (const unsigned short*)aux, mode)
    if (nt <= 1) CATAN_LINROWS(1);
    else if (nt <= 2) CATAN_LINROWS(2);
    else if (nt <= 4) CATAN_LINROWS(4);
    else if (nt <= 8) CATAN_LINROWS(8);
    else CATAN_LINROWS(12);
#undef CATAN_LINROWS
    return launched();
}

// the wide-row backward with the gradient of a second use of x added in (dx = LayerNorm'(dy) + dres): D = 64 (16-byte aligned rows), 128, 256, 512
template <class T>
static int lnw_res_dispatch(const void* x, const float* w, const float* b, const void* dy, const void* dres, void* dx, float* dw, float* db,
                            long rows, int D, float eps, int relu, hipStream_t st) {
#define CATAN_LNW_RES(EPL, GL) \
        hipLaunchKernelGGL((k_lnw_bwd<T, EPL, GL>), dim3(grid_for(rows, 256 / GL, 1024)), dim3(256), 0, st, (const T*)x, w, b, (const T*)dy, (T*)dx, dw, db, rows, eps, relu, (const T*)dres)
    switch (D) {
    case 64: CATAN_LNW_RES(8, 8); break;
    case 128: CATAN_LNW_RES(8, 16); break;               // (16-byte aligned: catan_layer_norm_bwd_res refuses anything else)
    case 256: CATAN_LNW_RES(8, 32); break;
    case 512: CATAN_LNW_RES(8, 64); break;
    default: return fail(CATAN_EINVAL, "catan_layer_norm_bwd_res: built for the widths 64, 128, 256, 512");
    }
#undef CATAN_LNW_RES
    return launched();
}
