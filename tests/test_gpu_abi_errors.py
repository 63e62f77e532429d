"""GPU: error behaviour of the C ABI (return codes + catan_last_error, no exceptions across the boundary)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_bad_arguments_are_reported_not_crashed(hip_lib):
    from settlers_of_catan_rl_amd import _lib
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    L = _lib.lib()
    env = VecCatanEnv(64, seed=0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(rc):
        assert rc != 0
        return L.catan_last_error().decode()

    assert "null" in err(L.catan_step(env.h, None, None, None, st))
    assert "bad arguments" in err(L.catan_random_rollout_deferred(env.h, 10, 0, st))
    assert "bad arguments" in err(L.catan_random_rollout(env.h, 0, -1, st))
    h = C.c_void_p()
    assert "bad arguments" in err(L.catan_create(C.byref(h), 0, 0, 0, 0, None))
    assert "bad device" in err(L.catan_create(C.byref(h), 99, 8, 0, 0, None))
    x = torch.zeros((128, 16), device="cuda", dtype=torch.bfloat16)
    dw = torch.zeros((300, 16), device="cuda")
    assert not L.catan_linear_wgrad_supported(128, 16, 300) and not L.catan_linear_wgrad_supported(128, 203, 16) and not L.catan_linear_wgrad_supported(128, 2048, 16)
    assert L.catan_linear_wgrad_supported(128, 200, 16)                      # (a wide input that is a multiple of 8: column slices)
    assert "unsupported" in err(L.catan_linear_wgrad(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(dw.data_ptr()), None, 128, 16, 300, st))
    q = torch.zeros((4, 7, 3, 2, 8), device="cuda")
    assert "unsupported" in err(L.catan_attention_fwd(C.c_void_p(q.data_ptr()), None, C.c_void_p(q.data_ptr()), 4, 7, 2, 8, 0, st))
    assert "unsupported" in err(L.catan_layer_norm_fwd(C.c_void_p(q.data_ptr()), C.c_void_p(q.data_ptr()), C.c_void_p(q.data_ptr()),
                                                       C.c_void_p(q.data_ptr()), 4, 48, 1e-5, 0, 0, st))
    # wide LayerNorm rows take 16-byte accesses: a misaligned x, y / dx or dy is refused at D >= 128 (no kernel is launched), taken below
    f32 = torch.zeros((8 * 512 + 4,), device="cuda")
    b16w = torch.zeros((8 * 512 + 8,), device="cuda", dtype=torch.bfloat16)
    for buf, isb in ((f32, 0), (b16w, 1)):
        ok, off = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + buf.element_size())
        for D in (128, 256, 512):
            assert "16-byte" in err(L.catan_layer_norm_fwd(off, ok, ok, ok, 4, D, 1e-5, 0, isb, st))
            assert "16-byte" in err(L.catan_layer_norm_fwd(ok, ok, ok, off, 4, D, 1e-5, 0, isb, st))
            assert "16-byte" in err(L.catan_layer_norm_bwd(off, ok, ok, ok, ok, ok, ok, 4, D, 1e-5, 0, isb, st))
            assert "16-byte" in err(L.catan_layer_norm_bwd(ok, ok, ok, off, ok, ok, ok, 4, D, 1e-5, 0, isb, st))
            assert "16-byte" in err(L.catan_layer_norm_bwd(ok, ok, ok, ok, off, ok, ok, 4, D, 1e-5, 0, isb, st))
    torch.cuda.synchronize()
    assert bool((f32 == 0).all()) and bool((b16w == 0).all())
    # round 3's learner / collector entry points: misaligned, odd-sized or missing buffers are refused, nothing is launched
    P = lambda t: C.c_void_p(t.data_ptr())
    b16 = torch.zeros((64, 512), device="cuda", dtype=torch.bfloat16)
    idx = torch.zeros((8,), device="cuda", dtype=torch.int64)
    assert "even" in err(L.catan_gather_rows(P(b16), 1024, P(idx), 8, P(b16), 1024, 7, st))
    assert "16-byte" in err(L.catan_expand_rows(P(b16), P(idx), 8, P(b16), 1000, st))
    assert "16-byte" in err(L.catan_segment_sum_rows(C.c_void_p(b16.data_ptr() + 2), 1024, P(idx), P(idx), 4, P(b16), 1024, st))
    srcs2 = (C.c_void_p * 2)(b16.data_ptr(), b16.data_ptr() + 2); rb2 = (C.c_int64 * 2)(1024, 1024)
    assert "16-byte" in err(L.catan_concat_rows(C.cast(srcs2, C.c_void_p), C.cast(rb2, C.c_void_p), 2, P(b16), 2048, 8, st))
    assert "1..4 sources" in err(L.catan_concat_rows(C.cast(srcs2, C.c_void_p), C.cast(rb2, C.c_void_p), 5, P(b16), 2048, 8, st))
    rng3 = (C.c_int64 * 3)(0, 9, 0)
    assert "16 ranges" in err(L.catan_scatter_rows_ranges(P(b16), 1024, P(idx), 8, C.cast(rng3, C.c_void_p), 17, None, None, P(b16), 1024, st))
    assert "outside the permutation" in err(L.catan_scatter_rows_ranges(P(b16), 1024, P(idx), 8, C.cast(rng3, C.c_void_p), 1, None, None, P(b16), 1024, st))
    rng6 = (C.c_int64 * 6)(0, 4, 0, 2, 6, 9)          # the second range's rows of dy do not follow the first's
    assert "consecutive" in err(L.catan_scatter_rows_ranges(P(b16), 1024, P(idx), 8, C.cast(rng6, C.c_void_p), 2, None, None, P(b16), 1024, st))
    ffn = lambda h, x: L.catan_ffn_outproj_bwd(P(b16), h, x, P(b16), P(b16), P(dw), P(dw), 1e-5, P(b16), P(dw), P(dw), P(dw), P(dw), P(dw), P(dw),
                                               P(b16), P(b16), P(b16), P(dw), P(dw), 16, st)
    qkv = lambda wt, ln_b: L.catan_qkv_bwd(P(b16), P(b16), P(b16), wt, P(dw), ln_b, 1e-5, P(b16), P(dw), P(dw), P(dw), P(dw), 16, st)
    assert "null or misaligned" in err(ffn(None, P(b16)))
    assert "null or misaligned" in err(ffn(P(b16), C.c_void_p(b16.data_ptr() + 8)))
    assert "null or misaligned" in err(qkv(P(b16), None))
    assert "null or misaligned" in err(qkv(C.c_void_p(b16.data_ptr() + 4), P(dw)))
    assert "bad arguments" in err(L.catan_weight_images(None, 3, st)) and "bad arguments" in err(L.catan_weight_images(P(b16), 0, st))
    saves = (C.c_void_p * 18)(*([b16.data_ptr()] * 16 + [0, b16.data_ptr()]))    # xfin missing (p, the last, is optional)
    assert "save buffer" in err(L.catan_tile_encoder_fwd_train(P(b16), P(b16), P(dw), P(b16), 475, C.cast(saves, C.c_void_p), 4, st))
    assert "bad arguments" in err(L.catan_tile_encoder_fwd_train(P(b16), P(b16), P(dw), P(b16), 400, C.cast(saves, C.c_void_p), 4, st))
    assert "bad arguments" in err(L.catan_collector_pre(64, 0, P(idx), P(idx), P(idx), P(idx), st))
    assert "null" in err(L.catan_collector_post(64, 4, *([None] * 23)))
    # round 4: the deferred step, the game-list views, the grouped weight gradients
    u8 = torch.zeros((64,), device="cuda", dtype=torch.uint8)
    assert "bad arguments" in err(L.catan_step_deferred(env.h, None, 4, P(dw), P(u8), P(u8), st))
    assert "bad arguments" in err(L.catan_step_deferred(env.h, P(idx), 0, P(dw), P(u8), P(u8), st))
    assert "null" in err(L.catan_step_flush(env.h, None, P(u8), P(u8), st))
    assert "bad" in err(L.catan_masks_of(env.h, P(dw), None, 4, st))
    assert "bad game list" in err(L.catan_obs_rows_of(env.h, 0, P(dw), None, None, None, None, None, None, None, None, 4, st))
    assert "bad arguments" in err(L.catan_linear_wgrad_grouped(None, 3, st))
    assert "bad arguments" in err(L.catan_head_chain(P(b16), 1536, P(b16), P(dw), 1e-5, 12, 0, P(dw), P(dw), P(dw), None, None, None, None, P(idx), P(dw), 64, st))
    # the card-list backward: n_unkeyed (the early return) needs only_unkeyed (the skip list it counts)
    i8 = torch.zeros((64, 25), device="cuda", dtype=torch.int8)
    i32 = torch.zeros((64,), device="cuda", dtype=torch.int32)
    assert "bad arguments" in err(L.catan_card_summary_bwd(P(i8), 1, 25, P(i32), P(dw), 1e-5, P(dw), P(dw), None, P(i32), 64, st))
    with pytest.raises(_lib.CatanHipError):
        _lib.check(L.catan_random_rollout_deferred(env.h, 10, -3, st))
    # the handle is still usable after the failed calls
    env.random_rollout_deferred(40, 8)
    assert env.invalid_action_count() == 0


def test_same_caller_on_libcatan_hip_and_libcatan_cpu(hip_lib):
    """One caller (tests/cpu_abi_driver.py) drives the env entry points of include/catan_hip.h through ctypes - create, sampled
    actions with illegal ones and a no-op mixed in, step, deciding seat, masks, observations, state export / import - once on
    libcatan_hip.so with device buffers and once on oracle/libcatan_cpu.so (the same ABI over the CPU oracle) with host buffers:
    every buffer the calls fill is identical, step by step (rewards, done flags, deciding seats, masks) and at the end
    (observations, card lists, exported states, the rejected-action count, the masks after importing the states)."""
    import numpy as np
    import cpu_abi_driver as drv
    from settlers_of_catan_rl_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    tdt = {np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}
    for dense in (False, True):
        n, seed, steps = 256, 9, 900
        dev = drv.drive(_lib.lib(), n, seed, steps, lambda s, d: torch.zeros(s, dtype=tdt[d], device="cuda"),
                        lambda b: (torch.cuda.synchronize(), b.cpu().numpy())[1], stream=st, dense=dense)
        cpu = drv.drive(drv.cpu_lib(), n, seed, steps, lambda s, d: drv.HostBuf(s, d), lambda b: b.a, dense=dense)
        assert dev["invalid"] == cpu["invalid"] > 0
        for k in ("rew", "done", "seat", "masks_crc", "obs", "lists", "lens", "blob", "masks_after_import"):
            assert np.array_equal(dev[k], cpu[k]), (dense, k)
        assert dev["done"].sum() > 0
