"""GPU: catan_state_fork (include/catan_hip_tuning.h, "search support") against its definition,
catan_state_export -> add the offset to the blob's rng_draws word -> catan_state_import.  Every comparison is between integer
states or between floats produced by the same arithmetic in the same order: exact."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N_SRC, K = 4096, 16


def _setup():
    from settlers_of_catan_rl_amd import spec
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    src = VecCatanEnv(N_SRC, seed=77)
    src.random_rollout(0, 400)                   # long enough that games have ended and been re-dealt
    n = N_SRC * K
    a = VecCatanEnv(n, seed=5, dense_reward=True, auto_reset=False)
    b = VecCatanEnv(n, seed=5, dense_reward=True, auto_reset=False)
    g = torch.Generator().manual_seed(3)
    src_idx = torch.arange(N_SRC).repeat_interleave(K).cuda()
    dst_idx = torch.randperm(n, generator=g).cuda()
    k = torch.arange(n) % K
    off = (k << 22).long()
    off[k == 5] = 0
    off[k == 7] = 0xFFFFFFFF                      # wraps past 2^32 for every game that has drawn at all
    off[k == 9] = 0xFFF00000
    off = off.cuda()
    return spec, src, a, b, src_idx, dst_idx, off


def _by_definition(spec, src, dst, src_idx, dst_idx, off):
    blobs = src.export_state(src_idx)
    w = spec.STATE_OFFSETS["rng_draws"][0]
    d = ((blobs[:, w].long() & 0xFFFFFFFF) + off) & 0xFFFFFFFF
    blobs[:, w] = torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32)
    dst.import_state(blobs, dst_idx)


def test_fork_equals_export_offset_import_and_the_copies_live_the_same_life(hip_lib):
    spec, src, a, b, src_idx, dst_idx, off = _setup()
    before = src.export_state().clone()
    assert int((before[:, spec.STATE_OFFSETS["rng_draws"][0]].long() & 0xFFFFFFFF).min()) > 0
    a.fork_from(src, src_idx, dst_idx, off)
    _by_definition(spec, src, b, src_idx, dst_idx, off)
    assert torch.equal(src.export_state(), before), "the call changed its source"
    ea, eb = a.export_state(), b.export_state()
    if not torch.equal(ea, eb):
        i = int((ea != eb).any(1).nonzero()[0, 0])
        raise AssertionError((i, spec.describe_state_diff(eb[i].cpu().numpy(), ea[i].cpu().numpy())))
    assert torch.equal(ea[dst_idx][:, :-1], before[src_idx][:, :-1])
    assert torch.equal(a.get_action_masks_packed(), b.get_action_masks_packed())
    for x, y in zip(a.get_obs(), b.get_obs()):
        assert torch.equal(x, y)
    # the pre-rolled states hold roads, cities, bought and played dev cards, a longest road and open trades
    f = lambda name: spec.state_field(before, name)
    assert bool((f("edge_owner") > 0).any()) and bool((f("corner_bld") == 2).any())
    assert bool((f("p1_n_hidden") > 0).any()) and bool((f("p2_n_played") > 0).any()) and bool((f("lr_player") > 0).any())
    assert bool((f("must_respond") > 0).any())
    # --- forked games live the same life
    ra, rb = a.enable_reward64(), b.enable_reward64()
    ctrl = a.deciding_player().clone()
    assert torch.equal(ctrl, b.deciding_player())
    a.randomise_uncertainty(ctrl); b.randomise_uncertainty(ctrl)
    assert torch.equal(a.export_state(), b.export_state())
    for step in range(40):
        aa, ab = a.sample_random_actions(step), b.sample_random_actions(step)
        assert torch.equal(aa, ab), step
        r1, d1 = a.step(aa); r1, d1 = r1.clone(), d1.clone()
        r2, d2 = b.step(ab)
        assert torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(ra, rb), step
        assert torch.equal(a.get_action_masks_packed(), b.get_action_masks_packed()), step
    assert torch.equal(a.export_state(), b.export_state())
    assert a.invalid_action_count() == 0 and b.invalid_action_count() == 0


def test_fork_between_handles_with_different_mask_limits_recomputes_the_masks(hip_lib):
    """max_proposed_trades_per_turn enters the packed masks: the destination's limits apply, as after an import (k_masks_of_list,
    with a permuted destination list and several copies per source)"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    src = VecCatanEnv(1024, seed=9)
    src.random_rollout(0, 300)
    a = VecCatanEnv(2048, seed=1, auto_reset=False, max_proposed_trades_per_turn=1, max_actions_per_turn=5)
    b = VecCatanEnv(2048, seed=1, auto_reset=False, max_proposed_trades_per_turn=1, max_actions_per_turn=5)
    src_idx = torch.arange(1024).repeat_interleave(2).cuda()
    dst_idx = torch.randperm(2048, generator=torch.Generator().manual_seed(8)).cuda()
    a.fork_from(src, src_idx, dst_idx)
    b.import_state(src.export_state(src_idx), dst_idx)
    assert torch.equal(a.export_state(), b.export_state())
    assert torch.equal(a.get_action_masks_packed(), b.get_action_masks_packed())
    assert not torch.equal(a.get_action_masks_packed()[dst_idx], src.get_action_masks_packed()[src_idx])


def test_fork_refusals_launch_nothing(hip_lib):
    """Every CATAN_EINVAL case of catan_state_fork returns it, leaves catan_last_error set and changes nothing in the destination
    (export and packed masks before and after).  The "handles on different devices" case needs a second GPU: on a one-GPU machine
    that branch is not exercised."""
    from settlers_of_catan_rl_amd import _lib
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = VecCatanEnv(64, seed=1)
    src.random_rollout(0, 50)
    dst = VecCatanEnv(32, seed=2, dense_reward=True, auto_reset=False)
    idx = torch.arange(64, dtype=torch.int64).cuda()
    P = lambda t: C.c_void_p(t.data_ptr())

    def snapshot(env):
        torch.cuda.synchronize()
        return env.export_state().clone(), env.get_action_masks_packed().clone()

    def unchanged(env, snap):
        now = snapshot(env)
        assert torch.equal(now[0], snap[0]) and torch.equal(now[1], snap[1])

    def refused(rc, word):
        assert rc == -1, rc                                       # CATAN_EINVAL
        assert word in L.catan_last_error().decode(), L.catan_last_error().decode()

    snap = snapshot(dst)
    for call, word in ((lambda: L.catan_state_fork(None, src.h, P(idx), None, None, 8, st), "bad arguments"),
                       (lambda: L.catan_state_fork(dst.h, None, P(idx), None, None, 8, st), "bad arguments"),
                       (lambda: L.catan_state_fork(dst.h, src.h, None, None, None, 8, st), "bad arguments"),
                       (lambda: L.catan_state_fork(dst.h, src.h, P(idx), None, None, 0, st), "bad arguments"),
                       (lambda: L.catan_state_fork(dst.h, src.h, P(idx), None, None, -3, st), "bad arguments"),
                       (lambda: L.catan_state_fork(dst.h, src.h, P(idx), None, None, 33, st), "bad arguments"),     # cnt > n of dst, no dst_idx
                       (lambda: L.catan_state_fork(dst.h, dst.h, P(idx), None, None, 8, st), "same")):
        refused(call(), word)
        unchanged(dst, snap)
    # an open deferred sequence on the source: the destination can be exported, and is what it was
    src.step_deferred(src.sample_random_actions(0), window=4)
    refused(L.catan_state_fork(dst.h, src.h, P(idx), None, None, 8, st), "deferred")
    unchanged(dst, snap)
    src.step_flush()
    # ... and on the destination: while its sequence is open it cannot be exported, so the packed records themselves are compared
    # through a fork of it into a third handle before the sequence opens and after it is flushed without any step taken in between
    dst.step_deferred(dst.sample_random_actions(0), window=4)
    refused(L.catan_state_fork(dst.h, src.h, P(idx), None, None, 8, st), "deferred")
    dst.step_flush()
    twin = VecCatanEnv(32, seed=2, dense_reward=True, auto_reset=False)
    twin.step_deferred(twin.sample_random_actions(0), window=4)
    twin.step_flush()
    unchanged(dst, snapshot(twin))                                # dst is where the same sequence without the refused call ends
    snap = snapshot(dst)
    # a handle under the MT19937 contract on either side
    mt = VecCatanEnv(1, seed=3)
    mt.seed_mt19937(1, 2)
    refused(L.catan_state_fork(dst.h, mt.h, P(idx), None, None, 1, st), "MT19937")
    unchanged(dst, snap)
    mt_snap = snapshot(mt)
    refused(L.catan_state_fork(mt.h, src.h, P(idx), None, None, 1, st), "MT19937")
    unchanged(mt, mt_snap)
    if torch.cuda.device_count() > 1:
        far = VecCatanEnv(8, seed=4, device="cuda:1")
        refused(L.catan_state_fork(dst.h, far.h, P(idx), None, None, 8, st), "different devices")
        unchanged(dst, snap)
    # ids outside either handle copy nothing (the kernel checks them)
    bad = torch.tensor([64, -1, 3], dtype=torch.int64).cuda()
    to = torch.tensor([0, 1, 40], dtype=torch.int64).cuda()
    _lib.check(L.catan_state_fork(dst.h, src.h, P(bad), P(to), None, 3, st))
    unchanged(dst, snap)
