"""GPU: the PPO update diagnostics (k_ppo_diag, csrc/catan_ppo.hip) - the kernel's twenty words against the numpy helper
(tests/ppo_diag_reference.py), accumulation into caller-owned blocks, the ABI's argument checks, the trainer's read-out on the device,
and that turning the read-out on leaves the update what it was."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_diag_reference as R

pytestmark = pytest.mark.gpu

ENT, GN, MAXGN = 1.25, 0.625, 0.5
_REFS = {}


def _case(B, seed, clip, norm):
    """inputs and the reference of one call (computed once, shared, never written to)"""
    key = (B, seed, clip, norm)
    if key not in _REFS:
        x = R.build_inputs(B, seed, clip, norm)
        a = (x["logp"], x["old_logp"], x["adv"], x["v"], x["vp"], x["ret"])
        _REFS[key] = (x, R.reference_words(*a, clip, norm), R.reference_words(*a, clip, norm, entropy=ENT, grad_norm=GN, max_grad_norm=MAXGN))
    return _REFS[key]


def _launch(L, x, clip, norm, block, ws, scalars):
    dev = {k: torch.from_numpy(x[k]).cuda() for k in ("logp", "old_logp", "adv", "v", "vp", "ret")}
    ent = torch.tensor([ENT], dtype=torch.float32, device="cuda") if scalars else None
    gn = torch.tensor([GN], dtype=torch.float32, device="cuda") if scalars else None
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    use, mean, std = (0, 0.0, 1.0) if norm is None else (1, norm[0], norm[1])
    rc = L.catan_ppo_diag(P(dev["logp"]), P(dev["old_logp"]), P(dev["adv"]), P(dev["v"]), P(dev["vp"]), P(dev["ret"]), x["logp"].size, clip, use, mean, std,
                          P(ent), P(gn), MAXGN, P(block), P(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.catan_last_error()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws.view(torch.int64))) == 0, "the workspace (partials and arrival counter) is all zero after every call"


def _workspace(L):
    assert L.catan_ppo_diag_words() == R.WORDS == 20
    return torch.zeros(L.catan_ppo_diag_workspace_doubles(), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("B,seed", R.CASES)
def test_kernel_against_the_helper(hip_lib, B, seed):
    """B = 1: one workgroup; 257: a partial second one; 65 537: all 256 populated and one wrap of the grid stride; 200 003: odd, near
    config 3's minibatch.  Integer words and the maxima exactly, the sums within 1e-10 * sum|term| (ppo_diag_reference.assert_words)."""
    L, ws = hip_lib, _workspace(hip_lib)
    for clip, norm in R.SETTINGS:
        x, plain, with_scalars = _case(B, seed, clip, norm)
        block = torch.zeros(20, dtype=torch.float64, device="cuda")
        _launch(L, x, clip, norm, block, ws, scalars=True)
        R.assert_words(block.cpu().numpy(), *with_scalars)
        # NULL scalars: words 16..19 keep their bits, whatever they hold
        block = torch.zeros(20, dtype=torch.float64, device="cuda")
        block[16:] = torch.tensor([1.5, -2.25, 3.0, 1e-300], dtype=torch.float64)
        before = block[16:].clone()
        _launch(L, x, clip, norm, block, ws, scalars=False)
        assert torch.equal(block[16:].view(torch.int64), before.view(torch.int64))
        R.assert_words(block.cpu().numpy(), *plain, untouched=R.SCALAR_WORDS)


def test_accumulation_into_caller_owned_blocks(hip_lib):
    L, ws = hip_lib, _workspace(hip_lib)
    calls = [(257, 12, 0.2, None, True), (65537, 13, 0.2, None, False), (257, 12, 0.1, (150.0, 150.0), True)]
    blocks = torch.zeros((3, 20), dtype=torch.float64, device="cuda")
    blocks[1] = 7.0                                                      # a neighbour's block
    for target in (0, 2):                                                # the same sequence into two zeroed blocks
        for B, seed, clip, norm, scalars in calls:
            _launch(L, _case(B, seed, clip, norm)[0], clip, norm, blocks[target], ws, scalars)
    ref = R.combine([_case(B, seed, clip, norm)[2 if scalars else 1] for B, seed, clip, norm, scalars in calls])
    R.assert_words(blocks[0].cpu().numpy(), *ref)
    assert blocks[0, 1] == 3 and blocks[0, 0] == 257 + 65537 + 257
    assert torch.equal(blocks[0], blocks[2]), "a given sequence of calls gives the same bits"
    assert torch.equal(blocks[1], torch.full((20,), 7.0, dtype=torch.float64, device="cuda"))


def test_through_the_package(hip_lib):
    """ppo.ppo_diag on device tensors runs the kernel (its own workspace per stream), not the torch form"""
    from settlers_of_catan_rl_amd import ppo
    clip, norm = 0.2, (150.0, 150.0)
    x, _, ref = _case(257, 12, clip, norm)
    t = {k: torch.from_numpy(x[k]).cuda() for k in x if k != "replaced"}
    block = torch.zeros(20, dtype=torch.float64, device="cuda")
    ppo.ppo_diag(block, t["logp"], t["v"].view(-1, 1), t["old_logp"], t["adv"], t["vp"], t["ret"], clip, norm,
                 entropy=torch.tensor(ENT, device="cuda"), grad_norm=torch.tensor([GN], device="cuda"), max_grad_norm=MAXGN)
    R.assert_words(block.cpu().numpy(), *ref)
    assert int(torch.count_nonzero(ppo._diag_workspace(block.device))) == 0
    with pytest.raises(ValueError):
        ppo.ppo_diag(torch.zeros(20, dtype=torch.float64), t["logp"], t["v"], t["old_logp"], t["adv"], t["vp"], t["ret"], clip, norm)   # a host block


def test_bad_arguments_are_refused(hip_lib):
    L, ws = hip_lib, _workspace(hip_lib)
    x = torch.zeros(8, dtype=torch.float32, device="cuda")
    block = torch.zeros(20, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    arrays = [P(x)] * 6
    tail = (0.2, 0, 0.0, 1.0, None, None, 0.5)
    assert L.catan_ppo_diag(*arrays, 0, *tail, P(block), P(ws), None) == -1 and b"catan_ppo_diag" in L.catan_last_error()       # CATAN_EINVAL
    assert L.catan_ppo_diag(*arrays, 8, *tail, None, P(ws), None) == -1 and b"catan_ppo_diag" in L.catan_last_error()
    assert L.catan_ppo_diag(*([None] + arrays[1:]), 8, *tail, P(block), P(ws), None) == -1 and b"catan_ppo_diag" in L.catan_last_error()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(block)) == 0


def _rollout(N, T, seed, warm, autocast):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    torch.manual_seed(0)
    env = VecCatanEnv(N, seed=seed)
    env.random_rollout(0, warm)
    net = CatanPolicy().cuda()
    return net, RolloutCollector(env, net, T, seed=1, autocast_dtype=autocast).gather_rollouts()


def test_trainer_read_out_on_device(hip_lib):
    """the N = 256, T = 12 rollout of test_rollout_and_update_on_device; two epochs of four minibatches under bf16 autocast"""
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    N, T = 256, 12
    net, st = _rollout(N, T, 5, 1500, None)
    tr = PPOTrainer(net, PPOConfig(ppo_epoch=2, num_mini_batch=4, diagnostics=True), autocast_dtype=torch.bfloat16, seed=3)
    norms, step = [], tr.optimiser.step

    def recording_step(*a, **kw):
        out = step(*a, **kw)
        norms.append(tr.optimiser.last_norm.clone())
        return out
    tr.optimiser.step = recording_step
    vl, al, el = tr.update(st)
    d = tr.diagnostics
    u = d["update"]
    assert u["rows"] == 2 * 4 * (T * N // 4) and u["steps"] == 8 and d["rows"] == [T * N] * 2 and d["steps"] == [4, 4]
    assert abs(u["entropy"] * tr.cfg.entropy_coef - el) <= 1e-5 * abs(el), (u["entropy"], el)
    rec = torch.cat(norms).double().cpu().numpy()
    assert len(rec) == 8 and abs(u["grad_norm_max"] - rec.max()) <= 1e-6 * rec.max() and abs(u["grad_norm_mean"] - rec.mean()) <= 1e-6 * rec.mean()
    assert u["grad_clipped_fraction"] == np.count_nonzero(rec.astype(np.float32) > np.float32(0.5)) / 8
    for e in (u, {k: v[0] for k, v in d.items() if k != "update"}, {k: v[1] for k, v in d.items() if k != "update"}):
        for k in ("clip_fraction", "policy_grad_zero_fraction", "value_clip_fraction", "value_grad_zero_fraction", "grad_clipped_fraction"):
            assert 0.0 <= e[k] <= 1.0, (k, e[k])
        assert e["policy_grad_zero_fraction"] <= e["clip_fraction"] and e["value_grad_zero_fraction"] <= e["value_clip_fraction"]
        assert e["approx_kl"] >= 0 and np.isfinite(e["explained_variance"]) and np.isfinite(e["approx_kl_k1"])
    assert set(tr.timings) == {"values_s", "gae_s", "minibatches_s"}
    assert all(np.isfinite(x) for x in (vl, al, el))


def test_turning_it_on_changes_nothing(hip_lib):
    """Three updates from the same copy of one net - diagnostics on, off, off - compared as test_weight_images_change_nothing compares:
    the backward kernels add with fp32 atomics, so two runs of the SAME setting differ in the last bits; on against off differs by no
    more than off against off does (x 4), while the net itself moved by more than 1e-2 (lr 5e-3 over eight steps)."""
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    N, T = 1024, 16
    net0, st = _rollout(N, T, 23, 700, torch.bfloat16)
    res, losses = [], []
    for on in (True, False, False):
        net = copy.deepcopy(net0)
        tr = PPOTrainer(net, PPOConfig(ppo_epoch=2, num_mini_batch=4, lr=5e-3, diagnostics=on), autocast_dtype=torch.bfloat16, seed=5)
        losses.append(tr.update(st))
        assert (tr.diagnostics is not None) == on
        res.append(torch.cat([p.detach().reshape(-1) for p in net.parameters()]))
    noise = float((res[1] - res[2]).abs().max())
    diff = float((res[0] - res[1]).abs().max())
    moved = float((res[1] - torch.cat([p.detach().reshape(-1) for p in net0.parameters()])).abs().max())
    assert moved > 1e-2 and diff <= 4.0 * noise + 1e-6, (diff, noise, moved)
