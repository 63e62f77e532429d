"""optim.FusedAdam == torch.optim.Adam(lr, eps) behind nn.utils.clip_grad_norm_(max_grad_norm) (RL/ppo/ppo.py:23,67-68): parameters
within 1e-6 after 50 steps - the torch-operation form on the CPU, the two-launch kernel form (csrc/catan_optim.hip) under -m gpu."""
import copy

import pytest
import torch

from settlers_of_catan_rl_amd.optim import FusedAdam


def _nets(device):
    torch.manual_seed(0)
    # tensor sizes around the chunk size (2 048) and not multiples of 4; one layer that never receives a gradient, one that receives
    # one only in some steps (torch.optim.Adam then keeps a step count per parameter: its bias corrections lag the others')
    net = torch.nn.ModuleDict({"a": torch.nn.Linear(37, 53), "ln": torch.nn.LayerNorm(53), "b": torch.nn.Linear(53, 4099), "c": torch.nn.Linear(4099, 3),
                               "unused": torch.nn.Linear(5, 7), "sometimes": torch.nn.Linear(53, 53)}).to(device)
    return net, copy.deepcopy(net)


def _fwd(net, x, s=0):
    h = net["ln"](net["a"](x))
    if s % 3 == 1 or s in (5, 6):
        h = h + net["sometimes"](h)
    return net["c"](torch.relu(net["b"](h)))


def _run(device, steps=50, clip=0.5, shared_grads=False, none_grad_is_zero=False):
    """shared_grads: both optimisers are handed the SAME gradient values (the reference net's backward; `net` only follows).  On the
    device the two nets' own backward passes are not bit-equal (the library GEMM's split-K sums depend on the launch), and fifty Adam
    steps of a training run amplify that last-bit noise to 1e-5 in the parameters whoever's optimiser is used: what the kernel form
    has to equal is torch's UPDATE of given gradients.  none_grad_is_zero: FusedAdam steps a parameter without a gradient as on a
    zero gradient; torch.optim.Adam is handed zeros for those."""
    net, ref = _nets(device)
    mine = FusedAdam(net.parameters(), lr=3e-4, eps=1e-5, none_grad_is_zero=none_grad_is_zero)
    theirs = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    g = torch.Generator().manual_seed(1)
    norms = []
    for s in range(steps):
        x = (torch.randn(16, 37, generator=g) * (1 + s % 5)).to(device)        # gradient norms on both sides of the clip threshold
        for n_, o in ((net, mine), (ref, theirs)):
            o.zero_grad()
            if shared_grads and n_ is net:
                continue
            (_fwd(n_, x, s) ** 2).mean().mul(0.02 if s % 3 else 5.0).backward()
        if shared_grads:
            for p, q in zip(net.parameters(), ref.parameters()):
                p.grad = None if q.grad is None else q.grad.clone()
        if none_grad_is_zero:
            for q in ref.parameters():
                if q.grad is None:
                    q.grad = torch.zeros_like(q)
        tn = torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
        theirs.step()
        mine.step(clip)
        norms.append((float(tn), float(mine.last_norm)))
        if s == 20:                                                              # train_loop's learning-rate decay writes param_groups
            for o in (mine, theirs):
                o.param_groups[0]["lr"] = 1e-4
    return net, ref, norms, mine


def _check(net, ref, norms, mine):
    assert any(a > 0.5 for a, _ in norms) and any(a < 0.5 for a, _ in norms), "the test is meant to clip in some steps only"
    for a, b in norms:
        assert abs(a - b) <= 5e-5 * max(1.0, a), (a, b)        # (torch's norm of norms is an fp32 sum; the kernel's partial sums are added in fp64)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert float((p - q).abs().max()) < 1e-6, (k, float((p - q).abs().max()))
    if not mine.none_grad_is_zero:
        assert all(float(m.abs().max()) == 0.0 for m, p in zip(mine._m, mine.params) if p.grad is None)    # no gradient: no step, as torch
    # the per-parameter step counts are torch's
    names = [k for k, _ in net.named_parameters()]
    steps = dict(zip(names, mine.param_steps.tolist()))
    if mine.none_grad_is_zero:
        assert set(steps.values()) == {mine.steps}, steps
    else:
        assert steps["unused.weight"] == 0 and 0 < steps["sometimes.weight"] < mine.steps and steps["a.weight"] == mine.steps, steps


def test_fused_adam_equals_torch_adam_with_clipping_cpu():
    _check(*_run("cpu"))


def test_state_dict_round_trip_cpu():
    net, ref, norms, mine = _run("cpu", steps=3)
    other = FusedAdam(net.parameters(), lr=1.0)
    other.load_state_dict(mine.state_dict())
    assert other.steps == 3 and other.param_groups[0]["lr"] == mine.param_groups[0]["lr"]
    assert all(torch.equal(a, b) for a, b in zip(other._m, mine._m)) and all(torch.equal(a, b) for a, b in zip(other._v, mine._v))
    assert other.param_steps.tolist() == mine.param_steps.tolist() and len(set(mine.param_steps.tolist())) > 1
    # a state of another parameter list is refused, even where its first entries' shapes match
    fewer = FusedAdam(list(net.parameters())[:4], lr=1.0)
    with pytest.raises(ValueError):
        fewer.load_state_dict(mine.state_dict())


def test_fused_adam_none_grad_is_zero_equals_torch_adam_on_zeros_cpu():
    _check(*_run("cpu", none_grad_is_zero=True))


def test_state_dict_continues_like_torch_adam_cpu():
    """per-parameter step counts travel both ways: FusedAdam's checkpoint loaded into torch.optim.Adam (and torch's into FusedAdam)
    continues with the same updates"""
    net, ref, norms, mine = _run("cpu", steps=8)
    theirs = torch.optim.Adam(ref.parameters(), lr=mine.param_groups[0]["lr"], eps=1e-5)
    sd = theirs.state_dict()                   # (torch's own param_groups entries, FusedAdam's state)
    sd["state"] = {i: s for i, s in mine.state_dict()["state"].items() if int(float(s["step"])) > 0}     # (torch keeps none for a parameter that never stepped)
    theirs.load_state_dict(sd)
    back = FusedAdam(net.parameters(), lr=1.0, eps=1e-5)
    back.load_state_dict(theirs.state_dict())
    assert back.param_steps.tolist() == mine.param_steps.tolist() and back.steps == mine.steps
    x = torch.randn(16, 37, generator=torch.Generator().manual_seed(5))
    for n_, o in ((net, back), (ref, theirs)):
        o.zero_grad()
        (_fwd(n_, x, 1) ** 2).mean().backward()
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
    theirs.step(); back.step(0.5)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert float((p - q).abs().max()) < 1e-6, k


@pytest.mark.gpu
def test_fused_adam_kernels_equal_torch_adam_with_clipping(hip_lib):
    _check(*_run("cuda", shared_grads=True))
    # two independent training runs (each net its own backward): equal up to the amplified last-bit noise of the backward passes
    # (measured 1.1e-5 .. 1.2e-4 after 50 steps; with torch.optim.Adam on both sides the two runs differ just as much)
    net, ref, norms, _ = _run("cuda")
    assert max(float((p - q).abs().max()) for p, q in zip(net.parameters(), ref.parameters())) < 2e-3


@pytest.mark.gpu
def test_fused_adam_kernels_none_grad_is_zero_equal_torch_adam_on_zeros(hip_lib):
    _check(*_run("cuda", shared_grads=True, none_grad_is_zero=True))


@pytest.mark.gpu
def test_fused_adam_on_the_policy_net_one_ppo_step(hip_lib):
    """the real parameter list (1.93 M parameters, ~300 tensors): one update of the kernel form against torch's on a copy"""
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(0)
    net = CatanPolicy().cuda()
    ref = copy.deepcopy(net)
    mine, theirs = FusedAdam(net.parameters(), lr=3e-4, eps=1e-5), torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    for s in range(5):
        for p, q in zip(net.parameters(), ref.parameters()):
            gr = torch.randn_like(p) * (0.001 if s % 2 else 0.1)
            p.grad, q.grad = gr, gr.clone()
        tn = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
        theirs.step(); mine.step(0.5)
        assert abs(float(tn) - float(mine.last_norm)) <= 5e-5 * float(tn)
    assert max(float((p - q).abs().max()) for p, q in zip(net.parameters(), ref.parameters())) < 1e-6


@pytest.mark.gpu
def test_fused_adam_reads_the_grad_bucket_views_in_place(hip_lib):
    """The multi-rank layout on the device: every .grad a view of dist.GradBucket's flat buffer.  The kernels take the views as they are
    (16-byte aligned by the bucket's padding): no gradient goes through a copy, no .grad is replaced, and the update equals the one on
    free-standing gradients."""
    from settlers_of_catan_rl_amd import dist as cdist
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(1)
    net = CatanPolicy().cuda()
    ref = copy.deepcopy(net)
    bucket = cdist.GradBucket(net.parameters())
    mine, theirs = FusedAdam(net.parameters(), lr=3e-4, eps=1e-5), FusedAdam(ref.parameters(), lr=3e-4, eps=1e-5)
    for s in range(3):
        bucket.zero()
        for p, q in zip(net.parameters(), ref.parameters()):
            gr = torch.randn_like(p) * 0.05
            p.grad.add_(gr); q.grad = gr
        mine.step(0.5); theirs.step(0.5)
        bucket.check()
    assert mine.copied_grads == 0 and theirs.copied_grads == 0
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), ref.parameters()))

