"""CPU: the plain-torch attention reference (tests/attention_reference.py) is itself held against autograd through policy._MHA's torch
branch in double, its yardsticks are sane, its key mask is a mask, and the acceptance rule rejects the planted errors on the very
case inputs tests/test_gpu_attention_fp64.py runs - that file leans on all of it."""
import pytest
import torch

import attention_reference as A


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _cases(L, H, HD, dtype=torch.bfloat16, B=A.MULTI_B):
    """the GPU file's case inputs at its multi-block size: (name, case) for unit / saturated, without and with lens"""
    for regime in ("unit", "saturated"):
        for masked in (False, True):
            lens = A.case_lens(L, B) if masked else None
            yield f"{L} {'lens' if masked else 'nolens'} {regime}", A.make_case(L, H, HD, B, regime, lens, dtype)


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_attention_ref_equals_autograd_through_the_module(L, H, HD, masked):
    """policy._MHA in double with the Q, K, V and output projections set to the identity and zero bias: its torch branch IS the
    reference formulation, its input x = q = k = v.  So the lifted formula on independent q, k, v leaves is checked as well: the
    branch's lines verbatim.  attention_ref's closed-form gradients equal autograd's to 1e-12 of each tensor's scale."""
    import math
    from settlers_of_catan_rl_amd import policy
    B, D = 23, H * HD
    g = torch.Generator().manual_seed(5 + L + masked)
    lens = A.case_lens(L, B, start=3) if masked else None
    dout = torch.randn((B, L, D), generator=g, dtype=torch.float64)
    # the module itself: q = k = v = x
    mha = policy._MHA(D, H).double()
    with torch.no_grad():
        for n in list(mha.qkv_nets) + [mha.out_proj_net]:
            n.weight.copy_(torch.eye(D, dtype=torch.float64))
            n.bias.zero_()
    x = torch.randn((B, L, D), generator=g, dtype=torch.float64).requires_grad_(True)
    y = mha(x, None if lens is None else lens.long())
    gx, = torch.autograd.grad((y * dout).sum(), x)
    xx = x.detach().view(B, L, H, HD)
    ref = A.attention_ref(torch.stack([xx, xx, xx], 2), lens, dout)
    assert ref["out"].dtype == torch.float64 and _rel(ref["out"], y.detach()) <= 1e-12
    assert _rel(ref["dq"] + ref["dk"] + ref["dv"], gx) <= 1e-12
    # the branch's formula on separate leaves
    qkv = (torch.randn((B, L, 3, H, HD), generator=g, dtype=torch.float64) * torch.tensor([0.9, 1.1, 1.7], dtype=torch.float64)[:, None, None]).requires_grad_(True)
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    scores = torch.matmul(q, k.transpose(-2, -1)) * (1.0 / math.sqrt(HD))
    if lens is not None:
        key_mask = torch.arange(L)[None, :] < lens[:, None]
        scores = scores.masked_fill(~key_mask[:, None, None, :], float("-inf"))
    o = torch.matmul(torch.softmax(scores, -1), v).transpose(1, 2).reshape(B, L, D)
    gq, = torch.autograd.grad((o * dout).sum(), qkv)
    ref = A.attention_ref(qkv.detach(), lens, dout)
    assert _rel(ref["out"], o.detach()) <= 1e-12
    for i, n in enumerate(("dq", "dk", "dv")):
        assert ref[n].shape == (B, L, D) and _rel(ref[n], gq[:, :, i].reshape(B, L, D)) <= 1e-12, (n, _rel(ref[n], gq[:, :, i].reshape(B, L, D)))


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
def test_yardsticks_are_sane(L, H, HD):
    """Each yardstick passes the rule against itself; a bf16 yardstick lies within 4 bf16 ulps of each tensor's scale (4 * 2^-8 * maxabs)
    of the reference and not ON it (it rounds); the fp32 yardstick lies within 2^-17 / 2^-15 of the scale - the floors the fp32 rule
    adds - on the unit cases.  per_sequence is the rule, sequence by sequence."""
    for path in A.PATHS:
        for name, c in _cases(L, H, HD, A.path_dtype(path), B=40):
            ref = A.attention_ref(c["qkv"], c["lens"], c["dout"])
            yard = A.attention_yardstick(c["qkv"], c["lens"], c["dout"], path)
            for o in A.OUTPUTS:
                ok, ek, ey, bound = A.accept(path, o, yard[o], ref[o], yard[o])
                scale = float(ref[o].abs().max())
                print(f"ATTN-CPU {path} {name} {o}: yardstick {ey:.4e} scale {scale:.4e} rel {ey / scale:.3e}")
                assert ok and ek == ey and bool(torch.isfinite(yard[o]).all()), (path, name, o)
                if path == "fp32":
                    if "unit" in name:
                        assert ey <= A.FP32_FLOOR[o] * scale, (path, name, o, ey, scale)
                else:
                    assert 0.0 < ey <= 4 * 2.0 ** -8 * scale, (path, name, o, ey, scale)
                oks, eks, bounds = A.per_sequence(path, o, yard[o], ref[o], yard[o])
                assert bool(oks.all())
                for b in (0, 7, 39):
                    one = A.accept(path, o, yard[o][b], ref[o][b], yard[o][b])
                    assert one[0] and one[1] == float(eks[b]) and one[3] == float(bounds[b])


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
def test_saturated_case_is_what_it_says(L, H, HD):
    """the stored bf16 inputs: scores reach +-50 at least; the row maximum sits on the planted key for 9 queries in 10 (the runner-up is
    close by design and bf16 storage moves scores by a few tenths) and in the planted lane half - upper, (j & 4) != 0, for the even
    queries of every sequence with more than 4 keys, lower for the odd ones - for 8 in 10; keys >= 16 and the last key are among the
    maxima; and the gradients did not vanish with the saturation"""
    for masked in (False, True):
        B = 40
        lens = A.case_lens(L, B) if masked else None
        c = A.make_case(L, H, HD, B, "saturated", lens, torch.bfloat16)
        q, k, _ = c["qkv"].double().permute(2, 0, 3, 1, 4)
        s = q @ k.transpose(-2, -1) / HD ** 0.5
        n = torch.full((B,), L) if lens is None else lens.long()
        s = s.masked_fill(torch.arange(L)[None, None, None, :] >= n[:, None, None, None], float("-inf"))
        am = s.argmax(-1)                                                                # [B, H, L]
        t = A.saturated_targets(L, H, lens, B)
        hard = ~A.soft_rows(L)
        am, t = am[:, :, hard], t[:, :, hard]                                            # (the soft rows have no planted maximum)
        assert float((am == t).double().mean()) >= 0.9
        assert float(s.max()) > 50 and float(s[torch.isfinite(s)].min()) < -50
        big = n > 4
        upper = ((am & 4) != 0).double()
        even = (torch.arange(L)[hard] & 1) == 0
        assert float(upper[big][:, :, even].mean()) >= 0.8 and float(upper[:, :, ~even].mean()) <= 0.2
        ref = A.attention_ref(c["qkv"], lens, c["dout"])
        for o in ("dq", "dk"):                                                           # no sequence of 2 keys or more is saturated in all its rows
            assert float(ref[o].abs().reshape(B, -1).amax(1)[n > 1].min()) > 1e-3, o
        full = n == L
        assert bool((am[full] == L - 1).any()) and bool((am[full] >= 16).any())
        assert min(float(ref[o].abs().max()) for o in A.OUTPUTS) > 0.5


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
def test_key_mask_of_the_reference(L, H, HD):
    """other K and V rows behind lens: out, dq and the rows < len of dk / dv do not move, the rows >= len of dk / dv are zero.  (Q rows
    >= len are queries like any other: the mask is a key mask.)"""
    B = 40
    lens = A.case_lens(L, B)
    c = A.make_case(L, H, HD, B, "unit", lens, torch.float32)
    a = A.attention_ref(c["qkv"], lens, c["dout"])
    b = A.attention_ref(A.replace_masked_rows(c, 1), lens, c["dout"])
    keep = (torch.arange(L)[None, :] < lens[:, None])[:, :, None].expand(B, L, H * HD)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dq"], b["dq"])
    for n in ("dk", "dv"):
        assert torch.equal(a[n][keep], b[n][keep]) and bool((a[n][~keep] == 0).all()) and bool((b[n][~keep] == 0).all()), n
    assert float((a["dk"][keep] != 0).double().mean()) > 0.9
    # and with dO's rows >= len zero, the Q rows >= len leave everything of the rows < len alone as well
    dz = torch.where(keep, c["dout"], torch.zeros(()))
    a = A.attention_ref(c["qkv"], lens, dz)
    b = A.attention_ref(A.replace_masked_rows(c, 2, ("q", "k", "v")), lens, dz)
    for n in A.OUTPUTS:
        assert torch.equal(a[n][keep], b[n][keep]), n
        if n != "out":
            assert bool((a[n][~keep] == 0).all()) and bool((b[n][~keep] == 0).all()), n


def _planted(name, c, path):
    """the result a kernel with the planted error would give, in the path's own arithmetic (the yardstick's), or None where the case
    cannot show the error by construction"""
    L, B, H, HD, lens = c["L"], c["B"], c["H"], c["HD"], c["lens"]
    y = lambda lens_, **kw: A.attention_yardstick(c["qkv"], lens_, c["dout"], path, **kw)
    if name == "key 18 dropped":
        if L != 19:
            return None
        return y(torch.full((B,), 18, dtype=torch.int32) if lens is None else lens.clamp(max=18))
    if name == "maximum over keys 0..15":                # (exact arithmetic cancels any constant: it shows as overflow only, on the probe rows)
        return y(lens, max_keys=16) if c["regime"] == "saturated" and L == 19 else None
    if name == "each lane half its own maximum":
        return y(lens, half_max=True)
    if name == "dk * 1.03":
        out = y(lens)
        out["dk"] = out["dk"] * 1.03
        return out
    if name == "heads 1 and 2 swapped":
        return {n: t.view(B, L, H, HD)[:, :, [0, 2, 1, 3]].reshape(B, L, H * HD) for n, t in y(lens).items()}
    if name == "lens + 1":
        return None if lens is None else y((lens + 1).clamp(max=L))
    if name == "lens - 1":
        return None if lens is None else y((lens - 1).clamp(min=1))
    raise KeyError(name)


PLANTS = ("key 18 dropped", "maximum over keys 0..15", "each lane half its own maximum", "dk * 1.03", "heads 1 and 2 swapped", "lens + 1", "lens - 1")


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
@pytest.mark.parametrize("path", A.PATHS)
def test_the_rule_rejects_planted_errors(L, H, HD, path):
    """On every case of the GPU file's multi-block size that can show it, each planted error is rejected by the whole-tensor rule on at
    least one output - and the unplanted yardstick is accepted on all four.  Which outputs reject is printed."""
    seen = set()
    for cname, c in _cases(L, H, HD, A.path_dtype(path)):
        ref = A.attention_ref(c["qkv"], c["lens"], c["dout"])
        yard = A.attention_yardstick(c["qkv"], c["lens"], c["dout"], path)
        assert all(A.accept(path, o, yard[o], ref[o], yard[o])[0] for o in A.OUTPUTS)
        for plant in PLANTS:
            bad = _planted(plant, c, path)
            if bad is None:
                continue
            rejected = [o for o in A.OUTPUTS if not A.accept(path, o, bad[o], ref[o], yard[o])[0]]
            print(f"ATTN-CPU plant {path} {cname}: {plant}: rejected on {rejected}")
            assert rejected, (path, cname, plant)
            if plant == "dk * 1.03":
                assert rejected == ["dk"]
            seen.add(plant)
    assert seen == set(PLANTS) - (set() if L == 19 else {"key 18 dropped", "maximum over keys 0..15"})


def test_length_cycle_and_lens():
    assert A.length_cycle(19) == [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 19]
    assert A.length_cycle(25) == [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 19, 20, 21, 23, 24, 25]
    for L in (19, 25):
        assert set(A.case_lens(L, A.MULTI_B).tolist()) == set(A.length_cycle(L))
        for Bs in (A.MFMA_BS, A.VALU_BS):                         # the small batches of a path continue the cycle where the one before ended
            seen, start = set(), 0
            for B in Bs:
                seen |= set(A.case_lens(L, B, start).tolist())
                start += B
            assert seen == set(A.length_cycle(L))
