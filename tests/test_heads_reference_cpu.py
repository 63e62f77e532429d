"""tests/heads_reference.py is checked before tests/test_gpu_heads_fp64.py trusts it: `chain_ref` in fp64 against the unfused
teacher-forced path of policy._ActionHeads (which tests/golden/policy_small.npz ties to the reference net) and against the entropies
and log records the reference returned (tests/golden/act_stats.npz); `head_ref` against a direct formula at every K and ncond of the
GPU test; the packs against nn_kernels' packers; and, for every case of the GPU test, the conditions its assertions rely on."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import heads_reference as H
import policy_fixture as pf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AMBIGUOUS_CAP = 0.15
_FF = {}


def _logits_keeping_dtype(self, pre, extra=None, custom=None):
    """policy._Head.logits without its final cast to fp32, so that a module in double stays in double (bound to the fixture's heads;
    `_fixture` first asserts that on the fp32 module it returns the bits of the real method)"""
    from settlers_of_catan_rl_amd.policy import _lin, _ln
    parts = [] if extra is None else [extra]
    if custom is not None:
        parts.append(_ln(self.custom_norm, _lin(custom, self.custom_mlp.weight, self.custom_mlp.bias), relu=True))
    if parts:
        e = parts[0] if len(parts) == 1 else torch.cat(parts, -1)
        pre = pre + _lin(e.to(pre.dtype), self.mlp_1.weight[:, self.mlp_1.in_features - e.shape[-1]:])
    h = _lin(_ln(self.norm, pre, relu=True), self.mlp_2.weight, self.mlp_2.bias)
    return _lin(h, self.distribution.linear.weight, self.distribution.linear.bias)


def _fixture():
    """the `ff` fixture net's action heads in fp64 (their `logits` without the cast to fp32) on its own inputs: main, the module's own pre_all, the unrounded fp64 packs (shared, never written)"""
    if not _FF:
        g = np.load(os.path.join(GOLD, "policy_small.npz"))
        net, _ = pf.load_fixture_policy(g, "ff", "cpu")
        x, B = pf.decode_inputs(g, "ff_")
        with torch.no_grad():
            main = net._main(x["obs_f"], x["lists"], x["lens"])[0].double()        # (the observation module stays fp32: the heads start at `main`)
        ahm = net.action_head_module
        gen = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for i, h in enumerate(ahm.action_heads):            # the stand-in is the real method, bit for bit, where both are fp32
                pre = torch.randn((64, 128), generator=gen)
                extra = torch.randint(0, 3, (64, H.HEAD_NCOND[i]), generator=gen).float() if H.HEAD_NCOND[i] and i != 5 else None
                custom = torch.randint(0, 4, (64, 12), generator=gen).float() if i == 5 else None
                assert torch.equal(_logits_keeping_dtype(h, pre, extra, custom), h.logits(pre, extra, custom)), i
        ahm = ahm.double()
        for h in ahm.action_heads:
            h.logits = types.MethodType(_logits_keeping_dtype, h)
        ahm.compact_evaluate = False
        with torch.no_grad():
            heads = ahm.action_heads
            pre_all = F.linear(main, torch.cat([h.mlp_1.weight[:, :ahm.D] for h in heads], 0), torch.cat([h.mlp_1.bias for h in heads], 0))
        cur_res, trade = net._custom(x["obs_f"])
        packs = [H.pack_module(h, ahm.D, torch.float64) for h in heads]
        _FF.update(g=g, ahm=ahm, main=main, pre_all=pre_all, masks=x["masks"], cur_res=cur_res.double(), trade=trade.double(), packs=packs,
                   custom=H.custom_pack_module(heads[5], torch.float64), eps=float(heads[0].norm.eps))
    return _FF


@pytest.mark.parametrize("which", ["ff_eval_actions", "ff_act_actions"])
def test_chain_ref_fp64_is_the_unfused_teacher_forced_module(which):
    """joint log-prob within 1e-9 of policy._ActionHeads.forward(actions=...) in double, row by row, and the mean of the per-row entropy
    within 1e-9 of its scalar; the evaluated columns that count are legal under chain_ref's own mask rows"""
    f = _fixture()
    A = torch.from_numpy(f["g"][which].astype(np.int64))
    with torch.no_grad():
        _, lp, ent = f["ahm"](f["main"], f["masks"].double(), f["cur_res"], f["trade"], actions=A)
        out = H.chain_ref(A, f["pre_all"], f["packs"], f["custom"], f["masks"], f["cur_res"], f["trade"], None, eps=f["eps"])
    assert bool(torch.isfinite(lp).all())
    assert float((out["logp"] - lp).abs().max()) <= 1e-9
    assert abs(float(out["entropy"].mean()) - float(ent)) <= 1e-9
    assert [(e["head"], e["step"]) for e in out["evals"]] == list(H.CHAIN_ORDER)
    for e in out["evals"]:
        counts = e["factor"] != 0
        assert bool((e["mask"].gather(1, A[:, e["col"]:e["col"] + 1]).squeeze(1)[counts] > 0).all()), (e["head"], e["step"])
    # every factor the glue can produce occurs in the fixture's evaluated actions: each head counts on some rows and not on others
    for e in out["evals"][1:] if which == "ff_eval_actions" else ():
        assert 0 < int((e["factor"] != 0).sum()) < A.shape[0], (e["head"], e["step"])


def test_chain_ref_fp64_matches_the_references_entropy_and_log_record():
    """free and forced rows of tests/golden/act_stats.npz (what the reference's own net returned from single-row calls) at that file's 1e-5"""
    f = _fixture()
    s = np.load(os.path.join(GOLD, "act_stats.npz"))
    for prefix in ("free_", "forced_"):
        idx = torch.arange(320) if prefix == "free_" else torch.from_numpy(s["forced_rows"].astype(np.int64))
        forced = None if prefix == "free_" else torch.from_numpy(s["forced_type"].astype(np.int64))
        A = torch.from_numpy(s[prefix + "actions"].astype(np.int64))
        with torch.no_grad():
            out = H.chain_ref(A, f["pre_all"][idx], f["packs"], f["custom"], f["masks"][idx], f["cur_res"][idx], f["trade"][idx], forced, eps=f["eps"])
        assert float((out["logp"] - torch.from_numpy(s[prefix + "logp"])).abs().max()) <= 1e-5, prefix
        assert float((out["entropy"] - torch.from_numpy(s[prefix + "entropy"])).abs().max()) <= 1e-5, prefix
        assert float((out["log"] - torch.from_numpy(s[prefix + "log"])).abs().max()) <= 1e-5, prefix
        # arg-max actions: every evaluation that counts picked its reference arg-max
        for e in out["evals"]:
            counts = e["factor"] != 0
            best, _ = H.top2_gap(e["logits"], e["mask"])
            assert torch.equal(best[counts], A[:, e["col"]][counts]), (prefix, e["head"], e["step"])
        if forced is not None:
            assert torch.equal(A[:, 0], forced) and float(out["log"][:, 1].abs().max()) == 0.0


def test_chain_ref_yardstick_stays_close_to_fp64_on_the_fixture():
    """the yardstick mode runs the same glue: with bf16 packs it is finite and differs from fp64 (same packs) by bf16 noise only - under
    0.25 in the joint log-prob of up to 18 evaluations whose logits are O(1), where a glue difference shows as O(1) on some row"""
    f = _fixture()
    heads = f["ahm"].action_heads
    packs = [H.pack_module(h, f["ahm"].D) for h in heads]
    custom = H.custom_pack_module(heads[5])
    A = torch.from_numpy(f["g"]["ff_eval_actions"].astype(np.int64))
    args = (A, f["pre_all"].to(torch.bfloat16), packs, custom, f["masks"], f["cur_res"], f["trade"], None)
    ref, yard = H.chain_ref(*args, eps=f["eps"]), H.chain_ref(*args, round_bf16=True, eps=f["eps"])
    assert yard["logp"].dtype == torch.float32 and bool(torch.isfinite(yard["logp"]).all()) and bool(torch.isfinite(yard["entropy"]).all())
    assert float((yard["logp"].double() - ref["logp"]).abs().max()) < 0.25
    assert torch.equal(yard["log"][:, 1].double(), ref["log"][:, 1]) and torch.equal(yard["log"][:, 3].double(), ref["log"][:, 3])


def test_packs_are_the_headers_layout_and_the_packers_agree():
    """pack_raw against the header's offsets element by element; nn_kernels.head_pack / head5_custom_pack bit-equal to pack_module /
    custom_pack_module for all twelve heads of the chained test's net"""
    from settlers_of_catan_rl_amd import nn_kernels
    c = H.head_case(41, 5, 16)
    raw, wts, vec = c["raw"], c["wts"], c["vec"]
    assert wts.numel() == H.WELEMS == 30720 and vec.numel() == H.VELEMS == 464 and wts.dtype == torch.bfloat16 and vec.dtype == torch.float32
    assert wts[3 * 128 + 7] == raw["W2"][3, 7] and wts[128 * 128 + 40 * 128 + 9] == raw["W3"][40, 9]
    assert bool((wts[128 * 128 + 41 * 128:128 * 128 + 80 * 128] == 0).all())                        # W3 rows >= K
    assert wts[128 * 128 + 80 * 128 + 4 * 128 + 11] == raw["W1e"][11, 4]                               # column j of the block as row j
    assert bool((wts[128 * 128 + 80 * 128 + 5 * 128:] == 0).all())
    assert vec[2] == raw["ln_w"][2] and vec[128 + 2] == raw["ln_b"][2] and vec[256 + 2] == raw["b2"][2] and vec[384 + 40] == raw["b3"][40]
    assert bool((vec[384 + 41:] == 0).all())
    ahm = H.chain_heads()
    for i, head in enumerate(ahm.action_heads):
        w0, v0 = nn_kernels.head_pack(head, ahm.D)
        w1, v1 = H.pack_module(head, ahm.D)
        assert w0.dtype == torch.bfloat16 and torch.equal(w0.view(torch.int16), w1.view(torch.int16)), i
        assert v0.dtype == torch.float32 and torch.equal(v0, v1), i
        assert H.HEAD_K[i] == head.distribution.linear.weight.shape[0] and H.HEAD_NCOND[i] == head.mlp_1.weight.shape[1] - ahm.D, i
    assert torch.equal(nn_kernels.head5_custom_pack(ahm.action_heads[5]), H.custom_pack_module(ahm.action_heads[5]))


@pytest.mark.parametrize("K", H.HEAD_KS)
def test_head_ref_fp64_against_the_direct_formula(K):
    """at every ncond of the GPU test: the logits from the RAW tensors with torch's own layer_norm / linear (head_ref reads the packs),
    log_softmax(logits + log(mask)), its cumulative sum and the entropy over p > 0 - all within 1e-10"""
    for ncond in H.HEAD_NCONDS:
        c = H.head_case(K, ncond, 193)
        ref, _, _ = H.head_case_refs(c)
        w = {k: (None if v is None else v.double()) for k, v in c["raw"].items()}
        x = c["pre"].double()
        if ncond:
            x = x + c["cond_op"].double() @ w["W1e"].t()
        logits = F.linear(F.linear(torch.relu(F.layer_norm(x, (128,), w["ln_w"], w["ln_b"], H.EPS)), w["W2"], w["b2"]), w["W3"], w["b3"])
        lp = torch.log_softmax(logits + torch.log(c["mask"].double()), -1)
        p = lp.exp()
        ent = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(-1)
        legal = c["mask"] > 0
        assert float((ref["logits"] - logits).abs().max()) <= 1e-10 * float(logits.abs().max()), ncond
        assert float((ref["logp_all"] - lp)[legal].abs().max()) <= 1e-10 and bool((ref["logp_all"][~legal] == float("-inf")).all()), ncond
        assert float((ref["cdf"] - p.cumsum(-1)).abs().max()) <= 1e-10 and float((ref["entropy"] - ent).abs().max()) <= 1e-10, ncond
        assert float((ref["cdf"][:, -1] - 1).abs().max()) <= 1e-10


def test_every_per_head_case_of_the_gpu_test_meets_its_conditions():
    """for each (K, ncond, B) of test_gpu_heads_fp64.py: every row has a legal column; the yardstick is finite (log-probs on the legal
    columns); at most 15 % of the rows are ambiguous for the arg-max rule; the planted rows are what they claim (one legal column /
    all legal; an underflow row's last column stands >= 100 above every other, so their probabilities are exact zeros in fp32, and no
    other row switches the spike unit on); the planted uniforms sit where the docstring says; cond holds values bf16 cannot, and the
    (257, 256) pairs cancel as operands"""
    assert len(set(H.HEAD_CASES)) == len(H.HEAD_CASES) == 15 * 8 + 7 * 6 + 6
    assert {K for K, _, _ in H.HEAD_CASES} == set(H.HEAD_KS) and {n for _, n, _ in H.HEAD_CASES} == set(H.HEAD_NCONDS)
    assert {B for _, _, B in H.HEAD_CASES} == set(H.HEAD_BS) | {H.WIDE_B}
    seen = set()
    for K, ncond, B in H.HEAD_CASES:
        c = H.head_case(K, ncond, B)
        ref, yard, is_uf = H.head_case_refs(c)
        legal = c["mask"] > 0
        assert bool(legal.any(1).all()), (K, ncond, B)
        for k in ("logits", "cdf", "entropy"):
            assert bool(torch.isfinite(yard[k]).all()), (K, ncond, B, k)
        assert bool(torch.isfinite(yard["logp_all"][legal]).all()), (K, ncond, B)
        _, _, amb = H.ambiguous_rows(ref, yard, c["mask"], ~is_uf)
        assert float(amb.float().mean()) <= AMBIGUOUS_CAP, (K, ncond, B, float(amb.float().mean()))
        h_spike = F.linear(torch.relu(F.layer_norm(c["pre"].double() if not ncond else c["pre"].double() + c["cond_op"].double() @ c["raw"]["W1e"].double().t(),
                                                   (128,), c["raw"]["ln_w"].double(), c["raw"]["ln_b"].double(), H.EPS)), c["raw"]["W2"].double()[H.G_SPIKE:H.G_SPIKE + 1])
        assert bool((h_spike[~is_uf] == 0).all()) and bool((h_spike[is_uf] > 30).all()), (K, ncond, B)
        for rw, kind in c["plant"].items():
            seen.add(kind)
            n = int(legal[rw].sum())
            if kind in ("first", "last", "middle"):
                col = {"first": 0, "last": K - 1, "middle": K // 2}[kind]
                assert n == 1 and bool(legal[rw, col]) and float(ref["logp_all"][rw, col]) == 0.0 and float(ref["entropy"][rw]) == 0.0
            else:
                assert n == K
            if kind == "underflow":
                assert float(ref["logits"][rw, K - 1] - ref["logits"][rw, :K - 1].max()) >= 100.0 and float(c["u"][rw]) == 0.0
                assert float(yard["entropy"][rw]) == 0.0 and bool((yard["logp_all"][rw, :K - 1].exp() == 0).all())
        assert float(c["u"].max()) <= H.U_TOP < 1.0 and float(c["u"][B - 1]) in (0.0, H.U_TOP)
        if B >= 191:                                                     # (smaller B: the last two rows take precedence over 0, 1, 15, 16)
            assert [float(c["u"][i]) for i in (0, 1, 15, 16)] == [0.0, H.U_TOP, 0.0, H.U_TOP]
            assert {float(c["u"][B - 1]), float(c["u"][B - 2])} == {0.0, H.U_TOP}
        if ncond:
            assert bool((c["cond"] != c["cond_op"]).any())
        if ncond >= 2 and B >= 2:
            assert float(c["cond"][0, 0]) == 257.0 and float(c["cond_op"][0, 0]) == 256.0 == float(c["cond_op"][0, 1])
            assert bool((c["raw"]["W1e"][:, 0] == -c["raw"]["W1e"][:, 1]).all())
    assert seen == set(H.PLANTS)


def test_chain_cases_of_the_gpu_test_meet_their_conditions():
    """every mask segment has a legal column, head 9's product of any two of its rows too; from 4 099 rows on all 13 forced types, free
    rows, empty and non-empty hands occur; index 0 of the hands is 0 (a hand of only "index 0" would leave step 0 no legal column)"""
    for B in H.CHAIN_BS:
        c = H.chain_case(B)
        m = c["masks"]
        for h, (off, K) in enumerate(zip(H.MASK_OFF, H.HEAD_K)):
            segs = {1: 3, 6: 3, 9: 4}.get(h, 1)
            rows = [m[:, off + s * K:off + (s + 1) * K] for s in range(segs)]
            assert all(bool((r > 0).any(1).all()) for r in rows), (B, h)
            if h == 9:
                assert all(bool(((a * b) > 0).any(1).all()) for a in rows for b in rows), B
        assert H.MASK_OFF[11] + H.HEAD_K[11] == 325 == m.shape[1]
        assert bool((c["cur_res"][:, 0] == 0).all()) and c["pre_all"].dtype == torch.bfloat16
        if B >= 4099:
            assert set(c["forced"].tolist()) == set(range(-1, 13))
            empty = c["cur_res"].sum(1) == 0
            assert 0.1 < float(empty.float().mean()) < 0.5
            assert bool((c["trade"] != c["trade"].to(torch.bfloat16).float()).any())


@pytest.mark.parametrize("B", [b for b in H.CHAIN_BS if b <= 4099])
def test_chain_cases_are_decisive_enough_for_the_arg_max_rule(B):
    """the 15 % cap of the arg-max rule for every one of the 18 evaluations of the chained GPU test's inputs, with the same packs: chain_ref
    teacher-forced at its own fp64 arg-max actions (the GPU test asserts it at the kernel's, which differ on ambiguous rows at most;
    49 153 rows are left to it: the fixed point costs minutes on the CPU)"""
    ahm = H.chain_heads()
    packs = [H.pack_module(h, ahm.D) for h in ahm.action_heads]
    custom = H.custom_pack_module(ahm.action_heads[5])
    c = H.chain_case(B)
    with torch.no_grad():
        A, ref = H.chain_argmax(c, packs, custom)
        yard = H.chain_ref(A, c["pre_all"], packs, custom, c["masks"], c["cur_res"], c["trade"], c["forced"], round_bf16=True)
    shares = H.chain_ambiguous_shares(c, A, ref, yard)
    assert max(shares) <= AMBIGUOUS_CAP, [(e["head"], e["step"], round(s, 3)) for e, s in zip(ref["evals"], shares)]
    for e in ref["evals"]:
        assert bool((e["mask"] > 0).any(1).all()), (e["head"], e["step"])
