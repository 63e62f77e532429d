"""GPU: the fused action-head kernel (k_head_fwd, csrc/catan_heads.hip) row by row against fp64 - per head through the C ABI
(catan_head_fwd, catan_head_fwd_entropy) and chained (catan_head_chain, catan_head_chain_ex through nn_kernels.heads_chain).

reference = tests/heads_reference.py in fp64 from the same inputs; yardstick = the same in fp32 with a bf16 rounding where the kernel's
header rounds.  Acceptance of a value (the rule of tests/pin_rule.py over the whole tensor, with the floor of a bf16 output):
    maxabs(kernel - reference) <= 2 * maxabs(yardstick - reference) + 2^-9 * maxabs(reference)
Nothing in a bound comes from the kernel's output.  Per case and output one `HEADS` line is printed (kernel error, yardstick error,
ratio, bound, scale): profiles/heads_kernel_tests.txt is that output.

Per row, with `ref` / `yard` = head_ref of the case:
  log-prob   logp[r] against ref.logp_all[r, action[r]]; the yardstick error is the maximum over ALL rows and ALL legal columns of
             |yard.logp_all - ref.logp_all|, so it does not depend on which column the kernel picked
  entropy    against ref.entropy
  arg-max    delta = the bound of the logits; a row is ambiguous when its two best legal reference logits are closer than 2 delta.
             Every other row: action == the reference arg-max, exactly.  Ambiguous rows: a legal action whose reference logit is within
             2 delta of the best.  At most 15 % of a case's rows are ambiguous (asserted here and, for the same inputs, on the CPU).
  sampled    tau = the bound of the cdf; the action is legal, ref.cdf[r, a] + tau > u[r] and ref.cdf[r, previous legal column] - tau
             <= u[r] (0 before the first legal column); u = 0 gives the first legal column
The reference is evaluated at the conditioning values as bf16 OPERANDS (the unfused path casts them before the product:
policy._Head.logits) while the kernel is handed the unrounded floats: a kernel that skipped that cast would be judged against values
it did not use (the (257, 256) pairs of heads_reference.head_case cancel only as operands).  The planted underflow rows, whose logits
reach +-100, are judged as a group of their own: inside the others' bound their scale alone would be a floor of 0.2.
Reference and yardstick of the per-head cases are computed on the CPU, where the inputs are drawn: the ambiguous rows are then the
very rows tests/test_heads_reference_cpu.py counted."""
import pytest
import torch

import guarded as G
import heads_reference as H
import pin_rule as PR
from guarded import NAN, ptr as P, stream as _stream

pytestmark = pytest.mark.gpu

GUARD = 64                       # rows behind every buffer: NaN behind the inputs, the sentinel behind the outputs
SENTINEL = 0x5A5B
AMBIGUOUS_CAP = 0.15


def _out_buffer(rows, dtype):
    """-> (whole, view): one element per row in front of GUARD sentinel rows"""
    return G.sentinel_output(rows, dtype, GUARD, sentinel=SENTINEL)


def _record(case, name, kernel, ref, yard):
    ok, ek, ey, bound = PR.whole(kernel, ref, yard, PR.BF16_FLOOR)
    finite = bool(torch.isfinite(kernel).all())
    print(f"HEADS {case} {name}: kernel {ek:.4e} yardstick {ey:.4e} ratio {PR.ratio(ek, ey, PR.INF):.3f} bound {bound:.4e} scale {float(ref.abs().max()):.4e}")
    return [] if (ok and finite) else [(case, name, ek, ey, bound, "finite" if finite else "NOT FINITE")]


# ----------------------------------------------------------------------------------------------------------------- per head
_CASES = {}


def _case(K, ncond, B):
    """inputs, reference and yardstick of a case: computed once, shared, never written"""
    if (K, ncond, B) not in _CASES:
        c = H.head_case(K, ncond, B)
        _CASES[(K, ncond, B)] = (c,) + H.head_case_refs(c)
    return _CASES[(K, ncond, B)]


def _run_head(L, c, rows, sampled, entropy, windowed):
    """the kernel on the first `rows` rows of case c -> (action, logp, ent or None) on the CPU; asserts the output guards intact.
    windowed: pre = the 128-column window (K % 12) of a [rows, 1536] matrix, mask = the window at column 13 of a [rows, 325] matrix
    whose other columns are 1 (legal: a read outside the window could be picked); else contiguous buffers.  cond always has 3 columns
    of NaN behind its ncond; every row-major input ends in GUARD rows of NaN, the two packs in 1 024 / GUARD NaN elements."""
    from settlers_of_catan_rl_amd import _lib
    K, ncond = c["K"], c["ncond"]
    if windowed:
        w = K % 12
        pre = torch.full((rows + GUARD, 1536), NAN, dtype=torch.bfloat16, device="cuda")
        pre[:rows, 128 * w:128 * (w + 1)] = c["pre"][:rows].cuda()
        pre_v = pre[:, 128 * w:]
        mask = torch.ones((rows + GUARD, 325), dtype=torch.float32, device="cuda")
        mask[rows:] = NAN
        mask[:rows, 13:13 + K] = c["mask"][:rows].cuda()
        mask_v = mask[:, 13:]
    else:
        pre = torch.full((rows + GUARD, 128), NAN, dtype=torch.bfloat16, device="cuda")
        pre[:rows] = c["pre"][:rows].cuda()
        mask = torch.full((rows + GUARD, K), NAN, dtype=torch.float32, device="cuda")
        mask[:rows] = c["mask"][:rows].cuda()
        pre_v, mask_v = pre, mask
    cond = None
    if ncond:
        cond = torch.full((rows + GUARD, ncond + 3), NAN, dtype=torch.float32, device="cuda")
        cond[:rows, :ncond] = c["cond"][:rows].cuda()
    u = None
    if sampled:
        u = G.guarded_input(c["u"][:rows], GUARD)[0]
    wts, vec = G.guarded_input(c["wts"], 1024)[0], G.guarded_input(c["vec"], GUARD)[0]            # (the packs end in NaN too)
    (hold_a, action), (hold_l, logp) = _out_buffer(rows, torch.int64), _out_buffer(rows, torch.float32)
    hold_e, ent = _out_buffer(rows, torch.float32) if entropy else (None, None)
    head = (P(pre_v), pre.stride(0), P(cond), cond.stride(0) if ncond else 0, ncond, P(wts), P(vec), H.EPS, K, P(mask_v), mask.stride(0), P(u), P(action), P(logp))
    if entropy:
        _lib.check(L.catan_head_fwd_entropy(*head, P(ent), rows, _stream()))
    else:
        _lib.check(L.catan_head_fwd(*head, rows, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hold_a, action) and G.intact(hold_l, logp) and (ent is None or G.intact(hold_e, ent)), (K, ncond, rows, sampled, entropy, windowed)
    return action.cpu(), logp.cpu(), None if ent is None else ent.cpu()


def _check_values(case, c, ref, yard, is_uf, action, logp, ent):
    """legality, log-prob and entropy of one run; the underflow rows as their own group -> the list of failures"""
    mask = c["mask"]
    bad = []
    assert bool(((action >= 0) & (action < c["K"])).all()), case
    legal_pick = mask.gather(1, action[:, None]).squeeze(1) > 0
    assert bool(legal_pick.all()), (case, "illegal action on rows", torch.nonzero(~legal_pick).flatten().tolist()[:8])
    rl, yl = H.legal_or_zero(ref["logp_all"], mask), H.legal_or_zero(yard["logp_all"], mask)
    for tag, rows in (("", ~is_uf), (" underflow rows", is_uf)):
        if not bool(rows.any()):
            continue
        got = rl[rows].clone()
        got.scatter_(1, action[rows][:, None], logp[rows].double()[:, None])
        bad += _record(case + tag, "logp", got, rl[rows], yl[rows])
        bad += _record(case + tag, "entropy", ent[rows], ref["entropy"][rows], yard["entropy"][rows])
    for rw, kind in c["plant"].items():                             # one legal column: log-prob 0 and entropy 0, exactly
        if kind in ("first", "last", "middle"):
            col = {"first": 0, "last": c["K"] - 1, "middle": c["K"] // 2}[kind]
            assert int(action[rw]) == col and float(logp[rw]) == 0.0 and float(ent[rw]) == 0.0, (case, rw, kind, int(action[rw]), float(logp[rw]), float(ent[rw]))
    return bad


def _check_argmax(case, c, ref, yard, is_uf, action):
    delta, best, amb = H.ambiguous_rows(ref, yard, c["mask"], ~is_uf)
    share = float(amb.float().mean())
    print(f"HEADS {case} argmax: delta {delta:.4e} ambiguous rows {int(amb.sum())} of {c['B']} ({share:.4f})")
    assert share <= AMBIGUOUS_CAP, (case, share)
    clear = ~amb                                                    # (the underflow rows are clear: the last column stands 100 above the rest)
    wrong = clear & (action != best)
    assert not bool(wrong.any()), (case, "arg-max differs on clear rows", [(r, int(action[r]), int(best[r])) for r in torch.nonzero(wrong).flatten().tolist()[:8]])
    z = ref["logits"].double()
    short = z.gather(1, best[:, None]).squeeze(1) - z.gather(1, action[:, None]).squeeze(1)
    assert bool((short[amb] <= 2 * delta).all()), (case, "ambiguous row picked a column more than 2 delta below the best")


def _check_sampled(case, c, ref, yard, is_uf, action, u, mask=None):
    mask = c["mask"] if mask is None else mask
    cdf = ref["cdf"].double()
    B = cdf.shape[0]
    for tag, rows in (("", ~is_uf), (" underflow rows", is_uf)):
        if not bool(rows.any()):
            continue
        tau, ey = PR.whole_bound(ref["cdf"][rows], yard["cdf"][rows], PR.BF16_FLOOR)
        print(f"HEADS {case}{tag} cdf: yardstick {ey:.4e} bound {tau:.4e}")
        a, uu = action[rows], u[rows].double()
        upper = cdf[rows].gather(1, a[:, None]).squeeze(1)
        lower = torch.where(a > 0, cdf[rows].gather(1, (a - 1).clamp(min=0)[:, None]).squeeze(1), torch.zeros_like(upper))
        ok = (upper + tau > uu) & (lower - tau <= uu)
        assert bool(ok.all()), (case + tag, "cdf bracket", [(int(r), int(action[r]), float(u[r])) for r in torch.nonzero(rows)[~ok].flatten().tolist()[:8]])
    first = (mask > 0).float().argmax(1)
    zero = (u == 0.0) & ~is_uf                                        # (an underflow row's first legal columns have probability 0)
    assert bool((action[zero] == first[zero]).all()), (case, "u = 0 must give the first legal column")


@pytest.mark.parametrize("K,ncond,B", H.HEAD_CASES)
def test_head_kernel_vs_fp64(hip_lib, K, ncond, B):
    """One head evaluation at (K, ncond, B): arg-max and sampled, one on window buffers and the other on contiguous ones (which is which
    alternates with K + ncond), each through catan_head_fwd and
    catan_head_fwd_entropy (same action and log-prob bits; the entropy does not depend on u or the layout).  K covers every column
    tile count KT = 1..5 at both edges and the categorical's 20-column lane split; ncond the four-column rounds of the conditioning
    loop up to the full pack; B the 16-row tiles and 192-row workgroups of the narrow configuration and 49 153 = the first row count of
    the wide one, whose last workgroup holds one row."""
    c, ref, yard, is_uf = _case(K, ncond, B)
    case = f"K={K} ncond={ncond} B={B}"
    win = (K + ncond) % 2 == 0                    # which of the two runs takes the window buffers: both layouts meet both modes over the cases
    a0, lp0, _ = _run_head(hip_lib, c, B, sampled=False, entropy=False, windowed=win)
    a1, lp1, e1 = _run_head(hip_lib, c, B, sampled=False, entropy=True, windowed=win)
    s0, slp0, _ = _run_head(hip_lib, c, B, sampled=True, entropy=False, windowed=not win)
    s1, slp1, se1 = _run_head(hip_lib, c, B, sampled=True, entropy=True, windowed=not win)
    assert torch.equal(a0, a1) and torch.equal(lp0.view(torch.int32), lp1.view(torch.int32)), (case, "arg-max: the statistics variant differs")
    assert torch.equal(s0, s1) and torch.equal(slp0.view(torch.int32), slp1.view(torch.int32)), (case, "sampled: the statistics variant differs")
    assert torch.equal(e1.view(torch.int32), se1.view(torch.int32)), (case, "the entropy depends on u or on the buffer layout")
    bad = _check_values(case + " argmax", c, ref, yard, is_uf, a1, lp1, e1)
    bad += _check_values(case + " sampled", c, ref, yard, is_uf, s1, slp1, se1)
    assert not bad, bad
    _check_argmax(case, c, ref, yard, is_uf, a1)
    # an underflow row: the last column holds all the probability - the arg-max, and the sample at u = 0 (the K - 1 legal columns before
    # it have probability 0 exactly: `cdf > u` passes over them, `cdf >= u` would stop at column 0)
    assert bool((a1[is_uf] == K - 1).all()) and bool((s1[is_uf] == K - 1).all()), (case, "underflow rows", a1[is_uf].tolist(), s1[is_uf].tolist())
    _check_sampled(case, c, ref, yard, is_uf, s1, c["u"])


@pytest.mark.parametrize("K", [13, 73, 80])
def test_head_rows_do_not_depend_on_the_row_count(hip_lib, K):
    """A row's action, log-prob and entropy depend on its own inputs only: the first 192 rows of the B = 193 and 4 099 runs (narrow
    configuration) are bit-equal to a run on those 192 rows alone.  The same rows of the wide B = 49 153 case are held to the yardstick
    by test_head_kernel_vs_fp64 like every other row; here they are also compared with a narrow run of the same rows (the two
    configurations run the same arithmetic per row: recorded, and asserted to pick the same actions on the rows that are not ambiguous)."""
    for ncond in (0, 9):
        for B in (193, 4099):
            c = _case(K, ncond, B)[0]
            for sampled in (False, True):
                full = _run_head(hip_lib, c, B, sampled, True, True)
                part = _run_head(hip_lib, c, 192, sampled, True, True)
                for f, p in zip(full, part):
                    assert torch.equal(f[:192].view(torch.int32 if f.dtype == torch.float32 else torch.int64), p.view(torch.int32 if p.dtype == torch.float32 else torch.int64)), (K, ncond, B, sampled)
    if K in (13, 80):
        c, ref, yard, is_uf = _case(K, 9, H.WIDE_B)
        wide = _run_head(hip_lib, c, H.WIDE_B, False, True, True)
        narrow = _run_head(hip_lib, c, 192, False, True, True)
        _, _, amb = H.ambiguous_rows(ref, yard, c["mask"], ~is_uf)
        same_bits = int((wide[1][:192].view(torch.int32) == narrow[1].view(torch.int32)).sum())
        print(f"HEADS K={K} ncond=9 wide vs narrow, rows 0..191: {same_bits} of 192 log-probs bit-equal")
        clear = ~amb[:192]
        assert torch.equal(wide[0][:192][clear], narrow[0][clear])


def test_head_kernel_with_the_packers_packs(hip_lib):
    """the packs as nn_kernels.head_pack makes them from a policy._Head - heads 0 (K = 13, no conditioning), 1 (54, 2), 2 (73, 0) and 10
    (5, 9) of the chained test's net - on the inputs of the raw case with the same K and ncond: the same assertions (the spike rows
    mean nothing to these weights: they are all-legal rows here)"""
    from settlers_of_catan_rl_amd import nn_kernels
    ahm = H.chain_heads().cuda()
    for i in (0, 1, 2, 10):
        K, ncond = H.HEAD_K[i], H.HEAD_NCOND[i]
        c = dict(H.head_case(K, ncond, 193))
        w, v = nn_kernels.head_pack(ahm.action_heads[i], ahm.D)
        c["wts"], c["vec"] = w.detach().cpu().clone(), v.detach().cpu().clone()
        c["underflow"] = torch.zeros(0, dtype=torch.long)
        c["plant"] = {rw: k for rw, k in c["plant"].items() if k in ("first", "last", "middle")}
        ref, yard, is_uf = H.head_case_refs(c)
        case = f"head_pack head {i} K={K} ncond={ncond} B=193"
        a1, lp1, e1 = _run_head(hip_lib, c, 193, sampled=False, entropy=True, windowed=True)
        s1, slp1, se1 = _run_head(hip_lib, c, 193, sampled=True, entropy=True, windowed=False)
        bad = _check_values(case + " argmax", c, ref, yard, is_uf, a1, lp1, e1) + _check_values(case + " sampled", c, ref, yard, is_uf, s1, slp1, se1)
        assert not bad, bad
        delta, best, amb = H.ambiguous_rows(ref, yard, c["mask"], ~is_uf)
        print(f"HEADS {case} argmax: delta {delta:.4e} ambiguous rows {int(amb.sum())} of 193")
        assert float(amb.float().mean()) <= AMBIGUOUS_CAP, (case, int(amb.sum()))
        assert torch.equal(a1[~amb], best[~amb]), case
        z = ref["logits"].double()
        assert bool(((z.gather(1, best[:, None]) - z.gather(1, a1[:, None])).squeeze(1)[amb] <= 2 * delta).all()), case
        _check_sampled(case, c, ref, yard, is_uf, s1, c["u"])


# ------------------------------------------------------------------------------------------------------------------ chained
_CHAIN = {}


def _chain_setup():
    if not _CHAIN:
        from settlers_of_catan_rl_amd import nn_kernels
        ahm = H.chain_heads().cuda()
        packs = []
        for h in ahm.action_heads:
            w, v = nn_kernels.head_pack(h, ahm.D)
            packs.append((w.detach().clone(), v.detach().clone()))
        _CHAIN.update(ahm=ahm, packs=packs, custom=nn_kernels.head5_custom_pack(ahm.action_heads[5]).detach().clone(), eps=float(ahm.action_heads[0].norm.eps))
    return _CHAIN


def _chain_eval_rules(case, e, yard_e, A, u, deterministic):
    """the arg-max rule / the cdf-bracket rule of the per-head mode for one evaluation of the pass, at its teacher-forced reference"""
    a = A[:, e["col"]]
    name = f"{case} head {e['head']} step {e['step']}"
    legal_pick = e["mask"].gather(1, a[:, None]).squeeze(1) > 0
    # head 0 writes the forced type into its column: the rules hold for the rows that were free
    rows = torch.ones_like(legal_pick) if e["head"] != 0 else e["factor"] != 0
    assert bool(legal_pick[rows].all()), (name, "illegal pick")
    if not bool(rows.any()):
        return 0.0
    if deterministic:
        delta, best, amb = H.ambiguous_rows(e, yard_e, e["mask"], rows)
        clear = rows & ~amb
        assert torch.equal(a[clear], best[clear]), (name, "arg-max differs on clear rows", int((a[clear] != best[clear]).sum()))
        z = e["logits"].double()
        short = z.gather(1, best[:, None]).squeeze(1) - z.gather(1, a[:, None]).squeeze(1)
        assert bool((short[amb] <= 2 * delta).all()), name
        return float(amb.float().sum() / rows.float().sum().clamp(min=1))
    tau, _ = PR.whole_bound(e["cdf"][rows], yard_e["cdf"][rows], PR.BF16_FLOOR)
    cdf = e["cdf"].double()
    upper = cdf.gather(1, a[:, None]).squeeze(1)
    lower = torch.where(a > 0, cdf.gather(1, (a - 1).clamp(min=0)[:, None]).squeeze(1), torch.zeros_like(upper))
    ok = ((upper + tau > u.double()) & (lower - tau <= u.double())) | ~rows
    assert bool(ok.all()), (name, "cdf bracket", int((~ok).sum()))
    return 0.0


@pytest.mark.parametrize("B", H.CHAIN_BS)
def test_chained_pass_vs_fp64(hip_lib, B):
    """A whole pass of the twelve heads in chained mode (18 launches) on synthetic inputs that reach every branch of the glue, arg-max
    and sampled, with and without statistics, against chain_ref teacher-forced at the kernel's own 18 action columns A.  A enters the
    reference and the yardstick only as the point of evaluation - which mask row, which conditioning columns, which factor - and only
    after its legality under the mask rows derived from its EARLIER columns was asserted; no bound contains a kernel output.
      A[:, 0] = the forced type where one was given; every column that enters the joint log-prob is legal
      joint log-prob, entropy (slot 26), the two probabilities of the log record (28, 30): within the yardstick; the legal counts (29, 31) exact
      statistics leave actions and log-prob bits alone
      per evaluation: the arg-max rule, its 15 % cap on the ambiguous rows included (arg-max pass) / the cdf-bracket rule with that
      evaluation's own u (sampled pass; u_all is re-drawn from the generator's seed as heads_chain draws it)
    The joint log-prob matching is also what covers the two rules of the lists: the step behind a pick of 0 counts nothing (its factor
    is 0), and head 8's give columns are zero where head 7's log-prob was filtered (action_heads_module.py:175) - such rows, empty hands
    among them, are asserted to occur.  From 4 099 rows on: all 13 types, both cards of heads 9 / 10, lists that end at step 0, 1, 2
    and 3, and empty hands of proposing rows occur."""
    from settlers_of_catan_rl_amd import nn_kernels
    s = _chain_setup()
    c = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in H.chain_case(B).items()}
    heads = s["ahm"].action_heads
    bad = []
    for deterministic in (True, False):
        case = f"chain B={B} {'argmax' if deterministic else 'sampled'}"
        runs = []
        for stats in (False, True):
            g = torch.Generator(device="cuda").manual_seed(77 + B)
            with torch.no_grad():
                runs.append(nn_kernels.heads_chain(heads, s["ahm"].D, c["pre_all"], c["masks"], c["cur_res"], c["trade"], deterministic, g, c["forced"], stats=stats))
        torch.cuda.synchronize()
        (A, lp), (A1, lp1, ent, rec) = runs
        assert torch.equal(A, A1) and torch.equal(lp.view(torch.int32), lp1.view(torch.int32)), (case, "the statistics change actions or log-probs")
        u_all = torch.rand((18, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(77 + B))
        forced = c["forced"] >= 0
        assert torch.equal(A[forced, 0], c["forced"][forced]), case
        assert bool(((A >= 0) & (A < torch.tensor(H.COL_K, device="cuda"))).all()), case
        args = (A, c["pre_all"], s["packs"], s["custom"], c["masks"], c["cur_res"], c["trade"], c["forced"])
        ref, yard = H.chain_ref(*args, eps=s["eps"]), H.chain_ref(*args, round_bf16=True, eps=s["eps"])
        worst_amb = 0.0
        for k, (e, ye) in enumerate(zip(ref["evals"], yard["evals"])):
            assert bool((e["mask"] > 0).any(1).all()), (case, e["head"], e["step"], "a mask row without a legal column")
            counts = e["factor"] != 0
            legal_pick = e["mask"].gather(1, A[:, e["col"]:e["col"] + 1]).squeeze(1) > 0
            assert bool(legal_pick[counts].all()), (case, e["head"], e["step"], "an illegal column enters the joint log-prob")
            worst_amb = max(worst_amb, _chain_eval_rules(case, e, ye, A, u_all[k], deterministic))
        if deterministic:
            print(f"HEADS {case}: largest ambiguous share of an evaluation {worst_amb:.4f}")
            assert worst_amb <= AMBIGUOUS_CAP, (case, worst_amb)
        bad += _record(case, "logp", lp, ref["logp"], yard["logp"])
        bad += _record(case, "entropy", ent, ref["entropy"], yard["entropy"])
        bad += _record(case, "log type p", rec[:, 0], ref["log"][:, 0], yard["log"][:, 0])
        bad += _record(case, "log head p", rec[:, 2], ref["log"][:, 2], yard["log"][:, 2])
        assert torch.equal(rec[:, 1].double(), ref["log"][:, 1]) and torch.equal(rec[:, 3].double(), ref["log"][:, 3]), (case, "legal counts")
        # the branches of the glue that this pass took
        typ, card = A[:, 0], A[:, 4]
        prop = typ == H.T_PROPOSE
        give, recv = A[:, 7:11], A[:, 11:15]
        filt = ref["filtered7"]
        assert bool(filt[~prop].all()) and bool((ref["evals"][14]["cond"][:, :6][filt] == 0).all())
        for lst, first in ((give, 10), (recv, 14)):                    # the step behind a 0 counts nothing
            for i in range(3):
                assert bool((ref["evals"][first + i + 1]["factor"][lst[:, i] == 0] == 0).all())
        if B >= 4099:
            assert set(typ.tolist()) == set(range(13)), case
            pd = typ == H.T_PLAYDEV
            assert bool((pd & (card == H.C_YOP)).any()) and bool((pd & (card == H.C_MONO)).any()) and bool((pd & (card != H.C_YOP) & (card != H.C_MONO)).any()), case
            assert bool((typ == H.T_EXCHANGE).any())
            for lst in (give, recv):
                stop = torch.where((lst == 0).any(1), (lst == 0).float().argmax(1), torch.full((B,), 4, device="cuda"))
                assert {0, 1, 2, 3} <= set(stop[prop].tolist()), (case, "list lengths")
            empty = c["cur_res"].sum(1) == 0
            assert bool((prop & empty).any()) and bool((prop & ~empty).any()) and bool((prop & filt).any()) and bool((prop & ~filt).any()), case
    assert not bad, bad
