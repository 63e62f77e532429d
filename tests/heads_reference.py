"""Plain-torch restatements of the fused action-head kernel (csrc/catan_heads.hip: k_head_fwd), per head (`head_ref`: catan_head_fwd,
catan_head_fwd_entropy) and for a whole teacher-forced pass of the twelve heads (`chain_ref`: catan_head_chain, catan_head_chain_ex),
with the seeded input generators the tests of both share.  No call into the library or into nn_kernels: torch ops only, on the CPU
or the GPU, written from include/catan_hip_nn.h and the reference's RL/models/build_agent_model.py:113-147 and
action_heads_module.py:66-179,258-329.

Both functions have the two modes of tests/te_reference.py.
  round_bf16=False  the REFERENCE: fp64 throughout, from the same inputs.
  round_bf16=True   the YARDSTICK: fp32 with a round-to-bf16 at the points the kernel's header lists - the conditioning value, the
                    conditioning product, after the add, after LayerNorm + ReLU, after each Linear (its bias added in fp32 first:
                    the second of them are the logits); head 5's trade features: the trade entries, custom_mlp's output, the
                    features.  Softmax statistics in fp32.  It shows what bf16 storage costs; it is not an oracle.
Operand casts are NOT treated alike by the two tests.  Per head, the GPU test hands both modes the conditioning values already cast to
bf16 (head_case's `cond_op`), so the kernel's own cast of them is required, not excused.  In chain_ref the fp64 mode takes head 5's
`trade` and its features unrounded while the kernel (and the yardstick) round them: there the cast is part of what the yardstick
measures - the module in double, which chain_ref must equal to 1e-9, does not round them either.
tests/test_heads_reference_cpu.py holds the reference against the unfused module, the golden statistics and a direct formula;
tests/test_gpu_heads_fp64.py holds the kernels against the reference with the rule of tests/pin_rule.py (`whole`, floor BF16_FLOOR)."""
import torch

from pin_rule import BF16_FLOOR, whole_bound
from te_reference import _ln_stats, _modes

# include/catan_hip_nn.h (catan_head_fwd): wts = W2 [128][128] | W3 [80][128] (rows >= K zero) | W1e^T [32][128]; vec = ln_w, ln_b, b2 [128 each], b3 [80]
KP, NCP = 80, 32
WELEMS = 128 * 128 + KP * 128 + NCP * 128
VELEMS = 3 * 128 + KP
# the twelve heads (build_agent_model.py:58-80): output columns, conditioning columns behind the trunk, first column of the [B, 325]
# mask matrix (EnvWrapper.get_action_masks: type 13, corner 3 x 54, edge 73, tile 19, card 5, accept 2, player 3 x 3, give 6, receive 6,
# resource A 4 x 5, resource B 5, discard 5)
HEAD_K = (13, 54, 73, 19, 5, 2, 3, 6, 6, 5, 5, 5)
HEAD_NCOND = (0, 2, 0, 0, 0, 32, 2, 6, 12, 4, 9, 0)
MASK_OFF = (0, 13, 175, 248, 267, 272, 274, 283, 289, 295, 315, 320)
# the pass's eighteen evaluations in the header's order, as (head, step), and the action column each one fills
CHAIN_ORDER = ((0, 0), (1, 0), (2, 0), (3, 0), (5, 0), (6, 0), (11, 0), (4, 0), (9, 0), (10, 0),
               (7, 0), (7, 1), (7, 2), (7, 3), (8, 0), (8, 1), (8, 2), (8, 3))
CHAIN_COL = (0, 1, 2, 3, 5, 6, 17, 4, 15, 16, 7, 8, 9, 10, 11, 12, 13, 14)
T_SETTLE, T_ROAD, T_CITY, T_BUYDEV, T_PLAYDEV, T_EXCHANGE, T_PROPOSE, T_RESPOND, T_ROBBER, T_ROLL, T_ENDTURN, T_STEAL, T_DISCARD = range(13)
C_YOP, C_MONO = 2, 4
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------------ packs
def pack_raw(W2, W3, W1e, ln_w, ln_b, b2, b3, dtype=torch.bfloat16):
    """The header's packs from raw tensors: W2 [128, 128] = mlp_2.weight, W3 [K, 128] = distribution.linear.weight, W1e [128, ncond] =
    the conditioning columns of mlp_1.weight (or None) -> (wts [WELEMS] of `dtype`, vec [VELEMS] fp32 - fp64 when dtype is fp64)"""
    K = W3.shape[0]
    w3 = torch.zeros((KP, 128), dtype=dtype, device=W2.device)
    w3[:K] = W3.to(dtype)
    w1 = torch.zeros((NCP, 128), dtype=dtype, device=W2.device)
    if W1e is not None and W1e.shape[1]:
        w1[:W1e.shape[1]] = W1e.t().to(dtype)
    vd = torch.float64 if dtype == torch.float64 else torch.float32
    bb = torch.zeros(KP, dtype=vd, device=W2.device)
    bb[:K] = b3.to(vd)
    return torch.cat([W2.to(dtype).reshape(-1), w3.reshape(-1), w1.reshape(-1)]), torch.cat([ln_w.to(vd), ln_b.to(vd), b2.to(vd), bb])


def pack_module(head, trunk_dim, dtype=torch.bfloat16):
    """pack_raw on a policy._Head.  bf16: what nn_kernels.head_pack must produce (the Linear biases rounded to bf16, as bf16 autocast
    hands them to the GEMM); fp64: the module's own numbers unrounded, for the comparison with the module itself."""
    rb = (lambda t: t.to(torch.bfloat16).float()) if dtype == torch.bfloat16 else (lambda t: t)
    d = lambda t: t.detach()
    return pack_raw(d(head.mlp_2.weight), d(head.distribution.linear.weight), d(head.mlp_1.weight)[:, trunk_dim:], d(head.norm.weight), d(head.norm.bias),
                    rb(d(head.mlp_2.bias)), rb(d(head.distribution.linear.bias)), dtype)


def custom_pack_module(head, dtype=torch.bfloat16):
    """head 5's custom_mlp W [32][12], b [32], custom_norm weight [32], bias [32] as catan_head_chain's `custom` (float [480]; bf16: W
    and b rounded to bf16 and kept in floats)"""
    vd = torch.float64 if dtype == torch.float64 else torch.float32
    rb = (lambda t: t.to(torch.bfloat16)) if dtype == torch.bfloat16 else (lambda t: t)
    d = lambda t: t.detach()
    return torch.cat([rb(d(head.custom_mlp.weight)).to(vd).reshape(-1), rb(d(head.custom_mlp.bias)).to(vd), d(head.custom_norm.weight).to(vd),
                      d(head.custom_norm.bias).to(vd)])


# --------------------------------------------------------------------------------------------------------------------- one head
def head_ref(pre, cond, wts, vec, eps, K, mask, round_bf16=False):
    """catan_head_fwd for every row at once.  pre [B, 128]; cond [B, ncond] or None; wts / vec the packs; mask [B, K] (> 0 = legal).
      x = pre + cond W1e^T   y = relu(LayerNorm(x))   h = y W2^T + b2   logits = h W3^T + b3
      logp_all = log_softmax over the legal columns (-inf on the others)   cdf = the cumulative probability over the legal columns in
      column order (an illegal column repeats the value before it)   entropy = -sum p log p over p > 0
    -> dict(logits [B, K], logp_all [B, K], cdf [B, K], entropy [B], nav [B] = the number of legal columns)"""
    wd, r = _modes(round_bf16)
    wts, vec = wts.to(wd), vec.to(wd)
    W2 = wts[:128 * 128].view(128, 128)
    W3 = wts[128 * 128:128 * 128 + KP * 128].view(KP, 128)[:K]
    W1t = wts[128 * 128 + KP * 128:].view(NCP, 128)
    ln_w, ln_b, b2, b3 = vec[:128], vec[128:256], vec[256:384], vec[384:384 + K]
    x = pre.to(wd)
    if cond is not None and cond.shape[1] > 0:
        x = r(x + r(r(cond.to(wd)) @ W1t[:cond.shape[1]]))
    y = r(torch.relu(_ln_stats(x, eps)[0] * ln_w + ln_b))
    h = r(y @ W2.t() + b2)
    out = categorical_ref(r(h @ W3.t() + b3), mask)
    return out


def categorical_ref(logits, mask):
    """the masked categorical of RL/distributions.py:10-40 on given logits, in the logits' dtype"""
    legal = mask > 0
    ninf = torch.full_like(logits, float("-inf"))
    mx = torch.where(legal, logits, ninf).max(-1, keepdim=True).values
    e = torch.where(legal, torch.exp(logits - mx), torch.zeros_like(logits))
    lse = mx + torch.log(e.sum(-1, keepdim=True))
    lp = logits - lse
    p = torch.where(legal, torch.exp(lp), torch.zeros_like(logits))
    return {"logits": logits, "logp_all": torch.where(legal, lp, ninf), "cdf": p.cumsum(-1),
            "entropy": -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(-1), "nav": legal.sum(-1).to(logits.dtype)}


# ------------------------------------------------------------------------------------------------------------- the whole pass
def chain_ref(actions, pre_all, packs, custom, masks, cur_res, trade, forced, round_bf16=False, eps=EPS):
    """The teacher-forced evaluation of a pass of catan_head_chain(_ex) at the 18 action columns `actions` [B, 18] (CHAIN_COL): every
    evaluation's mask row, conditioning columns and log-prob factor are derived from the EARLIER columns of `actions`, as the kernel's
    per-row state derives them from its own earlier picks.  pre_all [B, 12 * 128]; packs: the twelve heads' (wts, vec); custom: head 5's
    float [480]; masks [B, 325]; cur_res [B, 6]; trade [B, 12]; forced int64 [B] (>= 0: the type was given) or None.
    -> dict(evals = 18 dicts in CHAIN_ORDER: head_ref's fields + head, step, col, mask [B, K], cond, factor [B] (what the evaluation's
            log-prob and entropy are multiplied with before they enter the sums: log_prob_masks x the lists' "behind a stop" rule; 0 for a
            forced type), logp [B] (of the action in column `col`),
            logp [B] = the joint log-prob, entropy [B] = state slot 26, log [B, 4] = slots 28..31,
            filtered7 [B] = head 7's log-prob came out 0, so head 8 is conditioned on zeros)
    The glue:
      head 1 / 6     mask row 0 / 1 / 2 of 3 by the type (settlement, city, other / propose, steal, other); cond = the two type flags
      head 9         mask row (exchange ? 0 : 1) times, for a played card, row (Monopoly 2, Year of Plenty 3, other 1); cond = (play card,
                     exchange, played YoP, played Monopoly); counts for exchange, or a played YoP / Monopoly
      head 10        cond = head 9's + one-hot(resource A) where head 9 counted; counts for exchange or a played YoP
      head 7 / 8     four steps each from the start hand; mask: "stop" only at step 0 of an empty hand, later always; head 7: a resource
                     while the running hand holds it; cond = the running pick counts (column 0 cleared), head 8: head 7's final counts in
                     front, zeroed where head 7's log-prob came out 0 (action_heads_module.py:175); a step counts unless the
                     pick before it was 0 (the reference looks at the previous pick only, :306-312), and only for a proposal
    Statistics: entropy = sum factor x H; log = (p of the type | 1 forced, legal types | 0 forced, p and legal columns of the type's
    specific head: type 0 / 2 -> head 1, 1 -> 2, 8 -> 3, 4 -> 4, 11 -> 6; else 0, 0)."""
    wd, r = _modes(round_bf16)
    A = actions.long()
    B, dev = A.shape[0], A.device
    m = masks.to(wd)
    typ, card = A[:, 0], A[:, 4]
    is_ = lambda t: (typ == t).to(wd)
    one, zero = torch.ones(B, dtype=wd, device=dev), torch.zeros(B, dtype=wd, device=dev)
    was_forced = (forced >= 0) if forced is not None else torch.zeros(B, dtype=torch.bool, device=dev)
    ar = lambda n: torch.arange(n, device=dev)[None, :]
    rows_of = lambda h, width, row: m.gather(1, MASK_OFF[h] + width * row[:, None] + ar(width))
    window = lambda h: m[:, MASK_OFF[h]:MASK_OFF[h] + HEAD_K[h]]
    evals = []
    joint, ent = zero.clone(), zero.clone()

    def run(h, step, cond, mask, factor):
        nonlocal joint, ent
        col = CHAIN_COL[len(evals)]
        assert CHAIN_ORDER[len(evals)] == (h, step)
        o = head_ref(pre_all[:, 128 * h:128 * (h + 1)], cond, packs[h][0], packs[h][1], eps, HEAD_K[h], mask, round_bf16)
        lp = o["logp_all"].gather(1, A[:, col:col + 1]).squeeze(1)
        o.update(head=h, step=step, col=col, mask=mask, cond=cond, factor=factor, logp=lp)
        evals.append(o)
        joint = joint + torch.where(factor != 0, lp * factor, zero)
        ent = ent + torch.where(factor != 0, o["entropy"] * factor, zero)
        return o

    e0 = run(0, 0, None, window(0), (~was_forced).to(wd))
    flags = lambda a, b: torch.stack((is_(a), is_(b)), 1)
    row = torch.where(typ == T_SETTLE, 0, torch.where(typ == T_CITY, 1, 2))
    e1 = run(1, 0, flags(T_SETTLE, T_CITY), rows_of(1, 54, row), is_(T_SETTLE) + is_(T_CITY))
    e2 = run(2, 0, None, window(2), is_(T_ROAD))
    e3 = run(3, 0, None, window(3), is_(T_ROBBER))
    # head 5: accept / reject, conditioned on relu(custom_norm(custom_mlp(proposed_trade)))
    cu = custom.to(wd)
    t = r(r(trade.to(wd)) @ cu[:384].view(32, 12).t() + cu[384:416])
    feat = r(torch.relu(_ln_stats(t, eps)[0] * cu[416:448] + cu[448:480]))
    run(5, 0, feat, window(5), is_(T_RESPOND))
    row = torch.where(typ == T_PROPOSE, 0, torch.where(typ == T_STEAL, 1, 2))
    e6 = run(6, 0, flags(T_PROPOSE, T_STEAL), rows_of(6, 3, row), is_(T_PROPOSE) + is_(T_STEAL))
    run(11, 0, None, window(11), is_(T_DISCARD))
    e4 = run(4, 0, None, window(4), is_(T_PLAYDEV))
    playdev = typ == T_PLAYDEV
    yop, mono = (playdev & (card == C_YOP)).to(wd), (playdev & (card == C_MONO)).to(wd)
    base = is_(T_PLAYDEV) + is_(T_EXCHANGE)
    cond9 = torch.stack((is_(T_PLAYDEV), is_(T_EXCHANGE), yop, mono), 1)
    mask9 = rows_of(9, 5, torch.where(typ == T_EXCHANGE, 0, 1))
    row_c = torch.where(card == C_MONO, 2, torch.where(card == C_YOP, 3, 1))
    mask9 = mask9 * torch.where(playdev[:, None], rows_of(9, 5, row_c), torch.ones_like(mask9))
    cnt9 = base * torch.where(playdev, yop + mono, one)
    run(9, 0, cond9, mask9, cnt9)
    ra = torch.nn.functional.one_hot(A[:, 15], 5).to(wd) * (cnt9 != 0).to(wd)[:, None]
    run(10, 0, torch.cat((cond9, ra), 1), window(10), base * torch.where(playdev, yop, one))
    # heads 7 / 8: the give and receive lists
    prop = is_(T_PROPOSE)
    start = cur_res.to(wd)
    give = None
    for h in (7, 8):
        res, out = start.clone(), torch.zeros((B, 6), dtype=wd, device=dev)
        keep, lsum = one.clone(), zero.clone()
        for step in range(4):
            mask = (res > 0).to(wd) if h == 7 else torch.ones_like(res)
            mask[:, 0] = (res.sum(-1) == 0).to(wd) if step == 0 else 1.0
            if step > 0:
                keep = (A[:, CHAIN_COL[len(evals) - 1]] > 0).to(wd)         # (the previous pick of this list)
            o = run(h, step, out if h == 7 else torch.cat((give, out), 1), mask, keep * prop)
            lsum = lsum + torch.where(keep != 0, o["logp"], zero)
            hot = torch.nn.functional.one_hot(A[:, o["col"]], 6).to(wd)
            out = out + hot
            res = torch.clamp(res - hot, min=0)
            out[:, 0] = 0
        if h == 7:
            filtered = (torch.where(prop != 0, lsum, zero) == 0).to(wd)
            give, filtered7 = out * (1 - filtered)[:, None], filtered
    # the record of log_specific_head_probs
    p0 = torch.where(was_forced, one, torch.exp(e0["logp"]))
    n0 = torch.where(was_forced, zero, e0["nav"])
    sp, sn = zero.clone(), zero.clone()
    for e, types in ((e1, (T_SETTLE, T_CITY)), (e2, (T_ROAD,)), (e3, (T_ROBBER,)), (e4, (T_PLAYDEV,)), (e6, (T_STEAL,))):
        sel = sum((typ == t) for t in types) > 0
        sp, sn = torch.where(sel, torch.exp(e["logp"]), sp), torch.where(sel, e["nav"], sn)
    return {"evals": evals, "logp": joint, "entropy": ent, "log": torch.stack((p0, n0, sp, sn), 1), "filtered7": filtered7 != 0}


# ----------------------------------------------------------------------------------------------- bounds the GPU tests derive
def top2_gap(ref_logits, mask):
    """-> (arg-max over the legal columns [B], best legal logit minus the second best [B]; inf with one legal column)"""
    z = torch.where(mask > 0, ref_logits.double(), torch.full_like(ref_logits.double(), float("-inf")))
    top = z.topk(min(2, z.shape[1]), -1)
    gap = top.values[:, 0] - top.values[:, 1] if z.shape[1] > 1 else torch.full_like(top.values[:, 0], float("inf"))
    return top.indices[:, 0], gap


# ---------------------------------------------------------------------------------------------------- inputs: per-head mode
HEAD_KS = (2, 5, 13, 16, 17, 20, 21, 33, 41, 48, 54, 61, 65, 73, 80)
HEAD_NCONDS = (0, 1, 2, 4, 5, 9, 12, 32)
HEAD_BS = (1, 15, 16, 17, 191, 192, 193, 4099)
WIDE_B = 49153
# (K, ncond, B): K x ncond at B = 193; B at K in {13, 73, 80} x ncond in {0, 9}; the wide configuration's first row count at K in {13, 54, 80}
HEAD_CASES = tuple([(K, nc, 193) for K in HEAD_KS for nc in HEAD_NCONDS]
                   + [(K, nc, B) for B in HEAD_BS for K in (13, 73, 80) for nc in (0, 9) if B != 193]
                   + [(K, nc, WIDE_B) for K in (13, 54, 80) for nc in (0, 9)])
U_TOP = 1.0 - 2.0 ** -24            # the largest float below 1: what torch.rand can return at most
F_SPIKE, G_SPIKE = 5, 9             # the LayerNorm feature / hidden unit that only a planted "underflow" row switches on
PLANTS = ("first", "last", "middle", "all", "underflow")


def head_case(K, ncond, B):
    """The seeded, asymmetric inputs of one per-head case, drawn on the CPU -> dict.
    pre: the rows' mean (-1 .. 1.5) and scale (2.5 .. 0.5) vary across the rows; LayerNorm weight ~ 1.7 (1 +- 0.6), bias ~ -0.4 +- 0.8.
    W3 is heavy-tailed (cubed normals): a row's best logit stands clear of the second more often than with normal weights, which keeps
    the share of rows the arg-max rule calls ambiguous under its cap without a larger logit scale.
    cond (ncond > 0): small integers, a third of the entries with a fraction that bf16 cannot hold; from two columns on W1e's second
    column is minus its first and the even rows carry (257, 256) in the two: as bf16 operands (256, 256) they cancel exactly, unrounded
    they leave one whole W1e column in x.  `cond` is what the kernel is given; `cond_op` = the same values as the bf16 operands that
    bf16 autocast hands to the product (policy._Head.logits: `e.to(pre.dtype)`), which is where reference and yardstick are evaluated.
    Planted mask rows (`plant`: row -> kind; rows 0..4 and, from 32 rows on, rows B - 7 .. B - 3: the last two rows stay ordinary, so the
    uniforms planted there decide a pick; none at B = 1, whose row is an ordinary one): only column
    0 / only K - 1 / only K // 2 legal, all legal, and "underflow": all legal on a row whose pre is a spike at feature F_SPIKE - the
    only rows where relu(LayerNorm) lets that feature through (weight 1, bias -6), unit G_SPIKE of h reads nothing else, and W3 puts
    +2 of it on column K - 1 and -2 on the others: the LAST column ends > 100 above every other column, whose probabilities are exact
    zeros in fp32 - a sample must pass over K - 1 legal columns of probability 0, whatever its u.
    Planted u: 0 on rows 0, 15, one of the last two and the underflow rows (cdf > u, not >=: a column of probability 0 is never the
    pick), U_TOP on rows 1, 16 and the other of the last two."""
    g = torch.Generator().manual_seed(7919 * K + 131 * ncond + B)
    rn = lambda *s: torch.randn(s, generator=g)
    mean = torch.linspace(-1.0, 1.5, B)[:, None]
    scale = torch.linspace(0.5, 2.5, B).flip(0)[:, None]
    pre = rn(B, 128) * scale + mean
    ln_w, ln_b = (1.0 + 0.6 * rn(128)) * 1.7, 0.8 * rn(128) - 0.4
    W2, b2 = 0.12 * rn(128, 128), 0.3 * rn(128)
    W3, b3 = 0.1 * rn(K, 128), 0.3 * rn(K)
    W1e = 0.3 * rn(128, ncond) if ncond else None
    ln_w[F_SPIKE], ln_b[F_SPIKE] = 1.0, -6.0
    W2[G_SPIKE] = 0.0; W2[G_SPIKE, F_SPIKE] = 8.0; b2[G_SPIKE] = 0.0
    W3[:, G_SPIKE] = -2.0; W3[K - 1, G_SPIKE] = 2.0
    cond = None
    if ncond:
        cond = torch.randint(0, 3, (B, ncond), generator=g).float()
        cond = cond + (torch.rand((B, ncond), generator=g) < 0.33).float() * 0.3 * rn(B, ncond)
        if ncond >= 2:
            W1e[:, 0] = rn(128); W1e[:, 1] = -W1e[:, 0]
            cond[0::2, 0] = 257.0; cond[0::2, 1] = 256.0
    mask = (torch.rand((B, K), generator=g) < min(0.5, 1.5 / K)).float()
    sure = torch.randint(0, K, (B,), generator=g)
    mask[torch.arange(B), sure] = 1.0
    plant = {}
    if B > 1:
        for j, kind in enumerate(PLANTS):
            if j < B:
                plant[j] = kind
            if B >= 32:
                plant[B - 7 + j] = PLANTS[(j + 2) % 5]
    for rw, kind in plant.items():
        mask[rw] = 1.0 if kind in ("all", "underflow") else 0.0
        if kind in ("first", "last", "middle"):
            mask[rw, {"first": 0, "last": K - 1, "middle": K // 2}[kind]] = 1.0
        if kind == "underflow":
            pre[rw] = 0.5 * rn(128); pre[rw, F_SPIKE] = 200.0
    u = torch.rand(B, generator=g)
    flip = (K + ncond + B) % 2
    for rw, v in ((0, 0.0), (1, U_TOP), (15, 0.0), (16, U_TOP), (B - 2, (U_TOP, 0.0)[flip]), (B - 1, (0.0, U_TOP)[flip])):
        if 0 <= rw < B:
            u[rw] = v
    for rw, kind in plant.items():
        if kind == "underflow":
            u[rw] = 0.0
    bf = torch.bfloat16
    pre, W2, W3, W1e = pre.to(bf), W2.to(bf), W3.to(bf), None if W1e is None else W1e.to(bf)
    wts, vec = pack_raw(W2, W3, W1e, ln_w, ln_b, b2, b3)
    return dict(raw=dict(W2=W2, W3=W3, W1e=W1e, ln_w=ln_w, ln_b=ln_b, b2=b2, b3=b3), K=K, ncond=ncond, B=B, pre=pre, cond=cond, cond_op=None if cond is None else cond.to(bf).float(), wts=wts, vec=vec, mask=mask, u=u,
                plant=plant, underflow=torch.tensor([rw for rw, k in plant.items() if k == "underflow"], dtype=torch.long))


def head_case_refs(c, device=None):
    """reference and yardstick of a per-head case (on `device`), with the bounds the assertions use.  The planted underflow rows
    (logits of +-100) are judged apart from the others: their scale would put a floor of 2^-9 x 100 under every other row's bound."""
    t = (lambda x: x if (x is None or device is None) else x.to(device))
    args = (t(c["pre"]), t(c["cond_op"]), t(c["wts"]), t(c["vec"]), EPS, c["K"], t(c["mask"]))
    ref, yard = head_ref(*args), head_ref(*args, round_bf16=True)
    is_uf = torch.zeros(c["B"], dtype=torch.bool, device=ref["logits"].device)
    is_uf[t(c["underflow"])] = True
    return ref, yard, is_uf


def legal_or_zero(x, mask):
    """x on the legal columns, 0 on the others (logp_all's -inf must not enter a difference)"""
    return torch.where(mask > 0, x, torch.zeros_like(x))


def ambiguous_rows(ref, yard, mask, rows):
    """-> (delta, arg-max [B], ambiguous [B]) over the rows selected by `rows` (bool [B]): delta = the yardstick bound of the logits on
    those rows, ambiguous = the two best legal reference logits closer than 2 delta"""
    delta = whole_bound(ref["logits"][rows], yard["logits"][rows], BF16_FLOOR)[0] if bool(rows.any()) else 0.0
    best, gap = top2_gap(ref["logits"], mask)
    return delta, best, (gap < 2 * delta) & rows


# ------------------------------------------------------------------------------------------------------ inputs: chained mode
CHAIN_BS = (1, 17, 193, 4099, 49153)


def chain_heads(seed=0):
    """the twelve heads of a CatanPolicy whose parameters are perturbed by 0.05 N(0, 1) (decisive heads: the default init's output
    layers are near uniform), as the existing chained test makes them -> the _ActionHeads module, on the CPU in fp32"""
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(seed)
    ahm = CatanPolicy().action_head_module
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in ahm.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return ahm.eval()


def chain_case(B):
    """Synthetic inputs of a pass, drawn on the CPU, so that every branch of the glue runs at a few thousand rows:
    masks [B, 325] random (a row segment of K columns holds about min(K / 2, 2) legal ones: with dozens of legal corners or edges the two best
    logits of the perturbed net are too often closer than the arg-max rule can tell apart) with one sure legal column in every row segment - head 9's four rows share their sure
    column, so its product mask is never empty; forced: types 0..12 uniform on half the rows, -1 on the others; cur_res: hands of 0..3
    per resource (index 0 unused = 0), a quarter of them empty; trade: counts 0..3, a fifth of the entries with a fraction."""
    g = torch.Generator().manual_seed(40009 + B)
    masks = torch.zeros((B, 325))
    r_ = torch.arange(B)
    for h, (off, K) in enumerate(zip(MASK_OFF, HEAD_K)):
        segs = {1: 3, 6: 3, 9: 4}.get(h, 1)
        masks[:, off:off + segs * K] = (torch.rand((B, segs * K), generator=g) < min(0.5, 2.0 / K)).float()
        sure = torch.randint(0, K, (B,), generator=g)
        for s in range(segs):
            if h == 9 or s == 0:
                col = sure
            else:
                col = torch.randint(0, K, (B,), generator=g)
            masks[r_, off + s * K + col] = 1.0
    forced = torch.where(torch.rand(B, generator=g) < 0.5, torch.randint(0, 13, (B,), generator=g), torch.full((B,), -1, dtype=torch.long))
    cur_res = torch.randint(0, 4, (B, 6), generator=g).float()
    cur_res[:, 0] = 0.0
    cur_res[torch.rand(B, generator=g) < 0.25] = 0.0
    trade = torch.randint(0, 4, (B, 12), generator=g).float()
    trade = trade + (torch.rand((B, 12), generator=g) < 0.2).float() * torch.rand((B, 12), generator=g)
    pre_all = (torch.randn((B, 12 * 128), generator=g) * 1.5).to(torch.bfloat16)
    return dict(B=B, masks=masks, forced=forced, cur_res=cur_res, trade=trade, pre_all=pre_all)


# the number of output columns behind each of the 18 action columns
COL_K = tuple(HEAD_K[dict(zip(CHAIN_COL, (h for h, _ in CHAIN_ORDER)))[col]] for col in range(18))


def chain_argmax(c, packs, custom, eps=EPS):
    """the pass's arg-max actions by the fp64 reference itself: chain_ref at A, every column replaced by its evaluation's arg-max
    (column 0 by the forced type where one is given), until A stops changing - a column depends on earlier ones only, so at most 18
    rounds -> (A [B, 18], chain_ref's result at A)"""
    A = torch.zeros((c["B"], 18), dtype=torch.long, device=c["masks"].device)
    for _ in range(19):
        out = chain_ref(A, c["pre_all"], packs, custom, c["masks"], c["cur_res"], c["trade"], c["forced"], eps=eps)
        new = A.clone()
        for e in out["evals"]:
            new[:, e["col"]] = top2_gap(e["logits"], e["mask"])[0]
        new[:, 0] = torch.where(c["forced"] >= 0, c["forced"], new[:, 0])
        if torch.equal(new, A):
            return A, out
        A = new
    raise AssertionError("chain_argmax did not settle")


def chain_ambiguous_shares(c, A, ref, yard):
    """per evaluation, the share of rows the arg-max rule calls ambiguous (head 0: of the rows whose type was not forced) -> 18 floats"""
    shares = []
    for e, ye in zip(ref["evals"], yard["evals"]):
        rows = e["factor"] != 0 if e["head"] == 0 else torch.ones(c["B"], dtype=torch.bool, device=A.device)
        _, _, amb = ambiguous_rows(e, ye, e["mask"], rows)
        shares.append(float(amb.float().sum() / rows.float().sum().clamp(min=1)))
    return shares
