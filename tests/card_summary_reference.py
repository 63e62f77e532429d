"""Reference, yardstick, rule and cases for the dev-card list kernels of csrc/catan_nn.hip (k_card_summary_fwd / _lookup / _bwd and
k_card_pattern_sum; entry points catan_card_summary_fwd / _lookup / _bwd and catan_card_pattern_sum, include/catan_hip_nn.h).  Torch
only, no call into the library, CPU or GPU tensors.

The operation (RL/models/player_modules.py:55-69), per list r of ids a_0 .. a_{pitch-1} with n = min(len, 25) valid tokens, per TOKEN:
    score_h(i, j) = S[h][a_i][a_j]                      S[h][a][b] = q_h(a) . k_h(b) / sqrt(hd) of the embedded ids a, b
    p_h(i, .)     = softmax over the keys j < n         (key mask; the queries are not masked)
    attn(i)       = concat_h sum_j p_h(i, j) V[a_j][h]
    o(i)          = W attn(i) + bo;   rep(i) = LayerNorm_16(o(i)) * ln_w + ln_b
    out[r]        = sum over i < n of rep(i)            (rows i >= n are zeroed before the sum; n = 0: a zero row, no gradient)
`params` is the 544-float block the kernels read: S[4][6][6], V[6][16], W[16][16], bo[16], ln_w[16], ln_b[16] (params_from_weights
restates nn_kernels.card_summary_params).

    card_ref_tokens   the REFERENCE: exactly the lines above in fp64, token by token, gradients by autograd in double.  It never counts
                      ids and never forms a class: that algebra is what the kernels do and what is under test.
    card_ref_classes  the same value in fp64 in the class form (softmax over the ids b of S[h][a][b] + log count_b, count_a * rep(a) summed
                      over the classes) with a closed-form backward.  It exists for `abs_terms`: per parameter the sum over (list, query
                      class) of |contribution|, which the summation bound needs.  tests/test_card_summary_reference_cpu.py holds it to
                      card_ref_tokens at 1e-12.
    card_yardstick    the class form in fp32 in the kernels' order: maximum subtracted, exp, sum, 1 / sum multiplied in; dot products
                      term by term in index order; mean * (1/16), two-pass variance, rsqrt; count * rep accumulated over the classes 0..5.
                      torch's accurate exp / log (the kernels use __expf / __logf: what that costs has to fit under the floor).  Each
                      (list, class) contribution of the backward is rounded to fp32, their SUM is taken in fp64: the yardstick carries the
                      per-term rounding, the depth term of the rule carries the summation.  `plant=` swaps in one planted error (PLANTS).

Rule (tests/pin_rule.py; nothing in a bound comes from a kernel):
    out       pin_rule.whole with floor 2^-17 over the case (accept_out) AND pin_rule.per_group per list (per_list: the list's own
              yardstick error and scale)
    dparams   pin_rule.accept_sum per parameter: |kernel - (pre-fill + fp64)| <= 2 |yardstick - fp64| + depth 2^-24 (abs_terms +
              |pre-fill|), depth = bwd_depth
    dpat      per word |kernel - fp64| <= sum_depth 2^-24 sum |term|; with dout = small integers times a power of two every sum is exact
    keys      == pattern_of(counts), lookup == forward, bit for bit"""
import math

import torch

import pin_rule as PR

VOCAB, HEADS, HD, WIDTH, MAXLEN = 6, 4, 4, 16, 25
NPAR = 544
OFF_S, OFF_V, OFF_W, OFF_BO, OFF_LW, OFF_LB = 0, 144, 240, 496, 512, 528
SLICES = {"S": (0, 144), "V": (144, 240), "W": (240, 496), "bo": (496, 512), "ln_w": (512, 528), "ln_b": (528, 544)}
EPS = 1e-5
DECK = (1, 14, 5, 2, 2, 2)                    # the most a real list holds of ids 0..5 (id 0: the placeholder of an empty list)
PATTERNS = 2 * 15 * 6 * 3 * 3 * 3             # 4 860
OUT_FLOOR = 2.0 ** -17
PLANTS = ("no_log_count", "no_count_weight", "len_plus_1", "padding_counted", "absent_class_kept", "mean_15", "eps_outside", "ds_no_dot",
          "dv_wrong_head", "dln_w_ungated_by_count", "radix_c2_5", "replica_dropped")
REGIMES = ("unit", "saturated", "flat")


# --------------------------------------------------------------------------------------------------------------- the parameter block
def params_from_weights(emb, wqkv, bqkv, wo, bo, ln_w, ln_b):
    """nn_kernels.card_summary_params' expression in the dtype of its arguments: emb [6, 16], wqkv [48, 16] (q, k, v nets stacked),
    bqkv [48] -> [544]"""
    qkv = torch.nn.functional.linear(emb, wqkv, bqkv).view(VOCAB, 3, HEADS, HD)
    s_ab = torch.einsum("ahd,bhd->hab", qkv[:, 0], qkv[:, 1]) * (1.0 / math.sqrt(HD))
    return torch.cat((s_ab.reshape(-1), qkv[:, 2].reshape(-1), wo.reshape(-1), bo, ln_w, ln_b))


def split(p):
    return (p[OFF_S:OFF_V].view(HEADS, VOCAB, VOCAB), p[OFF_V:OFF_W].view(VOCAB, WIDTH), p[OFF_W:OFF_BO].view(WIDTH, WIDTH), p[OFF_BO:OFF_LW],
            p[OFF_LW:OFF_LB], p[OFF_LB:NPAR])


# ------------------------------------------------------------------------------------------------------------------------- reference
def card_ref_tokens(ids, lens, emb, wqkv, bqkv, wo, bo, ln_w, ln_b, eps, dout, params=None, chunk=2048):
    """The REFERENCE (module docstring), token by token in fp64.  ids [rows, pitch] integers in 0..5, lens [rows], dout [rows, 16] or
    None.  The block is built from the module weights in double by params_from_weights, or, with `params` (the fp32 block a kernel
    was given; the weights may then be None), is that block in double.  -> {out [rows, 16], dparams [544], dweights (the seven
    weights' gradients, through the block; None with `params`)}, all fp64."""
    dev = ids.device
    grad = dout is not None
    leaves = None
    if params is None:
        leaves = [t.detach().to(dev).double().requires_grad_(grad) for t in (emb, wqkv, bqkv, wo, bo, ln_w, ln_b)]
        built = params_from_weights(*leaves)
        p = built.detach().clone().requires_grad_(grad)
    else:
        p = params.detach().to(dev).double().clone().requires_grad_(grad)
    rows, pitch = ids.shape
    Lq = min(MAXLEN, pitch)
    out = torch.empty((rows, WIDTH), dtype=torch.float64, device=dev)
    pos = torch.arange(Lq, device=dev)
    for c0 in range(0, rows, chunk):
        c1 = min(rows, c0 + chunk)
        a = ids[c0:c1, :Lq].long()
        n = lens[c0:c1].long().clamp(min=0, max=MAXLEN)
        S, Vt, W, b_o, lw, lb = split(p)
        valid = pos[None, :] < n[:, None]                                              # [m, Lq]
        keys = valid | (n == 0)[:, None]                                               # (an empty list: keep the softmax finite, its rows are zeroed)
        sc = S[:, a[:, :, None], a[:, None, :]]                                        # [H, m, Lq(i), Lq(j)] = S[h][a_i][a_j]
        pr = torch.softmax(sc.masked_fill(~keys[None, :, None, :], float("-inf")), -1)
        v = Vt[a].view(c1 - c0, Lq, HEADS, HD)
        attn = torch.einsum("hmij,mjhd->mihd", pr, v).reshape(c1 - c0, Lq, WIDTH)
        o = attn @ W.t() + b_o
        mean = o.mean(-1, keepdim=True)
        var = ((o - mean) ** 2).mean(-1, keepdim=True)
        rep = (o - mean) / torch.sqrt(var + eps) * lw + lb
        oc = torch.where(valid[:, :, None], rep, torch.zeros_like(rep)).sum(1)
        out[c0:c1] = oc.detach()
        if grad:
            (oc * dout[c0:c1].to(dev).double()).sum().backward()
    res = {"out": out, "dparams": None, "dweights": None}
    if grad:
        res["dparams"] = p.grad.clone() if p.grad is not None else torch.zeros_like(p)
        if leaves is not None:
            built.backward(res["dparams"])
            res["dweights"] = [t.grad.clone() for t in leaves]
    return res


def counts(ids, lens, plant=None):
    """valid tokens per id -> int64 [rows, 6].  len_plus_1 / padding_counted: the planted readers of what lies behind `lens`"""
    rows, pitch = ids.shape
    Lq = min(MAXLEN, pitch)
    n = lens.long().clamp(min=0, max=MAXLEN)
    if plant == "len_plus_1":
        n = (n + 1).clamp(max=Lq)
    if plant == "padding_counted":
        n = torch.full_like(n, Lq)
    valid = torch.arange(Lq, device=ids.device)[None, :] < n[:, None]
    a = ids[:, :Lq].long()
    return torch.stack([((a == c) & valid).sum(1) for c in range(VOCAB)], 1)


def _seq_sum(t, dim=-1):
    """t summed along `dim` term by term in index order (the kernels' accumulation loops)"""
    parts = t.unbind(dim)
    acc = parts[0]
    for x in parts[1:]:
        acc = acc + x
    return acc


def _class_form(cnt, prm, eps, dy, T, plant=None):
    """The class form in dtype T over the lists of `cnt` (int64 [m, 6]) -> (out [m, 16] T, g, g_abs): g / g_abs [544] fp64 = the sum
    over (list, query class) of the contributions (each formed in T) / of their absolute values; None without dy."""
    m = cnt.shape[0]
    S, Vt, W, b_o, lw, lb = split(prm.to(T))
    c = cnt.to(T)
    present = c > 0
    ninf = torch.full_like(c, float("-inf"))
    logc = torch.where(present, torch.log(c.clamp_min(1.0)), ninf)
    if plant == "no_log_count":
        logc = torch.where(present, torch.zeros_like(c), ninf)
    if plant == "absent_class_kept":
        logc = torch.where(present, logc, torch.zeros_like(c))
    logc = torch.where(present.any(1, keepdim=True), logc, torch.zeros_like(c))         # (an empty list: finite, weighted by count 0 below)
    z = S[None] + logc[:, None, None, :]                                               # [m, H, a, b]
    e = torch.exp(z - z.amax(-1, keepdim=True))
    p = e * (1.0 / _seq_sum(e))[..., None]
    ph = p.permute(0, 2, 1, 3)                                                         # [m, a, H, b]
    Vh = Vt.view(VOCAB, HEADS, HD)                                                     # [b, H, d]
    attn = _seq_sum(ph[..., None] * Vh.permute(1, 0, 2)[None, None], 3).reshape(m, VOCAB, WIDTH)      # [m, a, H, b, d] over b
    o = b_o.expand(m, VOCAB, WIDTH)
    for j in range(WIDTH):
        o = o + W[:, j][None, None, :] * attn[:, :, j:j + 1]
    mean = _seq_sum(o) * (1.0 / (15 if plant == "mean_15" else 16))
    ctr = o - mean[..., None]
    var = _seq_sum(ctr * ctr)
    if plant == "eps_outside":
        rstd = 1.0 / (torch.sqrt(var * (1.0 / 16)) + eps)
    else:
        rstd = torch.rsqrt(var * (1.0 / 16) + eps)
    xh = ctr * rstd[..., None]
    rep = xh * lw + lb
    wgt = present.to(T) if plant == "no_count_weight" else c
    out = torch.zeros((m, WIDTH), dtype=T, device=cnt.device)
    for a in range(VOCAB):
        out = out + wgt[:, a, None] * rep[:, a]
    if dy is None:
        return out, None, None
    dy = dy.to(T)
    dr = wgt[:, :, None] * dy[:, None, :]                                              # [m, a, 16]
    g_lb = dr
    g_lw = (dy[:, None, :] * xh) if plant == "dln_w_ungated_by_count" else dr * xh
    dxh = dr * lw
    m1 = _seq_sum(dxh) * (1.0 / 16)
    m2 = _seq_sum(dxh * xh) * (1.0 / 16)
    d_o = rstd[..., None] * (dxh - m1[..., None] - xh * m2[..., None])
    g_W = d_o[..., :, None] * attn[..., None, :]                                       # [m, a, i, j]
    dattn = _seq_sum(d_o[..., :, None] * W[None, None], 2)                             # over i -> [m, a, j]
    dat = dattn.view(m, VOCAB, HEADS, HD)
    pv = ph.roll(1, 2) if plant == "dv_wrong_head" else ph
    g_V = (pv[..., None] * dat[:, :, :, None, :]).permute(0, 1, 3, 2, 4)               # [m, a, H, b, d] -> [m, a, b, H, d]
    dp = _seq_sum(dat[:, :, :, None, :] * Vh.permute(1, 0, 2)[None, None], -1)         # [m, a, H, b]
    dot = _seq_sum(ph * dp)
    g_S = ph * (dp if plant == "ds_no_dot" else dp - dot[..., None])                   # [m, a, H, b]: lands in S[h][a][b], nowhere else

    def total(f):
        return torch.cat((f(g_S).double().sum(0).permute(1, 0, 2).reshape(-1), f(g_V).double().sum((0, 1)).reshape(-1),
                          f(g_W).double().sum((0, 1)).reshape(-1), f(d_o).double().sum((0, 1)), f(g_lw).double().sum((0, 1)),
                          f(g_lb).double().sum((0, 1))))
    return out, total(lambda t: t), total(torch.abs)


def _chunked(ids, lens, params, eps, dout, T, plant, chunk):
    cnt = counts(ids, lens, plant)
    rows = cnt.shape[0]
    out = torch.empty((rows, WIDTH), dtype=T, device=ids.device)
    g = torch.zeros(NPAR, dtype=torch.float64, device=ids.device)
    ga = torch.zeros_like(g)
    for c0 in range(0, rows, chunk):
        c1 = min(rows, c0 + chunk)
        o, gc, gac = _class_form(cnt[c0:c1], params.to(ids.device), eps, None if dout is None else dout[c0:c1].to(ids.device), T, plant)
        out[c0:c1] = o
        if gc is not None:
            g += gc
            ga += gac
    return out, g, ga


def card_ref_classes(ids, lens, params, eps, dout, chunk=4096):
    """the class form in fp64 -> {out [rows, 16], dparams [544], abs_terms [544]} (module docstring)"""
    out, g, ga = _chunked(ids, lens, params.double(), eps, dout, torch.float64, None, chunk)
    return {"out": out, "dparams": g if dout is not None else None, "abs_terms": ga if dout is not None else None}


def card_yardstick(ids, lens, params, eps, dout, plant=None, chunk=4096):
    """the class form in fp32 in the kernels' order -> {out fp32 [rows, 16], dparams fp64 [544] (a sum of fp32 terms)}"""
    out, g, _ = _chunked(ids, lens, params.float(), eps, dout, torch.float32, plant, chunk)
    return {"out": out, "dparams": g if dout is not None else None}


# -------------------------------------------------------------------------------------------------------------------------- patterns
def pattern_of(cnt, plant=None):
    """cs_pattern: int64 [rows, 6] counts -> the pattern number, -1 outside the deck.  radix_c2_5: the planted radix error"""
    c = [cnt[:, i].long() for i in range(VOCAB)]
    inside = torch.ones_like(c[0], dtype=torch.bool)
    for i in range(VOCAB):
        inside &= c[i] <= DECK[i]
    r2 = 5 if plant == "radix_c2_5" else 6
    key = c[0] + 2 * (c[1] + 15 * (c[2] + r2 * (c[3] + 3 * (c[4] + 3 * c[5]))))
    return torch.where(inside, key, torch.full_like(key, -1))


def pattern_counts():
    """the header's formula: pattern k has counts c0 = k % 2, c1 = k / 2 % 15, c2 = k / 30 % 6, c3 = k / 180 % 3, c4 = k / 540 % 3,
    c5 = k / 1620 -> int64 [4860, 6]"""
    k = torch.arange(PATTERNS)
    return torch.stack((k % 2, k // 2 % 15, k // 30 % 6, k // 180 % 3, k // 540 % 3, k // 1620), 1)


def pattern_lists(live_padding_seed=None):
    """nn_kernels._pattern_lists restated: (ids int8 [4860, 25], lens int32 [4860]); list k holds its counts' ids in ascending order.
    The one pattern of 26 cards (every count at the deck's limit) is cut to its first 25 ids.  The padding is zero as there, or, with
    a seed, live ids 1..5."""
    cnt = pattern_counts()
    total = cnt.sum(1)
    edges = cnt.cumsum(1)                                                              # [P, 6]
    pos = torch.arange(MAXLEN)
    ids = (pos[None, :, None] >= edges[:, None, :]).sum(-1)                            # the id at position i: how many classes end at or before i
    valid = pos[None, :] < total[:, None]
    if live_padding_seed is None:
        pad = torch.zeros_like(ids)
    else:
        pad = torch.randint(1, VOCAB, ids.shape, generator=torch.Generator().manual_seed(live_padding_seed))
    ids = torch.where(valid, ids.clamp(max=VOCAB - 1), pad)
    return ids.to(torch.int8), total.clamp(max=MAXLEN).to(torch.int32)


# --------------------------------------------------------------------------------------------------------------- launches and depths
BWD_RPL_FROM = 65536
SUM_ROWS, SUM_SLOTS, SUM_PROBES = 1024, 512, 16


def bwd_launch(rows):
    """catan_card_summary_bwd's host rule -> {rpl, nb, row_blocks, grid}"""
    rpl = 4 if rows >= BWD_RPL_FROM else 1
    nb = (rows + 256 * rpl - 1) // (256 * rpl)
    row_blocks = nb if rows < BWD_RPL_FROM else 0
    return {"rpl": rpl, "nb": nb, "row_blocks": row_blocks, "grid": ((VOCAB * nb if row_blocks else nb), 7)}


def sum_launch(rows, replicas):
    """k_card_pattern_sum -> {workgroups, copy_of (workgroup -> the copy it writes), per_copy (the most workgroups on one copy)}"""
    wgs = (rows + SUM_ROWS - 1) // SUM_ROWS
    return {"workgroups": wgs, "copy_of": [b % replicas for b in range(wgs)], "per_copy": (wgs + replicas - 1) // replicas}


def bwd_depth(rows):
    """the longest chain of fp32 additions one parameter's word can see: a lane's lists times the classes it walks for them, 6 shuffle
    levels, 4 waves on the LDS word, the workgroups that add to the global word (rpl = 1: a workgroup per query class and row block,
    and all six classes reach every parameter outside S), the pre-fill"""
    la = bwd_launch(rows)
    per_lane = la["rpl"] * (1 if la["row_blocks"] else VOCAB)
    return per_lane + 6 + 4 + la["grid"][0] + 1


def sum_depth(rows, replicas, shared=None):
    """the same for one word of one copy of dpat: the rows of a workgroup that share a key (`shared`; at worst all of them) on the LDS
    word or, after the probes, on the global one, and one addition per workgroup of the copy"""
    shared = min(rows, SUM_ROWS) if shared is None else shared
    return shared + sum_launch(rows, replicas)["per_copy"]


def hash_slot(key):
    """k_card_pattern_sum's first slot of a key (python int or int64 tensor)"""
    return ((key * 2654435761) % (1 << 32)) >> 23


def window_keys(start=6, width=8):
    """the patterns whose first slot lies in [start, start + width): their 16 probes stay inside width + 15 slots"""
    k = torch.arange(PATTERNS)
    s = hash_slot(k)
    return k[((s - start) % SUM_SLOTS) < width]


def provable_fallback_rows(keys):
    """a lower bound, whatever the race order, on the rows of `keys` (int [rows], -1 = no key) that cannot have found a slot: per
    workgroup of 1 024 rows the distinct keys beyond 512, or beyond the width + 15 slots that the keys starting in one window of
    `width` can reach, hold no slot, and every row of such a key goes to global memory.  The bound takes the keys with the fewest rows."""
    total = 0
    for c0 in range(0, keys.numel(), SUM_ROWS):
        k = keys[c0:c0 + SUM_ROWS].long().cpu()
        k = k[k >= 0]
        if k.numel() == 0:
            continue
        uniq, n = torch.unique(k, return_counts=True)
        m = max(0, uniq.numel() - SUM_SLOTS)
        per_slot = torch.zeros(SUM_SLOTS, dtype=torch.long).index_add_(0, hash_slot(uniq), torch.ones_like(uniq))
        two = torch.cat((per_slot, per_slot))
        run = two.cumsum(0)
        for width in (1, 2, 4, 8, 16, 32):
            inside = run[width - 1:] - torch.cat((torch.zeros(1, dtype=torch.long), run[:-width]))
            m = max(m, int(inside.max()) - (width + SUM_PROBES - 1))
        total += int(n.sort().values[:m].sum())
    return total


def pattern_sum_ref(keys, dout, replicas, plant=None):
    """dpat in fp64 -> (copies [replicas, 4860, 16], their sum [4860, 16], abs [4860, 16] = sum |term| per word, unkeyed rows).
    replica_dropped: the planted caller that leaves the last copy out of the sum"""
    keys = keys.long()
    rows = keys.numel()
    dev = keys.device
    keyed = keys >= 0
    r = torch.arange(rows, device=dev)[keyed]
    copy = (r // SUM_ROWS) % replicas
    flat = copy * PATTERNS + keys[keyed]
    d = dout[keyed].double()
    copies = torch.zeros((replicas * PATTERNS, WIDTH), dtype=torch.float64, device=dev).index_add_(0, flat, d).view(replicas, PATTERNS, WIDTH)
    ab = torch.zeros((PATTERNS, WIDTH), dtype=torch.float64, device=dev).index_add_(0, keys[keyed], d.abs())
    summed = (copies[:-1] if plant == "replica_dropped" and replicas > 1 else copies).sum(0)
    return copies, summed, ab, int((~keyed).sum())


# ------------------------------------------------------------------------------------------------------------------------------ rule
def accept_out(kernel, ref, yard):
    """pin_rule.whole for `out` with its floor -> (ok, kernel error, yardstick error, bound)"""
    return PR.whole(kernel, ref, yard, OUT_FLOOR)


def per_list(kernel, ref, yard):
    """pin_rule.per_group with that floor: every list with ITS yardstick error and ITS scale -> (ok [rows], kernel error [rows], bound [rows])"""
    return PR.per_group(kernel, ref, yard, OUT_FLOOR)


# ----------------------------------------------------------------------------------------------------------------------------- cases
def make_weights(seed):
    """a CatanPolicy-sized module as initialised (nn.Embedding: N(0, 1); nn.Linear(16, 16): U(+-1/4); LayerNorm: 1, 0) plus 0.1 noise
    -> (emb, wqkv, bqkv, wo, bo, ln_w, ln_b) fp32"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.25
    w = [torch.randn(VOCAB, WIDTH, generator=g), u(3 * WIDTH, WIDTH), u(3 * WIDTH), u(WIDTH, WIDTH), u(WIDTH), torch.ones(WIDTH), torch.zeros(WIDTH)]
    return tuple(t + 0.1 * torch.randn(t.shape, generator=g) for t in w)


def make_params(regime, seed=0):
    """-> (params fp32 [544], weights or None)
    unit       make_weights through params_from_weights in fp32, as nn_kernels builds the block
    saturated  the unit block with S replaced: per (head, query class) one key class at +30, the others at -30 + U(-2, 2) - where
               the dominant class is in the list its argument is exactly 0 and the others sit near -60; where it is not, the rest compete
    flat       W = 0, bo constant, ln_b = k / 8: every class's o is constant, xhat = 0 exactly, rep = ln_b, out = len * ln_b to the bit"""
    weights = make_weights(seed)
    p = params_from_weights(*weights).clone()
    if regime == "unit":
        return p, weights
    g = torch.Generator().manual_seed(seed + 77)
    if regime == "saturated":
        h = torch.arange(HEADS)[:, None, None]
        a = torch.arange(VOCAB)[None, :, None]
        b = torch.arange(VOCAB)[None, None, :]
        S = torch.where(b == (a + h) % VOCAB, torch.full((HEADS, VOCAB, VOCAB), 30.0), -30.0 + (torch.rand(HEADS, VOCAB, VOCAB, generator=g) * 4 - 2))
        p[OFF_S:OFF_V] = S.reshape(-1)
    elif regime == "flat":
        p[OFF_W:OFF_BO] = 0.0
        p[OFF_BO:OFF_LW] = 0.5
        p[OFF_LB:NPAR] = torch.randint(-8, 9, (WIDTH,), generator=g).float() / 8
    else:
        raise ValueError(regime)
    return p, None


LIST_KINDS = ("deck", "arbitrary", "single", "edge")


def make_lists(kind, rows, pitch=25, seed=0):
    """-> (ids int64 [rows, pitch] in 0..5, lens int64 [rows]).  Every position at or behind min(len, 25) holds a live id 1..5
    (never zeros): read by mistake it changes the counts.
    deck        a shuffled deck's prefix of a random length 0..min(25, pitch) (keyed); every tenth list begins with the placeholder 0
    arbitrary   ids 0..5 at random, any length (mostly outside the deck)
    single      class r % 6 with count 1 + (r / 6) % min(25, pitch)
    edge        len cycles through 0, 1, 2, 24, 25 and 30 (pitch < 25: 0, 1, 2, pitch - 1, pitch), deck prefixes and arbitrary ids in turn
    mixed       the four in turn"""
    g = torch.Generator().manual_seed(seed * 1000 + rows * 7 + pitch)
    Lq = min(MAXLEN, pitch)
    r = torch.arange(rows)
    deck = torch.tensor([1] * 14 + [2] * 5 + [3] * 2 + [4] * 2 + [5] * 2)
    dealt = deck[torch.rand(rows, 25, generator=g).argsort(1)]
    dealt = torch.cat((dealt, dealt[:, :max(0, pitch - 25)]), 1)[:, :pitch]
    dealt[r % 10 == 3, 0] = 0
    anyid = torch.randint(0, VOCAB, (rows, pitch), generator=g)
    anylen = torch.randint(0, Lq + 1, (rows,), generator=g)
    cyc = torch.tensor((0, 1, 2, 24, 25, 30) if pitch >= 25 else (0, 1, 2, pitch - 1, pitch, pitch))
    single = (r % VOCAB)[:, None].expand(rows, pitch)
    per = {"deck": (dealt, anylen), "arbitrary": (anyid, torch.where(r % 3 == 0, anylen, anylen.clamp(min=Lq - 5))),
           "single": (single, 1 + (r // VOCAB) % Lq), "edge": (torch.where((r % 2 == 0)[:, None], dealt, anyid), cyc[(r // 4) % 6])}
    if kind == "mixed":
        which = r % 4
        ids = torch.zeros((rows, pitch), dtype=torch.long)
        lens = torch.zeros(rows, dtype=torch.long)
        for i, k in enumerate(LIST_KINDS):
            ids = torch.where((which == i)[:, None], per[k][0], ids)
            lens = torch.where(which == i, per[k][1], lens)
    else:
        ids, lens = per[kind]
    live = torch.randint(1, VOCAB, (rows, pitch), generator=g)
    ids = torch.where(torch.arange(pitch)[None, :] < lens.clamp(max=MAXLEN)[:, None], ids, live)
    return ids.contiguous(), lens.contiguous()


def make_dout(rows, seed=0, exact=False):
    """normal fp32, or (exact) small integers times 2^-4: every sum of fewer than 2^19 of them is exact in fp32 in any order"""
    g = torch.Generator().manual_seed(seed * 31 + rows)
    if exact:
        return torch.randint(-8, 9, (rows, WIDTH), generator=g).float() / 16
    return torch.randn(rows, WIDTH, generator=g)
