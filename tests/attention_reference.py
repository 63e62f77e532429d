"""Plain-torch restatement of the small-sequence attention of csrc/catan_nn.hip (catan_attention_fwd / catan_attention_bwd), with the
seeded case builders that tests/test_attention_reference_cpu.py and tests/test_gpu_attention_fp64.py share.  No call into the library
or into nn_kernels: torch ops only, on the CPU or the GPU, written from include/catan_hip_nn.h and the reference formulation
multi_headed_attention.py:25-36 as policy._MHA._forward's torch branch states it:
    S = Q K^T / sqrt(HD), keys j >= lens[b] at -inf       P = softmax_j(S)       O = P V           (per sequence b and head h)
and, closed form, with dO the gradient of O:
    dV = P^T dO      dP = dO V^T      delta_i = sum_j P_ij dP_ij      dS = P * (dP - delta)      dQ = dS K / sqrt(HD)      dK = dS^T Q / sqrt(HD)
The mask is a KEY mask only: a query row i >= lens[b] still attends to the keys < lens[b] and its output and gradients are defined.
lens[b] >= 1 (include/catan_hip_nn.h): a sequence without keys has no softmax.

qkv [B, L, 3, H, HD]; lens int [B] or None; dout [B, L, H * HD] -> {out, dq, dk, dv}, [B, L, H * HD] each (dq | dk | dv are the three
slices of the kernel's dqkv [B, L, 3, H * HD]).

  attention_ref        the REFERENCE: fp64 throughout from the inputs as stored (bf16 inputs upcast exactly).
  attention_yardstick  fp32, with a round-to-bf16 exactly where the kernel of `path` rounds.  It shows what the number formats cost
                       against the reference; it is not an oracle.
    path "mfma"       k_attn_mfma_fwd / k_attn_mfma_bwd (bf16, 16-byte aligned buffers).  Scores are fp32 MFMA sums of bf16 products.
                      forward : e = 2^((s - max) C), C = log2(e) / sqrt(HD), fp32; the row sum is taken over the UNROUNDED e; the
                                unnormalised e is rounded to bf16 as the operand of P.V; 1 / sum is applied to the fp32 product; the
                                output is rounded on store.
                      backward: p = e / sum in fp32; delta from the unrounded p and the fp32 dP; for dV the normalised p is rounded to
                                bf16; for dQ and dK the product p (dP - delta) - BEFORE the 1 / sqrt(HD) factor, a power of two applied
                                to the fp32 sums afterwards - is rounded to bf16; dQ, dK and dV are rounded on store.
    path "valu_bf16"  k_attn_fwd / k_attn_bwd on bf16 buffers that are not 16-byte aligned: fp32 throughout, rounded only on store
                      (out; dq, dk, dv).
    path "fp32"       k_attn_fwd / k_attn_bwd on float32: plain fp32, no rounding - the error of fp32 arithmetic itself.

Acceptance of a kernel output is the rule of tests/pin_rule.py with the floor of the path: pin_rule.BF16_FLOOR on the bf16 paths, the fp32
floors below on the fp32 path.  `accept` applies it to a whole tensor, `per_sequence` to every sequence with that sequence's own yardstick
error and scale."""
import math

import torch

from pin_rule import BF16_FLOOR, per_group, whole

SHAPES = ((19, 4, 16), (25, 4, 4))
PATHS = ("mfma", "valu_bf16", "fp32")
OUTPUTS = ("out", "dq", "dk", "dv")
FP32_FLOOR = {"out": 2.0 ** -17, "dq": 2.0 ** -15, "dk": 2.0 ** -15, "dv": 2.0 ** -15}
LOG2E = 1.44269504088896340736
# the batch sizes of the GPU tests: the MFMA kernels take 4 sequences per block, the VALU kernels 3 (L = 19) or 2 (L = 25)
MFMA_BS = (1, 2, 3, 4, 5, 7, 8, 9)
VALU_BS = (1, 2, 3, 4, 5, 6, 7)
MULTI_B = 1030


def path_dtype(path):
    return torch.float32 if path == "fp32" else torch.bfloat16


def _split(qkv, dout, wd):
    """-> q, k, v, do as [B, H, L, HD] of dtype wd"""
    B, L, three, H, HD = qkv.shape
    assert three == 3 and tuple(dout.shape) == (B, L, H * HD)
    q, k, v = qkv.to(wd).permute(2, 0, 3, 1, 4)
    return q, k, v, dout.to(wd).view(B, L, H, HD).transpose(1, 2)


def _merge(t):
    """[B, H, L, HD] -> [B, L, H * HD]"""
    B, H, L, HD = t.shape
    return t.transpose(1, 2).reshape(B, L, H * HD)


def _key_mask(lens, B, L, device):
    """[B, 1, 1, L] bool, True = the key takes part"""
    if lens is None:
        return torch.ones((B, 1, 1, L), dtype=torch.bool, device=device)
    assert lens.shape == (B,) and int(lens.min()) >= 1
    return (torch.arange(L, device=device)[None, :] < lens.to(device)[:, None])[:, None, None, :]


def attention_ref(qkv, lens, dout):
    q, k, v, do = _split(qkv, dout, torch.float64)
    B, H, L, HD = q.shape
    scale = 1.0 / math.sqrt(HD)
    s = (q @ k.transpose(-2, -1)) * scale
    s = s.masked_fill(~_key_mask(lens, B, L, s.device), float("-inf"))
    p = torch.softmax(s, -1)
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return {"out": _merge(p @ v), "dq": _merge(ds @ k) * scale, "dk": _merge(ds.transpose(-2, -1) @ q) * scale, "dv": _merge(p.transpose(-2, -1) @ do)}


def _row_max(s, max_keys, half_max):
    """the subtracted row maximum; with the two planted errors of the sensitivity test: over keys 0 .. max_keys - 1 only / each key with
    the maximum of the keys of its own lane half (j & 4), which the MFMA kernels would use without their exchange across the halves"""
    if half_max:
        up = (torch.arange(s.shape[-1], device=s.device) & 4) != 0
        neg = float("-inf")
        return torch.where(up, s.masked_fill(~up, neg).amax(-1, keepdim=True), s.masked_fill(up, neg).amax(-1, keepdim=True))
    return (s if max_keys is None else s[..., :max_keys]).amax(-1, keepdim=True)


def attention_yardstick(qkv, lens, dout, path, max_keys=None, half_max=False):
    """max_keys, half_max: NOT part of the yardstick - two planted errors of the sensitivity test (_row_max).  The first exists in finite
    precision only (in exact arithmetic a constant subtracted from a whole row cancels)."""
    assert path in PATHS
    f32 = torch.float32
    r = (lambda t: t.to(torch.bfloat16).to(f32)) if path != "fp32" else (lambda t: t)
    q, k, v, do = _split(qkv, dout, f32)
    B, H, L, HD = q.shape
    scale = 1.0 / math.sqrt(HD)
    mask = _key_mask(lens, B, L, q.device)
    dp = do @ v.transpose(-2, -1)
    if path == "mfma":
        C = scale * LOG2E
        s = (q @ k.transpose(-2, -1)).masked_fill(~mask, float("-inf"))
        mx = _row_max(s, max_keys, half_max)
        e = torch.exp2(s * C - mx * C)
        inv = 1.0 / e.sum(-1, keepdim=True)
        out = r((r(e) @ v) * inv)
        p = e * inv
        dsu = p * (dp - (p * dp).sum(-1, keepdim=True))                   # dS / scale
        return {"out": _merge(out), "dq": _merge(r((r(dsu) @ k) * scale)), "dk": _merge(r((r(dsu).transpose(-2, -1) @ q) * scale)),
                "dv": _merge(r(r(p).transpose(-2, -1) @ do))}
    s = ((q @ k.transpose(-2, -1)) * scale).masked_fill(~mask, float("-inf"))
    mx = _row_max(s, max_keys, half_max)
    e = torch.exp(s - mx)
    p = e * (1.0 / e.sum(-1, keepdim=True))
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    return {"out": _merge(r(p @ v)), "dq": _merge(r(ds @ k)), "dk": _merge(r(ds.transpose(-2, -1) @ q)), "dv": _merge(r(p.transpose(-2, -1) @ do))}


# ------------------------------------------------------------------------------------------------------------------------ rule
def path_floor(path, name):
    return FP32_FLOOR[name] if path == "fp32" else BF16_FLOOR


def accept(path, name, kernel, ref, yardstick):
    """pin_rule.whole with the floor of `path` for output `name` -> (ok, kernel error, yardstick error, bound)"""
    return whole(kernel, ref, yardstick, path_floor(path, name))


def per_sequence(path, name, kernel, ref, yardstick):
    """pin_rule.per_group with that floor: every sequence b with ITS yardstick error and ITS scale -> (ok [B], kernel error [B], bound [B])"""
    return per_group(kernel, ref, yardstick, path_floor(path, name))


# ----------------------------------------------------------------------------------------------------------------------- cases
def length_cycle(L):
    """the key counts the tests cycle over: 1, 2; 3, 4, 5 (the first 4-key register group and the step into the second lane half); 7, 8,
    9; 11, 12, 13; 15, 16, 17 (the k-step boundary); L - 1, L; for L = 25 also 19 .. 21 and 23 .. 25.  Keys sit in the MFMA kernels'
    registers as j = (r & 3) + 8 (r >> 2) + 4 hf."""
    base = [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, L - 1, L]
    if L == 25:
        base += [19, 20, 21, 23, 24, 25]
    return sorted(set(base))


def case_lens(L, B, start=0):
    """lens[b] = length_cycle(L)[(start + b) % n], int32"""
    cyc = length_cycle(L)
    return torch.tensor([cyc[(start + b) % len(cyc)] for b in range(B)], dtype=torch.int32)


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def _scaled(g, shape, H, HD, s_lo, s_hi, o_amp):
    """randn with a scale and an offset of its own for every (head, dim): nothing in the result is symmetric under a swap of heads,
    of dims, or of two of the four tensors"""
    sc = s_lo + (s_hi - s_lo) * torch.rand((H, HD), generator=g)
    of = o_amp * (2.0 * torch.rand((H, HD), generator=g) - 1.0)
    return torch.randn(shape, generator=g) * sc + of


def saturated_targets(L, H, lens, B):
    """[B, H, L] long: the key t that query i of head h gets its row maximum on.  Even queries take a key of the UPPER lane half of the
    MFMA kernels' key registers ((j & 4) != 0), odd queries one of the LOWER half, both from the sequence's last keys downwards (so the
    keys behind the k-step boundary and the last key are among them); a sequence of at most 4 keys has lower keys only.  The PROBE
    queries (probe_rows) take one of the keys 16 .. 18, lower ones, as an odd query does."""
    probes = probe_rows(L, lens, B)
    n_all = torch.full((B,), L) if lens is None else lens.long()
    table = {}
    for n in sorted(set(n_all.tolist())):                          # the pattern depends on the key count only
        lower = [j for j in range(n - 1, -1, -1) if not j & 4]
        upper = [j for j in range(n - 1, -1, -1) if j & 4] or lower
        plain = torch.tensor([[(lower if i & 1 else upper)[(i // 2 + h) % len(lower if i & 1 else upper)] for i in range(L)] for h in range(H)])
        probe = torch.tensor([[16 + (i // 2 + h) % max(1, min(n - 16, 3)) for i in range(L)] for h in range(H)])
        table[n] = (plain, probe)
    plain = torch.stack([table[n][0] for n in n_all.tolist()])
    probe = torch.stack([table[n][1] for n in n_all.tolist()])
    return torch.where(probes[:, None, :], probe, plain)


def soft_rows(L):
    """[L] bool: the queries 5, 13, 21 of the saturated case, drawn as in the unit case.  Against keys of norm kappa their scores are
    some +-10: an ordinary softmax in every sequence.  Without them a sequence of 2 or 3 keys would be saturated in ALL its rows, its
    dq and dk of the order e^-80, and the per-sequence rule would weigh fp32's rounding of a score of 85 - a relative error of some
    1e-4 in such a probability, harmless in absolute terms - against that scale instead of the sequence's O(1) gradients."""
    return torch.arange(L) % 8 == 5


def probe_rows(L, lens, B):
    """[B, L] bool: the probe queries of the saturated case at L = 19 - queries 15 and 17 of every sequence with more than 16 keys.
    A probe scores about +70 on its key >= 16 and -25 .. -60 on EVERY key < 16: a softmax that took its maximum over keys 0 .. 15 only
    would overflow there (e^89 is fp32's end), which is the only way such an error can show - in exact arithmetic any subtracted
    constant cancels.  (L = 25 has none: its heads have 4 dims, and no direction of R^4 is far on the negative side of 16 spread keys.)"""
    n = torch.full((B,), L) if lens is None else lens.long()
    rows = torch.zeros((B, L), dtype=torch.bool)
    if L == 19:
        rows[:, 15] = rows[:, 17] = True
        rows &= (n > 16)[:, None]
    return rows


def _runner_up(k, t, lens):
    """[B, H, L] long: for the target t of each query the valid key of the OTHER lane half whose direction is closest to k_t (of either
    half where the sequence has at most 4 keys); t itself where no other key comes within a cosine of 0.2.  k [B, L, H, HD] unit rows."""
    B, L, H, HD = k.shape
    kk = k.permute(0, 2, 1, 3)
    cos = kk @ kk.transpose(-2, -1)                                                             # [B, H, L, L]
    ct = torch.gather(cos, 2, t[..., None].expand(B, H, L, L))                                  # row t[b, h, i]: cosines of k_t to every key
    j = torch.arange(L)
    n = torch.full((B,), L) if lens is None else lens.long()
    bad = (j[None, None, None, :] >= n[:, None, None, None]) | (j[None, None, None, :] == t[..., None])
    bad = bad | ((((j[None, None, None, :] ^ t[..., None]) & 4) == 0) & (n > 4)[:, None, None, None])
    val, t2 = ct.masked_fill(bad, -2.0).max(-1)
    return torch.where(val >= 0.2, t2, t)


def make_case(L, H, HD, B, regime, lens, dtype, seed=0):
    """-> {qkv [B, L, 3, H, HD], dout [B, L, H * HD]} of `dtype` on the CPU (drawn in fp32, then stored: what the kernel is handed), lens as
    given.  regime "unit": O(1) scores, Q, K, V and dO each with per-(head, dim) scales and offsets of their own.
    "saturated": keys of norm kappa, kappa^2 / sqrt(HD) = 85, every odd key close to the negative of the key before it, query i of head
    h along k_t + 0.9 k_t2 (t = saturated_targets, t2 = _runner_up): the score of t is about 60, that of t2 a little below it (so the softmax is peaked
    but its gradients are not all zero), that of t ^ 1 about -60, and the row maximum sits in the lane half it was planted in; the
    queries of soft_rows are drawn as in "unit"; V and dO as in "unit".  At HD = 16 every key also carries a common direction u, -u/2 for the keys < 16 and +u/2 for the others, which the
    probe queries (probe_rows) point along."""
    assert regime in ("unit", "saturated") and (L, H, HD) in SHAPES
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * B + (17 if regime == "unit" else 29) + (0 if lens is None else 5))
    v = _scaled(g, (B, L, H, HD), H, HD, 0.5, 2.0, 1.0)
    do = _scaled(g, (B, L, H, HD), H, HD, 0.5, 1.5, 0.5)
    if regime == "unit":
        q = _scaled(g, (B, L, H, HD), H, HD, 0.6, 1.4, 0.3)
        k = _scaled(g, (B, L, H, HD), H, HD, 0.7, 1.3, 0.2)
    else:
        kappa = math.sqrt(85.0 * math.sqrt(HD))
        gk = torch.randn((B, L, H, HD), generator=g)
        if HD == 4:
            # 25 random directions of R^4 crowd each other (some key always lies closer to a query than the planted one): keys 0..23 are
            # the 24-cell's vertices instead (pairwise cosines -1, -1/2, 0, 1/2), as 12 +- pairs in an order and with signs drawn per
            # (sequence, head), slightly perturbed; key 24 is a random direction
            cell = torch.tensor([[float(d == a) for d in range(4)] for a in range(4)] + [[0.5, x, y, z] for x in (0.5, -0.5) for y in (0.5, -0.5) for z in (0.5, -0.5)])
            order = torch.rand((B, H, 12), generator=g).argsort(-1)
            sign = 2.0 * torch.randint(0, 2, (B, H, 12, 1), generator=g) - 1.0
            pairs = cell[order] * sign                                                          # [B, H, 12, 4]
            gk[:, 0:24:2] = pairs.permute(0, 2, 1, 3) + 0.03 * gk[:, 0:24:2]
        else:
            u = _unit(torch.randn((B, 1, H, HD), generator=g))
            gk = gk - (gk * u).sum(-1, keepdim=True) * u                                        # the keys' own parts: orthogonal to u
        gk[:, 1::2] = -gk[:, 0:L - 1:2] + (0.03 if HD == 4 else 0.3) * gk[:, 1::2]
        k = _unit(gk)
        if HD == 16:
            side = torch.where(torch.arange(L) < 16, -1.0, 1.0)[None, :, None, None]
            k = 0.5 * side * u + math.sqrt(0.75) * k
        t = saturated_targets(L, H, lens, B)                                                    # [B, H, L]
        t2 = _runner_up(k, t, lens)
        pick = lambda idx: torch.gather(k.permute(0, 2, 1, 3), 2, idx[..., None].expand(B, H, L, HD)).permute(0, 2, 1, 3)   # key idx[b, h, i] as [B, L, H, HD]
        q = kappa * _unit(pick(t) + 0.9 * pick(t2) + 0.05 * torch.randn((B, L, H, HD), generator=g) / math.sqrt(HD))
        if HD == 16:
            q = torch.where(probe_rows(L, lens, B)[:, :, None, None], 1.2 * kappa * _unit(u + 0.35 * pick(t)), q)
        q = torch.where(soft_rows(L)[None, :, None, None], _scaled(g, (B, L, H, HD), H, HD, 0.6, 1.4, 0.3), q)
        k = kappa * k
    qkv = torch.stack([q, k, v], 2).to(dtype)
    return {"qkv": qkv, "dout": do.reshape(B, L, H * HD).to(dtype), "lens": lens, "L": L, "H": H, "HD": HD, "B": B, "regime": regime}


def replace_masked_rows(case, seed, which=("k", "v")):
    """a copy of the case's qkv with the rows >= lens[b] of the tensors named in `which` (of "q", "k", "v") replaced by large finite
    values (+-3e4, signs from another seed): what the key mask must keep out of every result"""
    qkv = case["qkv"].clone()
    B, L = case["B"], case["L"]
    g = torch.Generator().manual_seed(424243 + seed)
    big = (3.0e4 * (2.0 * torch.randint(0, 2, qkv.shape, generator=g) - 1.0)).to(qkv.dtype)
    masked = torch.arange(L)[None, :] >= case["lens"][:, None].long()                             # [B, L]
    for n in which:
        sl = "qkv".index(n)
        qkv[:, :, sl] = torch.where(masked[:, :, None, None], big[:, :, sl], qkv[:, :, sl])
    return qkv
