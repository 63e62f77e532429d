"""Plain-torch restatement of the masked-categorical kernels of csrc/catan_nn.hip (k_categorical_fwd / _bwd, k_categorical_bits_fwd / _bwd;
catan_categorical_fwd / _bwd, catan_categorical_bits_fwd / _bwd), with the seeded case builders and the launch table that
tests/test_categorical_reference_cpu.py and tests/test_gpu_categorical_fp64.py share.  No call into the library or into nn_kernels: torch
ops only, on the CPU or the GPU, written from include/catan_hip_nn.h and the formulas of RL/distributions.py:10-40.

    legal = mask > 0            mx = max over legal z          lse = mx + log sum_legal exp(z - mx)
    logp_all = z - lse on the legal columns, -inf elsewhere    p = exp(logp_all)     entropy = -sum p logp over p > 0
    cdf_k = sum_{j <= k} p_j (column order; an illegal column adds 0)
    action = given clamped into [0, K - 1] | arg-max: the LOWEST index among the largest legal logits (exact: it compares inputs) |
             sampled: the first legal k with cdf_k > u, else the last legal column
    logp = (legal[a] ? z[a] : -inf) - lse         (an illegal given action: -inf; a row with no legal column: NaN, and lse = -inf)
    dlogits = dlogp (onehot(a) - p) - dent p (logp + H) on the legal columns (the entropy term only where p > 0), 0 elsewhere.
    The closed form is also the reference where the given action is illegal: autograd gives NaN there, the kernel finite values.
  Bits form: bit i of a packed row is word i >> 5, bit i & 31; row j of the launch reads packed row rows_idx[j] (None: j); its segment is
  0 for j < n0, 1 for j < n1, else 2; the segment's bit offset selects K bits, and where its AND offset is >= 0 a second range of K bits
  multiplies in (`bits_mask`).  The float formulas then run on that mask.

  cat_ref        the REFERENCE: fp64 throughout from the inputs as stored.
  cat_yardstick  the same formulas in fp32.  It shows what the number format costs against the reference; it is not an oracle.  `plant` is
                 NOT part of it: the planted errors of the CPU test's rejection cases (PLANTS).

Acceptance: the rule of tests/pin_rule.py per row r (per_group with scale_r, over the rows asked about) and over the whole case (whole).
Floors: the attention suite's, 2^-17 for logp, entropy, lse and 2^-15 for dlogits; none was moved.  scale_r = max(1, largest |logp_all| over the row's legal columns with a finite one) for logp, entropy, lse (`fwd_scale`).
For dlogits the whole case takes the case's largest reference magnitude and a row takes
    scale_r = max(the row's largest reference magnitude, |dlogp_r| + |dent_r|)                                      (`grad_scale`)
because `onehot - p` and `p (logp + H)` are differences and products of numbers of size 1: whatever the size of the result, a row's
gradient carries an absolute error of an fp32 ulp of 1 times |dlogp| + |dent|, in the kernels and in the yardstick alike.  Where the taken
action has p within 1e-4 of 1 the whole row's gradient is 1e-4 of that, and under the row's own magnitude alone such rows needed a floor
of up to 7.5e-4 on the MI355X (unit regime, K = 2, 4 097 rows: the yardstick's rounding fell luckily where the kernel's p, from __expf,
did not) - a floor that would have loosened every ordinary row 32-fold.  With |dlogp| + |dent| in the scale the ordinary rows keep 2^-15
of their own magnitude or of their incoming gradients', whichever is larger; profiles/categorical_kernel_tests.txt has what the rows need.
The yardstick returns p = 0 below the normal range (2^-126), as the kernels' __expf does; with torch's denormal p the `wide` rows whose
whole gradient is of that size disagreed by the flushed value.  The exact cases (one legal column, an illegal given action, a row without
a legal column) are compared as values, not through the rule.

Sampled actions: the bracket rule of tests/test_gpu_heads_fp64.py with tau = pin_rule.whole_bound(ref cdf, yardstick cdf, BF16_FLOOR)
(`bracket_ok`), on every row; only where u is the largest float below 1 may the pick also be the last legal column.  tau is 2^-9 (the
cdf's scale is 1), so the rule brackets the pick within 2^-9 of cdf mass; it cannot tell two neighbouring columns of less mass apart.  u = 0: the pick is a legal column whose fp64 probability is above 2^-152 (below it no fp32 evaluation has p > 0) and no
legal column before it has one of 2^-125 or more (from there every fp32 evaluation has p > 0, flushed denormals or not): `first_ok`."""
import torch

import pin_rule as PR
from heads_reference import HEAD_K, MASK_OFF, U_TOP

FLOOR = {"logp": 2.0 ** -17, "entropy": 2.0 ** -17, "lse": 2.0 ** -17, "dlogits": 2.0 ** -15}
PLANTS = ("ent_all", "cdf_ge", "fall_last", "argmax_illegal", "no_max", "and_ignored", "seg_le", "bit_off")
REGIMES = ("unit", "wide", "single", "all_legal", "ties", "empty", "neginf")
BITS_REGIMES = ("unit", "wide", "ties", "empty", "neginf")
MODES = ("given_legal", "given_illegal", "given_oor", "argmax", "sampled")
P_NEVER, P_SURE = 2.0 ** -152, 2.0 ** -125
FLT_MIN = 2.0 ** -126
EMPTY_EVERY = 13

# ------------------------------------------------------------------------------------------------------------------- launch table
# catan_categorical_fwd / _bwd / _bits_fwd / _bits_bwd (csrc/catan_abi_nn.h): one lane per row, 256 rows per block, ceil(rows / 256) blocks,
# no cap and no loop.
BLOCK = 256
ROWS = (1, 255, 256, 257, 4097)
KS = (1, 2, 3, 5, 6, 13, 19, 54, 73)                     # heads_reference.HEAD_K plus 1 and 19
MASK_LD = 325
PITCH = 11                                               # words of a packed row: 352 bits
GIVEN_LDS = (1, 18)
assert set(HEAD_K) | {1, 19} == set(KS)


def window_off(K):
    """the first column of the K-wide window in the [rows][325] mask matrix: the head's own (the first head of that width), for K = 1 the
    matrix's last column"""
    return MASK_LD - 1 if K == 1 else MASK_OFF[HEAD_K.index(K)]


# per K: the (bit offset, AND offset) of the three segments.  Segment 0 is the head's real offset (13 with K = 54 crosses words), segment 2
# ends exactly on bit 32 * PITCH - 1, and where there is an AND range it is in segment 1 only
BITS_SEGS = {
    1: ((324, -1), (31, -1), (351, -1)),
    2: ((272, -1), (62, 127), (350, -1)),
    3: ((274, -1), (280, 283), (349, -1)),
    5: ((267, -1), (295, 315), (347, -1)),
    6: ((283, -1), (289, -1), (346, -1)),
    13: ((0, -1), (19, 51), (339, -1)),
    19: ((248, -1), (13, -1), (333, -1)),
    54: ((13, -1), (94, 121), (298, -1)),
    73: ((175, -1), (248, -1), (279, -1)),
}


def seg_layouts(B):
    """the (n0, n1) of a launch of B rows: no row, every row in segment 1, every row in segment 0, the first block's edge inside segment 1,
    both boundaries on it, one row in each outer segment"""
    full = ((0, 0), (0, B), (B, B), (255, 257), (256, 256), (1, B - 1))
    return full if B >= 257 else full[:3]


def bits_cases(K):
    """-> [(B, (n0, n1), with rows_idx, given_ld, regime)] of one K: every layout with and without a row list; the regime and the pitch of
    the given column go round with the case"""
    out = []
    for B in ROWS:
        for s, (n0, n1) in enumerate(seg_layouts(B)):
            for with_idx in (False, True):
                t = len(out) + KS.index(K)
                out.append((B, (n0, n1), with_idx, GIVEN_LDS[(s + with_idx) % 2], BITS_REGIMES[t % len(BITS_REGIMES)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------- formulas
def _lowest(cond, K):
    """the lowest column where cond holds, K where none does"""
    idx = torch.arange(K, device=cond.device).expand_as(cond)
    return torch.where(cond, idx, torch.full_like(idx, K)).min(-1).values


def _core(logits, mask, wd, plant=None):
    """everything in dtype wd -> {legal, lse, logp_all, p, cdf, entropy, argmax, last}"""
    z = logits.to(wd)
    K = z.shape[1]
    legal = mask > 0
    ninf = torch.full_like(z, float("-inf"))
    zero = torch.zeros_like(z)
    zl = torch.where(legal, z, ninf)
    mx = zl.max(-1, keepdim=True).values
    sub = torch.zeros_like(mx) if plant == "no_max" else mx
    lse = sub + torch.log(torch.where(legal, torch.exp(z - sub), zero).sum(-1, keepdim=True))
    lp = z - lse
    p = torch.where(legal, torch.exp(lp), zero)
    if wd == torch.float32:
        p = torch.where(p < FLT_MIN, zero, p)                         # (the kernels' __expf returns 0 below the normal range)
    counted = legal if plant == "ent_all" else p > 0
    ent = -torch.where(counted, p * lp, zero).sum(-1)
    if plant == "argmax_illegal":
        amax = _lowest(z == z.max(-1, keepdim=True).values, K)
    else:
        amax = _lowest(zl == mx, K)                                  # (a row without a legal column: every zl is -inf = mx -> 0, the kernel's)
    last = (K - 1 - _lowest(legal.flip(-1), K)).clamp(min=0)
    return {"legal": legal, "lse": lse.squeeze(-1), "logp_all": torch.where(legal, lp, ninf), "p": p, "cdf": p.cumsum(-1), "entropy": ent,
            "argmax": amax.clamp(max=K - 1), "last": last, "z": z}


def sample(o, u, plant=None):
    """the inverse-CDF pick of `o` (a _core dict) at u [B]"""
    K = o["cdf"].shape[1]
    uu = u.to(o["cdf"].dtype)[:, None]
    hit = o["legal"] & ((o["cdf"] >= uu) if plant == "cdf_ge" else (o["cdf"] > uu))
    k = _lowest(hit, K)
    if plant == "fall_last":                                          # a pick in the upper half of the cdf falls through to the last legal column
        k = torch.where(uu.squeeze(1) > 0.5, torch.full_like(k, K), k)
    return torch.where(k < K, k, o["last"])


def logp_at(o, a):
    z = o["z"].gather(1, a[:, None]).squeeze(1)
    ok = o["legal"].gather(1, a[:, None]).squeeze(1)
    return torch.where(ok, z, torch.full_like(z, float("-inf"))) - o["lse"]


def grad(o, a, dlogp, dent):
    """the closed form -> dlogits [B, K] in o's dtype"""
    wd = o["z"].dtype
    K = o["z"].shape[1]
    lp = o["z"] - o["lse"][:, None]
    onehot = (torch.arange(K, device=a.device)[None] == a[:, None]).to(wd)
    zero = torch.zeros_like(lp)
    g = dlogp.to(wd)[:, None] * (onehot - o["p"]) - torch.where(o["p"] > 0, dent.to(wd)[:, None] * o["p"] * (lp + o["entropy"][:, None]), zero)
    return torch.where(o["legal"], g, zero)


def _eval(logits, mask, mode, wd, given=None, u=None, dlogp=None, dent=None, plant=None):
    o = _core(logits, mask, wd, plant)
    K = logits.shape[1]
    if mode.startswith("given"):
        a = given.clamp(0, K - 1)
    elif mode == "argmax":
        a = o["argmax"]
    else:
        a = sample(o, u, plant)
    o["action"] = a
    o["logp"] = logp_at(o, a)
    if dlogp is not None:
        o["dlogits"] = grad(o, a, dlogp, dent)
    return o


def cat_ref(logits, mask, mode, given=None, u=None, dlogp=None, dent=None):
    return _eval(logits, mask, mode, torch.float64, given, u, dlogp, dent)


def cat_yardstick(logits, mask, mode, given=None, u=None, dlogp=None, dent=None, plant=None):
    return _eval(logits, mask, mode, torch.float32, given, u, dlogp, dent, plant)


def bits_mask(packed, rows_idx, segs, B, K, plant=None):
    """the float mask [B, K] the bits form reads: packed int32 [n, pitch] (the uint32 words as stored); rows_idx int64 [B] or None; segs =
    the ABI's 8 ints (n0, n1, then (bit offset, AND offset or -1) x 3)"""
    dev = packed.device
    pitch = packed.shape[1]
    words = packed.long() & 0xFFFFFFFF
    j = torch.arange(B, device=dev)
    src = j if rows_idx is None else rows_idx
    n0, n1 = segs[0], segs[1]
    first = (j <= n0) if plant == "seg_le" else (j < n0)
    seg = torch.where(first, 0, torch.where(j < n1, 1, 2))
    off = torch.tensor(segs[2::2], device=dev)[seg]
    aoff = torch.tensor(segs[3::2], device=dev)[seg]

    def bits(o):
        i = o[:, None] + torch.arange(K, device=dev)[None] + (1 if plant == "bit_off" else 0)
        if plant == "bit_off":
            i = i % (32 * pitch)                                      # (the planted index stays inside the row)
        return (words[src[:, None], i >> 5] >> (i & 31)) & 1

    m = bits(off)
    if plant != "and_ignored":
        m = m & torch.where((aoff >= 0)[:, None], bits(aoff.clamp(min=0)), torch.ones_like(m))
    return m.float()


# -------------------------------------------------------------------------------------------------------------------------- rule
def fwd_scale(ref):
    """[B]: max(1, the largest finite |logp_all| over the row's legal columns)"""
    lp = ref["logp_all"].abs()
    lp = torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp))
    return lp.amax(-1).clamp(min=1.0)


def grad_scale(ref_grad, dlogp, dent):
    """[B]: max(the row's largest reference gradient, |dlogp| + |dent|) - see the module docstring"""
    return torch.maximum(ref_grad.double().abs().amax(1), dlogp.double().abs() + dent.double().abs())


def bracket_ok(ref, yard, action, u):
    """the bracket rule for every row -> (ok [B] bool, tau)"""
    tau, _ = PR.whole_bound(ref["cdf"], yard["cdf"], PR.BF16_FLOOR)
    cdf = ref["cdf"].double()
    uu = u.double()
    upper = cdf.gather(1, action[:, None]).squeeze(1)
    lower = torch.where(action > 0, cdf.gather(1, (action - 1).clamp(min=0)[:, None]).squeeze(1), torch.zeros_like(upper))
    legal = ref["legal"].gather(1, action[:, None]).squeeze(1)
    return legal & (upper + tau > uu) & (lower - tau <= uu), tau


def first_ok(ref, action):
    """u = 0 -> [B] bool (see the module docstring)"""
    K = ref["p"].shape[1]
    pa = ref["p"].gather(1, action[:, None]).squeeze(1)
    sure = _lowest(ref["legal"] & (ref["p"] >= P_SURE), K)
    return ref["legal"].gather(1, action[:, None]).squeeze(1) & (pa > P_NEVER) & (action <= sure)


def near_boundary_share(ref, u):
    """among the rows whose u is a draw of torch.rand (not one of the planted 0 and largest-float-below-1, which sit ON a boundary by
    design and have rules of their own), the share whose u lies within K 2^-20 of an fp64 cdf boundary of a legal column below the last
    one: where the bracket rule could not tell two neighbours apart"""
    K = ref["cdf"].shape[1]
    d = (ref["cdf"].double() - u.double()[:, None]).abs()
    inner = ref["legal"] & (torch.arange(K, device=u.device)[None] < ref["last"][:, None])
    drawn = (u != 0) & (u != U_TOP)
    return float(((d <= K * 2.0 ** -20) & inner).any(1)[drawn].double().mean())


# ------------------------------------------------------------------------------------------------------------------------- cases
def _gen(tag, B, K, regime, seed):
    return torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * B + 101 * REGIMES.index(regime) + tag)


def make_mask(regime, B, K, g):
    """[B, K] of 0 / 1.  unit, wide, ties, empty, neginf: density 0.6 with at least one legal column per row (wide, neginf: the first and
    the last column legal on the planted rows r % 8 == 0, whose u is 0; wide: column 1 illegal there from K = 3); single: exactly one; all_legal; empty: every 13th row (0, 13, ..) none"""
    if regime == "all_legal":
        return torch.ones(B, K)
    keep = torch.randint(0, K, (B,), generator=g)
    r = torch.arange(B)
    if regime == "single":
        m = torch.zeros(B, K)
    else:
        m = (torch.rand(B, K, generator=g) < 0.6).float()
    m[r, keep] = 1.0
    if regime in ("wide", "neginf"):
        m[::8, 0] = 1.0
        m[::8, K - 1] = 1.0
        if regime == "wide" and K >= 3:
            m[::8, 1] = 0.0
    if regime == "empty":
        m[::EMPTY_EVERY] = 0.0
    return m


def make_logits(regime, mask, g):
    """fp32 [B, K] for a given mask.
    unit, single, all_legal, empty: randn * 2.
    wide:   randn * 12 with one legal column per row raised by 80 (by 120 on the planted rows: exp of it is inf in fp32, so row 0 alone
            shows a log-sum-exp without the max subtraction; an ILLEGAL column 1 there is raised by 200: an arg-max or a max that looked
            at illegal columns would take it) - a good share of the p underflow to 0 in fp32 (more where denormals are flushed).  On the rows r % 8 == 0 (whose u is planted
            0) the raised column is the LAST legal one and the first legal column, if another, is lowered by 60: its fp64 probability is
            below 2^-152, so `cdf >= u` at u = 0 picks a column no fp32 evaluation can.
    ties:   drawn from {-1.5, 0.25, 2}: many equal maxima.
    neginf: unit, with a third of the legal columns at -inf (on the planted rows r % 8 == 0 the last legal one among them) but never the
            row's first legal one: p = 0 with logp = -inf, where the
            entropy's and the gradient's `p > 0` guards are what keeps 0 * inf out."""
    B, K = mask.shape
    r = torch.arange(B)
    legal = mask > 0
    any_legal = legal.any(1)
    first = _lowest(legal, K).clamp(max=K - 1)
    last = (K - 1 - _lowest(legal.flip(-1), K)).clamp(min=0)
    if regime == "wide":
        z = torch.randn(B, K, generator=g) * 12
        pick = torch.multinomial(mask + 1e-9, 1, generator=g).squeeze(1)
        planted = (r % 8 == 0)
        pick = torch.where(planted, last, pick)
        z[r, pick] += torch.where(any_legal, torch.where(planted, 120.0, 80.0), torch.zeros(B))
        low = planted & (first != pick) & any_legal
        z[r[low], first[low]] -= 60.0
        if K >= 3:
            ill = planted & ~legal[:, 1]
            z[ill, 1] += 200.0
        return z
    if regime == "ties":
        return torch.tensor([-1.5, 0.25, 2.0])[torch.randint(0, 3, (B, K), generator=g)]
    z = torch.randn(B, K, generator=g) * 2
    if regime == "neginf":
        drop = (torch.rand(B, K, generator=g) < 1 / 3) & legal
        drop[r, first] = False
        z[drop] = float("-inf")
        planted = (r % 8 == 0) & (last != first)                      # (row 0 alone shows an entropy sum without its guard)
        z[r[planted], last[planted]] = float("-inf")
    return z


def make_aux(mask, g):
    """what a case carries besides logits and mask -> {given_legal, given_illegal, has_illegal, given_oor, u, dlogp, dent}.  A row without
    an illegal (legal) column takes column 0 as its given_illegal (given_legal).  u: torch.rand, 0 on the rows r % 8 == 0, the largest
    float below 1 on the rows r % 8 == 4."""
    B, K = mask.shape
    r = torch.arange(B)
    legal = mask > 0
    gl = torch.multinomial(mask + 1e-9, 1, generator=g).squeeze(1)
    gl = torch.where(legal.any(1), gl, torch.zeros_like(gl))
    gi = torch.multinomial((1 - mask) + 1e-9, 1, generator=g).squeeze(1)
    has_illegal = (~legal).any(1)
    gi = torch.where(has_illegal, gi, torch.zeros_like(gi))
    oor = torch.tensor([-1, K, -3, K + 5, 1000, -(2 ** 31) + 1])[torch.randint(0, 6, (B,), generator=g)]
    u = torch.rand(B, generator=g)
    u[r % 8 == 0] = 0.0
    u[r % 8 == 4] = U_TOP
    return {"given_legal": gl, "given_illegal": gi, "has_illegal": has_illegal, "given_oor": oor, "u": u,
            "dlogp": torch.randn(B, generator=g), "dent": torch.randn(B, generator=g)}


def make_case(regime, B, K, seed=0):
    """a float-mask case on the CPU -> {logits, mask [B, K]; the make_aux entries; regime, B, K}"""
    g = _gen(0, B, K, regime, seed)
    mask = make_mask(regime, B, K, g)
    c = {"logits": make_logits(regime, mask, g), "mask": mask, "regime": regime, "B": B, "K": K}
    c.update(make_aux(mask, g))
    return c


# ------------------------------------------------------------------------------------------------------------------------ verdict
def _same(a, b):
    """equal as values, NaN equal to NaN (a signed zero is a zero)"""
    a, b = a.double(), b.double()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def judge(c, mode, got):
    """everything the GPU test asks of one launch (forward, and with got["dlogits"] the backward) of case `c` in `mode`; `got` = {action,
    logp, entropy, lse[, dlogits]} as the kernel (or a planted yardstick) returned them.  Reference and yardstick are evaluated at the
    action that was returned, once that action has passed its mode's rule.  -> (failures, {output: (kernel error, yardstick error, largest
    share of a bound, the smallest floor under which every row would pass)}).  Nothing in a bound comes from `got`."""
    z, mask, K = c["logits"], c["mask"], c["K"]
    bad, stats = [], {}
    a = got["action"]
    if not bool(((a >= 0) & (a < K)).all()):
        return [("action", "outside [0, K - 1]")], stats
    given = c[mode] if mode.startswith("given") else None
    ref0 = cat_ref(z, mask, mode, given, c["u"])
    yard0 = cat_yardstick(z, mask, mode, given, c["u"])
    legal_rows = ref0["legal"].any(1)
    empty = ~legal_rows
    # the action
    if mode != "sampled":
        if not torch.equal(a, ref0["action"]):
            bad.append(("action", mode, f"{int((a != ref0['action']).sum())} rows differ, first {int((a != ref0['action']).nonzero()[0])}"))
    else:
        ok, tau = bracket_ok(ref0, yard0, a, c["u"])
        # (the largest float below 1 may also fall through to the last legal column; no other u may)
        ok = ok | ((c["u"] == U_TOP) & (a == ref0["last"]) & ref0["legal"].gather(1, a[:, None]).squeeze(1))
        ok = ok & torch.where(c["u"] == 0, first_ok(ref0, a), torch.ones_like(ok))
        ok = torch.where(empty, a == 0, ok)
        stats["tau"] = tau
        if not bool(ok.all()):
            bad.append(("action", "cdf bracket", [(int(r), int(a[r]), float(c["u"][r])) for r in (~ok).nonzero().flatten().tolist()[:8]]))
    # reference and yardstick at the returned action
    ref = cat_ref(z, mask, "given", a, None, c["dlogp"], c["dent"])
    yard = cat_yardstick(z, mask, "given", a, None, c["dlogp"], c["dent"])
    scale = fwd_scale(ref)
    exact = c["regime"] == "single"
    for n in ("logp", "entropy", "lse"):
        finite = torch.isfinite(ref[n]) & legal_rows
        if not _same(got[n][~finite], ref[n][~finite]):
            bad.append((n, "a non-finite value differs from the reference's (-inf for an illegal action; NaN logp, -inf lse on an empty row)"))
        if bool(torch.isnan(got[n][legal_rows]).any()):
            bad.append((n, "NaN outside the empty rows"))
        if exact and not _same(got[n], ref[n]):
            bad.append((n, "one legal column: not the exact value"))
        ok, ek, bnd = PR.per_group(got[n], ref[n], yard[n], FLOOR[n], scale, finite)
        ey = torch.where(finite, PR.group_error(yard[n], ref[n]), torch.zeros_like(ek))
        # the whole case: the largest error against twice the yardstick's largest plus the floor at the case's largest scale
        whole = PR.whole(got[n][finite], ref[n][finite], yard[n][finite], FLOOR[n], float(scale.max()))[0]
        stats[n] = (float(ek.max()), float(ey.max()), PR.share(ek, bnd), PR.need_floor(ek, ey, scale.double()))
        if not (bool(ok.all()) and whole):
            r = int((~ok).nonzero()[0]) if not bool(ok.all()) else -1
            bad.append((n, f"{int((~ok).sum())} rows, first {r}", float(ek[r]), float(bnd[r])))
    if not _same(got["entropy"][empty], torch.zeros_like(got["entropy"][empty])):
        bad.append(("entropy", "an empty row's is not 0"))
    if "dlogits" in got:
        g, rg, yg = got["dlogits"], ref["dlogits"], yard["dlogits"]
        if not bool(torch.isfinite(g).all()):
            bad.append(("dlogits", "not finite"))
        if not _same(g[empty], torch.zeros_like(g[empty])):
            bad.append(("dlogits", "an empty row's gradient is not 0"))
        if not _same(torch.where(ref["legal"], torch.zeros_like(g), g), torch.zeros_like(g)):
            bad.append(("dlogits", "an illegal column's gradient is not 0"))
        if exact and not _same(g, rg):
            bad.append(("dlogits", "one legal column: not exactly 0"))
        gscale = grad_scale(rg, c["dlogp"], c["dent"])
        ok, ek, bnd = PR.per_group(g, rg, yg, FLOOR["dlogits"], gscale, legal_rows)
        w_ok, w_ek, w_ey, w_b = PR.whole(g[legal_rows], rg[legal_rows], yg[legal_rows], FLOOR["dlogits"])
        ey = torch.where(legal_rows, PR.group_error(yg, rg), torch.zeros_like(ek))
        stats["dlogits"] = (w_ek, w_ey, max(PR.share(ek, bnd), PR.whole_share(w_ek, w_b)), PR.need_floor(ek, ey, gscale))
        if not (bool(ok.all()) and w_ok):
            r = int((~ok).nonzero()[0]) if not bool(ok.all()) else -1
            bad.append(("dlogits", f"{int((~ok).sum())} rows, first {r}", float(ek[r]), float(bnd[r]), w_ek, w_b))
    return bad, stats


def stats_line(stats):
    """per output: kernel error, yardstick error, their ratio, the largest share of a bound used, the floor the rows need"""
    out = []
    for n in ("logp", "entropy", "lse", "dlogits"):
        if n in stats:
            out.append(PR.fmt_stat(n, stats[n]))
    if "tau" in stats:
        out.append(f"tau {stats['tau']:.2e}")
    return " | ".join(out)


def pack_bits(dense):
    """[n, 32 * pitch] of 0 / 1 -> int32 [n, pitch] (bit i -> word i >> 5, bit i & 31)"""
    n, nb = dense.shape
    w = (dense.long().view(n, nb // 32, 32) << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def make_bits_case(regime, B, K, n0n1, with_idx, given_ld, seed=0):
    """a bits-form case on the CPU -> {packed int32 [n, PITCH], rows_idx int64 [B] (with repeats) or None, segs (8 ints), mask [B, K] =
    bits_mask of these, logits, the make_aux entries, given_ld}.  All 352 bits of a packed row are drawn (density 0.6; the AND ranges
    0.8); in `empty` the packed row of every 13th launch row is cleared.  Every other row keeps a legal column: where the draw left none,
    the bits of the row's first column are set."""
    g = _gen(7 + 2 * given_ld + with_idx + 1000 * n0n1[0] + 10 * n0n1[1], B, K, regime, seed)
    n = B // 2 + 3 if with_idx else B
    rows_idx = torch.randint(0, n, (B,), generator=g) if with_idx else None
    segs = [int(n0n1[0]), int(n0n1[1])] + [int(v) for pair in BITS_SEGS[K] for v in pair]
    dense = (torch.rand(n, 32 * PITCH, generator=g) < 0.6).long()
    for off, aoff in BITS_SEGS[K]:
        if aoff >= 0:
            dense[:, aoff:aoff + K] = (torch.rand(n, K, generator=g) < 0.8).long()
    src = torch.arange(B) if rows_idx is None else rows_idx
    if regime == "empty":
        dense[src[::EMPTY_EVERY]] = 0
    else:
        for off, aoff in BITS_SEGS[K]:                               # (whatever segment a row lands in, it has a legal column)
            none = (dense[:, off:off + K] * (dense[:, aoff:aoff + K] if aoff >= 0 else 1)).sum(1) == 0
            dense[none, off] = 1
            if aoff >= 0:
                dense[none, aoff] = 1
    packed = pack_bits(dense)
    mask = bits_mask(packed, rows_idx, segs, B, K)
    c = {"packed": packed, "rows_idx": rows_idx, "segs": segs, "mask": mask, "logits": make_logits(regime, mask, g), "regime": regime,
         "B": B, "K": K, "given_ld": given_ld, "dense": dense}
    c.update(make_aux(mask, g))
    return c
