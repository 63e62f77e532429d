"""Plain-torch restatement of the scalar tail of the PPO update - k_gae / k_adv_stats / k_adv_normalise and k_ppo_loss (csrc/catan_ppo.hip;
catan_gae, catan_adv_normalise, catan_ppo_loss) and k_grad_sumsq / k_adam_step (csrc/catan_optim.hip, through optim.FusedAdam.step) - with
the seeded case builders and launch tables that tests/test_ppo_tail_reference_cpu.py and tests/test_gpu_ppo_tail_fp64.py share.  No call
into the library: torch ops only, on the CPU.

Every operation has a REFERENCE (fp64 throughout, from the fp32 inputs as stored) and a YARDSTICK (the same formula in torch fp32: what
the number format costs; it is not an oracle).  `plant` is not part of either: the planted arithmetic slips of the CPU test's rejection
cases (PLANTS).  Acceptance of an output, per element (pin_rule.per_element, the rule of tests/pin_rule.py):

    |kernel - fp64| <= 2 |yardstick - fp64| + floor * scale          floor: FLOOR["value"] = 2^-17, FLOOR["grad"] = 2^-15

computed from reference and yardstick alone.  Where the reference is not finite the kernel must return that value (inf as inf, NaN as
NaN); where reference and yardstick are both exactly 0 the bound is 0.

A. GAE (RL/ppo/process_batch.py:134-142), gamma = 0.999 and lambda = 0.95 as doubles (a double scalar meets an fp32 tensor as fp32):
    delta = r[t] + gamma * v[t+1] * m[t+1] - v[t]      gae = delta + gamma * lambda * m[t+1] * gae      returns[t] = gae + v[t]
    adv_raw = returns - v[:-1]                         adv = (adv_raw - mean) / (unbiased std + 1e-5)
  The yardstick is that recurrence step by step in torch fp32: the kernel's returns and adv_raw must equal it BIT FOR BIT (the header's
  claim).  stats3 = (sum, sum of squares, count) of adv_raw: the kernel adds the fp32 elements in fp64, so its sums are compared with the
  fp64 sums of those same fp32 elements (the yardstick's, which the kernel's elements have to equal) within T N 2^-52 sum|a| and
  T N 2^-52 sum a^2 - a bound on the ORDER of an fp64 summation; against the sums of the fp64 recurrence's elements the fp32 rounding of
  each element (2^-24 |v|) would be what is measured, thousands of times that bound.  Normalised advantages: scale max(1, |reference|).
  Regimes: GAE_REGIMES (`gae_inputs`).  T N = 1: the unbiased variance is 0 / 0; nothing is asked of the normalised value.

B. PPO loss (RL/ppo/ppo.py:46-66), per row, B rows:
    vp, ret = (old_values - mean) / (std + 1e-4), same for returns, with use_norm          ratio = exp(logp - old)
    s1 = ratio adv      s2 = clamp(ratio, 1 - clip, 1 + clip) adv      action term = -min(s1, s2)      inside = lo <= ratio <= hi
    d_logp = -s1 / B where (s1 <= s2 or inside), else 0
    dv = v - vp      vc = vp + clamp(dv, -clip, clip)      e1 = v - ret, e2 = vc - ret      value term = 0.5 max(e1^2, e2^2)
    vin = |dv| <= clip (with equality: clamp passes its gradient on the boundary)
    d_values = value_coef / B * (e1 where e1^2 > e2^2; (e2 if vin else 0) where e1^2 < e2^2; on a tie half of each, as autograd's
               maximum gives: 0.5 (e1 + (e2 if vin else 0)))
    losses = the means of the two terms.  min, max and clamp pass NaN on (torch.min / torch.max / torch.clamp); a NaN row has a NaN
    gradient.
  THE RULE FOR AN INFINITE RATIO.  `ratio` is what an fp32 number can hold: above the largest fp32 it is +inf, below 2^-150 it is 0, in
  the reference too (in fp64 exp(100) is finite).  With ratio = +inf and adv > 0, s1 = +inf > s2: the clipped side is active, the term
  is -s2 and the gradient 0 - autograd forms 0 * inf = NaN there, which is not copied.  With adv < 0, s1 = -inf: the term is +inf and
  the gradient -s1 / B = +inf.  (adv = 0 with ratio = inf is NaN in every form and is not planted.)
  Which rows are clipped: adv > 0 above hi and adv < 0 below lo have s1 > s2, the clipped side is active, gradient exactly 0; adv < 0
  above hi and adv > 0 below lo keep the unclipped side.
  Regimes: LOSS_REGIMES (`loss_inputs`); planted rows: POLICY_PLANTS x VALUE_PLANTS at `plant_positions`.  With the value normaliser on
  (vp - 150) / 150.0001 is no dyadic number, so the planted VALUE rows are only planted with use_norm off; the policy plants always.
  Near-boundary rows (`near_boundary`): where an fp64 quantity lies within a relative 2^-18 of its branch boundary, fp32 may take the
  other branch; such a row's gradient must equal one of the branches' values under the same floor.  Planted rows are exempt: they sit
  exactly on a boundary with dyadic numbers, or well off it.
  Scales: the losses, the mean of the rows' absolute terms; a gradient row, its own reference magnitude.

C. Clip + Adam (torch.nn.utils.clip_grad_norm_ then torch.optim.Adam.step, RL/ppo/ppo.py:23,67-68), per tensor with ITS step count t:
    norm = sqrt(sum g^2) over all tensors with a gradient      coef = min(max_norm / (norm + 1e-6), 1)      g = g coef
    m = m + (g - m) (1 - beta1)      v = v beta2 + (1 - beta2) g g      denom = sqrt(v) / sqrt(1 - beta2^t) + eps
    p = p - lr / (1 - beta1^t) * m / denom
  Yardstick: torch.optim.Adam(foreach=False) behind clip_grad_norm_ in fp32.  Scales: p, max(|p before the step|, lr) (a step is about
  lr); m and v, the element's own reference magnitude; the norm, the reference norm (floor: value).  Because m is judged relative to
  ITSELF, the cases keep `m + (g - m) (1 - beta1)` away from cancellation: a loaded exp_avg lies in [4, 8] times the gradient scale of
  its tensor (9 m then exceeds every |g| of a normal draw of 1.2 M elements for three steps), a tensor with step count 0 starts from zero
  state as in torch, and the gradients of steps 2 and 3 are those of step 1 times positive factors - where 0.9 m = -0.1 g to a part in
  10^4 the element's relative error measures the conditioning of that sum, in the yardstick as in the kernel, not the kernel.
  Gradients keep |g| >= 0.05 of their scale, so that (1 - beta2) g g is no fp32 denormal in any regime."""
import functools
import math

import torch

import pin_rule as PR

FLOOR = {"value": 2.0 ** -17, "grad": 2.0 ** -15}
PLANTS = ("mask_t", "gl_gamma", "cnt", "inside_only", "vin_lt", "no_half", "bias_eps", "no_bias1")
FLT_MAX = 3.4028234663852886e38
NAN, INF = float("nan"), float("inf")
BAND = 2.0 ** -18

# ----------------------------------------------------------------------------------------------------------------------------- GAE
# catan_gae: ceil(N / 256) blocks of 256 lanes, one lane per column; k_adv_stats: ONE block whose lanes stride over the per-block
# partials (a second trip from 257 blocks = 65 537 columns); catan_adv_normalise: min(4096, ceil(T N / 256)) blocks, grid-stride.
GAMMA, LAM = 0.999, 0.95
GAE_CASES = ((1, 1), (2, 255), (3, 256), (33, 257), (200, 257), (7, 4097), (2, 65793))
GAE_REGIMES = ("game", "no_done", "all_done", "edges", "big", "zero", "const")
CONST_C = 0.375


def edge_masks(T, N):
    """the (t, n) of the single zero masks of the `edges` regime that the shape has room for"""
    want = [(T, N - 1), (1, 0), (T - 1, 255), (T - 1, 256)]
    return sorted({(t, n) for t, n in want if 1 <= t <= T and 0 <= n < N})


def gae_inputs(T, N, regime):
    """-> rewards [T, N], values [T + 1, N], masks [T + 1, N], fp32"""
    g = PR.gen("gae", T, N, regime)
    r = (torch.rand(T, N, generator=g) < 0.01).float() * 500.0 * (1.0 - 2.0 * (torch.rand(T, N, generator=g) < 0.5).float())
    v = 150.0 + 50.0 * torch.randn(T + 1, N, generator=g)
    m = (torch.rand(T + 1, N, generator=g) > 0.01).float()
    if regime == "no_done":
        m = torch.ones(T + 1, N)
    elif regime == "all_done":
        m = torch.zeros(T + 1, N)
    elif regime == "edges":
        m = torch.ones(T + 1, N)
        for t, n in edge_masks(T, N):
            m[t, n] = 0.0
    elif regime == "big":
        v = 1.0e6 + (2.0 * torch.rand(T + 1, N, generator=g) - 1.0)
    elif regime == "zero":
        r, v, m = torch.zeros(T, N), torch.zeros(T + 1, N), torch.zeros(T + 1, N)
    elif regime == "const":
        r, v, m = torch.full((T, N), CONST_C), torch.zeros(T + 1, N), torch.zeros(T + 1, N)
    return r, v, m


def gae_eval(r, v, m, wd, plant=None):
    """the recurrence step by step in dtype wd -> returns [T, N], adv_raw [T, N]"""
    r, v, m = r.to(wd), v.to(wd), m.to(wd)
    T = r.shape[0]
    gae = torch.zeros_like(r[0])
    rets = torch.empty_like(r)
    for t in reversed(range(T)):
        m1 = m[t] if plant == "mask_t" else m[t + 1]
        delta = r[t] + GAMMA * v[t + 1] * m1 - v[t]
        gae = delta + (GAMMA if plant == "gl_gamma" else GAMMA * LAM) * m1 * gae
        rets[t] = gae + v[t]
    return rets, rets - v[:-1]


def adv_normalise(adv, plant=None):
    """(adv - mean) / (unbiased std + 1e-5) in adv's dtype"""
    if adv.numel() < 2:
        return torch.full_like(adv, NAN)                                  # 0 / 0, in torch too
    std = adv.std(unbiased=False) if plant == "cnt" else adv.std()
    return (adv - adv.mean()) / (std + 1e-5)


@functools.lru_cache(maxsize=None)
def gae_case(T, N, regime):
    """-> {r, v, m; yard_ret, yard_raw, yard_adv (fp32); ref_ret, ref_raw, ref_adv (fp64); sum, sumsq, abs (fp64 sums of yard_raw)}"""
    r, v, m = gae_inputs(T, N, regime)
    yr, ya = gae_eval(r, v, m, torch.float32)
    rr, ra = gae_eval(r, v, m, torch.float64)
    a64 = ya.double()
    return {"T": T, "N": N, "regime": regime, "r": r, "v": v, "m": m, "yard_ret": yr, "yard_raw": ya, "yard_adv": adv_normalise(ya),
            "ref_ret": rr, "ref_raw": ra, "ref_adv": adv_normalise(ra),
            "sum": float(a64.sum()), "sumsq": float((a64 * a64).sum()), "abs": float(a64.abs().sum())}


def gae_judge(c, got, label=""):
    """everything asked of one catan_gae + catan_adv_normalise run of case `c`: got = {ret, raw, adv (fp32 [T, N]), stats (3 doubles)}
    -> (failures, stats per output)"""
    T, N = c["T"], c["N"]
    bad, st = [], {}
    for n, y, rf in (("ret", c["yard_ret"], c["ref_ret"]), ("raw", c["yard_raw"], c["ref_raw"])):
        if not PR.same_bits(got[n], y):
            bad.append((label, n, "not bit-equal to the fp32 recurrence", int((got[n] != y).sum())))
        nb, first, st[n] = PR.per_element(got[n], rf, y, FLOOR["value"], rf.abs().clamp(min=1.0))
        if nb:
            bad.append((label, n, "against fp64", nb, first))
    s = [float(x) for x in got["stats"]]
    cnt = float(T * N)
    if s[2] != cnt:
        bad.append((label, "stats[2]", s[2], cnt))
    u = cnt * 2.0 ** -52
    if not abs(s[0] - c["sum"]) <= u * c["abs"]:
        bad.append((label, "stats[0]", s[0], c["sum"], u * c["abs"]))
    if not abs(s[1] - c["sumsq"]) <= u * c["sumsq"]:
        bad.append((label, "stats[1]", s[1], c["sumsq"], u * c["sumsq"]))
    st["sum"] = (abs(s[0] - c["sum"]), 0.0, abs(s[0] - c["sum"]) / (u * c["abs"]) if c["abs"] > 0 else float(s[0] != c["sum"]), 0.0)
    st["sumsq"] = (abs(s[1] - c["sumsq"]), 0.0, abs(s[1] - c["sumsq"]) / (u * c["sumsq"]) if c["sumsq"] > 0 else float(s[1] != c["sumsq"]), 0.0)
    if T * N > 1:
        bad += gae_judge_adv(c, got["adv"], st, label)
    return bad, st


def gae_judge_adv(c, adv, st, label="", name="adv"):
    """the normalised advantages [T, N] of case c (one rank, or the two halves put together)"""
    bad = []
    if bool(torch.isnan(adv).any()):
        bad.append((label, name, "NaN"))
    if c["regime"] in ("zero", "const"):
        if not bool((adv == 0).all()):
            bad.append((label, name, "a constant advantage does not normalise to exactly 0", float(adv.abs().max())))
        st[name] = (float(adv.abs().max()), 0.0, 0.0, 0.0)
        return bad
    nb, first, st[name] = PR.per_element(adv, c["ref_adv"], c["yard_adv"], FLOOR["value"], c["ref_adv"].abs().clamp(min=1.0))
    if nb:
        bad.append((label, name, "against fp64", nb, first))
    return bad


# ------------------------------------------------------------------------------------------------------------------------ PPO loss
# catan_ppo_loss: min(256, ceil(B / 1024)) workgroups of 256 lanes, grid-stride; the workgroup that arrives last folds the partials.
LOSS_ROWS = (1, 2, 255, 256, 257, 1024, 1025, 4097, 65537, 261120, 261121, 262145)
LOSS_REGIMES = ("unit", "onpolicy", "far", "planted")
CLIPS = (0.2, 0.25, 0.0)
COEFS = (1.0, 0.5)
NORM = (150.0, 150.0)
OLD0 = -2.5
# (logp - old, adv): adv = 0 inside and outside; the four sign pairs outside; inside; ratio exactly 1; ratio = +inf; ratio = 0
POLICY_PLANTS = ((0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (0.125, 1.0), (0.125, -1.0),
                 (0.0, 1.5), (100.0, 1.0), (100.0, -1.0), (-200.0, 1.0), (-200.0, -1.0))
# (v, vp, ret) at clip = 0.25: v - vp = +clip, -clip; v == vp; the vin tie e1 == e2; the symmetric tie e1 == -e2 outside, and mirrored;
# outside with l1 > l2; outside with l2 > l1 (gradient 0); inside
VALUE_PLANTS = ((0.25, 0.0, 1.0), (-0.25, 0.0, 1.0), (0.5, 0.5, 0.125), (0.5, 0.375, 0.25), (0.75, 0.0, 0.5), (-0.75, 0.0, -0.5),
                (1.0, 0.0, 0.25), (1.0, 0.0, 2.0), (0.125, 0.0, 2.0))
SYM_TIE = 4                                                               # VALUE_PLANTS[4]: expected d_values = value_coef 0.5 e1 / B


def loss_configs(B):
    """-> [(regime, use_norm, value_coef, clip)] of one row count: every regime with the normaliser off and on, clip and value_coef going
    round with the case; `planted` (B >= 16) at clip 0.25 and 0 with it off, at 0.25 with it on"""
    out, k = [], LOSS_ROWS.index(B)
    for regime in LOSS_REGIMES[:3]:
        for use_norm in (False, True):
            out.append((regime, use_norm, COEFS[k % 2], CLIPS[k % 3]))
            k += 1
    if B >= 16:
        out += [("planted", False, COEFS[k % 2], 0.25), ("planted", False, COEFS[(k + 1) % 2], 0.0), ("planted", True, COEFS[k % 2], 0.25)]
    return out


def plant_positions(B):
    """the rows of the planted cases: 0, B - 1, 255 and 256 where they exist, the rest spread evenly -> len(POLICY_PLANTS) distinct rows"""
    n = len(POLICY_PLANTS)
    pos = [0, B - 1] + [x for x in (255, 256) if x < B - 1]
    for j in range(1, 4 * n):
        x = (j * B) // (n + 3)
        if len(pos) < n and 0 < x < B - 1 and x not in pos:
            pos.append(x)
    for x in range(1, B):                                                  # (a B too small to spread: the first free rows)
        if len(pos) < n and x not in pos:
            pos.append(x)
    assert len(pos) == n == len(set(pos))
    return pos


def loss_inputs(B, regime, use_norm):
    """-> {logp, old, adv, v, v_old, ret (fp32 [B]), planted (bool [B])}"""
    g = PR.gen("loss", B, regime, int(use_norm))
    old = OLD0 + 0.4 * torch.randn(B, generator=g)
    d = 0.3 * torch.randn(B, generator=g)
    if regime == "onpolicy":
        d = torch.zeros(B)
    elif regime == "far":
        d = (3.0 * torch.randn(B, generator=g)).clamp(-80.0, 80.0)
    adv = torch.randn(B, generator=g)
    v = torch.randn(B, generator=g)
    vp = v + 0.3 * torch.randn(B, generator=g)
    ret = torch.randn(B, generator=g)
    logp = old + d
    planted = torch.zeros(B, dtype=torch.bool)
    if regime == "planted":
        for k, row in enumerate(plant_positions(B)):
            dd, aa = POLICY_PLANTS[k]
            old[row], logp[row], adv[row] = OLD0, OLD0 + dd, aa
            if not use_norm:
                v[row], vp[row], ret[row] = VALUE_PLANTS[k % len(VALUE_PLANTS)]
            planted[row] = True
    if use_norm:                                                           # old values and returns 150 +- 150
        vp, ret = NORM[0] + NORM[1] * vp, NORM[0] + NORM[1] * ret
    return {"logp": logp, "old": old, "adv": adv, "v": v, "v_old": vp, "ret": ret, "planted": planted, "B": B}


def _nan_where(x, *srcs):
    bad = torch.zeros_like(x, dtype=torch.bool)
    for s in srcs:
        bad = bad | torch.isnan(s)
    return torch.where(bad, torch.full_like(x, NAN), x)


def loss_eval(c, clip, value_coef, use_norm, wd, plant=None, detail=False):
    """the closed form in dtype wd -> {losses [2], d_logp [B], d_values [B]} (detail: the per-row quantities too)"""
    logp, old, adv, v, vp, ret = (c[k].to(wd) for k in ("logp", "old", "adv", "v", "v_old", "ret"))
    B = logp.numel()
    if use_norm:
        vp, ret = (vp - NORM[0]) / (NORM[1] + 1e-4), (ret - NORM[0]) / (NORM[1] + 1e-4)
    lo, hi = 1.0 - clip, 1.0 + clip
    ratio = torch.exp(logp - old)
    ratio = torch.where(ratio > FLT_MAX, torch.full_like(ratio, INF), ratio)
    ratio = torch.where(ratio < 2.0 ** -150, torch.zeros_like(ratio), ratio)
    s1 = ratio * adv
    s2 = torch.clamp(ratio, lo, hi) * adv
    ta = -torch.min(s1, s2)
    inside = (ratio >= lo) & (ratio <= hi)
    act = inside if plant == "inside_only" else ((s1 <= s2) | inside)
    zero = torch.zeros_like(s1)
    d_logp = _nan_where(torch.where(act, -s1 / B, zero), s1, s2)
    dv = v - vp
    vc = vp + dv.clamp(-clip, clip)
    e1, e2 = v - ret, vc - ret
    l1, l2 = e1 * e1, e2 * e2
    tv = (1.0 if plant == "no_half" else 0.5) * torch.max(l1, l2)
    vin = ((dv > -clip) & (dv < clip)) if plant == "vin_lt" else ((dv >= -clip) & (dv <= clip))
    e2v = torch.where(vin, e2, zero)
    sel = torch.where(l1 > l2, e1, torch.where(l1 < l2, e2v, 0.5 * (e1 + e2v)))
    d_values = _nan_where(value_coef / B * sel, l1, l2)
    out = {"losses": torch.stack([ta.mean(), tv.mean()]), "d_logp": d_logp, "d_values": d_values}
    if detail:
        out.update(ratio=ratio, s1=s1, s2=s2, ta=ta, tv=tv, dv=dv, l1=l1, l2=l2, e1=e1, e2=e2, e2v=e2v, lo=lo, hi=hi)
    return out


def loss_autograd(c, clip, value_coef, use_norm):
    """torch autograd in float64 on the formula of ppo.py:46-66 -> {losses, d_logp, d_values}"""
    t = {k: c[k].double() for k in ("logp", "old", "adv", "v", "v_old", "ret")}
    logp, v = t["logp"].clone().requires_grad_(True), t["v"].clone().requires_grad_(True)
    vp, ret = t["v_old"], t["ret"]
    if use_norm:
        vp, ret = (vp - NORM[0]) / (NORM[1] + 1e-4), (ret - NORM[0]) / (NORM[1] + 1e-4)
    ratio = torch.exp(logp - t["old"])
    al = -torch.min(ratio * t["adv"], torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * t["adv"]).mean()
    vpc = vp + (v - vp).clamp(-clip, clip)
    vl = 0.5 * torch.max((v - ret).pow(2), (vpc - ret).pow(2)).mean()
    (vl * value_coef + al).backward()
    return {"losses": torch.stack([al.detach(), vl.detach()]), "d_logp": logp.grad, "d_values": v.grad}


def near_boundary(c, ref):
    """-> {ratio, vclip, l1l2 (bool [B])}: the rows whose fp64 quantity lies within a relative 2^-18 of its branch boundary (ref: the
    detail of loss_eval in fp64).  Planted rows and rows with logp == old (ratio exactly 1 in every format) are never among them."""
    ratio, lo, hi = ref["ratio"], ref["lo"], ref["hi"]
    free = ~c["planted"]
    moved = (c["logp"] != c["old"]) & free
    nr = moved & (((ratio - lo).abs() <= BAND * lo) | ((ratio - hi).abs() <= BAND * hi))
    # s1 against s2 outside the clip range: |ratio - rc| |adv| against |ratio adv| - the same band on the ratio (adv = 0: both 0, no branch)
    clip = hi - 1.0
    gap = ref["dv"].abs()
    nv = free & ((gap - clip).abs() <= BAND * clip)
    nl = free & (gap > clip) & ((ref["l1"] - ref["l2"]).abs() <= BAND * torch.maximum(ref["l1"], ref["l2"]))
    return {"ratio": nr, "vclip": nv, "l1l2": nl}


@functools.lru_cache(maxsize=None)
def loss_case(B, regime, use_norm, value_coef, clip):
    c = loss_inputs(B, regime, use_norm)
    ref = loss_eval(c, clip, value_coef, use_norm, torch.float64, detail=True)
    yard = loss_eval(c, clip, value_coef, use_norm, torch.float32)
    c.update(regime=regime, use_norm=use_norm, value_coef=value_coef, clip=clip, ref=ref, yard=yard, near=near_boundary(c, ref))
    return c


def _either(kernel, cands, yard, floor, rows):
    """near-boundary rows: the kernel's value equals one of the candidates under the rule, with the yardstick's error against ITS nearest
    candidate and the largest candidate magnitude as the scale -> bool [rows]"""
    k, y = kernel.double()[rows], yard.double()[rows]
    cs = torch.stack([x[rows] for x in cands])
    ey = (y[None] - cs).abs().amin(0)
    bound = 2.0 * ey + floor * cs.abs().amax(0)
    return ((k[None] - cs).abs() <= bound[None]).any(0)


def loss_judge(c, got):
    """everything asked of one catan_ppo_loss launch of case `c`: got = {losses [2], d_logp [B], d_values [B]} -> (failures, stats)"""
    ref, yard, B = c["ref"], c["yard"], c["B"]
    bad, st = [], {}
    for i, (n, t) in enumerate((("action_loss", "ta"), ("value_loss", "tv"))):
        scale = float(ref[t].abs().mean())
        nb, _, st[n] = PR.per_element(got["losses"][i:i + 1], ref["losses"][i:i + 1], yard["losses"][i:i + 1], FLOOR["value"], scale)
        if nb:
            bad.append((n, float(got["losses"][i]), float(ref["losses"][i]), float(yard["losses"][i])))
    near_p, near_v = c["near"]["ratio"], c["near"]["vclip"] | c["near"]["l1l2"]
    zero = torch.zeros_like(ref["d_logp"])
    for n, near, cands in (("d_logp", near_p, (ref["d_logp"], zero)),
                           ("d_values", near_v, tuple(c["value_coef"] / B * x for x in (ref["e1"], ref["e2"], zero, 0.5 * (ref["e1"] + ref["e2"]), 0.5 * ref["e1"])))):
        k = got[n].clone()
        if bool(near.any()):
            ok = _either(got[n], cands, yard[n], FLOOR["grad"], near)
            if not bool(ok.all()):
                bad.append((n, "near-boundary rows on neither branch", near.nonzero().flatten()[~ok].tolist()[:8]))
            k[near] = ref[n][near].float()                                 # (judged above)
        nb, first, st[n] = PR.per_element(k, ref[n], yard[n], FLOOR["grad"], ref[n].abs())
        if nb:
            bad.append((n, f"{nb} rows, first {first}", float(got[n][first]), float(ref[n][first]), float(yard[n][first])))
    if c["regime"] == "onpolicy":
        want = -c["adv"] * (torch.tensor(1.0) / torch.tensor(float(B)))
        if not bool((got["d_logp"] == want).all()):
            bad.append(("d_logp", "on policy: not bit-equal to -adv * (1 / B)"))
    return bad, st


# --------------------------------------------------------------------------------------------------------------------------- Adam
# catan_adam_step: one workgroup per chunk of 2 048 elements (a chunk never spans two tensors); k_adam_step's lanes stride over the
# per-chunk partial sums: a second trip from 257 chunks.
CHUNK = 2048
HYPER = {"lr": 3e-4, "eps": 1e-5, "betas": (0.9, 0.999)}
MAX_NORM = 0.5
STEP_COUNTS = (0, 1, 10, 1000, 100000)
ADAM_LISTS = {"one": (1,), "tails": (3, 4, 5, 2047, 2048, 2049, 4099), "c255": (255 * CHUNK,), "c256": (256 * CHUNK,), "c257": (256 * CHUNK + 1,),
              "trips": (CHUNK * 600 + 7, 5)}
ADAM_REGIMES = ("unit", "small", "large", "zero", "mixed", "threshold", "none_skip", "none_zero")
ADAM_STEPS = 3
ADAM_CASES = tuple([("tails", r, mn) for r in ADAM_REGIMES for mn in (MAX_NORM, None)]
                   + [("one", r, MAX_NORM) for r in ("unit", "small", "large", "threshold")] + [("one", "unit", None)]
                   + [("c255", "unit", MAX_NORM), ("c256", "large", MAX_NORM), ("c257", "small", MAX_NORM), ("c257", "unit", None), ("c256", "threshold", MAX_NORM),
                      ("trips", "unit", MAX_NORM), ("trips", "mixed", None), ("trips", "threshold", MAX_NORM)])
ZERO_TENSOR, NONE_TENSORS, LOUD_TENSOR = 3, (1, 5), 0


def step_count(i):
    """the loaded step count of tensor i: 1 for the first (a list of one tensor has state), every count of STEP_COUNTS from five tensors"""
    return STEP_COUNTS[(i + 1) % len(STEP_COUNTS)]


def _away(x):
    """|x| >= 0.05, the sign kept (0 counts as positive)"""
    return torch.where(x.abs() < 0.05, torch.where(x < 0, -0.05, 0.05).to(x.dtype), x)


def grad_norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))


def to_threshold(grads):
    """scales the gradients in fp64 so that their norm, rounded to fp32, is max_norm = 0.5 to the last bit"""
    for _ in range(30):
        n = grad_norm64(grads)
        if float(torch.tensor(n, dtype=torch.float64).float()) == MAX_NORM and abs(n - MAX_NORM) < 2.0 ** -27:
            break
        grads = [(g.double() * (MAX_NORM / n)).float() for g in grads]
    return grads


@functools.lru_cache(maxsize=None)
def adam_case(name, regime, max_norm):
    """-> {sizes, p0, m0, v0 (lists of fp32), steps0, grads [ADAM_STEPS][tensor] (fp32 or None), none_is_zero, max_norm}"""
    sizes = ADAM_LISTS[name]
    g = PR.gen("adam", name, regime, 0 if max_norm is None else 1)
    scale = {"unit": 0.05, "small": 1e-15, "large": 1e15, "zero": 0.05, "mixed": 1e-4, "threshold": 0.05, "none_skip": 0.05, "none_zero": 0.05}[regime]
    scales = [1e3 if (regime == "mixed" and i == LOUD_TENSOR) else scale for i in range(len(sizes))]
    steps0 = [step_count(i) for i in range(len(sizes))]
    p0 = [0.1 * torch.randn(n, generator=g) for n in sizes]
    m0 = [(s * (4.0 + 4.0 * torch.rand(n, generator=g))) * (t > 0) for n, s, t in zip(sizes, scales, steps0)]
    v0 = [(s * s * (0.1 + 0.9 * torch.rand(n, generator=g))) * (t > 0) for n, s, t in zip(sizes, scales, steps0)]
    g1 = [s * _away(torch.randn(n, generator=g)) for n, s in zip(sizes, scales)]
    if regime == "threshold":
        g1 = to_threshold(g1)
    grads = [g1]
    for k in range(1, ADAM_STEPS):                                         # the same signs, other sizes: see the module docstring
        f = (0.7, 1.3)[k - 1]
        grads.append([x * (f * (0.5 + torch.rand(x.shape, generator=g))) for x in g1])
    if regime == "zero" and len(sizes) > ZERO_TENSOR:
        for gs in grads:
            gs[ZERO_TENSOR] = torch.zeros(sizes[ZERO_TENSOR])
    if regime.startswith("none"):
        for gs in grads:
            for i in NONE_TENSORS:
                gs[i] = None
    return {"name": name, "regime": regime, "sizes": sizes, "p0": p0, "m0": m0, "v0": v0, "steps0": steps0, "grads": grads,
            "none_is_zero": regime == "none_zero", "max_norm": max_norm}


def adam_ref(c, wd=torch.float64, plant=None):
    """the update written out in dtype wd -> [per step {p, m, v (lists), norm, steps}]"""
    lr, eps, (b1, b2) = HYPER["lr"], HYPER["eps"], HYPER["betas"]
    p, m, v = ([x.to(wd).clone() for x in c[k]] for k in ("p0", "m0", "v0"))
    steps = list(c["steps0"])
    out = []
    for gs in c["grads"]:
        present = [x.to(wd) for x in gs if x is not None]
        norm = torch.sqrt(sum((x * x).sum() for x in present)) if present else torch.zeros((), dtype=wd)
        coef = torch.clamp(c["max_norm"] / (norm + 1e-6), max=1.0) if c["max_norm"] is not None else torch.ones((), dtype=wd)
        for i, x in enumerate(gs):
            if x is None and not c["none_is_zero"]:
                continue
            steps[i] += 1
            gc = torch.zeros_like(p[i]) if x is None else x.to(wd) * coef
            m[i] = m[i] + (gc - m[i]) * (1.0 - b1)
            v[i] = v[i] * b2 + (1.0 - b2) * gc * gc
            bc1, bc2s = 1.0 - b1 ** steps[i], math.sqrt(1.0 - b2 ** steps[i])
            denom = v[i].sqrt() / (bc2s + eps) if plant == "bias_eps" else v[i].sqrt() / bc2s + eps
            p[i] = p[i] - (lr if plant == "no_bias1" else lr / bc1) * (m[i] / denom)
        out.append({"p": [x.clone() for x in p], "m": [x.clone() for x in m], "v": [x.clone() for x in v], "norm": float(norm), "steps": list(steps)})
    return out


def adam_torch(c, wd=torch.float32):
    """torch.optim.Adam(foreach=False) behind clip_grad_norm_ in dtype wd -> the same list"""
    ps = [x.to(wd).clone().requires_grad_(True) for x in c["p0"]]
    opt = torch.optim.Adam(ps, lr=HYPER["lr"], eps=HYPER["eps"], betas=HYPER["betas"], foreach=False)
    for q, m, v, t in zip(ps, c["m0"], c["v0"], c["steps0"]):
        if t > 0:
            opt.state[q] = {"step": torch.tensor(float(t)), "exp_avg": m.to(wd).clone(), "exp_avg_sq": v.to(wd).clone()}
    out = []
    for gs in c["grads"]:
        for q, x in zip(ps, gs):
            q.grad = (torch.zeros_like(q) if c["none_is_zero"] else None) if x is None else x.to(wd).clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, INF if c["max_norm"] is None else c["max_norm"], foreach=False)
        opt.step()
        st = [opt.state[q] if q in opt.state else None for q in ps]
        out.append({"p": [q.detach().clone() for q in ps],
                    "m": [torch.zeros_like(q) if s is None else s["exp_avg"].clone() for q, s in zip(ps, st)],
                    "v": [torch.zeros_like(q) if s is None else s["exp_avg_sq"].clone() for q, s in zip(ps, st)],
                    "norm": float(norm), "steps": [0 if s is None else int(float(s["step"])) for s in st]})
    return out


@functools.lru_cache(maxsize=None)
def adam_expected(name, regime, max_norm):
    c = adam_case(name, regime, max_norm)
    return c, adam_ref(c), adam_torch(c)


def adam_judge(c, ref, yard, k, got):
    """step k (0-based) of case c: got = {p, m, v (lists of fp32), norm (float), steps} -> (failures, stats)"""
    bad, st = [], {}
    before = c["p0"] if k == 0 else ref[k - 1]["p"]
    for i in range(len(c["sizes"])):
        pscale = before[i].double().abs().clamp(min=HYPER["lr"])
        for n, scale in (("p", pscale), ("m", ref[k]["m"][i].abs()), ("v", ref[k]["v"][i].abs())):
            nb, first, s = PR.per_element(got[n][i], ref[k][n][i], yard[k][n][i], FLOOR["grad"], scale)
            PR.merge_stat(st, n, s)
            if nb:
                bad.append((k, n, i, f"{nb} elements, first {first}", float(got[n][i][first]), float(ref[k][n][i][first]), float(yard[k][n][i][first])))
    nb, _, st["norm"] = PR.per_element(torch.tensor([got["norm"]]), torch.tensor([ref[k]["norm"]], dtype=torch.float64), torch.tensor([yard[k]["norm"]]),
                              FLOOR["value"], ref[k]["norm"])
    if nb:
        bad.append((k, "norm", got["norm"], ref[k]["norm"], yard[k]["norm"]))
    if list(got["steps"]) != ref[k]["steps"] or ref[k]["steps"] != yard[k]["steps"]:
        bad.append((k, "step counts", list(got["steps"]), ref[k]["steps"], yard[k]["steps"]))
    return bad, st
