"""Plain-torch restatement of the LayerNorm (+ fused ReLU) kernels of csrc/catan_nn.hip (k_ln_*, k_lnw_*, k_lnr_*; catan_layer_norm_fwd /
catan_layer_norm_bwd), with the seeded case builders and the launch table that tests/test_layer_norm_reference_cpu.py and
tests/test_gpu_layer_norm_fp64.py share.  No call into the library or into nn_kernels: torch ops only, on the CPU or the GPU.

    mean = sum_j x_j / D      c = x - mean      rstd = (sum_j c_j^2 / D + eps)^-1/2      x_hat = c rstd      (biased, TWO-pass variance)
    pre = x_hat w + b         y = relu ? max(pre, 0) : pre
    g = dy, and 0 where relu and pre <= 0        (torch's relu backward: no gradient AT 0)
    dw_j = sum_r g x_hat      db_j = sum_r g      dx = rstd (g w - mean_j(g w) - x_hat mean_j(g w x_hat))              (closed form)

  ln_fwd_ref / ln_bwd_ref   the REFERENCE: fp64 throughout from the inputs as stored (bf16 inputs upcast exactly).
  ln_yardstick              the same formulas in fp32, x - mean as the one fused multiply-add the kernels perform; bf16 storage rounds ONCE, at the store of y and of dx - the kernels keep x_hat, the
                            gate and the moments in fp32.  dw / db are fp32 sums of fp32 per-row terms in both storage types.  It shows
                            what the number formats cost against the reference; it is not an oracle.  `plant` is NOT part of it: the planted
                            errors of the CPU test's rejection cases (PLANTS).

Acceptance: the rule of tests/pin_rule.py.  y, dx: floor pin_rule.BF16_FLOOR (bf16) / FP32_FLOOR (fp32), over the whole case (`accept`)
and for every row with that row's own yardstick error and scale (`per_row`).  dw, db: pin_rule.sum_bound per column, with `depth` =
iterations per lane + rows per block + blocks (`launch_depth`, from the launch table below)."""
import math

import torch

from pin_rule import BF16_FLOOR, per_group, rbf, whole, whole_bound

EPS = 1e-5
WIDTHS = (16, 25, 32, 64, 128, 256, 512)
FP32_FLOOR = {"y": 2.0 ** -17, "dx": 2.0 ** -15}        # the attention suite's for out / dq: the same kind of arithmetic
PLANTS = ("one_pass", "d_minus_1", "eps_outside", "no_m2", "gate_lt", "dw_ungated", "swap_pairs", "drop_last", "dw_scale")

# ------------------------------------------------------------------------------------------------------------------- launch table
# ln_dispatch / ln_launch / lnw_launch (csrc/catan_abi_nn_launch.h): 256 threads, GL lanes per row, RPB = 256 / GL rows per block and pass; the
# grid is ceil(rows / RPB) blocks up to a cap, above which a block's grid-stride loop runs again.  k_lnr: a lane per row, 256 rows per block.
FWD_CAP = 8192
BWD_CAP = {"ln": 2048, "lnw": 1024, "lnr": 2048}
LNR_MIN_ROWS = 4096
LNR_CAP = 2048                                           # forward and backward
ALIGNED_GL = {16: ("ln", 16), 25: ("ln", 32), 32: ("ln", 32), 64: ("lnw", 8), 128: ("lnw", 16), 256: ("lnw", 32), 512: ("lnw", 64)}
MISALIGNED_GL = {16: ("ln", 16), 25: ("ln", 32), 32: ("ln", 32), 64: ("ln", 64)}
# (name, D, dtype, align): align "aligned" = every tensor 16-byte aligned, "misaligned" = every tensor one element into an aligned
# allocation, "lnr" = aligned, bf16, D = 25 and rows >= 4096
PATHS = ([("aligned", D, dt) for D in WIDTHS for dt in ("float32", "bfloat16")]
         + [("misaligned", D, dt) for D in (16, 25, 32, 64) for dt in ("float32", "bfloat16")] + [("lnr", 25, "bfloat16")])


def path_kernel(align, D):
    """-> (family, rows per block) of the kernel the path's launches take"""
    if align == "lnr":
        return "lnr", 256
    fam, GL = (MISALIGNED_GL if align == "misaligned" else ALIGNED_GL)[D]
    return fam, 256 // GL


def path_rows(align, D, dtype):
    """-> [(rows, forward_only)]: 1, RPB - 1, RPB, RPB + 1, 255, 257, and both sides of the forward and of the backward cap (the forward
    cap's counts are launched forward only).  The aligned bf16 D = 25 path ends at 4095 (k_ln<25, 32>'s last row count); k_lnr takes
    4096, 4097, 4099 (rows * 25 not a multiple of 8: a 16-byte tail piece), 4351 (a last workgroup of 255 rows), 4352 = 17 * 256, and both
    sides of its cap, where a workgroup's loop runs twice."""
    fam, rpb = path_kernel(align, D)
    if align == "lnr":
        return [(r, False) for r in (4096, 4097, 4099, 4351, 4352, LNR_CAP * 256, LNR_CAP * 256 + 1)]
    small = sorted({r for r in (1, rpb - 1, rpb, rpb + 1, 255, 257) if r >= 1})
    if align == "aligned" and D == 25 and dtype == "bfloat16":
        return [(r, False) for r in small + [LNR_MIN_ROWS - 1]]
    bwd, fwd = BWD_CAP[fam] * rpb, FWD_CAP * rpb
    return [(r, False) for r in small + [bwd, bwd + 1]] + [(fwd, True), (fwd + 1, True)]


def launch_depth(align, D, rows):
    """the longest chain of fp32 additions a backward launch can form for one dw / db column: iterations per lane + rows per block (the
    block's reduction; for k_lnr the wave shuffles and the LDS atomics, at most its 256 lanes) + blocks (the global atomics)"""
    fam, rpb = path_kernel(align, D)
    blocks = min(BWD_CAP[fam], -(-rows // rpb))
    iters = -(-rows // (blocks * rpb))
    return iters + rpb + blocks


# ---------------------------------------------------------------------------------------------------------------------- formulas
def _core(x, w, b, dy, eps, relu, wd, plant=None):
    """everything in dtype wd -> {pre, y, dx, dw, db, aw, ab} (aw, ab = sum_r |term| in fp64); dy None: forward only"""
    x, w, b = x.to(wd), w.to(wd), b.to(wd)
    dy = None if dy is None else dy.to(wd)
    D = x.shape[-1]
    if plant == "drop_last":                                        # D treated as D - 1: the last column never touched
        o = _core(x[:, :D - 1], w[:D - 1], b[:D - 1], None if dy is None else dy[:, :D - 1], eps, relu, wd)
        pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (1,), dtype=t.dtype, device=t.device)], -1)
        return {k: pad(v) for k, v in o.items()}
    inv = 1.0 / D
    tot = x.sum(-1, keepdim=True)
    mean = tot * inv
    if wd == torch.float32:
        # the kernels never round the mean on its own: the compiler contracts x - sum * (1.0f / D) into one fused multiply-add, so at
        # D = 25, where fp32's 1 / 25 is 2.2e-8 short, c carries 2.2e-8 |mean| instead of the mean's rounding (the product of two fp32
        # numbers is exact in fp64, so this is that fma but for a second rounding at 2^-53)
        c = (x.double() - tot.double() * torch.tensor(inv, dtype=torch.float32).double()).float()
    else:
        c = x - mean
    if plant == "one_pass":
        var = ((x * x).sum(-1, keepdim=True) * inv - mean * mean).clamp_min(0.0)
    elif plant == "d_minus_1":
        var = (c * c).sum(-1, keepdim=True) / (D - 1)
    else:
        var = (c * c).sum(-1, keepdim=True) * inv
    rstd = 1.0 / (var.sqrt() + eps) if plant == "eps_outside" else (var + eps) ** -0.5
    xh = c * rstd
    pre = xh * w + b
    out = {"pre": pre, "y": pre.clamp_min(0.0) if relu else pre}
    if dy is not None:
        g = dy
        if relu:
            g = torch.where((pre < 0) if plant == "gate_lt" else (pre <= 0), torch.zeros((), dtype=wd, device=x.device), dy)
        tw = (dy if plant == "dw_ungated" else g) * xh
        gw = g * w
        m1 = gw.sum(-1, keepdim=True) * inv
        m2 = (gw * xh).sum(-1, keepdim=True) * inv
        out["dx"] = rstd * (gw - m1) if plant == "no_m2" else rstd * (gw - m1 - xh * m2)
        out["dw"] = tw.sum(0) * (1.03 if plant == "dw_scale" else 1.0)
        out["db"] = g.sum(0)
        out["aw"], out["ab"] = tw.double().abs().sum(0), g.double().abs().sum(0)
    if plant == "swap_pairs":                                       # columns 2k and 2k + 1 exchanged in everything that leaves
        idx = torch.arange(D, device=x.device)
        idx[:D - D % 2] ^= 1
        out = {k: v[..., idx] for k, v in out.items()}
    return out


def ln_fwd_ref(x, w, b, eps, relu):
    return _core(x, w, b, None, eps, relu, torch.float64)["y"]


def ln_bwd_ref(x, w, b, dy, eps, relu):
    """-> (dx, dw, db), fp64"""
    o = _core(x, w, b, dy, eps, relu, torch.float64)
    return o["dx"], o["dw"], o["db"]


def ln_ref(x, w, b, dy, eps, relu):
    """the reference's whole dict (pre, y, and with dy: dx, dw, db, aw, ab)"""
    return _core(x, w, b, dy, eps, relu, torch.float64)


def ln_yardstick(x, w, b, dy, eps, relu, bf16, plant=None):
    o = _core(x, w, b, dy, eps, relu, torch.float32, plant)
    if bf16:
        o["y"] = rbf(o["y"])
        if "dx" in o:
            o["dx"] = rbf(o["dx"])
    return o


def gate_delta(x, w, b, eps):
    """the rule's bound on an fp32 pre-activation of the case: 2 maxabs(fp32 - fp64) + 2^-17 maxabs(fp64)"""
    p64 = _core(x, w, b, None, eps, False, torch.float64)["pre"]
    p32 = _core(x, w, b, None, eps, False, torch.float32)["pre"]
    return whole_bound(p64, p32, FP32_FLOOR["y"])[0]


def near_gate(x, w, b, eps, delta):
    """[rows, D] bool: the elements whose fp64 pre-activation lies within delta of 0"""
    return _core(x, w, b, None, eps, False, torch.float64)["pre"].abs() <= delta


def gated_dy(case):
    """the ReLU regime's dy: 0 at every element near_gate marks (delta = gate_delta), where fp32 may decide the gate either way - except
    on the case's exact rows, whose pre-activation is b to the bit in the kernels and in the reference -> (dy, zeroed share, delta)"""
    x, w, b, dy = case["x"], case["w"], case["b"], case["dy"]
    delta = gate_delta(x, w, b, EPS)
    near = near_gate(x, w, b, EPS, delta)
    for r in case["exact_rows"]:
        near[r] = False
    return torch.where(near, torch.zeros((), dtype=dy.dtype, device=dy.device), dy), float(near.double().mean()), delta


# -------------------------------------------------------------------------------------------------------------------------- rule
def accept(bf16, name, kernel, ref, yardstick):
    """pin_rule.whole for y or dx with the floor of the storage type -> (ok, kernel error, yardstick error, bound)"""
    return whole(kernel, ref, yardstick, BF16_FLOOR if bf16 else FP32_FLOOR[name])


def per_row(bf16, name, kernel, ref, yardstick):
    """pin_rule.per_group with that floor: every row with ITS yardstick error and ITS scale -> (ok [rows], kernel error [rows], bound [rows])"""
    return per_group(kernel, ref, yardstick, BF16_FLOOR if bf16 else FP32_FLOOR[name])


# ------------------------------------------------------------------------------------------------------------------------- cases
def planted_rows(D, rows, edge):
    """-> (zero rows, constant rows) of a unit case: row 0, both sides of the first block edge (edge - 1, edge) and the last row,
    alternately all-zero and constant at 1.5; all-zero only where D is no power of two (25 * (1 / 25) is not exact in fp32, so a
    constant row there is no exact row); none below 3 rows, which stay ordinary."""
    if rows < 3:
        return [], []
    at = sorted({r for r in (0, edge - 1, edge, rows - 1) if 0 <= r < rows})
    pow2 = D & (D - 1) == 0
    return [r for k, r in enumerate(at) if k % 2 == 0 or not pow2], [r for k, r in enumerate(at) if k % 2 == 1 and pow2]


def make_case(D, rows, regime, edge, dtype, seed=0):
    """-> {x, dy [rows, D] of `dtype`; w, b fp32 [D]; zero_rows, const_rows, exact_rows} on the CPU, drawn in fp32 and then stored.
    w, b, the column scales of x and of dy differ from column to column: no permutation of columns, lanes or element pairs maps a case
    onto itself.  b is exactly 0 in the columns j % 8 == 2, 0.7 in column 0, -0.9 in column 1 and at least 0.05 from 0 elsewhere.
    "unit":   x = randn * row scale * column scale + row mean, row means -1 .. 2, row scales 2.5 .. 0.5, with planted_rows written over it.
    "offset": row r is m_r + s_r k, m_r an integer of 64 .. 255, s_r the bf16 spacing there (0.5 below 128, 1 from 128), k = 1 in about
              an eighth of the columns (at least one) and 0 in the others (at least one): every value is representable in bf16, the
              variance is about 0.1 s^2 under a mean^2 of up to 65 000 - where a one-pass variance loses its digits.  At a power-of-two
              D the mean of such a row is an fp32 number.  At D = 25 it is not, and what an fp32 evaluation makes of it (up to
              2^-24 * 256 * rstd in x_hat, the whole error of such a row) depends on where it rounds: the per-row and per-column
              rules would compare two evaluation orders, not a kernel with a yardstick.  So there k is +1 in round(D / 16) columns, -1 in as many and 0 elsewhere: the mean is m_r
              exactly, and sum x^2 * (1 / 25) still rounds at 65 000, so one pass still shows.  The columns where b == 0 are always
              among the +-1 (a column at the mean has pre = b exactly, and near_gate would take every such element out of dy), the
              others and the signs are drawn per row."""
    assert regime in ("unit", "offset")
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * D + 31 * rows + (17 if regime == "unit" else 29))
    w = (1.0 + 0.6 * torch.randn(D, generator=g)) * 1.7
    b = 0.8 * torch.randn(D, generator=g) - 0.4
    b = torch.where(b.abs() < 0.05, torch.where(b < 0, -0.05, 0.05), b)
    b[0], b[1] = 0.7, -0.9
    b[torch.arange(D) % 8 == 2] = 0.0
    dy = torch.randn((rows, D), generator=g) * torch.linspace(0.25, 2.0, D) + 0.05
    zero_rows, const_rows = [], []
    if regime == "unit":
        mean = torch.linspace(-1.0, 2.0, rows)[:, None]
        scale = torch.linspace(2.5, 0.5, rows)[:, None]
        x = torch.randn((rows, D), generator=g) * scale * torch.linspace(0.6, 1.6, D) + mean
        zero_rows, const_rows = planted_rows(D, rows, edge)
        x[zero_rows] = 0.0
        x[const_rows] = 1.5
    else:
        m = torch.randint(64, 256, (rows, 1), generator=g).float()
        s = torch.where(m < 128, 0.5, 1.0)
        u = torch.rand((rows, D), generator=g)
        if D & (D - 1) == 0:
            k = (u < 0.125).float()
            r = torch.arange(rows)
            k[r, r % D] = 1.0
            k[r, (r + 1) % D] = 0.0
        else:
            zb = b == 0
            n = max(1, round(D / 16), (int(zb.sum()) + 1) // 2)
            chosen = (u - zb.float()).argsort(1).argsort(1) < 2 * n
            rank = (torch.rand((rows, D), generator=g) + 2.0 * (~chosen).float()).argsort(1).argsort(1)
            k = (rank < n).float() - ((rank >= n) & (rank < 2 * n)).float()
        x = m + s * k
        assert torch.equal(x.to(torch.bfloat16).float(), x)
    return {"x": x.to(dtype), "dy": dy.to(dtype), "w": w, "b": b, "zero_rows": zero_rows, "const_rows": const_rows,
            "exact_rows": zero_rows + const_rows, "D": D, "rows": rows, "regime": regime}


def positive_bias(case):
    """a bias under which every pre-activation is > 0 (|x_hat| <= sqrt(D - 1)): relu = 1 must then equal relu = 0 bit for bit"""
    return 1.0 + case["w"].abs() * math.sqrt(case["D"])
