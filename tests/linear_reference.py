"""Plain-torch restatement of the row-split linear kernels of csrc/catan_nn.hip and csrc/catan_wgrad_big.hip - k_linear_rows<KS, NT>
(catan_linear_rows / catan_linear_rows_fused), k_wgrad / k_wgrad_tr<OTW, IT> and their _grouped forms (catan_linear_wgrad /
catan_linear_wgrad_grouped), k_wgrad_big + k_wgrad_big_reduce (catan_linear_wgrad_big) - with the launch table of csrc/catan_abi_nn_launch.h, the
seeded case builders, the bounds and the planted errors that tests/test_linear_reference_cpu.py and tests/test_gpu_linear_fp64.py share.
No call into the library or into nn_kernels: torch ops only, on the CPU or the GPU.

    forward   a = x W^T + b      y = a (mode 0) | max(a, 0) (1) | a + aux (2) | a where aux > 0, else 0 (3)
    backward  dw = dy^T x        db = sum_r dy            each ADDED to what the accumulator held (the pre-fill)

  linear_ref / wgrad_ref    the REFERENCE: fp64 from the operands as stored (bf16 upcasts exactly).
  linear_yardstick          the same in fp32 with exactly the roundings the header specifies ("applied to the bf16-rounded product exactly as
                            the separate op would"): a is rounded to bf16; the epilogue (ReLU, + aux, the gate) is applied to that bf16
                            value; in mode 2 the fp32 sum is rounded to bf16 a second time.  It shows what the formats cost; it is not an oracle.
  wgrad_yardstick           fp32 product and sum.

Two regimes.
  exact   every operand is a small integer times a power of two, so every product and every partial sum in any order is exact in fp32
          (`*_headroom` asserts sum |term| + |pre-fill| < 2^24 in the operands' common unit for every case built): the kernel's result is
          fixed to the bit whatever the order inside the MFMA, of the stages or of the atomics.  Forward: x in {-4..4}/4, W in {-4..4}/8,
          bias multiples of 1/32 up to 4, aux multiples of 1/16 up to 4 with exact zeros; a quarter of the rows of x and of W carry one
          shared sign pattern, so that |a| reaches 16 .. 64 at K = 192 and the bf16 rounding moves elements by 1/16 and more, ties
          included.  Weight gradients: x, dy in {-3..3}, pre-fill integers up to 1000.
          y must equal the yardstick bit for bit (a zero may carry either sign); dw, db must equal pre-fill + reference exactly.
  real    randn times a linspace over the columns, an offset on dy; every row different; no subnormals.  Per element, with the summation
          unit U = 2^-23 (twice fp32's half-ulp: the ISA does not say that the MFMA's internal adder rounds to nearest; a derivation, not a
          measurement):
            y     S = sum_k |x_k W_nk| + |b_n|, e = (K + 1) U S:  |y - ref| <= e + 2^-8 (|a| + e)  (modes 0, 1, 3),
                  mode 2 adds 2^-8 (|a + aux| + that);  2^-8 = a bf16 half-ulp relative to the bottom of its binade
            dw,db |kernel - (pre-fill + ref)| <= depth U (sum_r |dy x| + |pre-fill|), depth = per + nb + 1 (k_wgrad / k_wgrad_tr) or
                  per + groups + 1 (k_wgrad_big) from the launch table
          and the rule of tests/pin_rule.py (floor BF16_FLOOR) over the case and for every row.
At ~10^5 rows the real-regime bound on a weight gradient is wider than one row's term - a dropped row would pass - so the exact regime
runs at EVERY row count and the real regime only below REAL_BELOW = 5 000 rows.  Nothing in a bound comes from a kernel."""
import torch

import pin_rule as PR

U = 2.0 ** -23
HALF_ULP_BF16 = 2.0 ** -8
REAL_BELOW = 5000
WG_KT = 64
WG_MAX_UNITS = 24
WB_T = 128


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------- launch table
LINROWS_KS = (1, 2, 3, 4, 6)
LINROWS_NT = (1, 2, 4, 8, 12)
LINROWS_INSTANCES = [(ks, nt) for ks in LINROWS_KS for nt in LINROWS_NT if ks * nt <= 32]        # 21
LINROWS_GRID_CAP = 2048


def _ks_nt(K, N):
    ks, nt = _cdiv(K, 32), _cdiv(N, 16)
    return (ks if ks <= 4 else 6), next(v for v in LINROWS_NT if nt <= v) if nt <= 12 else 99


def rows_supported(rows, K, N):
    """catan_linear_rows_supported"""
    if not (rows >= 1 and 8 <= K <= 192 and K % 8 == 0 and 1 <= N <= 192):
        return False
    ks, nt = _ks_nt(K, N)
    return ks * nt <= 32


def rows_launch(rows, K, N):
    """linrows_dispatch_nt -> {KS, NT, grid, passes}: 4 waves x 16 rows per block, the grid capped at 2048, above which a wave's
    grid-stride loop takes a second tile"""
    assert rows_supported(rows, K, N)
    ks, nt = _ks_nt(K, N)
    tiles = _cdiv(rows, 16)
    grid = min(_cdiv(tiles, 4), LINROWS_GRID_CAP)
    return {"KS": ks, "NT": nt, "grid": grid, "passes": _cdiv(tiles, grid * 4)}


def wgrad_sliced(I, O):
    return I + 1 > 160 and I <= 1024 and I % 8 == 0 and O % 8 == 0 and O <= 256


def wgrad_supported(rows, I, O):
    return rows >= 1 and (wgrad_sliced(I, O) or (I >= 1 and O >= 1 and I + 1 <= 160 and O <= 256))


def wgrad_grid(R, I, O):
    """wgrad_grid -> {stages, cap, spb, nb, per}: stages of 64 rows, 8 (16 from 131 072 rows) per block up to a cap that the tile size sets"""
    stages = _cdiv(R, WG_KT)
    tile = _cdiv(O, 16) * 16 * (_cdiv(I + 1, 16) * 16)
    cap = 256 if tile >= 24576 else (512 if tile >= 3072 else 1024)
    spb = 16 if R >= 131072 else 8
    nb = max(1, min(stages // spb, cap))
    per = _cdiv(stages, nb) * WG_KT
    return {"stages": stages, "cap": cap, "spb": spb, "nb": _cdiv(R, per), "per": per}


def wgrad_launches(R, I, O):
    """catan_linear_wgrad -> one dict per launch: {tr (the transposing-read staging), OTW, IT, col0, W, nb, per, db (whether this launch
    forms the bias gradient)}; a sliced input takes column slices of 128 through k_wgrad_tr<OTW, 10>, the first of which carries db"""
    assert wgrad_supported(R, I, O)
    otw = _cdiv(_cdiv(O, 16), 4)
    if wgrad_sliced(I, O):
        out = []
        for c0 in range(0, I, 128):
            W = min(128, I - c0)
            g = wgrad_grid(R, W, O)
            out.append({"tr": True, "OTW": otw, "IT": 10, "col0": c0, "W": W, "nb": g["nb"], "per": g["per"], "db": c0 == 0})
        return out
    it = _cdiv(I + 1, 16)
    g = wgrad_grid(R, I, O)
    return [{"tr": I % 8 == 0 and O % 8 == 0, "OTW": otw, "IT": 2 if it <= 2 else (5 if it <= 5 else 10), "col0": 0, "W": I,
             "nb": g["nb"], "per": g["per"], "db": True}]


WGRAD_INSTANCES = [(tr, otw, it) for tr in (True, False) for otw in (1, 2, 3, 4) for it in (2, 5, 10)]        # 24


def wgrad_depth(R, I, O):
    """the longest chain of fp32 additions into one dw / db element: the rows of a block, the blocks' atomics, the pre-fill"""
    return max(l["per"] + l["nb"] + 1 for l in wgrad_launches(R, I, O))


def big_supported(rows, I, O):
    return rows >= 1 and I >= 8 and I % 8 == 0 and O >= WB_T and O % WB_T == 0


def big_launch(rows, I, O):
    """catan_linear_wgrad_big -> {groups, per, tiles_o, tiles_i, blocks, workspace (floats)}"""
    assert big_supported(rows, I, O)
    groups = 16 if rows >= 65536 else 8
    per = _cdiv(_cdiv(rows, groups), WG_KT) * WG_KT
    tiles_o, tiles_i = O // WB_T, _cdiv(I + 1, WB_T)
    return {"groups": groups, "per": per, "tiles_o": tiles_o, "tiles_i": tiles_i, "blocks": groups * tiles_o * tiles_i,
            "workspace": groups * O * tiles_i * WB_T}


def big_depth(rows, I, O):
    g = big_launch(rows, I, O)
    return g["per"] + g["groups"] + 1


# ------------------------------------------------------------------------------------------------------- the GPU test's shapes
# catan_linear_rows: one (K, N) per instantiation.  K: a partial k-step (8, 24, 40, 72, 104), full ones (32, 64, 96, 128, 192), five k-steps
# in the six-step kernel (136, 160).  N: the element-wise store path (1, 25, 100), a partial n-tile (24, 40, 72, 136), full tiles, an N
# below the instantiated NT (40 and 72 run NT = 4 and 8 with 3 and 5 tiles, 136 runs NT = 12 with 9).
FWD_CASES = [(8, 1), (24, 25), (32, 40), (8, 100), (24, 136),
             (40, 16), (64, 24), (40, 64), (64, 72), (40, 192),
             (72, 8), (96, 32), (72, 40), (96, 128),
             (104, 16), (128, 25), (104, 64), (128, 128),
             (136, 8), (160, 24), (192, 64)]
FWD_ROWS = (1, 15, 16, 17, 63, 64, 65, 4099)
FWD_FULL_GRID = LINROWS_GRID_CAP * 4 * 16                                  # 131 072 rows: every wave one tile
FWD_BIG_ROWS = (FWD_FULL_GRID, FWD_FULL_GRID + 1, FWD_FULL_GRID + 64 * 3 + 17)
FWD_BIG_CASES = [(8, 1), (24, 136), (40, 16), (40, 192), (72, 8), (96, 128), (104, 16), (128, 128), (136, 8), (192, 64)]   # narrow, wide per KS


def fwd_modes(N, with_nobias=True):
    """[(mode, bias?)]: 0 with and without bias; 1, 2, 3 where N % 8 == 0"""
    m = [(0, True)] + ([(0, False)] if with_nobias else [])
    return m + ([(1, True), (2, True), (3, True)] if N % 8 == 0 else [])


# catan_linear_wgrad: (I, O).  OTW 1-4 <- O <= 64, 128, 192, 256; IT 2, 5, 10 <- I + 1 <= 32, 80, 160.  I = 31, 79, 159: the bias column is the
# tile's last; I = 32, 80: it opens a new tile.  Transposing-read staging: I and O multiples of 8; otherwise k_wgrad.
WGRAD_CASES = [(24, 16), (32, 8), (80, 16), (8, 72), (72, 72), (152, 72), (24, 136), (32, 136), (80, 136), (16, 256), (32, 200), (80, 256),
               (31, 13), (79, 8), (159, 16), (31, 72), (32, 100), (159, 72), (24, 129), (79, 136), (159, 136), (31, 200), (79, 256), (80, 201)]
WGRAD_SLICED_CASES = [(I, O) for I in (160, 264, 512, 1024) for O in (8, 128, 256)]
# 961: the first launch of two blocks; 1023 / 1024 / 1025: a full last stage, and one row into a 17th; 4609: a last block of ONE row
WGRAD_ROWS = (1, 63, 64, 65, 961, 1023, 1024, 1025, 4099, 4609)
WGRAD_BIG_ROWS = (131071, 131073)                                          # across 8 -> 16 stages per block
WGRAD_BIG_ROWS_CASES = [(64, 64), (31, 13), (264, 128)]
BIG_CASES = [(I, O) for I in (8, 120, 128, 256, 264, 1016) for O in (128, 256)]
BIG_ROWS = (1, 63, 64, 65, 512, 513, 4099)
BIG_ROWS_EXACT = (65535, 65536, 65537)


def grouped_problems():
    """catan_linear_wgrad_grouped's list -> [{I, O, rows, ld, col0, db}] (ld = 0: dw is [O][I]): 25 problems of one tile shape (24 per
    launch), sliced ones with and without a window, the non-transposing staging with a window, a one-row problem between large ones,
    problems without db"""
    p = [{"I": 40, "O": 24, "rows": 17 * k + 1, "ld": 0, "col0": 0, "db": k % 3 != 1} for k in range(25)]
    p += [{"I": 264, "O": 128, "rows": 1500, "ld": 0, "col0": 0, "db": True},
          {"I": 160, "O": 8, "rows": 700, "ld": 184, "col0": 16, "db": True},
          {"I": 512, "O": 136, "rows": 333, "ld": 515, "col0": 3, "db": False},
          {"I": 31, "O": 13, "rows": 200, "ld": 40, "col0": 5, "db": True},
          {"I": 79, "O": 72, "rows": 1025, "ld": 80, "col0": 1, "db": False},
          {"I": 64, "O": 64, "rows": 4099, "ld": 0, "col0": 0, "db": True},
          {"I": 64, "O": 64, "rows": 1, "ld": 70, "col0": 6, "db": True},
          {"I": 64, "O": 64, "rows": 4999, "ld": 0, "col0": 0, "db": False}]
    return p


# ---------------------------------------------------------------------------------------------------------------------- formulas
def linear_terms(x, W, b):
    """-> (a, S) in fp64: a = x W^T + b, S = sum_k |x_k W_nk| + |b_n|"""
    xd, Wd = x.double(), W.double()
    a, S = xd @ Wd.t(), xd.abs() @ Wd.abs().t()
    if b is not None:
        a, S = a + b.double(), S + b.double().abs()
    return a, S


def epilogue(a, aux, mode):
    if mode == 0:
        return a
    if mode == 1:
        return a.clamp_min(0.0)
    if mode == 2:
        return a + aux.to(a.dtype)
    return torch.where(aux > 0, a, torch.zeros((), dtype=a.dtype, device=a.device))


def linear_ref(x, W, b, aux, mode):
    return epilogue(linear_terms(x, W, b)[0], aux, mode)


def linear_yardstick(x, W, b, aux, mode, wd=torch.float32, plant=None):
    """-> y bf16.  Roundings: a (the fp32 product plus bias) is rounded to bf16; the epilogue sees that bf16 value; mode 2 rounds the fp32
    sum a second time.  wd = torch.float64 gives "the reference with the specified roundings" (the exact regime: equal to the bit).
    `plant` is NOT part of the yardstick: the planted errors of PLANTS that concern the forward."""
    xs, Ws = x.to(wd), W.to(wd)
    K = x.shape[1]
    if plant == "drop_k_chunk":
        xs = torch.cat([xs[:, :K - 8], torch.zeros_like(xs[:, K - 8:])], 1)
    a = xs @ Ws.t()
    if b is not None:
        a = a + b.to(wd) * (_cdiv(K, 32) if plant == "bias_per_kstep" else 1)
    if plant == "relu_before_round" and mode == 1:
        y = PR.rbf(a.clamp_min(0.0))
    elif plant == "no_second_round" and mode == 2:
        y = PR.rbf(a + aux.to(wd))
    elif plant == "gate_ge" and mode == 3:
        y = torch.where(aux >= 0, PR.rbf(a), torch.zeros((), dtype=wd, device=a.device))
    else:
        y = epilogue(PR.rbf(a), aux, mode)
        y = PR.rbf(y) if mode == 2 else y
    y = y.to(torch.bfloat16)
    R = y.shape[0]
    if plant == "perm_tile_rows":                                  # rows 4 g + r of every 16-row tile leave as 4 r + g
        idx = torch.arange(R, device=y.device)
        j = idx % 16
        src = idx - j + (j % 4) * 4 + j // 4
        y = y[torch.where(src < R, src, idx)]
    if plant == "second_pass_first_tile":                          # the grid-stride loop's second pass stores at the first pass's rows
        y = y.clone()
        n = R - FWD_FULL_GRID
        assert n > 0
        y[:n] = y[FWD_FULL_GRID:].clone()
        y[FWD_FULL_GRID:] = 0
    return y


def wgrad_ref(x, dy, with_abs=True, chunk=16384):
    """-> {dw [O, I], db [O], and with_abs: aw = sum_r |dy x|, ab = sum_r |dy|} in fp64, in row chunks (the reference must not round, and
    x in double must fit)"""
    O, I = dy.shape[1], x.shape[1]
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=x.device)
    out = {"dw": z(O, I), "db": z(O)}
    if with_abs:
        out["aw"], out["ab"] = z(O, I), z(O)
    for r0 in range(0, x.shape[0], chunk):
        xd, gd = x[r0:r0 + chunk].double(), dy[r0:r0 + chunk].double()
        out["dw"] += gd.t() @ xd
        out["db"] += gd.sum(0)
        if with_abs:
            out["aw"] += gd.abs().t() @ xd.abs()
            out["ab"] += gd.abs().sum(0)
    return out


def wgrad_yardstick(x, dy, chunk=16384):
    """-> (dw, db) fp32: fp32 products and sums of the same operands"""
    dw = torch.zeros((dy.shape[1], x.shape[1]), dtype=torch.float32, device=x.device)
    db = torch.zeros(dy.shape[1], dtype=torch.float32, device=x.device)
    for r0 in range(0, x.shape[0], chunk):
        dw += dy[r0:r0 + chunk].float().t() @ x[r0:r0 + chunk].float()
        db += dy[r0:r0 + chunk].float().sum(0)
    return dw, db


def wgrad_result(x, dy, dw0, db0, col0=0, plant=None):
    """what a launch leaves behind, in fp32: (dw0 with dy^T x added into its columns col0 .. col0 + I - 1, db0 + sum dy); db0 None: no
    bias gradient.  `plant`: the planted errors of PLANTS that concern the weight gradients."""
    R, I = x.shape
    xs, gs = x, dy
    if plant == "drop_last_row":
        xs, gs = x[:R - 1], dy[:R - 1]
    elif plant == "stale_last_stage":                               # the last, partial stage of 64 rows holds the previous stage's rows
        full = (R - 1) // WG_KT * WG_KT
        assert 0 < full < R and R % WG_KT
        xs, gs = torch.cat([x[:full], x[full - WG_KT:full]]), torch.cat([dy[:full], dy[full - WG_KT:full]])
    dw, db = wgrad_yardstick(xs, gs)
    if plant == "dw_transposed":
        assert dw.shape[0] == dw.shape[1]
        dw = dw.t()
    if plant == "db_every_slice":
        assert wgrad_sliced(I, dy.shape[1])
        db = db * _cdiv(I, 128)
    if plant == "window_shift":
        col0 += 1
    outw, outb = dw0.clone(), None if db0 is None else db0.clone()
    if plant == "overwrite":
        outw[:, col0:col0 + I] = dw
        outb = None if db0 is None else db
    else:
        outw[:, col0:col0 + I] += dw
        if db0 is not None:
            outb += db
    return outw, outb


PLANTS = ("drop_last_row", "stale_last_stage", "drop_k_chunk", "perm_tile_rows", "dw_transposed", "relu_before_round", "no_second_round",
          "gate_ge", "bias_per_kstep", "db_every_slice", "window_shift", "overwrite", "second_pass_first_tile")
FORWARD_PLANTS = ("drop_k_chunk", "perm_tile_rows", "relu_before_round", "no_second_round", "gate_ge", "bias_per_kstep", "second_pass_first_tile")


# -------------------------------------------------------------------------------------------------------------------------- rules
def same_but_zero_sign(y, want):
    """the exact regime's forward rule: equal bit for bit, except that a zero may carry either sign; a NaN fails"""
    return bool((y.float() == want.float()).all())


def forward_bound(a, S, aux, mode, K):
    """[rows, N] fp64: the real regime's per-element bound on |y - ref|"""
    e = (K + 1) * U * S
    bound = e + HALF_ULP_BF16 * (a.abs() + e)
    if mode == 2:
        bound = bound + HALF_ULP_BF16 * ((a + aux.double()).abs() + bound)
    return bound


def judge_forward(y, x, W, b, aux, mode, regime, terms=None):
    """one forward output against the rule of its regime -> (failures [str], kernel error, yardstick error, largest share of a bound)"""
    a, S = terms if terms is not None else linear_terms(x, W, b)
    ref = epilogue(a, aux, mode)
    yard = linear_yardstick(x, W, b, aux, mode)
    bad = []
    if not bool(torch.isfinite(y.float()).all()):
        bad.append("NOT FINITE")
    ek = float((y.double() - ref).abs().nan_to_num(float("inf")).max())
    ey = float((yard.double() - ref).abs().max())
    if mode == 3 and not bool((y.view(torch.int16)[aux <= 0] == 0).all()):
        bad.append("a gated element is not +0 (either regime)")
    if regime == "exact":
        if not torch.equal(yard, linear_yardstick(x, W, b, aux, mode, wd=torch.float64)):
            bad.append("the exact regime's yardstick is not exact")
        if not same_but_zero_sign(y, yard):
            bad.append(f"{int((y.float() != yard.float()).sum())} elements differ from the exact result")
        return bad, ek, ey, float("inf") if bad else 0.0
    bound = forward_bound(a, S, aux, mode, x.shape[1])
    err = (y.double() - ref).abs()
    sh = PR.share(err, bound)
    if not bool((err <= bound).all()):
        bad.append(f"{int((~(err <= bound)).sum())} elements over their bound, share {sh:.2f}")
    ok = PR.whole(y, ref, yard, PR.BF16_FLOOR)[0]
    oks = PR.per_group(y, ref, yard, PR.BF16_FLOOR)[0]
    if not ok:
        bad.append("within_yardstick over the case")
    if not bool(oks.all()):
        bad.append(f"within_yardstick on {int((~oks).sum())} rows, first {int((~oks).nonzero()[0])}")
    return bad, ek, ey, sh


def judge_wgrad(got, pre, ref, abs_terms, regime, depth):
    """one dw or db (fp32, as left in the accumulator) against pre-fill + reference -> (failures, kernel error, largest share)"""
    want = pre.double() + ref
    err = (got.double() - want).abs()
    bad = []
    if not bool(torch.isfinite(got).all()):
        bad.append("NOT FINITE")
    ek = float(err.nan_to_num(float("inf")).max())
    if regime == "exact":
        if not torch.equal(got.double(), want):
            bad.append(f"{int((got.double() != want).sum())} elements differ from the exact result")
        return bad, ek, float("inf") if bad else 0.0
    bound = PR.sum_bound(abs_terms, depth, pre, unit=U)
    sh = PR.share(err, bound)
    if not bool((err <= bound).all()):
        bad.append(f"{int((~(err <= bound)).sum())} elements over their bound, share {sh:.2f}")
    return bad, ek, sh


# ------------------------------------------------------------------------------------------------------------------------- cases
def forward_headroom(K):
    """the exact regime's forward in units of 2^-5: |x W| <= 16 per term, |b| <= 128, and the mode-2 sum adds |aux| <= 128 -> the largest
    magnitude any partial sum can reach; must stay below 2^24"""
    return 16 * K + 128 + 128


def wgrad_headroom(rows):
    """the exact regime's weight gradient in units of 1: |dy x| <= 9 per row, |pre-fill| <= 1000"""
    return 9 * rows + 1000


def _gen(device, *key):
    return PR.gen(*key, start=12345, device=device)


def _no_subnormals(*ts):
    for t in ts:
        if t is not None:
            f = t.float().abs()
            assert bool(((f == 0) | (f >= 2.0 ** -126)).all()) and bool(torch.isfinite(f).all())


def make_forward_case(K, N, rows, regime, device="cpu", seed=0):
    """-> {x [rows, K], W [N, K], b [N], aux [rows, N]} bf16 on `device` (+ K, N, rows, regime)"""
    assert regime in ("exact", "real")
    g = _gen(device, seed, K, N, rows, regime == "exact")
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).float()
    if regime == "exact":
        assert forward_headroom(K) < 2 ** 24
        pat = torch.where(torch.arange(K, device=device) % 3 == 0, -1.0, 1.0)           # the sign pattern some rows of x and of W share
        x, W = ri(-4, 4, rows, K), ri(-4, 4, N, K)
        xr, wr = torch.arange(rows, device=device) % 4 == 1, torch.arange(N, device=device) % 4 == 2
        x[xr] = x[xr].abs() * pat
        W[wr] = W[wr].abs() * pat
        x, W = x / 4, W / 8
        b = ri(-128, 128, N) / 32
        aux = ri(-64, 64, rows, N) / 16
        aux[ri(0, 3, rows, N) == 0] = 0.0                                               # exact zeros: `> 0` against `>= 0`
        assert float((x.abs() @ W.abs().t()).max()) * 32 + 256 < 2 ** 24
    else:
        rn = lambda *s: torch.randn(s, generator=g, device=device)
        x = rn(rows, K) * torch.linspace(0.5, 1.5, K, device=device)
        W = rn(N, K) * torch.linspace(1.4, 0.6, K, device=device) * K ** -0.5
        b = rn(N) * 0.5 + 0.1
        aux = rn(rows, N) * torch.linspace(0.4, 1.6, N, device=device) + 0.05
    c = {"x": x.to(torch.bfloat16), "W": W.to(torch.bfloat16), "b": b.to(torch.bfloat16), "aux": aux.to(torch.bfloat16)}
    if regime == "exact":
        for n, t in (("x", x), ("W", W), ("b", b), ("aux", aux)):
            assert torch.equal(c[n].float(), t), n
    _no_subnormals(*c.values())
    c.update(K=K, N=N, rows=rows, regime=regime)
    return c


def make_wgrad_case(I, O, rows, regime, device="cpu", seed=0, ones=False):
    """-> {x [rows, I], dy [rows, O]} bf16 on `device`; ones: the counting case, every element 1"""
    assert regime in ("exact", "real")
    g = _gen(device, seed, I, O, rows, regime == "exact", 77)
    if ones:
        x, dy = torch.ones((rows, I), device=device), torch.ones((rows, O), device=device)
    elif regime == "exact":
        x = torch.randint(-3, 4, (rows, I), generator=g, device=device).float()
        dy = torch.randint(-3, 4, (rows, O), generator=g, device=device).float()
    else:
        x = torch.randn((rows, I), generator=g, device=device) * torch.linspace(0.5, 1.5, I, device=device)
        dy = torch.randn((rows, O), generator=g, device=device) * torch.linspace(0.25, 2.0, O, device=device) + 0.05
    if regime == "exact" or ones:
        assert wgrad_headroom(rows) < 2 ** 24
    c = {"x": x.to(torch.bfloat16), "dy": dy.to(torch.bfloat16), "I": I, "O": O, "rows": rows, "regime": regime}
    _no_subnormals(c["x"], c["dy"])
    return c


def prefill(shape, regime, k, device="cpu"):
    """a non-constant fp32 pre-fill of an accumulator; integer-valued (|.| <= 1000) in the exact regime"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, device=device, dtype=torch.float32)
    if regime == "exact":
        return ((i * 37 + 11 * k) % 2001 - 1000).reshape(shape)
    return (torch.sin(i * 0.37 + k) * 1.5 + 0.25 * k).reshape(shape)
