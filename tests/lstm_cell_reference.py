"""Plain-torch restatement of the LSTM-cell kernels of csrc/catan_nn.hip (k_lstm_cell_fwd<T> / k_lstm_cell_bwd<T>; catan_lstm_cell_fwd /
catan_lstm_cell_bwd), with the seeded case builders and the launch table that tests/test_lstm_cell_reference_cpu.py and
tests/test_gpu_lstm_cell_fp64.py share.  No call into the library or into nn_kernels: torch ops only, on the CPU or the GPU, written from
include/catan_hip_nn.h and torch.nn.LSTM's cell.

    a = gx + gh, [rows][4 L] in the gate order i, f, g, o       cin = c_prev * mask (mask [rows] or None = 1)
    c = sigmoid(f) cin + sigmoid(i) tanh(g)                     h = sigmoid(o) tanh(c)
    with I, F, G, O the activations and tc = tanh(c):           d = dc + dh O (1 - tc^2)
    dgates = (d G I (1 - I), d cin F (1 - F), d I (1 - G^2), dh tc O (1 - O))         dc_prev = d F mask          (closed form)
    One dgates tensor is the gradient of gx and of gh alike.

  lstm_ref        the REFERENCE: fp64 throughout from the inputs as stored (bf16 gates upcast exactly).
  lstm_yardstick  the same formulas in fp32 (gx + gh is an fp32 sum of the upcast values, as in the kernels), the activations as the
                  kernels write them: sigmoid(x) = 1 / (1 + exp(-x)) with 0 below the normal range, tanh(x) = 1 - 2 / (1 + exp(2 x)).
                  With torch.sigmoid / torch.tanh the `saturated` rows whose every h is O * tanh(1e-14) or sigmoid(-90) disagreed by
                  100 % of a value of 1e-20 or less: that tanh returns 0 for |x| < 3e-8, and exp(90) is inf in fp32.  It rounds to bf16
                  only where the kernel stores bf16: dgates of the bf16 instantiation.  It shows what the formats cost; it is not an oracle.
                  A change to sigmoid_f / tanh_f in csrc/catan_nn.hip has to be mirrored in `_core` by hand.
                  `plant` is NOT part of it: the planted errors of the CPU test's rejection cases (PLANTS).

Acceptance: the rule of tests/pin_rule.py per row and over the whole case, scale = the largest reference magnitude (of the row / of the
case).  fp32 outputs with the attention suite's floors, 2^-17 for h, c and 2^-15 for dgates, dc_prev; bf16 dgates with
pin_rule.BF16_FLOOR.  No floor was moved: on the MI355X the kernels use
at most half of a bound (saturated; 0.16 of one in the unit regime) and their rows would need a floor of 3.8e-6 at most
(profiles/lstm_cell_kernel_tests.txt).  The exact cases (`zero`; the masked rows of `masked` against
the same case with c_prev = 0 there) are compared as values and bit for bit."""
import torch

import pin_rule as PR

FLOOR = {"h": 2.0 ** -17, "c": 2.0 ** -17, "dgates": 2.0 ** -15, "dc_prev": 2.0 ** -15}
PLANTS = ("gate_order", "mask_on_c", "dcp_no_mask", "one_minus_tc")
REGIMES = ("unit", "saturated", "zero", "masked")
FLT_MIN = 2.0 ** -126
BIG = 1e30                                               # c_prev of a masked row in `masked`

# ------------------------------------------------------------------------------------------------------------------- launch table
# lstm_cell_launch (csrc/catan_abi_nn_launch.h): an item = four consecutive hidden units of one row, a lane per item, 256 lanes per block;
# ceil(rows (L / 4) / 256) blocks, at most 16 384, above which a lane's grid-stride loop runs again.
BLOCK = 256
CAP = 16384
HIDDEN = (4, 8, 12, 64, 256)                             # 1, 2, 3, 16, 64 items per row; at 12 a row straddles two blocks
ROWS = (1, 63, 64, 65, 255, 256, 257)
CAP_L = 256
CAP_ROWS = (CAP * BLOCK // (CAP_L // 4), CAP * BLOCK // (CAP_L // 4) + 1)      # 65 536: exactly the cap; 65 537: the first second pass
CAP_SLICE = 4096                                         # the first and the last rows of a cap case that are compared with fp64
DTYPES = ("float32", "bfloat16")


def launch(rows, L):
    """-> (blocks, passes of the busiest lane)"""
    items = rows * (L // 4)
    blocks = min(CAP, -(-items // BLOCK))
    return blocks, -(-items // (blocks * BLOCK))


def small_cases():
    """-> [(L, rows, regime, with mask pointer)]: every regime at every L and row count; with and without a mask pointer except `masked`,
    which needs one"""
    return [(L, n, reg, mp) for L in HIDDEN for n in ROWS for reg in REGIMES for mp in ((True,) if reg == "masked" else (False, True))]


def cap_cases():
    """-> [(dtype, rows, with mask pointer)]: both sides of the cap in both storage types, the mask pointer going round"""
    return [(dt, n, bool((i + j) % 2)) for i, dt in enumerate(DTYPES) for j, n in enumerate(CAP_ROWS)]


# ---------------------------------------------------------------------------------------------------------------------- formulas
def _core(gx, gh, c_prev, mask, dh, dc, wd, plant=None):
    """everything in dtype wd -> {h, c, and with dh: dgates, dc_prev}"""
    L = c_prev.shape[1]
    if wd == torch.float32:
        a = gx.float() + gh.float()
    else:
        a = gx.to(wd) + gh.to(wd)
    i, f, g, o = a[:, :L], a[:, L:2 * L], a[:, 2 * L:3 * L], a[:, 3 * L:]
    if plant == "gate_order":
        g, o = o, g
    m = torch.ones((c_prev.shape[0], 1), dtype=wd, device=c_prev.device) if mask is None else mask.to(wd)[:, None]
    if wd == torch.float32:
        # the kernels' own activations (sigmoid_f, tanh_f of csrc/catan_nn.hip), so that the yardstick shows what THEY cost in fp32:
        # tanh as 1 - 2 / (1 + exp(2 x)) loses the digits of a small x, exp overflows to inf, and what falls below the normal range is 0
        flush = lambda t: torch.where(t.abs() < FLT_MIN, torch.zeros_like(t), t)
        sig = lambda x: flush(1.0 / (1.0 + torch.exp(-x)))
        tanh = lambda x: 1.0 - 2.0 / (1.0 + torch.exp(2.0 * x))
    else:
        sig, tanh = torch.sigmoid, torch.tanh
    I, F, G, O = sig(i), sig(f), tanh(g), sig(o)
    if plant == "mask_on_c":
        cin = c_prev.to(wd)
        c = (F * cin + I * G) * m
    else:
        cin = c_prev.to(wd) * m
        c = F * cin + I * G
    tc = tanh(c)
    out = {"c": c, "h": O * tc}
    if dh is not None:
        dh, dc = dh.to(wd), dc.to(wd)
        d = dc + dh * O * ((1 - tc) if plant == "one_minus_tc" else (1 - tc * tc))
        dg = [d * G * I * (1 - I), d * cin * F * (1 - F), d * I * (1 - G * G), dh * tc * O * (1 - O)]
        if plant == "gate_order":
            dg[2], dg[3] = dg[3], dg[2]
        out["dgates"] = torch.cat(dg, 1)
        out["dc_prev"] = d * F if plant == "dcp_no_mask" else d * F * m
    return out


def lstm_ref(gx, gh, c_prev, mask, dh=None, dc=None):
    return _core(gx, gh, c_prev, mask, dh, dc, torch.float64)


def lstm_yardstick(gx, gh, c_prev, mask, dh=None, dc=None, plant=None):
    o = _core(gx, gh, c_prev, mask, dh, dc, torch.float32, plant)
    if gx.dtype == torch.bfloat16 and "dgates" in o:
        o["dgates"] = PR.rbf(o["dgates"])
    return o


# -------------------------------------------------------------------------------------------------------------------------- rule
def floor_of(bf16, name):
    return PR.BF16_FLOOR if (bf16 and name == "dgates") else FLOOR[name]


def judge(bf16, got, ref, yard):
    """the rule over the case and per row for every output in `got` -> (failures, {output: (kernel error, yardstick error, largest share
    of a bound, the smallest floor under which every row would pass)}).  Nothing in a bound comes from `got`."""
    bad, stats = [], {}
    for n in ("h", "c", "dgates", "dc_prev"):
        if n not in got:
            continue
        ok, ek, ey, bound = PR.whole(got[n], ref[n], yard[n], floor_of(bf16, n))
        oks, eks, bnds = PR.per_group(got[n], ref[n], yard[n], floor_of(bf16, n))
        finite = bool(torch.isfinite(got[n].float()).all())
        need = PR.need_floor(eks, PR.group_error(yard[n], ref[n]), PR.group_scale(ref[n]))
        stats[n] = (ek, ey, max(PR.whole_share(ek, bound), PR.share(eks, bnds)), need)
        if not (ok and finite):
            bad.append((n, "whole", ek, ey, bound, "finite" if finite else "NOT FINITE"))
        if not bool(oks.all()):
            r = int((~oks).nonzero()[0])
            bad.append((n, f"{int((~oks).sum())} rows, first {r}", float(eks[r]), float(bnds[r])))
    return bad, stats


def stats_line(stats):
    """per output: kernel error, yardstick error, their ratio, the largest share of a bound used, the floor the rows need"""
    return " | ".join(PR.fmt_stat(n, s) for n, s in stats.items())


# ------------------------------------------------------------------------------------------------------------------------- cases
def make_case(regime, n, L, dtype, with_mask, seed=0, device="cpu"):
    """-> {gx, gh [n, 4 L] of `dtype`; c_prev, dh, dc fp32 [n, L]; mask fp32 [n] of 0 / 1 or None; masked_rows}, drawn in fp32 on `device`
    (the cap cases draw on the GPU; every other case on the CPU, the same numbers for the CPU and the GPU test) and then stored.
    unit:      gates randn * 1.5 each (the pre-activation is their sum), c_prev randn, mask 0 on three rows in ten.
    saturated: every pre-activation is +-(30 .. 100), the sign drawn per element: gx and gh carry half of it each, with the same sign.
    zero:      gates and c_prev 0 (dh, dc drawn): c and h are exactly 0.
    masked:    unit, and the rows with mask 0 carry c_prev = 1e30, which c, h, dgates and dc_prev must not see."""
    assert regime in REGIMES and (with_mask or regime != "masked")
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 7919 * L + 31 * n + 101 * REGIMES.index(regime) + int(with_mask))
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    ru = lambda *s: torch.rand(*s, generator=g, device=device)
    if regime == "saturated":
        mag = 15.0 + 35.0 * ru(n, 4 * L)
        sign = torch.where(ru(n, 4 * L) < 0.5, -1.0, 1.0)
        gx, gh = sign * mag, sign * (15.0 + 35.0 * ru(n, 4 * L))
    elif regime == "zero":
        gx, gh = torch.zeros(n, 4 * L, device=device), torch.zeros(n, 4 * L, device=device)
    else:
        gx, gh = rn(n, 4 * L) * 1.5, rn(n, 4 * L) * 1.5
    c_prev = torch.zeros(n, L, device=device) if regime == "zero" else rn(n, L)
    mask = (ru(n) > 0.3).float() if with_mask else None
    masked_rows = None
    if regime == "masked":
        mask[::3] = 0.0                                               # (row 0 and the last row of 64, 256, 257 among them)
        masked_rows = mask == 0
        c_prev[masked_rows] = BIG
    return {"gx": gx.to(dtype), "gh": gh.to(dtype), "c_prev": c_prev, "mask": mask, "dh": rn(n, L), "dc": rn(n, L), "masked_rows": masked_rows,
            "regime": regime, "n": n, "L": L}
