"""GPU: the LayerNorm kernels of csrc/catan_nn.hip (k_ln_fwd / k_ln_bwd, k_lnw_fwd / k_lnw_bwd, k_lnr_fwd / k_lnr_bwd) row by row against
fp64 on every path of ln_dispatch (csrc/catan_abi_nn_launch.h), through the C ABI (catan_layer_norm_fwd / catan_layer_norm_bwd), with relu 0 and 1.

reference = tests/layer_norm_reference.py (its docstring has the formulas and the yardstick's roundings; the rule is tests/pin_rule.py's):
    y, dx   maxabs(kernel - fp64) <= 2 maxabs(yardstick - fp64) + floor maxabs(fp64), floor 2^-9 (bf16) / 2^-17 for y, 2^-15 for dx (fp32, the
            attention suite's), over the whole case AND for every row with that row's own yardstick error and scale
    dw, db  per column: |kernel - fp64| <= 2 |yardstick - fp64| + depth 2^-24 (sum_r |term| + |pre-fill|), depth = launch_depth
Nothing in a bound comes from a kernel.  Every case prints one `LN` line: per output the kernel's error, the yardstick's error, their ratio
and the largest share of a bound used (y, dx: by the case or by a single row; dw, db: by a column), and with relu the gate's delta and the
share of dy it zeroed: profiles/layer_norm_kernel_tests.txt is that output.

The test never reads which kernel ran: pointers and row counts leave ln_dispatch one choice (layer_norm_reference.PATHS, path_rows).
    aligned      every tensor 16-byte aligned: k_ln<16,16>, <25,32>, <32,32>, k_lnw<8,8> (64), <8,16> (128), <8,32> (256), <8,64> (512); bf16 at
                 D = 25 only below 4096 rows (4095 is its last row count)
    misaligned   every tensor one element into an aligned allocation: k_ln<16,16>, <25,32> (bf16 below AND above 4096 rows), <32,32>, <64,64>
    lnr          bf16, D = 25, aligned, rows >= 4096: k_lnr<25>
Row counts: 1, RPB - 1, RPB, RPB + 1, 255, 257, both sides of the backward cap (cap * RPB, + 1: the grid-stride loop's second pass) and,
forward only, both sides of the forward cap; k_lnr's own in path_rows.  Regimes: unit (with the planted all-zero and constant rows) at
every row count, offset below 5 000 rows.  relu = 1 zeroes dy where fp32 may decide the gate either way (layer_norm_reference.gated_dy;
at most 1 % of a case), so dx, dw and db are compared everywhere.

Buffers: inputs lie in NaN (a guard of rows behind them, and the element in front on the misaligned path), y / dx between sentinel
margins, dw / db pre-filled with a non-constant pattern.  Exact rows: an all-zero row, and at a power-of-two D a row constant at 1.5, gives
y = relu?(b) as stored, to the bit, wherever it is planted.  A case of all-zero rows alone must leave dw's pre-fill untouched to the bit
and add exactly the gated dy to db; b is exactly 0 in some columns, where pre = 0 decides the gate `<=` against `<`.

Further: rows do not depend on the grid (the first RPB + 1 rows of a launch equal a launch over those rows alone, bit for bit; k_lnr:
the first 4096, its smallest launch); relu = 1 with every pre-activation > 0 equals relu = 0 bit for bit; the aligned and the misaligned
path agree within the sum of their bounds.

Last, the autograd functions nn_kernels builds on these entry points (_SmallLayerNorm, _PreNorm): what autograd returns for x, w and b
against torch's own layer_norm differentiated in fp64, under the same rule (_judge_function)."""
import pytest
import torch

import guarded as G
import layer_norm_reference as LN
import pin_rule as PR
from guarded import ptr as P, stream as _stream
from pin_rule import same_bits

pytestmark = pytest.mark.gpu

EPS = LN.EPS
GUARD = 64                       # rows behind every row-major buffer
SENTINEL = 0x5A5B
OFFSET_BELOW = 5000


def _margins(mis, D):
    """-> (lead, tail): the view begins one element into the allocation on the misaligned path (at its start otherwise) and is followed
    by GUARD rows (and 8 elements more on the misaligned path)"""
    return (1, GUARD * D + 8) if mis else (0, GUARD * D)


def _placed(mis, whole, view):
    assert view.data_ptr() % 16 == (whole.element_size() if mis else 0)
    return whole, view


def _input(mis, t):
    lead, tail = _margins(mis, t.shape[1])
    return _placed(mis, *G.guarded_input(t, tail, lead))


def _output(mis, rows, D, dtype):
    lead, tail = _margins(mis, D)
    return _placed(mis, *G.sentinel_output(rows * D, dtype, tail, lead, SENTINEL))


def _launch(lib, mis, x, w, b, dy, relu):
    """forward, and with dy the backward, on device tensors -> {y, dx [rows, D] of the storage dtype; dw, db fp32 as left in the
    pre-filled accumulators; dw0, db0 the pre-fill}"""
    from settlers_of_catan_rl_amd import _lib
    rows, D = x.shape
    is_bf16 = int(x.dtype == torch.bfloat16)
    hold_x, x_d = _input(mis, x)
    whole_y, y_d = _output(mis, rows, D, x.dtype)
    _lib.check(lib.catan_layer_norm_fwd(P(x_d), P(w), P(b), P(y_d), rows, D, EPS, relu, is_bf16, _stream()))
    out = {}
    if dy is not None:
        hold_g, g_d = _input(mis, dy)
        whole_dx, dx_d = _output(mis, rows, D, x.dtype)
        dw, db = G.pattern(D, 1), G.pattern(D, 2)
        out["dw0"], out["db0"] = dw.clone(), db.clone()
        _lib.check(lib.catan_layer_norm_bwd(P(x_d), P(w), P(b), P(g_d), P(dx_d), P(dw), P(db), rows, D, EPS, relu, is_bf16, _stream()))
    torch.cuda.synchronize()
    assert G.intact(whole_y, y_d), (mis, rows, D, "a write outside y")
    out["y"] = y_d.view(rows, D).clone()
    if dy is not None:
        assert G.intact(whole_dx, dx_d), (mis, rows, D, "a write outside dx")
        out["dx"], out["dw"], out["db"] = dx_d.view(rows, D).clone(), dw, db
    return out


def _judge(name, bf16, got, ref, yard, depth, note=""):
    """the rule over the case, per row and per column; one LN line -> (failures, {output: whole-case bound})"""
    bad, bounds, line = [], {}, []
    fmt = lambda n, ek, ey, share: f"{n} {ek:.2e} {ey:.2e} {PR.ratio(ek, ey, PR.INF):.2f} {share:.2f}"
    for n in ("y", "dx"):
        if n not in got:
            continue
        ok, ek, ey, bound = LN.accept(bf16, n, got[n], ref[n], yard[n])
        oks, eks, bnds = LN.per_row(bf16, n, got[n], ref[n], yard[n])
        finite = bool(torch.isfinite(got[n].float()).all())
        bounds[n] = bound
        line.append(fmt(n, ek, ey, max(PR.whole_share(ek, bound), PR.share(eks, bnds))))
        if not (ok and finite):
            bad.append((name, n, "whole", ek, ey, bound, "finite" if finite else "NOT FINITE"))
        if not bool(oks.all()):
            r = int((~oks).nonzero()[0])
            bad.append((name, n, f"{int((~oks).sum())} rows, first {r}", float(eks[r]), float(bnds[r])))
    for n, a in (("dw", "aw"), ("db", "ab")):
        if n not in got:
            continue
        oks, ek, bnd = PR.accept_sum(got[n], got[n + "0"], ref[n], yard[n], ref[a], depth)
        ey = (yard[n].double() - ref[n]).abs()
        finite = bool(torch.isfinite(got[n]).all())
        bounds[n] = bnd
        line.append(fmt(n, float(ek.max()), float(ey.max()), PR.share(ek, bnd)))
        if not (finite and bool(oks.all())):
            j = int((~oks).nonzero()[0]) if finite else -1
            bad.append((name, n, f"{int((~oks).sum())} columns, first {j}", float(ek[j]), float(bnd[j]), "finite" if finite else "NOT FINITE"))
    print(f"LN {name}: " + " | ".join(line) + note)
    return bad, bounds


def _exact_row_checks(name, c, relu, got):
    """the planted rows: y = relu?(b) as stored, to the bit"""
    want = (c["b"].clamp_min(0.0) if relu else c["b"]).to(got["y"].dtype)
    for r in c["exact_rows"]:
        assert same_bits(got["y"][r], want), (name, r, "an exact row's y is not relu?(b) to the bit")


def _run_case(lib, align, c, relu, fwd_only):
    """one case on one path with one relu -> (name, got, the dy launched, failures, bounds)"""
    D, rows, bf16 = c["D"], c["rows"], c["x"].dtype == torch.bfloat16
    mis = align == "misaligned"
    name = f"{align} D={D} {'bf16' if bf16 else 'fp32'} rows={rows} {c['regime']} relu={relu}"
    dyr, note = c["dy"], ""
    if relu and not fwd_only:
        dyr, share, delta = LN.gated_dy(c)
        note = f" | gate {delta:.1e} {share:.5f}"
        assert share <= 0.01, (name, share)
    dyr = None if fwd_only else dyr
    got = _launch(lib, mis, c["x"], c["w"], c["b"], dyr, relu)
    ref = LN.ln_ref(c["x"], c["w"], c["b"], dyr, EPS, relu)
    yard = LN.ln_yardstick(c["x"], c["w"], c["b"], dyr, EPS, relu, bf16)
    bad, bounds = _judge(name, bf16, got, ref, yard, LN.launch_depth(align, D, rows), note)
    _exact_row_checks(name, c, relu, got)
    return name, got, dyr, bad, bounds


def _device_case(D, rows, regime, edge, dtype):
    c = LN.make_case(D, rows, regime, edge, getattr(torch, dtype))
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


IDS = [f"{a}-{D}-{dt}" for a, D, dt in LN.PATHS]


@pytest.mark.parametrize("align,D,dtype", LN.PATHS, ids=IDS)
def test_layer_norm_kernel_vs_fp64(hip_lib, align, D, dtype):
    """One path of ln_dispatch at one width and storage type, forward and backward, relu 0 and 1, at every row count of path_rows.  See
    the module docstring for what is asserted.

    Measured on the MI355X: profiles/layer_norm_kernel_tests.txt."""
    edge = LN.path_kernel(align, D)[1]
    mis = align == "misaligned"
    bad = []
    for rows, fwd_only in LN.path_rows(align, D, dtype):
        for regime in ("unit", "offset") if rows < OFFSET_BELOW else ("unit",):
            c = _device_case(D, rows, regime, edge, dtype)
            for relu in (0, 1):
                name, got, dyr, b, _ = _run_case(hip_lib, align, c, relu, fwd_only)
                bad += b
                if regime != "unit" or not relu:
                    continue
                # rows do not depend on the grid
                n = min(rows, LN.LNR_MIN_ROWS if align == "lnr" else edge + 1)
                if n < rows:
                    sub = _launch(hip_lib, mis, c["x"][:n].contiguous(), c["w"], c["b"], None if dyr is None else dyr[:n].contiguous(), relu)
                    for o in ("y", "dx"):
                        if o in sub:
                            assert same_bits(sub[o], got[o][:n]), (name, o, f"the first {n} rows depend on the grid")
        del c
    # relu = 1 where no pre-activation is <= 0
    for rows in sorted({r for r, f in LN.path_rows(align, D, dtype) if not f})[2:5]:
        c = _device_case(D, rows, "unit", edge, dtype)
        bpos = LN.positive_bias(c)
        assert float(LN.ln_ref(c["x"], c["w"], bpos, None, EPS, 0)["pre"].min()) > 0.5
        a0 = _launch(hip_lib, mis, c["x"], c["w"], bpos, c["dy"], 0)
        a1 = _launch(hip_lib, mis, c["x"], c["w"], bpos, c["dy"], 1)
        for o in ("y", "dx"):
            assert same_bits(a0[o], a1[o]), (align, D, dtype, rows, o, "relu = 1 with every pre-activation > 0 differs from relu = 0")
    # every row all-zero: dw keeps its pre-fill to the bit, db takes exactly the gated dy (its yardstick is exact, so the column bound is
    # the summation bound alone), and with relu the columns where b == 0 decide `<=` against `<`
    for rows in (edge + 1, 257) if align != "lnr" else (4097,):
        c = _device_case(D, rows, "unit", edge, dtype)
        c["x"] = torch.zeros_like(c["x"])
        c["zero_rows"], c["const_rows"], c["exact_rows"], c["regime"] = list(range(rows)), [], list(range(rows)), "zero"
        for relu in (0, 1):
            name, got, dyr, b, _ = _run_case(hip_lib, align, c, relu, False)
            bad += b
            assert same_bits(got["dw"], got["dw0"]), (name, "all-zero rows changed dw")
            assert torch.equal(dyr, c["dy"]), (name, "an exact row's dy was zeroed")
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("D", [16, 25, 32, 64])
def test_aligned_and_misaligned_agree(hip_lib, D, dtype):
    """The same inputs through the aligned and through the misaligned path (at D = 64 two different kernels, k_lnw<8,8> and k_ln<64,64>; at
    D = 25 bf16 and 4097 rows k_lnr<25> and k_ln<25,32>): the results differ by no more than the sum of their two bounds against the
    reference.  A consistency check between the paths, not a substitute for the reference."""
    edge = LN.path_kernel("aligned", D)[1]
    for rows in (edge + 1, 257, 4097):
        c = _device_case(D, rows, "unit", edge, dtype)
        for relu in (0, 1):
            path_a = "lnr" if (D == 25 and dtype == "bfloat16" and rows >= LN.LNR_MIN_ROWS) else "aligned"
            _, ga, _, bad_a, ba = _run_case(hip_lib, path_a, c, relu, False)
            _, gm, _, bad_m, bm = _run_case(hip_lib, "misaligned", c, relu, False)
            assert not bad_a and not bad_m, (bad_a, bad_m)
            for o in ("y", "dx"):
                d = float((ga[o].double() - gm[o].double()).abs().max())
                print(f"LN-PATHS D={D} {dtype} rows={rows} relu={relu} {o}: {path_a} - misaligned {d:.2e} bounds {ba[o]:.2e} + {bm[o]:.2e}")
                assert d <= ba[o] + bm[o], (D, dtype, rows, relu, o, d, ba[o], bm[o])
            for o in ("dw", "db"):
                d = (ga[o].double() - gm[o].double()).abs()
                assert bool((d <= ba[o] + bm[o]).all()), (D, dtype, rows, relu, o)


# ------------------------------------------------------------------------------------- the autograd functions over these kernels
def _torch_fp64(c, dy, relu, dres=None):
    """torch's own layer_norm (+ relu) differentiated in fp64 on the case's inputs -> {dx, dw, db}; dres: the gradient of a second
    use of x (the residual stream beside a pre-norm LayerNorm)"""
    x, w, b = (c[k].double().requires_grad_() for k in ("x", "w", "b"))
    y = torch.nn.functional.layer_norm(x, (c["D"],), w, b, EPS)
    loss = ((torch.relu(y) if relu else y) * dy.double()).sum()
    if dres is not None:
        loss = loss + (x * dres.double()).sum()
    return dict(zip(("dx", "dw", "db"), torch.autograd.grad(loss, (x, w, b))))


def _judge_function(name, c, relu, dy, got, dres=None):
    """this file's rule (_judge) on what an autograd function returned: the reference's dx, dw, db are torch's in fp64; the yardstick,
    the summation terms of the column bound and the launch depth are layer_norm_reference's for the aligned path of this width.  With
    dres the yardstick adds it to the LayerNorm term as the kernel does - that term rounded to the storage type first, then the sum."""
    bf16 = c["x"].dtype == torch.bfloat16
    ref = LN.ln_ref(c["x"], c["w"], c["b"], dy, EPS, relu)
    ref.update(_torch_fp64(c, dy, relu, dres))
    yard = LN.ln_yardstick(c["x"], c["w"], c["b"], dy, EPS, relu, bf16)
    if dres is not None:
        yard["dx"] = yard["dx"] + dres.float()
        if bf16:
            yard["dx"] = yard["dx"].to(torch.bfloat16).float()
    got = dict(got, dw0=torch.zeros_like(got["dw"]), db0=torch.zeros_like(got["db"]))            # (fresh accumulators)
    bad, _ = _judge(name, bf16, got, ref, yard, LN.launch_depth("aligned", c["D"], c["rows"]))
    assert not bad, bad
    _exact_row_checks(name, c, relu, got)


def _layer(c):
    ln = torch.nn.LayerNorm(c["D"], eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(c["w"])
        ln.bias.copy_(c["b"])
    return ln


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("D", [25, 64])
def test_small_layer_norm_function_vs_torch_fp64(hip_lib, D, rows, dtype):
    """nn_kernels._SmallLayerNorm (small_layer_norm), with and without ReLU: y, and dx, dw, db from autograd, under the rule the kernel
    behind it is held to above.  67 rows leave a row block partly filled; one row is the smallest launch."""
    from settlers_of_catan_rl_amd import nn_kernels
    c = _device_case(D, rows, "unit", LN.path_kernel("aligned", D)[1], dtype)
    ln = _layer(c)
    for relu in (0, 1):
        dy = LN.gated_dy(c)[0] if relu else c["dy"]
        x = c["x"].clone().requires_grad_()
        assert nn_kernels.ln_supported(x, ln)
        y = nn_kernels.small_layer_norm(x, ln, relu=bool(relu))
        dx, dw, db = torch.autograd.grad(y, (x, ln.weight, ln.bias), dy)
        assert dx.dtype == x.dtype and dw.dtype == db.dtype == torch.float32
        _judge_function(f"function small D={D} {dtype} rows={rows} relu={relu}", c, relu, dy, {"y": y.detach(), "dx": dx, "dw": dw, "db": db})


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 67])
def test_pre_norm_function_vs_torch_fp64(hip_lib, rows, dtype):
    """nn_kernels._PreNorm (pre_norm) at D = 64 in its three uses: both outputs consumed (x's whole gradient from
    catan_layer_norm_bwd_res), only the normalised output, only the residual stream (x's gradient is dres, to the bit, and the LayerNorm's
    parameters get nothing).  autograd hands a backward zeros for an output nobody used, so the `None` branches of the backward are
    also called directly - the one for `dy is None` with no context at all: it returns before it reads or allocates anything."""
    from types import SimpleNamespace
    from settlers_of_catan_rl_amd import nn_kernels
    D = 64
    c = _device_case(D, rows, "unit", LN.path_kernel("aligned", D)[1], dtype)
    ln = _layer(c)
    dres = (c["dy"].float().flip(0) * 0.75 - 0.05).to(c["x"].dtype)
    name = f"function pre_norm D={D} {dtype} rows={rows}"

    def run(use_y, use_res):
        x = c["x"].clone().requires_grad_()
        assert nn_kernels.pre_norm_supported(x, ln)
        y, res = nn_kernels.pre_norm(x, ln)
        assert same_bits(res.detach(), c["x"])
        outs, grads = zip(*[p for p, used in (((y, c["dy"]), use_y), ((res, dres), use_res)) if used])
        dx, dw, db = torch.autograd.grad(outs, (x, ln.weight, ln.bias), grads, allow_unused=True)
        return y.detach(), dx, dw, db

    y, dx, dw, db = run(True, True)
    _judge_function(name + " both", c, 0, c["dy"], {"y": y, "dx": dx, "dw": dw, "db": db}, dres)
    y, dx, dw, db = run(True, False)
    _judge_function(name + " norm only", c, 0, c["dy"], {"y": y, "dx": dx, "dw": dw, "db": db})
    _, dx, dw, db = run(False, True)
    assert same_bits(dx, dres), (name, "only the residual stream used: x's gradient is not dres")
    assert all(g is None or not bool(g.any()) for g in (dw, db))
    # the backward's own branches for a missing gradient
    out = nn_kernels._PreNorm.backward(None, None, dres)
    assert out[0] is dres and out[1:] == (None, None, None)
    x = c["x"].clone()
    ctx = SimpleNamespace(saved_tensors=(x, c["w"].contiguous(), c["b"].contiguous()), eps=EPS)
    dx, dw, db, _ = nn_kernels._PreNorm.backward(ctx, c["dy"], None)
    _judge_function(name + " dres None", c, 0, c["dy"], {"y": y, "dx": dx, "dw": dw, "db": db})
