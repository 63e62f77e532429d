"""CPU: tests/layer_norm_reference.py itself - the fp64 reference against autograd and against te_reference, the acceptance rule against
planted errors, and the input caps of the GPU test's generators.  tests/test_gpu_layer_norm_fp64.py holds the kernels to this reference.

Rejection: every planted error (layer_norm_reference.PLANTS) is computed as the yardstick is - fp32, rounded as the storage type rounds -
so it is what a kernel with that one error would return, and the rule must refuse it in the regime named in REJECTED_IN."""
import pytest
import torch

import layer_norm_reference as LN
import pin_rule as PR
import te_reference as R

EPS = LN.EPS


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("D", LN.WIDTHS)
def test_reference_matches_autograd_in_double(D, relu):
    c = LN.make_case(D, 37, "unit", 8, torch.float32, seed=3)
    x = c["x"].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    b = c["b"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (D,), w, b, EPS)
    y = torch.relu(y) if relu else y
    dx, dw, db = torch.autograd.grad(y, (x, w, b), c["dy"].double())
    assert float((LN.ln_fwd_ref(c["x"], c["w"], c["b"], EPS, relu) - y.detach()).abs().max()) <= 1e-12
    rx, rw, rb = LN.ln_bwd_ref(c["x"], c["w"], c["b"], c["dy"], EPS, relu)
    for got, want in ((rx, dx), (rw, dw), (rb, db)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_reference_matches_te_reference_without_residual(D):
    c = LN.make_case(D, 21, "unit", 8, torch.bfloat16, seed=4)
    rx, rw, rb = LN.ln_bwd_ref(c["x"], c["w"], c["b"], c["dy"], EPS, 0)
    t = R.layer_norm_bwd_res_ref(c["x"], c["w"], c["dy"], torch.zeros_like(c["dy"]), EPS)
    for got, want in ((rx, t["dx"]), (rw, t["dw"]), (rb, t["db"])):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def _rejected(c, relu, bf16, plant, align="aligned"):
    """-> the names of the outputs on which the rule (whole case, per row, per column) refuses the planted error; asserts that the
    unplanted yardstick itself passes everywhere"""
    D, rows = c["D"], c["rows"]
    dy = LN.gated_dy(c)[0] if relu else c["dy"]
    ref = LN.ln_ref(c["x"], c["w"], c["b"], dy, EPS, relu)
    yard = LN.ln_yardstick(c["x"], c["w"], c["b"], dy, EPS, relu, bf16)
    bad = LN.ln_yardstick(c["x"], c["w"], c["b"], dy, EPS, relu, bf16, plant=plant)
    depth = LN.launch_depth(align, D, rows)
    out = set()
    for who, o in (("yardstick", yard), ("planted", bad)):
        for n in ("y", "dx"):
            ok = LN.accept(bf16, n, o[n], ref[n], yard[n])[0] and bool(LN.per_row(bf16, n, o[n], ref[n], yard[n])[0].all())
            assert ok or who == "planted", (n, "the yardstick fails its own rule")
            if not ok:
                out.add(n)
        for n, a in (("dw", "aw"), ("db", "ab")):
            ok = bool(((o[n].double() - ref[n]).abs() <= PR.sum_bound(ref[a], depth, torch.zeros(D), yard[n], ref[n])).all())
            assert ok or who == "planted"
            if not ok:
                out.add(n)
    return out


# plant -> (regime, relu, the widths x storage types it must be refused at, an output that must refuse it)
_ALL = [(D, bf) for D in LN.WIDTHS for bf in (False, True)]
REJECTED_IN = {
    # mean^2 of up to 65 000 carries an fp32 rounding of 4e-3 under a variance of 0.03 .. 0.1.  Not at D = 16: a row of bf16 values m + s k
    # has a mean of (16 m / s + sum k) s / 16, an integer below 2^12 times a power of two, whose square fp32 holds exactly - one pass
    # returns the two-pass result there to the bit, and there is nothing to refuse
    # dw refuses it in both storage types (its terms are fp32 whatever the storage); y and dx do in fp32, and in bf16 where the rows are many
    "one_pass": ("offset", 0, [(D, bf) for D, bf in _ALL if D != 16], "dw"),
    # rstd off by 1 / (2 D): above the fp32 floor at every width, above bf16's three half-ulps up to D = 32
    "d_minus_1": ("unit", 0, [(D, False) for D in LN.WIDTHS] + [(D, True) for D in (16, 25, 32)], "y"),
    # the planted zero rows: variance 0, rstd 1 / eps instead of 1 / sqrt(eps) multiplies their dx
    "eps_outside": ("unit", 0, _ALL, "dx"),
    "no_m2": ("unit", 0, _ALL, "dx"),
    # the planted zero rows: pre = b exactly, 0 in the columns j % 8 == 2, where `<` lets dy through
    "gate_lt": ("unit", 1, _ALL, "db"),
    "dw_ungated": ("unit", 1, _ALL, "dw"),
    "swap_pairs": ("unit", 0, _ALL, "y"),
    "drop_last": ("unit", 0, [(25, False), (25, True)], "y"),
    "dw_scale": ("unit", 0, _ALL, "dw"),
}


@pytest.mark.parametrize("plant", LN.PLANTS)
def test_rule_rejects_planted_error(plant):
    regime, relu, where, must = REJECTED_IN[plant]
    for D, bf16 in where:
        edge = LN.path_kernel("aligned", D)[1]
        for rows in (edge + 1, 257):
            c = LN.make_case(D, rows, regime, edge, torch.bfloat16 if bf16 else torch.float32)
            refused = _rejected(c, relu, bf16, plant)
            print(f"LN-PLANT {plant} D={D} {'bf16' if bf16 else 'fp32'} rows={rows} {regime} relu={relu}: refused on {sorted(refused)}")
            assert must in refused, (plant, D, bf16, rows, refused)


def _cpu_cases():
    """the GPU test's cases up to 4352 rows (the larger ones repeat the same generator at sizes the CPU would spend minutes on; the GPU
    test asserts the same caps on every case it runs)"""
    for align, D, dtype in LN.PATHS:
        edge = LN.path_kernel(align, D)[1]
        for rows, _ in LN.path_rows(align, D, dtype):
            if rows <= 4352:
                yield align, D, dtype, edge, rows


def test_input_caps_of_the_gpu_cases():
    seen = set()
    for align, D, dtype, edge, rows in _cpu_cases():
        key = (D, dtype, edge, rows)
        if key in seen:
            continue
        seen.add(key)
        for regime in ("unit", "offset"):
            c = LN.make_case(D, rows, regime, edge, getattr(torch, dtype))
            dy, share, delta = LN.gated_dy(c)
            assert share <= 0.01, (D, dtype, rows, regime, share)
            assert 0 < delta < 1e-3
            assert torch.isfinite(c["x"].float()).all() and torch.isfinite(dy.float()).all()
            for r in c["exact_rows"]:
                assert torch.equal(dy[r], c["dy"][r])
        c = LN.make_case(D, rows, "unit", edge, getattr(torch, dtype))
        want = sorted({r for r in (0, edge - 1, edge, rows - 1) if 0 <= r < rows}) if rows >= 3 else []
        assert sorted(c["exact_rows"]) == want and sorted(c["zero_rows"] + c["const_rows"]) == want
        for r in c["zero_rows"]:
            assert bool((c["x"][r] == 0).all())
        for r in c["const_rows"]:
            assert bool((c["x"][r] == 1.5).all()) and D & (D - 1) == 0
        if rows >= 3:
            assert c["zero_rows"] and (c["const_rows"] or D == 25 or len(want) < 2)
        b = c["b"]
        assert bool((b == 0).any()) and bool((b > 0).any()) and bool((b < 0).any()) and float(b[b != 0].abs().min()) >= 0.05


def test_launch_table():
    """the row counts sit on the seams they are meant for"""
    assert LN.path_kernel("aligned", 64) == ("lnw", 32) and LN.path_kernel("misaligned", 64) == ("ln", 4) and LN.path_kernel("lnr", 25) == ("lnr", 256)
    assert max(r for r, _ in LN.path_rows("aligned", 64, "float32")) == 262145
    assert [r for r, _ in LN.path_rows("aligned", 25, "bfloat16")][-1] == 4095 and min(r for r, _ in LN.path_rows("lnr", 25, "bfloat16")) == 4096
    assert (2048 * 256 + 1, False) in LN.path_rows("lnr", 25, "bfloat16") and (4099 * 25) % 8 != 0 and 4351 % 256 == 255
    assert LN.launch_depth("aligned", 64, 1024 * 32 + 1) == 2 + 32 + 1024 and LN.launch_depth("misaligned", 64, 3) == 1 + 4 + 1
    assert LN.launch_depth("lnr", 25, 2048 * 256 + 1) == 2 + 256 + 2048
