"""CPU: tests/lstm_cell_reference.py itself - the fp64 reference against torch.nn.LSTMCell and against autograd of its own forward, the
acceptance rule against planted errors, and the launch table.  tests/test_gpu_lstm_cell_fp64.py holds the kernels to this reference.

Rejection: every planted error (lstm_cell_reference.PLANTS) is computed as the yardstick is - fp32, rounded as the storage type rounds -
so it is what a kernel with that one error would return, and the rule must refuse it in the regime named in REJECTED_IN, at ONE row
of the narrowest cell (L = 4: one lane's work) and at 257 rows, in both storage types."""
import pytest
import torch

import lstm_cell_reference as LS


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("L", [4, 12, 64])
def test_reference_matches_torch_lstm_cell_in_double(L, with_mask):
    """torch.nn.LSTMCell on the input (gx | gh) with W_ih = (I | I), W_hh = 0 and no bias: its gates are gx + gh"""
    c = LS.make_case("unit", 37, L, torch.float32, with_mask, seed=3)
    cell = torch.nn.LSTMCell(8 * L, L, bias=False).double()
    eye = torch.eye(4 * L, dtype=torch.float64)
    m = torch.ones(37, 1, dtype=torch.float64) if c["mask"] is None else c["mask"].double()[:, None]
    with torch.no_grad():
        cell.weight_ih.copy_(torch.cat((eye, eye), 1))
        cell.weight_hh.zero_()
        h, cc = cell(torch.cat((c["gx"].double(), c["gh"].double()), 1), (torch.zeros(37, L, dtype=torch.float64), c["c_prev"].double() * m))
    ref = LS.lstm_ref(c["gx"], c["gh"], c["c_prev"], c["mask"])
    assert float((ref["h"] - h).abs().max()) <= 1e-13 and float((ref["c"] - cc).abs().max()) <= 1e-13


@pytest.mark.parametrize("regime,with_mask", [("unit", False), ("unit", True), ("saturated", True), ("masked", True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_closed_form_gradients_match_autograd_of_the_forward(regime, with_mask, dtype):
    c = LS.make_case(regime, 65, 12, dtype, with_mask, seed=5)
    if regime == "masked":
        c["c_prev"] = torch.where(c["masked_rows"][:, None], torch.full_like(c["c_prev"], 3.0), c["c_prev"])    # (1e30 dh has no fp64 product)
    gx, gh, cp = (c[k].double().requires_grad_(True) for k in ("gx", "gh", "c_prev"))
    o = LS._core(gx, gh, cp, c["mask"], None, None, torch.float64)
    dgx, dgh, dcp = torch.autograd.grad((o["h"] * c["dh"].double()).sum() + (o["c"] * c["dc"].double()).sum(), (gx, gh, cp))
    ref = LS.lstm_ref(c["gx"], c["gh"], c["c_prev"], c["mask"], c["dh"], c["dc"])
    assert torch.equal(dgx, dgh)
    for got, want in ((ref["dgates"], dgx), (ref["dc_prev"], dcp)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_exact_regimes():
    """zero: c = h = 0 in the reference and in the yardstick; saturated: finite, |h| <= 1, every gate activation within 1e-13 of 0 or 1;
    masked: the reference equals the same case with c_prev = 0 on the masked rows"""
    for dtype in (torch.float32, torch.bfloat16):
        c = LS.make_case("zero", 65, 8, dtype, True)
        for o in (LS.lstm_ref(c["gx"], c["gh"], c["c_prev"], c["mask"]), LS.lstm_yardstick(c["gx"], c["gh"], c["c_prev"], c["mask"])):
            assert not bool(o["h"].any()) and not bool(o["c"].any())
        c = LS.make_case("saturated", 65, 8, dtype, True)
        a = (c["gx"].double() + c["gh"].double()).abs()
        assert 30.0 - 0.5 <= float(a.min()) and float(a.max()) <= 100.0 + 0.5
        o = LS.lstm_ref(c["gx"], c["gh"], c["c_prev"], c["mask"], c["dh"], c["dc"])
        assert all(bool(torch.isfinite(v).all()) for v in o.values()) and float(o["h"].abs().max()) <= 1.0
        c = LS.make_case("masked", 65, 8, dtype, True)
        assert bool(c["masked_rows"][0]) and bool((c["c_prev"][c["masked_rows"]] == LS.BIG).all())
        o = LS.lstm_ref(c["gx"], c["gh"], c["c_prev"], c["mask"], c["dh"], c["dc"])
        cp0 = torch.where(c["masked_rows"][:, None], torch.zeros_like(c["c_prev"]), c["c_prev"])
        o0 = LS.lstm_ref(c["gx"], c["gh"], cp0, c["mask"], c["dh"], c["dc"])
        assert all(torch.equal(o[k], o0[k]) for k in o)


# plant -> (regime, with mask pointer, an output that must refuse it)
REJECTED_IN = {
    "gate_order": ("unit", False, "h"),
    "mask_on_c": ("masked", True, "c"),          # row 0 is masked: (F 1e30 + I G) * 0 = 0 instead of I G
    "dcp_no_mask": ("masked", True, "dc_prev"),  # row 0 is masked: d F instead of 0
    "one_minus_tc": ("unit", False, "dgates"),
}


@pytest.mark.parametrize("plant", LS.PLANTS)
def test_rule_rejects_planted_error(plant):
    regime, with_mask, must = REJECTED_IN[plant]
    for dtype in (torch.float32, torch.bfloat16):
        for n, L in ((1, 4), (257, 4), (1, 256)):
            c = LS.make_case(regime, n, L, dtype, with_mask)
            args = (c["gx"], c["gh"], c["c_prev"], c["mask"], c["dh"], c["dc"])
            ref, yard = LS.lstm_ref(*args), LS.lstm_yardstick(*args)
            bf16 = dtype == torch.bfloat16
            clean, _ = LS.judge(bf16, yard, ref, yard)
            assert not clean, ("the yardstick fails its own rule", clean)
            bad, _ = LS.judge(bf16, LS.lstm_yardstick(*args, plant=plant), ref, yard)
            refused = sorted({b[0] for b in bad})
            print(f"LSTM-PLANT {plant} {regime} n={n} L={L} {'bf16' if bf16 else 'fp32'}: refused on {refused}")
            assert must in refused, (plant, dtype, n, L, refused)


def test_launch_table():
    """the row counts sit on the seams they are meant for"""
    assert LS.CAP_ROWS == (65536, 65537)
    assert LS.launch(65536, 256) == (16384, 1) and LS.launch(65537, 256) == (16384, 2)
    assert LS.launch(256, 4) == (1, 1) and LS.launch(257, 4) == (2, 1) and LS.launch(255, 4) == (1, 1)
    assert LS.launch(64, 64) == (4, 1) and LS.launch(65, 64) == (5, 1) and LS.launch(63, 64) == (4, 1)
    assert (256 % (12 // 4)) != 0                                     # L = 12: a row's three items straddle a block edge
    assert LS.launch(1, 4) == (1, 1) and LS.launch(64, 256) == (16, 1) and LS.launch(65, 256) == (17, 1)
    cases = LS.small_cases()
    assert {(L, n) for L, n, _, _ in cases} == {(L, n) for L in LS.HIDDEN for n in LS.ROWS}
    assert {(reg, mp) for _, _, reg, mp in cases} == {("unit", False), ("unit", True), ("saturated", False), ("saturated", True),
                                                      ("zero", False), ("zero", True), ("masked", True)}
    caps = LS.cap_cases()
    assert {(dt, n) for dt, n, _ in caps} == {(dt, n) for dt in LS.DTYPES for n in LS.CAP_ROWS}
    for dt in LS.DTYPES:
        assert {mp for d, _, mp in caps if d == dt} == {False, True}
    assert all(L % 4 == 0 for L in LS.HIDDEN)
