"""CPU: tests/linear_reference.py itself - the fp64 reference against autograd through F.linear, the yardstick against the rule in both
regimes, the exact regime's headroom, the rule against planted errors, and the launch table against hand-computed values.
tests/test_gpu_linear_fp64.py holds the kernels to this reference.

Rejection: every planted error (linear_reference.PLANTS) is computed as the yardstick is, so it is what a kernel with that one error would
return, and the rule must refuse it in the exact regime at a shape and row count where it bites (REJECTED_AT); the plants that move an
element by more than its bound there are refused in the real regime too.  One entry cannot be refused by any rule: `relu_before_round`.
Rounding to bf16 is monotone and keeps the sign, so max(round(a), 0) and round(max(a, 0)) are the same number for every a (only a zero's
sign can differ, which the rule leaves open); test_relu_commutes_with_the_rounding pins that instead."""
import pytest
import torch

import linear_reference as L


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_reference_matches_autograd_in_double(mode):
    c = L.make_forward_case(40, 24, 37, "real", seed=3)
    x = c["x"].double()
    W = c["W"].double().requires_grad_(True)
    b = c["b"].double().requires_grad_(True)
    aux = c["aux"].double()
    a = torch.nn.functional.linear(x, W, b)
    y = {0: a, 1: torch.relu(a), 2: a + aux, 3: a * (aux > 0)}[mode]
    assert float((L.linear_ref(c["x"], c["W"], c["b"], c["aux"], mode) - y.detach()).abs().max()) <= 1e-12
    g = L.make_wgrad_case(40, 24, 37, "real", seed=3)
    dw, db = torch.autograd.grad(a, (W, b), g["dy"].double())           # a's weight gradient, from the case's x
    ref = L.wgrad_ref(c["x"], g["dy"])
    assert float((ref["dw"] - dw).abs().max()) <= 1e-12 * float(dw.abs().max())
    assert float((ref["db"] - db).abs().max()) <= 1e-12 * float(db.abs().max())
    assert bool((ref["aw"] >= ref["dw"].abs()).all()) and bool((ref["ab"] >= ref["db"].abs()).all())


def test_exact_regime_is_exact_and_exercises_the_roundings():
    c = L.make_forward_case(192, 64, 257, "exact")
    x, W, b = c["x"], c["W"], c["b"]
    a64 = L.linear_terms(x, W, b)[0]
    perm = torch.randperm(192, generator=torch.Generator().manual_seed(1))
    a32 = x.float() @ W.float().t() + b.float()
    a32p = x.float()[:, perm] @ W.float()[:, perm].t() + b.float()
    assert torch.equal(a32.double(), a64) and torch.equal(a32p.double(), a64)
    moved = (a64 - a64.float().to(torch.bfloat16).double()).abs()
    assert float(moved.max()) >= 0.0625                                  # an element of 16 .. 32 (or beyond) lost its low bits
    mag = a64.abs()
    tie = ((mag >= 8) & (mag < 16) & (moved == 1 / 32)) | ((mag >= 16) & (mag < 32) & (moved == 1 / 16))
    assert int(tie.sum()) > 0 and int((moved > 0).sum()) > 100           # ties (exactly half an ulp) among them
    for mode in (0, 1, 2, 3):
        y32, y64 = L.linear_yardstick(x, W, b, c["aux"], mode), L.linear_yardstick(x, W, b, c["aux"], mode, wd=torch.float64)
        assert torch.equal(y32, y64)
    assert int((c["aux"] == 0).sum()) > 0 and int((c["aux"] < 0).sum()) > 0
    assert 9 * 262145 < 2 ** 24 and L.wgrad_headroom(262145) < 2 ** 24


def test_headroom_of_every_gpu_case():
    for K, N in L.FWD_CASES:
        assert L.forward_headroom(K) < 2 ** 24
        for rows in (1, 17, 65):
            L.make_forward_case(K, N, rows, "exact")                     # asserts its own headroom and exact storage
            L.make_forward_case(K, N, rows, "real")                      # asserts: no subnormals
    every = [(I, O, r) for I, O in L.WGRAD_CASES + L.WGRAD_SLICED_CASES for r in L.WGRAD_ROWS]
    every += [(I, O, r) for I, O in L.WGRAD_BIG_ROWS_CASES for r in L.WGRAD_BIG_ROWS]
    every += [(I, O, r) for I, O in L.BIG_CASES for r in L.BIG_ROWS + L.BIG_ROWS_EXACT]
    every += [(p["I"], p["O"], p["rows"]) for p in L.grouped_problems()]
    for I, O, rows in every:
        assert L.wgrad_headroom(rows) < 2 ** 24
    for I, O in L.WGRAD_CASES:
        L.make_wgrad_case(I, O, 65, "exact")
        L.make_wgrad_case(I, O, 65, "real")
    for regime in ("exact", "real"):
        p = L.prefill((13, 40), regime, 3)
        assert float(p.abs().max()) <= 1000 and p.unique().numel() > 100
    assert torch.equal(L.prefill((256, 1032), "exact", 2), L.prefill((256, 1032), "exact", 2).round())


@pytest.mark.parametrize("regime", ["exact", "real"])
def test_yardstick_is_accepted(regime):
    for K, N in ((8, 8), (72, 40), (192, 64)):
        c = L.make_forward_case(K, N, 65, regime)
        for mode, bias in L.fwd_modes(N):
            b = c["b"] if bias else None
            y = L.linear_yardstick(c["x"], c["W"], b, c["aux"], mode)
            bad, ek, ey, sh = L.judge_forward(y, c["x"], c["W"], b, c["aux"], mode, regime)
            assert not bad and sh <= 1.0, (K, N, mode, bad)
    for I, O in ((31, 13), (64, 64), (264, 8)):
        c = L.make_wgrad_case(I, O, 129, regime)
        ref = L.wgrad_ref(c["x"], c["dy"])
        dw0, db0 = L.prefill((O, I), regime, 1), L.prefill((O,), regime, 2)
        dw, db = L.wgrad_result(c["x"], c["dy"], dw0, db0)
        depth = L.wgrad_depth(129, I, O)
        assert not L.judge_wgrad(dw, dw0, ref["dw"], ref["aw"], regime, depth)[0]
        assert not L.judge_wgrad(db, db0, ref["db"], ref["ab"], regime, depth)[0]


def _forward_refused(plant, regime, K, N, rows, mode):
    c = L.make_forward_case(K, N, rows, regime)
    args = (c["x"], c["W"], c["b"], c["aux"], mode)
    assert not L.judge_forward(L.linear_yardstick(*args), *args, regime)[0], "the yardstick fails its own rule"
    return L.judge_forward(L.linear_yardstick(*args, plant=plant), *args, regime)[0]


def _wgrad_refused(plant, regime, I, O, rows, ld=0, col0=0):
    """-> failures of dw (inside the window by the rule, outside it bit for bit) and of db"""
    c = L.make_wgrad_case(I, O, rows, regime)
    ref = L.wgrad_ref(c["x"], c["dy"])
    dw0, db0 = L.prefill((O, ld or I), regime, 1), L.prefill((O,), regime, 2)
    depth = L.wgrad_depth(rows, I, O)
    out = []
    for p in (None, plant):
        dw, db = L.wgrad_result(c["x"], c["dy"], dw0, db0, col0, plant=p)
        win = slice(col0, col0 + I)
        bad = L.judge_wgrad(dw[:, win], dw0[:, win], ref["dw"], ref["aw"], regime, depth)[0]
        bad += L.judge_wgrad(db, db0, ref["db"], ref["ab"], regime, depth)[0]
        keep = torch.ones(ld or I, dtype=torch.bool)
        keep[win] = False
        if not torch.equal(dw[:, keep], dw0[:, keep]):
            bad.append("a column outside the window changed")
        out.append(bad)
    assert not out[0], "the yardstick fails its own rule"
    return out[1]


# plant -> (forward?, arguments, the regimes that must refuse it)
REJECTED_AT = {
    "drop_last_row": (False, dict(I=8, O=8, rows=131073), ("exact",)),
    "stale_last_stage": (False, dict(I=24, O=16, rows=129), ("exact", "real")),
    "drop_k_chunk": (True, dict(K=24, N=24, rows=65, mode=0), ("exact", "real")),
    "perm_tile_rows": (True, dict(K=24, N=24, rows=65, mode=0), ("exact", "real")),
    "dw_transposed": (False, dict(I=24, O=24, rows=65), ("exact", "real")),
    "no_second_round": (True, dict(K=192, N=64, rows=257, mode=2), ("exact",)),       # (real: one bf16 ulp, inside the bound)
    "gate_ge": (True, dict(K=40, N=16, rows=65, mode=3), ("exact",)),                  # (real: aux has no exact zero)
    "bias_per_kstep": (True, dict(K=96, N=32, rows=65, mode=0), ("exact", "real")),
    "db_every_slice": (False, dict(I=264, O=8, rows=65), ("exact", "real")),
    "window_shift": (False, dict(I=31, O=13, rows=65, ld=40, col0=5), ("exact", "real")),
    "overwrite": (False, dict(I=24, O=16, rows=65), ("exact", "real")),
    "second_pass_first_tile": (True, dict(K=8, N=8, rows=131073, mode=0), ("exact",)),
}


@pytest.mark.parametrize("plant", [p for p in L.PLANTS if p != "relu_before_round"])
def test_rule_rejects_planted_error(plant):
    forward, kw, regimes = REJECTED_AT[plant]
    for regime in regimes:
        bad = (_forward_refused if forward else _wgrad_refused)(plant, regime, **kw)
        print(f"LIN-PLANT {plant} {regime} {kw}: {bad}")
        assert bad, (plant, regime)
    if plant == "drop_last_row":                                  # one row among 65 is far above the real regime's bound; among 10^5 it is not
        assert _wgrad_refused(plant, "real", 8, 8, 65) and _wgrad_refused(plant, "exact", 8, 8, 4099)


def test_relu_commutes_with_the_rounding():
    """`relu_before_round` is no error: the two orders give the same bf16 number for every a (a zero's sign apart)"""
    assert set(REJECTED_AT) | {"relu_before_round"} == set(L.PLANTS)
    for regime in ("exact", "real"):
        c = L.make_forward_case(192, 64, 257, regime)
        args = (c["x"], c["W"], c["b"], c["aux"], 1)
        assert L.same_but_zero_sign(L.linear_yardstick(*args, plant="relu_before_round"), L.linear_yardstick(*args))
    a = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()     # every bf16 value ...
    a = a[torch.isfinite(a)]
    a = torch.cat([a, a * (1 + 2.0 ** -9), a * (1 + 2.0 ** -8), a * (1 - 2.0 ** -9)])                      # ... and fp32 values between them
    r = lambda t: t.to(torch.bfloat16).float()
    assert torch.equal(r(a.clamp_min(0.0)), r(a).clamp_min(0.0))


def test_rows_supported_enumerated():
    for K in range(8, 193, 8):
        for N in range(1, 193):
            want = N <= 192 if K <= 64 else (N <= 128 if K <= 128 else N <= 64)
            assert L.rows_supported(1, K, N) == want, (K, N)
            if want:
                l = L.rows_launch(1, K, N)
                assert (l["KS"], l["NT"]) in L.LINROWS_INSTANCES and l["KS"] * 32 >= K and l["NT"] * 16 >= N
    assert not L.rows_supported(1, 12, 8) and not L.rows_supported(1, 200, 8) and not L.rows_supported(1, 8, 193) and not L.rows_supported(0, 8, 8)
    assert len(L.LINROWS_INSTANCES) == 21
    assert L.rows_launch(1, 160, 8)["KS"] == 6 and L.rows_launch(1, 136, 8)["KS"] == 6 and L.rows_launch(1, 40, 40)["NT"] == 4


def test_launch_table_at_the_boundaries():
    g = lambda R: {k: L.wgrad_grid(R, 64, 64)[k] for k in ("nb", "per")}           # tile 64 x 80 = 5120: cap 512
    assert g(64) == {"nb": 1, "per": 64} and g(65) == {"nb": 1, "per": 128}
    assert g(960) == {"nb": 1, "per": 960} and g(961) == {"nb": 2, "per": 512}
    assert g(1023) == {"nb": 2, "per": 512} and g(1024) == {"nb": 2, "per": 512} and g(1025) == {"nb": 2, "per": 576}
    assert g(4609) == {"nb": 9, "per": 576} and 4609 - 8 * 576 == 1               # a last block of one row
    assert g(131071) == {"nb": 256, "per": 512} and g(131072) == {"nb": 128, "per": 1024} and g(131073) == {"nb": 121, "per": 1088}  # 2049 stages over 128 blocks: 17 each
    assert L.wgrad_grid(131071, 159, 256)["cap"] == 256 and L.wgrad_grid(2 ** 21, 8, 8) == {"stages": 32768, "cap": 1024, "spb": 16, "nb": 1024, "per": 2048}
    assert L.wgrad_depth(131071, 64, 64) == 512 + 256 + 1 and L.wgrad_depth(1, 31, 13) == 64 + 1 + 1
    s = L.wgrad_launches(700, 264, 128)
    assert [(l["col0"], l["W"], l["db"], l["IT"], l["OTW"], l["tr"]) for l in s] == [(0, 128, True, 10, 2, True), (128, 128, False, 10, 2, True), (256, 8, False, 10, 2, True)]
    assert [l["W"] for l in L.wgrad_launches(1, 160, 8)] == [128, 32] and len(L.wgrad_launches(1, 1024, 256)) == 8
    assert not L.wgrad_sliced(159, 8) and not L.wgrad_sliced(160, 13) and L.wgrad_supported(1, 159, 13) and not L.wgrad_supported(1, 161, 8)
    r = lambda R: (L.rows_launch(R, 8, 8)["grid"], L.rows_launch(R, 8, 8)["passes"])
    assert r(1) == (1, 1) and r(65) == (2, 1) and r(131072) == (2048, 1) and r(131073) == (2048, 2) and L.FWD_FULL_GRID == 131072
    b = lambda R: {k: L.big_launch(R, 128, 256)[k] for k in ("groups", "per", "tiles_i", "tiles_o", "workspace")}
    assert b(65535) == {"groups": 8, "per": 8192, "tiles_i": 2, "tiles_o": 2, "workspace": 8 * 256 * 256}
    assert b(65536) == {"groups": 16, "per": 4096, "tiles_i": 2, "tiles_o": 2, "workspace": 16 * 256 * 256}
    assert b(1)["per"] == 64 and L.big_launch(1, 120, 128)["tiles_i"] == 1 and L.big_launch(1, 1016, 128)["tiles_i"] == 8
    assert L.big_depth(65537, 8, 128) == 4160 + 16 + 1


def test_the_gpu_cases_cover_the_launch_table():
    assert sorted({(l["KS"], l["NT"]) for l in (L.rows_launch(1, K, N) for K, N in L.FWD_CASES)}) == sorted(L.LINROWS_INSTANCES) and len(L.FWD_CASES) == 21
    assert {(l["KS"]) for l in (L.rows_launch(1, K, N) for K, N in L.FWD_BIG_CASES)} == set(L.LINROWS_KS) and set(L.FWD_BIG_CASES) <= set(L.FWD_CASES)
    assert {(l["tr"], l["OTW"], l["IT"]) for I, O in L.WGRAD_CASES for l in L.wgrad_launches(1, I, O)} == set(L.WGRAD_INSTANCES)
    assert all(L.wgrad_sliced(I, O) for I, O in L.WGRAD_SLICED_CASES)
    assert {l["OTW"] for I, O in L.WGRAD_SLICED_CASES for l in L.wgrad_launches(1, I, O)} == {1, 2, 4}
    units = [(l["tr"], l["OTW"], l["IT"]) for p in L.grouped_problems() for l in L.wgrad_launches(p["rows"], p["I"], p["O"])]
    assert max(units.count(u) for u in set(units)) > L.WG_MAX_UNITS and all(1 <= p["rows"] <= 5000 for p in L.grouped_problems())
    assert all(L.big_supported(r, I, O) for I, O in L.BIG_CASES for r in L.BIG_ROWS)
