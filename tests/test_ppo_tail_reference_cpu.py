"""CPU checks of tests/ppo_tail_reference.py, the fp64 reference that tests/test_gpu_ppo_tail_fp64.py holds k_gae / k_adv_stats /
k_adv_normalise, k_ppo_loss and k_grad_sumsq / k_adam_step to: it reproduces the golden fixtures of the reference implementation, it
equals torch autograd (loss) and torch.optim.Adam behind clip_grad_norm_ (optimiser) in float64, its case tables reach what they name,
near-boundary rows are rare, and `judge` rejects every planted arithmetic slip."""
import math

import numpy as np
import pytest
import torch

import golden_util as gu
import ppo_tail_reference as R


def test_gae_reference_reproduces_the_goldens():
    """the fp64 recurrence against gae*_returns / gae*_adv of tests/golden/gae_ppo.npz, within the fixture's fp32 precision (the
    tolerances tests/test_gpu_obs_ppo.py grants an fp32 evaluation of the same recurrence)"""
    g = gu.load("gae_ppo.npz")
    for ci in range(3):
        r, v, m = (torch.from_numpy(g[f"gae{ci}_{k}"]) for k in ("rewards", "values", "masks"))
        ret, raw = R.gae_eval(r, v, m, torch.float64)
        assert np.allclose(ret.numpy(), g[f"gae{ci}_returns"], rtol=2e-6, atol=1e-4)
        assert np.allclose(R.adv_normalise(raw).numpy(), g[f"gae{ci}_adv"], rtol=1e-4, atol=1e-5)
        y_ret, _ = R.gae_eval(r, v, m, torch.float32)
        assert np.array_equal(y_ret.numpy(), g[f"gae{ci}_returns"]), "the fp32 yardstick is the reference implementation's recurrence bit for bit"


def test_gae_case_tables():
    assert {(t, n) for t, n in R.GAE_CASES} >= {(1, 1), (2, 255), (3, 256), (33, 257), (200, 257), (7, 4097), (2, 65793)}
    assert (65793 + 255) // 256 == 258 > 256                              # the second trip of k_adv_stats's loop
    assert R.edge_masks(33, 257) == [(1, 0), (32, 255), (32, 256), (33, 256)]
    for T, N in R.GAE_CASES:
        c = R.gae_case(T, N, "const")
        # every raw advantage is c, and N T c, N T c^2 are exact: mean = c and var = 0 exactly
        assert bool((c["yard_raw"] == R.CONST_C).all()) and c["sum"] == T * N * R.CONST_C and c["sumsq"] == T * N * R.CONST_C ** 2
        assert bool((R.gae_case(T, N, "zero")["yard_raw"] == 0).all())
        e = R.gae_case(T, N, "edges")
        assert int((e["m"] == 0).sum()) == len(R.edge_masks(T, N)) >= 1
        if T * N > 1:
            # a mask read one step early changes a result
            wrong, _ = R.gae_eval(e["r"], e["v"], e["m"], torch.float32, plant="mask_t")
            assert not torch.equal(wrong, e["yard_ret"]), (T, N)
    for regime in R.GAE_REGIMES:                                         # no fp32 denormal among inputs and results
        c = R.gae_case(33, 257, regime)
        for k in ("r", "v", "m", "yard_ret", "yard_raw"):
            a = c[k].abs()
            assert not bool(((a > 0) & (a < 2.0 ** -126)).any()), (regime, k)


def _rows_autograd_covers(c):
    d = c["logp"].double() - c["old"].double()
    return (d < 88.0) & (d > -100.0)


@pytest.mark.parametrize("B", (257, 4097))
def test_loss_reference_equals_autograd_fp64(B):
    """on every row whose ratio an fp32 number holds (the ties included: autograd's halves are the reference's), and the stated rule on
    the others"""
    for regime, use_norm, coef, clip in R.loss_configs(B):
        c = R.loss_case(B, regime, use_norm, coef, clip)
        ref, ag = c["ref"], R.loss_autograd(c, clip, coef, use_norm)
        rows = _rows_autograd_covers(c)
        for n in ("d_logp", "d_values"):
            assert torch.allclose(ref[n][rows], ag[n][rows], rtol=1e-12, atol=1e-300), (regime, use_norm, clip, n)
        assert torch.allclose(ref["d_values"], ag["d_values"], rtol=1e-12, atol=1e-300)
        if regime != "planted":
            assert bool(rows.all()) and torch.allclose(ref["losses"], ag["losses"], rtol=1e-12)
            continue
        pos = R.plant_positions(B)
        k = lambda d, a: pos[R.POLICY_PLANTS.index((d, a))]
        # ratio = +inf: adv > 0 clipped (term -s2, gradient 0; fp32 autograd forms 0 * inf there), adv < 0 the term +inf and the gradient +inf
        assert float(ref["d_logp"][k(100.0, 1.0)]) == 0.0 and float(ref["ta"][k(100.0, 1.0)]) == -(1.0 + clip)
        assert float(ref["d_logp"][k(100.0, -1.0)]) == R.INF and float(ref["ta"][k(100.0, -1.0)]) == R.INF and float(ref["losses"][0]) == R.INF
        # ratio = 0
        assert float(ref["d_logp"][k(-200.0, 1.0)]) == 0.0 and float(ref["d_logp"][k(-200.0, -1.0)]) == 0.0
        # clipped rows: exactly 0; unclipped outside rows: -ratio adv / B
        if clip == 0.25:
            assert float(ref["d_logp"][k(1.0, 1.0)]) == 0.0 and float(ref["d_logp"][k(-1.0, -1.0)]) == 0.0
            assert float(ref["d_logp"][k(1.0, -1.0)]) == math.e / B and float(ref["d_logp"][k(-1.0, 1.0)]) == -math.exp(-1.0) / B
            assert float(ref["d_logp"][k(0.125, 1.0)]) == -math.exp(0.125) / B
        else:
            assert float(ref["d_logp"][k(0.0, 1.5)]) == -1.5 / B and float(ref["d_logp"][k(0.125, 1.0)]) == 0.0
        if not use_norm and clip == 0.25:
            sym = pos[R.SYM_TIE]
            assert tuple(float(c[x][sym]) for x in ("v", "v_old", "ret")) == (0.75, 0.0, 0.5)
            assert float(ref["d_values"][sym]) == coef * 0.5 * 0.25 / B == float(ag["d_values"][sym])
            assert float(ref["d_values"][pos[0]]) == coef * (0.25 - 1.0) / B           # v - vp = +clip: vin holds with equality
            assert float(ref["d_values"][pos[7]]) == 0.0                                  # outside, the clipped error the larger
        assert not bool((c["near"]["ratio"] | c["near"]["vclip"] | c["near"]["l1l2"])[c["planted"]].any())


def test_loss_reference_reproduces_the_goldens():
    """ppoU*: the reference implementation's own PPO.update (losses as it returns them, the gradients its backward hands over)"""
    g = gu.load("gae_ppo.npz")
    coef, clip = float(g["ppoU_value_loss_coef"]), float(g["ppoU_clip"])
    for ci in range(3):
        c = {k: torch.from_numpy(g[f"ppoU{ci}_{k}"]).reshape(-1) for k in ("logp", "old", "adv", "v", "v_old", "ret")}
        out = R.loss_eval(c, clip, coef, bool(int(g[f"ppoU{ci}_use_norm"])), torch.float64)
        assert abs(float(out["losses"][0]) - float(g[f"ppoU{ci}_action_loss"])) < 1e-5
        assert abs(float(out["losses"][1]) * coef - float(g[f"ppoU{ci}_value_loss_x_coef"])) < 1e-5
        assert np.allclose(out["d_logp"].numpy(), g[f"ppoU{ci}_dlogp"].reshape(-1), atol=1e-7, rtol=1e-4)
        assert np.allclose(out["d_values"].numpy(), g[f"ppoU{ci}_dv"].reshape(-1), atol=1e-7, rtol=1e-3)


def test_loss_case_tables():
    assert {min(256, -(-B // 1024)) for B in R.LOSS_ROWS} >= {1, 2, 5, 65, 255, 256}
    assert (-(-261120 // 1024), -(-261121 // 1024), -(-1024 // 1024), -(-1025 // 1024)) == (255, 256, 1, 2)
    seen = set()
    for B in R.LOSS_ROWS:
        cfg = R.loss_configs(B)
        seen |= {(r, n) for r, n, _, _ in cfg} | {("clip", cl) for *_, cl in cfg} | {("coef", co) for _, _, co, _ in cfg}
        if B >= 16:
            pos = R.plant_positions(B)
            assert pos[0] == 0 and pos[1] == B - 1 and (B <= 257 or {255, 256} <= set(pos)) and all(0 <= x < B for x in pos)
            c = R.loss_inputs(B, "planted", False)
            assert int(c["planted"].sum()) == len(R.POLICY_PLANTS) >= len(R.VALUE_PLANTS)
    assert seen >= {(r, n) for r in R.LOSS_REGIMES for n in (False, True)} | {("clip", x) for x in R.CLIPS} | {("coef", x) for x in R.COEFS}
    for regime in R.LOSS_REGIMES:                                        # no fp32 denormal among the finite results
        c = R.loss_case(262145, regime, False, 1.0, 0.25)
        for n in ("d_logp", "d_values"):
            a = c["yard"][n].abs()
            assert not bool(((a > 0) & (a < 2.0 ** -126)).any()), (regime, n)


def test_near_boundary_rows_are_rare():
    """at most 0.1 % of any random case, on the reference alone"""
    worst = 0.0
    for B in (4097, 65537, 262145):
        for regime, use_norm, coef, clip in R.loss_configs(B):
            c = R.loss_case(B, regime, use_norm, coef, clip)
            for k, rows in c["near"].items():
                share = float(rows.double().mean())
                worst = max(worst, share)
                assert share <= 1e-3, (B, regime, use_norm, clip, k, share)
    print(f"largest near-boundary share {worst:.1e}")


@pytest.mark.parametrize("name,regime,max_norm", [x for x in R.ADAM_CASES if x[0] in ("one", "tails")] + [("c257", "unit", None), ("trips", "threshold", R.MAX_NORM)])
def test_adam_reference_equals_torch_fp64(name, regime, max_norm):
    """the written-out update against torch.optim.Adam + clip_grad_norm_ on float64 copies: every step, p, exp_avg, exp_avg_sq, the norm
    and the per-tensor step counts"""
    c = R.adam_case(name, regime, max_norm)
    ref, th = R.adam_ref(c), R.adam_torch(c, torch.float64)
    for k in range(R.ADAM_STEPS):
        assert ref[k]["steps"] == th[k]["steps"] and math.isclose(ref[k]["norm"], th[k]["norm"], rel_tol=1e-12)
        for n in ("p", "m", "v"):
            for i, (a, b) in enumerate(zip(ref[k][n], th[k][n])):
                assert torch.allclose(a, b, rtol=1e-11, atol=0.0), (k, n, i, float((a - b).abs().max()))


def test_adam_case_tables():
    chunks = {name: sum(-(-n // R.CHUNK) for n in sizes) for name, sizes in R.ADAM_LISTS.items()}
    assert (chunks["c255"], chunks["c256"], chunks["c257"]) == (255, 256, 257) and chunks["trips"] > 2 * 256 and chunks["one"] == 1
    assert {n % 4 for n in R.ADAM_LISTS["tails"]} == {0, 1, 3} and {R.step_count(i) for i in range(7)} == set(R.STEP_COUNTS)
    assert {r for _, r, _ in R.ADAM_CASES} == set(R.ADAM_REGIMES) and {m for _, _, m in R.ADAM_CASES} == {R.MAX_NORM, None}
    assert {n for n, _, _ in R.ADAM_CASES} == set(R.ADAM_LISTS)
    for name, regime, max_norm in R.ADAM_CASES:
        if name in ("c255", "c256", "c257"):
            continue
        c = R.adam_case(name, regime, max_norm)
        if regime == "threshold":                                        # the norm is 0.5 to the last fp32 bit, the coefficient just below 1
            n = R.grad_norm64(c["grads"][0])
            assert float(torch.tensor(n, dtype=torch.float64).float()) == 0.5 and 0.5 / (0.5 + 1e-6) < 1.0
        for gs in c["grads"]:                                            # no fp32 denormal, squares and the (1 - beta2) term included
            for x in gs:
                if x is not None:
                    sq = (x * x) * (1.0 - R.HYPER["betas"][1])
                    assert not bool(((x != 0) & (sq < 2.0 ** -126)).any()), (name, regime)
        assert all(bool((m >= 0).all()) and bool((v >= 0).all()) for m, v in zip(c["m0"], c["v0"]))
        if regime.startswith("none"):
            assert all(c["grads"][k][i] is None for k in range(R.ADAM_STEPS) for i in R.NONE_TENSORS)


def _gae_got(c, plant):
    ret, raw = R.gae_eval(c["r"], c["v"], c["m"], torch.float32, plant=plant if plant != "cnt" else None)
    a = raw.double()
    return {"ret": ret, "raw": raw, "adv": R.adv_normalise(raw, plant=plant), "stats": [float(a.sum()), float((a * a).sum()), float(a.numel())]}


def test_judge_accepts_the_yardstick_and_rejects_planted_slips():
    """each wrong "kernel output" is the fp32 yardstick with ONE arithmetic slip (the lines the planted builds of
    profiles/ppo_tail_kernel_tests.txt change in the kernels): the bounds can fail, and do for every output"""
    c = R.gae_case(33, 257, "game")
    assert R.gae_judge(c, _gae_got(c, None))[0] == []
    for plant, outs in (("mask_t", {"ret", "raw", "stats[0]"}), ("gl_gamma", {"ret", "raw", "stats[0]"}), ("cnt", {"adv"})):
        bad = R.gae_judge(c, _gae_got(c, plant))[0]
        assert outs <= {b[1] for b in bad}, (plant, bad)
    for plant, outs, regime, clip in (("inside_only", {"d_logp"}, "far", 0.2), ("vin_lt", {"d_values"}, "planted", 0.25),
                                      ("no_half", {"value_loss"}, "unit", 0.2)):
        c = R.loss_case(4097, regime, False, 0.5, clip)
        good = {k: c["yard"][k] for k in ("losses", "d_logp", "d_values")}
        assert R.loss_judge(c, good)[0] == []
        bad = R.loss_judge(c, R.loss_eval(c, clip, 0.5, False, torch.float32, plant=plant))[0]
        assert outs <= {b[0] for b in bad}, (plant, bad)
    # the symmetric tie taken in full, and a swallowed NaN, as k_ppo_loss had them
    c = R.loss_case(4097, "planted", False, 0.5, 0.25)
    got = {k: c["yard"][k].clone() for k in ("losses", "d_logp", "d_values")}
    got["d_values"][R.plant_positions(4097)[R.SYM_TIE]] *= 2.0
    assert {b[0] for b in R.loss_judge(c, got)[0]} == {"d_values"}
    cc, ref, yard = R.adam_expected("tails", "unit", R.MAX_NORM)
    as_got = lambda o: {"p": o["p"], "m": o["m"], "v": o["v"], "norm": o["norm"], "steps": o["steps"]}
    for k in range(R.ADAM_STEPS):
        assert R.adam_judge(cc, ref, yard, k, as_got(yard[k]))[0] == []
    for plant in ("bias_eps", "no_bias1"):
        wrong = R.adam_ref(cc, torch.float32, plant=plant)
        bad = R.adam_judge(cc, ref, yard, 0, as_got(wrong[0]))[0]
        assert {b[1] for b in bad} == {"p"}, (plant, bad)
    wrong = as_got(R.adam_ref(cc, torch.float32)[0])
    wrong["m"] = [x * (1.0 + 2.0 ** -13) for x in wrong["m"]]
    wrong["v"] = [x * (1.0 + 2.0 ** -13) for x in wrong["v"]]
    wrong["norm"] = wrong["norm"] * (1.0 + 2.0 ** -15)
    wrong["steps"] = [s + 1 for s in wrong["steps"]]
    assert {b[1] for b in R.adam_judge(cc, ref, yard, 0, wrong)[0]} == {"m", "v", "norm", "step counts"}
    # the written-out fp32 update itself passes: the rule does not ask for torch's own rounding
    assert R.adam_judge(cc, ref, yard, 0, as_got(R.adam_ref(cc, torch.float32)[0]))[0] == []
