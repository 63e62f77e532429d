"""GPU: the scalar tail of the PPO update against fp64 - k_gae / k_adv_stats / k_adv_normalise and k_ppo_loss (csrc/catan_ppo.hip) through
the C ABI (catan_gae, catan_adv_normalise, catan_ppo_loss), k_grad_sumsq / k_adam_step (csrc/catan_optim.hip) through
optim.FusedAdam.step, whose host half (chunk table, per-tensor bias pairs, pointer ring) is part of what is under test.

reference = tests/ppo_tail_reference.py (its docstring has the formulas, the rule, the scales and the case tables):
    every output   per element |kernel - fp64| <= 2 |yardstick - fp64| + floor * scale, floor 2^-17 (values) / 2^-15 (gradients, p, moments)
    GAE            returns and raw advantages BIT-EQUAL to the step-by-step torch fp32 recurrence; stats[2] = T N exactly, stats[0..1]
                   within T N 2^-52 (sum|a|, sum a^2) of the fp64 sums; constant advantages normalise to exactly 0; the two-rank form
                   (two catan_gae calls on the column halves, their stats3 added on the device) under the one-rank bound
    PPO loss       exact zeros where the reference is 0, inf where it is inf, NaN where it is NaN; on-policy rows bit-equal to
                   -adv * (1 / B); near-boundary rows on one of the two branches; two launches into one workspace bit-equal, the
                   arrival counter back at 0, another B into the used workspace bit-equal to a fresh one
    Adam           p, exp_avg, exp_avg_sq per element after each of three steps from a loaded state; last_norm; torch's per-tensor
                   step counts; a tensor that takes no step keeps every bit; an unaligned gradient goes through the temporary copy

Buffers: every float input lies in front of NaN; every output starts as a sentinel pattern, none of which may be left, in front of
guard elements that must be intact (the workspaces too; the parameters are views into one flat buffer with sentinels between and
behind them; the pad elements between the tensors' slices of FusedAdam's flat state must stay 0).
Every case prints one line (GAE / LOSS / ADAM): per output the kernel's error, the yardstick's, their ratio, the largest share of a bound
used and the floor its elements would need.  Measured on the MI355X: profiles/ppo_tail_kernel_tests.txt is that output."""
import pytest
import torch

import guarded as G
import pin_rule as PR
import ppo_tail_reference as R
from guarded import NAN, ptr as P, stream as _stream

pytestmark = pytest.mark.gpu

GUARD = 512                      # elements behind every buffer
SENTINEL = 0x5A5B5A5B
F32, F64 = torch.float32, torch.float64


def _check(rc):
    from settlers_of_catan_rl_amd import _lib
    _lib.check(rc)


def _input(t, guard=NAN):
    """-> (whole, view): t's elements on the device followed by GUARD elements of `guard`"""
    return G.guarded_input(t, GUARD, guard=guard)


def _output(n, dtype=F32):
    return G.sentinel_output(n, dtype, GUARD, sentinel=SENTINEL)


def _written(whole, view):
    return G.written(whole, view, SENTINEL)


def _line(tag, st, order):
    return tag + ": " + " | ".join(PR.fmt_stat(n, st[n]) for n in order if n in st)


# ----------------------------------------------------------------------------------------------------------------------------- GAE
def _gae(lib, r, v, m):
    """catan_gae on CPU inputs r [T, N], v, m [T + 1, N] -> (ret, raw: device views [T N]; stats: (whole, view) of 3 doubles)"""
    T, N = r.shape
    hold = [_input(x.contiguous()) for x in (r, v, m)]
    ret, raw = _output(T * N), _output(T * N)
    ws, stats = _output(int(lib.catan_gae_workspace_doubles(N)), F64), _output(3, F64)
    nb = (N + 255) // 256
    assert ws[1].numel() >= 2 * nb
    _check(lib.catan_gae(P(hold[0][1]), P(hold[1][1]), P(hold[2][1]), T, N, R.GAMMA, R.LAM, P(ret[1]), P(raw[1]), P(ws[1]), P(stats[1]), _stream()))
    torch.cuda.synchronize()
    for n, (whole, view) in (("returns", ret), ("adv_raw", raw), ("stats3", stats)):
        assert _written(whole, view) and G.intact(whole, view), (T, N, n, "an element left unwritten, or a write behind the output")
    assert G.intact(*ws) and _written(ws[0], ws[1][:2 * nb]), (T, N, "workspace")
    return ret[1], raw[1], stats


def _normalise(lib, raw, stats_view):
    """catan_adv_normalise on a copy of raw (device [n]) -> device [n]"""
    whole, view = _output(raw.numel())
    view.copy_(raw)
    _check(lib.catan_adv_normalise(P(view), raw.numel(), P(stats_view), _stream()))
    torch.cuda.synchronize()
    assert _written(whole, view) and G.intact(whole, view), "catan_adv_normalise wrote behind its array"
    return view


@pytest.mark.parametrize("T,N", R.GAE_CASES)
def test_gae_kernels_vs_fp64(hip_lib, T, N):
    """catan_gae + catan_adv_normalise at one shape in every regime, one rank and two.  See the module docstring for what is asserted.

    Measured on the MI355X: profiles/ppo_tail_kernel_tests.txt."""
    bad = []
    for regime in R.GAE_REGIMES:
        c = R.gae_case(T, N, regime)
        ret, raw, stats = _gae(hip_lib, c["r"], c["v"], c["m"])
        adv = _normalise(hip_lib, raw, stats[1])
        got = {"ret": ret.cpu().view(T, N), "raw": raw.cpu().view(T, N), "adv": adv.cpu().view(T, N), "stats": stats[1].cpu().tolist()}
        b, st = R.gae_judge(c, got, regime)
        bad += b
        if T * N == 1:
            print(f"GAE T=1 N=1 {regime}: raw {float(got['raw']):.9g} stats {got['stats']} -> normalised {float(got['adv'])!r} (torch: nan; nothing asserted)")
        if N >= 2:
            # two ranks: each its columns, the three statistics added in fp64 on the device, each half normalised with the sum
            h = N // 2
            parts = [_gae(hip_lib, c["r"][:, a:z], c["v"][:, a:z], c["m"][:, a:z]) for a, z in ((0, h), (h, N))]
            total = _input(torch.zeros(3, dtype=F64))
            total[1].copy_(parts[0][2][1] + parts[1][2][1])
            halves = [_normalise(hip_lib, p[1], total[1]).cpu().view(T, -1) for p in parts]
            for n, k in (("ret", 0), ("raw", 1)):
                both = torch.cat([parts[0][k].cpu().view(T, -1), parts[1][k].cpu().view(T, -1)], 1)
                if not PR.same_bits(both, got[n]):
                    bad.append((regime, n, "the two halves differ from the whole"))
            ts = total[1].cpu().tolist()
            u = T * N * 2.0 ** -52
            if ts[2] != T * N or not abs(ts[0] - c["sum"]) <= u * c["abs"] or not abs(ts[1] - c["sumsq"]) <= u * c["sumsq"]:
                bad.append((regime, "two-rank stats", ts))
            bad += R.gae_judge_adv(c, torch.cat(halves, 1), st, regime, "adv2")
        print(_line(f"GAE T={T} N={N} {regime}", st, ("ret", "raw", "sum", "sumsq", "adv", "adv2")))
    assert not bad, bad[:12]


# ------------------------------------------------------------------------------------------------------------------------ PPO loss
LOSS_KEYS = ("logp", "old", "adv", "v", "v_old", "ret")


def _workspace(lib):
    """catan_ppo_loss_workspace_doubles() zeros in front of a sentinel guard -> (whole, view)"""
    whole, view = _output(int(lib.catan_ppo_loss_workspace_doubles()), F64)
    view.zero_()
    return whole, view


def _loss(lib, c, ws, clip=None, value_coef=None, use_norm=None):
    """one catan_ppo_loss launch of case c (CPU tensors) into workspace ws -> {losses, d_logp, d_values} on the CPU"""
    B = c["logp"].numel()
    clip, value_coef, use_norm = (c[k] if x is None else x for k, x in (("clip", clip), ("value_coef", value_coef), ("use_norm", use_norm)))
    hold = [_input(c[k]) for k in LOSS_KEYS]
    outs = {"losses": _output(2), "d_logp": _output(B), "d_values": _output(B)}
    mean, std = R.NORM if use_norm else (0.0, 1.0)
    _check(lib.catan_ppo_loss(*[P(h[1]) for h in hold], B, clip, value_coef, int(use_norm), mean, std, P(outs["losses"][1]), P(outs["d_logp"][1]),
                              P(outs["d_values"][1]), P(ws[1]), _stream()))
    torch.cuda.synchronize()
    for n, (whole, view) in outs.items():
        assert _written(whole, view) and G.intact(whole, view), (B, n, "an element left unwritten, or a write behind the output")
    assert G.intact(*ws), (B, "a write behind the workspace")
    assert ws[1].view(torch.int64)[-1].item() == 0, (B, "the arrival counter is not back at 0")
    return {n: v[1].cpu() for n, v in outs.items()}


def _same(a, b):
    return all(PR.same_bits(a[n], b[n]) for n in ("losses", "d_logp", "d_values"))


@pytest.mark.parametrize("B", R.LOSS_ROWS)
def test_ppo_loss_kernel_vs_fp64(hip_lib, B):
    """catan_ppo_loss at one row count: every regime with the value normaliser off and on, each launched twice into one workspace.

    Measured on the MI355X: profiles/ppo_tail_kernel_tests.txt."""
    bad = []
    ws = _workspace(hip_lib)
    for regime, use_norm, coef, clip in R.loss_configs(B):
        c = R.loss_case(B, regime, use_norm, coef, clip)
        got = _loss(hip_lib, c, ws)
        again = _loss(hip_lib, c, ws)
        if not _same(got, again):
            bad.append((regime, use_norm, "two launches into one workspace differ"))
        b, st = R.loss_judge(c, got)
        bad += [(regime, use_norm, coef, clip) + x for x in b]
        near = sum(int(v.sum()) for v in c["near"].values())
        print(_line(f"LOSS B={B} {regime} norm={int(use_norm)} coef={coef} clip={clip} near={near}", st, ("action_loss", "value_loss", "d_logp", "d_values")))
    assert not bad, bad[:12]


def test_ppo_loss_symmetric_tie_takes_half(hip_lib):
    """l1 == l2 with e1 == -e2 outside the clip range (v = 0.75, vp = 0, ret = 0.5, clip = 0.25): autograd's maximum gives half to each
    side and the clipped side has derivative 0: d_values = value_coef 0.5 e1 / B, exactly"""
    B, coef = 257, 0.5
    c = R.loss_case(B, "planted", False, coef, 0.25)
    got = _loss(hip_lib, c, _workspace(hip_lib))
    for k in (R.SYM_TIE, R.SYM_TIE + 1):
        row = R.plant_positions(B)[k]
        e1 = float(c["v"][row] - c["ret"][row])
        want = torch.tensor(coef, dtype=F32) * (torch.tensor(1.0) / torch.tensor(float(B))) * torch.tensor(0.5 * e1)
        print(f"LOSS tie row {row}: d_values {float(got['d_values'][row])!r}, 0.5 e1 coef / B = {float(want)!r}, e1 in full {2 * float(want)!r}")
        assert float(got["d_values"][row]) == float(want), (row, float(got["d_values"][row]), float(want))


def test_ppo_loss_workspace_carries_nothing_over(hip_lib):
    """a call leaves the workspace as a call needs it: another B launched into a used workspace gives the bits of a fresh one"""
    for first, then in ((262145, 257), (261121, 1025), (2, 65537), (4097, 1)):
        used = _workspace(hip_lib)
        a = R.loss_case(first, "unit", False, R.loss_configs(first)[0][2], R.loss_configs(first)[0][3])
        _loss(hip_lib, a, used)
        regime, use_norm, coef, clip = R.loss_configs(then)[1]
        c = R.loss_case(then, regime, use_norm, coef, clip)
        assert _same(_loss(hip_lib, c, used), _loss(hip_lib, c, _workspace(hip_lib))), (first, then)


def test_ppo_loss_passes_non_finite_rows_on(hip_lib):
    """B = 257, a NaN logp at row 3 and a NaN value at row 256: both losses NaN, those two gradients NaN (torch.min / max / clamp pass
    NaN on), every other gradient the bits of the same case without the poison"""
    B = 257
    regime, use_norm, coef, clip = R.loss_configs(B)[0]
    c = dict(R.loss_case(B, regime, use_norm, coef, clip))
    clean = _loss(hip_lib, c, _workspace(hip_lib))
    c["logp"], c["v"] = c["logp"].clone(), c["v"].clone()
    c["logp"][3], c["v"][256] = NAN, NAN
    ref = R.loss_eval(c, clip, coef, use_norm, F64)
    assert bool(torch.isnan(ref["losses"]).all()) and bool(torch.isnan(ref["d_logp"][3])) and bool(torch.isnan(ref["d_values"][256]))
    got = _loss(hip_lib, c, _workspace(hip_lib))
    print(f"LOSS non-finite: losses {got['losses'].tolist()} d_logp[3] {float(got['d_logp'][3])!r} d_values[256] {float(got['d_values'][256])!r}")
    assert bool(torch.isnan(got["losses"][0])) and bool(torch.isnan(got["d_logp"][3])), "a NaN logp is swallowed"
    assert bool(torch.isnan(got["losses"][1])) and bool(torch.isnan(got["d_values"][256])), "a NaN value is swallowed"
    keep_p, keep_v = torch.arange(B) != 3, torch.arange(B) != 256
    assert PR.same_bits(got["d_logp"][keep_p], clean["d_logp"][keep_p]) and PR.same_bits(got["d_values"][keep_v], clean["d_values"][keep_v])
    assert PR.same_bits(got["d_values"][3:4], clean["d_values"][3:4]) and PR.same_bits(got["d_logp"][256:], clean["d_logp"][256:])


# --------------------------------------------------------------------------------------------------------------------------- Adam
def _layout(sizes):
    """offsets of the views in the flat parameter buffer (16-byte aligned, at least 4 sentinel elements around each) and its length"""
    offs, o = [], 4
    for n in sizes:
        offs.append(o)
        o += ((n + 3) & ~3) + 4
    return offs, o + GUARD


class _Run(object):
    """FusedAdam over views of one sentinel-filled flat buffer, loaded with case c's state"""

    def __init__(self, c):
        from settlers_of_catan_rl_amd.optim import FusedAdam
        self.c, sizes = c, c["sizes"]
        self.offs, total = _layout(sizes)
        self.flat = torch.empty(total, dtype=F32, device="cuda")
        self.flat.view(torch.int32).fill_(SENTINEL)
        self.free = torch.ones(total, dtype=torch.bool, device="cuda")
        self.params = []
        for o, n, p0 in zip(self.offs, sizes, c["p0"]):
            self.flat[o:o + n].copy_(p0)
            self.free[o:o + n] = False
            self.params.append(self.flat[o:o + n].detach().requires_grad_(True))
        assert all(p.data_ptr() % 16 == 0 for p in self.params)
        self.opt = FusedAdam(self.params, lr=R.HYPER["lr"], betas=R.HYPER["betas"], eps=R.HYPER["eps"], none_grad_is_zero=c["none_is_zero"])
        group = {"lr": R.HYPER["lr"], "betas": R.HYPER["betas"], "eps": R.HYPER["eps"], "params": list(range(len(sizes)))}
        self.opt.load_state_dict({"state": {i: {"step": torch.tensor(float(t)), "exp_avg": c["m0"][i], "exp_avg_sq": c["v0"][i]}
                                            for i, t in enumerate(c["steps0"]) if t > 0}, "param_groups": [group]})
        assert self.opt.param_steps.tolist() == list(c["steps0"])
        pad, o = torch.ones(self.opt.exp_avg.numel(), dtype=torch.bool, device="cuda"), 0
        for n in sizes:
            pad[o:o + n] = False
            o += (n + 3) & ~3
        assert o == pad.numel()
        self.pad = pad
        self.hold = []

    def step(self, k, unaligned=None):
        grads = self.c["grads"][k]
        self.hold = []
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif i == unaligned:                                          # a view 4 bytes into a larger buffer
                whole, p.grad = G.guarded_input(g, GUARD, lead=1)
                assert p.grad.data_ptr() % 16 == 4
                self.hold.append(whole)
            else:
                whole, view = _input(g)
                p.grad = view
                self.hold.append(whole)
        given = [p.grad for p in self.params]
        self.opt.step(self.c["max_norm"])
        torch.cuda.synchronize()
        assert all(p.grad is g for p, g in zip(self.params, given)), "step() replaced a .grad"
        assert bool((self.flat.view(torch.int32)[self.free] == SENTINEL).all()), "a write between or behind the parameters"
        assert bool((self.opt.exp_avg[self.pad] == 0).all()) and bool((self.opt.exp_avg_sq[self.pad] == 0).all()), "a pad element of the flat state was written"
        return {"p": [p.detach().cpu() for p in self.params], "m": [m.cpu() for m in self.opt._m], "v": [v.cpu() for v in self.opt._v],
                "norm": float(self.opt.last_norm), "steps": self.opt.param_steps.tolist()}


@pytest.mark.parametrize("name,regime,max_norm", R.ADAM_CASES)
def test_fused_adam_vs_fp64(hip_lib, name, regime, max_norm):
    """three FusedAdam.step calls from a loaded state, every step judged.  See the module docstring for what is asserted.

    Measured on the MI355X: profiles/ppo_tail_kernel_tests.txt."""
    c, ref, yard = R.adam_expected(name, regime, max_norm)
    run = _Run(c)
    bad, total = [], {}
    for k in range(R.ADAM_STEPS):
        got = run.step(k)
        b, st = R.adam_judge(c, ref, yard, k, got)
        bad += b
        for n, s in st.items():
            PR.merge_stat(total, n, s)
        for i, g in enumerate(c["grads"][k]):
            if g is None and not c["none_is_zero"]:                       # no gradient, no step: every bit stays
                if not (PR.same_bits(got["p"][i], c["p0"][i]) and PR.same_bits(got["m"][i], c["m0"][i]) and PR.same_bits(got["v"][i], c["v0"][i])
                        and got["steps"][i] == c["steps0"][i]):
                    bad.append((k, i, "a tensor without a gradient changed"))
    assert run.opt.copied_grads == 0
    print(_line(f"ADAM {name} {regime} max_norm={max_norm}", total, ("p", "m", "v", "norm")))
    assert not bad, bad[:12]


def test_fused_adam_unaligned_gradient_is_copied(hip_lib):
    """a gradient that is a 4-byte-offset view goes through the temporary aligned copy: copied_grads == 1, .grad the same object, the
    result the bits of the aligned case"""
    c, _, _ = R.adam_expected("tails", "unit", R.MAX_NORM)
    a, b = _Run(c), _Run(c)
    ga, gb = a.step(0), b.step(0, unaligned=4)
    assert a.opt.copied_grads == 0 and b.opt.copied_grads == 1
    for n in ("p", "m", "v"):
        assert all(PR.same_bits(x, y) for x, y in zip(ga[n], gb[n])), n
    assert ga["norm"] == gb["norm"] and ga["steps"] == gb["steps"]
