"""CPU: tests/pin_rule.py on hand-made tensors - every bound below is worked out by hand, so an edit to the factor 2, to a floor or to the
summation unit fails here."""
import math

import pytest
import torch

import pin_rule as PR

F64 = torch.float64
NAN, INF = float("nan"), float("inf")
FLOOR = 2.0 ** -9

# three groups of four; the yardstick is off by 0.25, 0 and 0.125 at most in them, their scales are 4, 2 and 1
REF = torch.tensor([[1.0, 0.0, -4.0, 0.5], [2.0, 0.0, -1.0, 0.5], [0.0, -1.0, 0.25, 0.5]], dtype=F64)
YARD = REF + torch.tensor([[0.25, 0.0, 0.0, -0.125], [0.0, 0.0, 0.0, 0.0], [0.0, 0.125, 0.0, 0.0]], dtype=F64)
GROUP_BOUND = (2 * 0.25 + 4.0 / 512, 2.0 / 512, 2 * 0.125 + 1.0 / 512)
WHOLE_BOUND = 2 * 0.25 + 4.0 / 512                      # 0.5078125
ZERO_AT = ((0, 1), (1, 1), (2, 0))                       # an element of every group whose reference is 0: kernel - ref is exact there


def _next(x):
    return math.nextafter(x, INF)


def _kernel(at, value):
    k = REF.clone()
    k[at] = value
    return k


def test_whole_passes_at_the_bound_and_fails_one_ulp_above():
    assert WHOLE_BOUND == 0.5078125
    ok, ek, ey, bound = PR.whole(_kernel((1, 1), WHOLE_BOUND), REF, YARD, FLOOR)
    assert ok and (ek, ey, bound) == (WHOLE_BOUND, 0.25, WHOLE_BOUND)
    assert not PR.whole(_kernel((1, 1), _next(WHOLE_BOUND)), REF, YARD, FLOOR)[0]
    assert not PR.whole(_kernel((1, 1), -_next(WHOLE_BOUND)), REF, YARD, FLOOR)[0]
    assert PR.whole_bound(REF, YARD, FLOOR) == (WHOLE_BOUND, 0.25)
    # a given scale replaces the tensor's own
    ok, _, _, bound = PR.whole(_kernel((1, 1), 0.5 + 1.0 / 512), REF, YARD, FLOOR, scale=1.0)
    assert ok and bound == 0.5 + 1.0 / 512
    assert not PR.whole(_kernel((1, 1), _next(0.5 + 1.0 / 512)), REF, YARD, FLOOR, scale=1.0)[0]
    # the yardstick passes its own rule, in fp32 and bf16 storage too
    assert PR.whole(YARD, REF, YARD, FLOOR)[0] and PR.whole(YARD.float(), REF, YARD.to(torch.bfloat16), FLOOR)[0]


def test_per_group_passes_at_each_groups_bound_and_fails_one_ulp_above():
    for g, at in enumerate(ZERO_AT):
        ok, ek, bound = PR.per_group(_kernel(at, GROUP_BOUND[g]), REF, YARD, FLOOR)
        assert ok.tolist() == [True, True, True] and bound.tolist() == list(GROUP_BOUND)
        assert ek[g].item() == GROUP_BOUND[g] and ek.sum().item() == GROUP_BOUND[g]
        ok, _, _ = PR.per_group(_kernel(at, _next(GROUP_BOUND[g])), REF, YARD, FLOOR)
        assert ok.tolist() == [i != g for i in range(3)]
    # group 1 has the smallest bound: what the whole tensor allows fails it
    assert PR.whole(_kernel((1, 1), 0.25), REF, YARD, FLOOR)[0] and PR.per_group(_kernel((1, 1), 0.25), REF, YARD, FLOOR)[0].tolist() == [True, False, True]
    # a given scale [G], and trailing dimensions of any shape
    scale = torch.tensor([1.0, 8.0, 0.0], dtype=F64)
    want = [2 * 0.25 + 1.0 / 512, 8.0 / 512, 2 * 0.125]
    shaped = lambda t: t.view(3, 2, 2)
    for g, at in enumerate(ZERO_AT):
        ok, _, bound = PR.per_group(shaped(_kernel(at, want[g])), shaped(REF), shaped(YARD), FLOOR, scale)
        assert ok.all() and bound.tolist() == want
        assert PR.per_group(shaped(_kernel(at, _next(want[g]))), shaped(REF), shaped(YARD), FLOOR, scale)[0].tolist() == [i != g for i in range(3)]
    # one value per group
    ok, ek, bound = PR.per_group(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0], dtype=F64), torch.tensor([1.0, 2.25]), 0.0)
    assert ok.tolist() == [True, True] and ek.tolist() == [0.0, 0.5] and bound.tolist() == [0.0, 0.5]


def test_per_element_passes_at_the_bound_and_fails_one_ulp_above():
    scale = REF.abs().clamp(min=1.0)
    bound = 2.0 * (YARD - REF).abs() + FLOOR * scale
    assert bound[0, 0].item() == 0.5 + 1.0 / 512 and bound[0, 2].item() == 4.0 / 512 and bound[1, 1].item() == 1.0 / 512
    for at in ((0, 1), (1, 1), (2, 0)):
        b = bound[at].item()
        n_bad, first, (ek, ey, share, need) = PR.per_element(_kernel(at, b), REF, YARD, FLOOR, scale)
        assert (n_bad, first) == (0, -1) and ek == b and ey == 0.25 and share == 1.0 and need == FLOOR
        n_bad, first, (_, _, share, need) = PR.per_element(_kernel(at, _next(b)), REF, YARD, FLOOR, scale)
        assert (n_bad, first) == (1, at[0] * 4 + at[1]) and share > 1.0 and need > FLOOR
    # a number as the scale
    assert PR.per_element(_kernel((1, 1), 2.0 / 512), REF, YARD, FLOOR, 2.0)[0] == 0
    assert PR.per_element(_kernel((1, 1), _next(2.0 / 512)), REF, YARD, FLOOR, 2.0)[0] == 1


def test_per_element_where_the_reference_is_not_finite():
    ref = torch.tensor([INF, -INF, NAN, 1.0], dtype=F64)
    yard = torch.tensor([INF, -INF, NAN, INF])                     # (a yardstick that left the finite range widens nothing)
    k = lambda last: torch.tensor([INF, -INF, NAN, last], dtype=F64)
    assert PR.per_element(k(1.0), ref, yard, FLOOR, 1.0)[0] == 0
    assert PR.per_element(k(1.0 + FLOOR), ref, yard, FLOOR, 1.0)[0] == 0
    assert PR.per_element(k(_next(1.0 + FLOOR)), ref, yard, FLOOR, 1.0)[:2] == (1, 3)
    for i, wrong in ((0, 3e38), (0, -INF), (0, NAN), (1, INF), (2, 0.0), (2, INF)):
        bad = k(1.0)
        bad[i] = wrong
        assert PR.per_element(bad, ref, yard, FLOOR, 1.0)[:2] == (1, i), (i, wrong)


def test_a_nan_fails_the_whole_tensor_and_its_own_group_only():
    k = _kernel((2, 3), NAN)
    ok, ek, _, _ = PR.whole(k, REF, YARD, FLOOR)
    assert not ok and math.isnan(ek)
    ok, ek, bound = PR.per_group(k, REF, YARD, FLOOR)
    assert ok.tolist() == [True, True, False] and ek[:2].tolist() == [0.0, 0.0] and math.isnan(ek[2].item())
    assert PR.share(ek, bound) == INF
    n_bad, first, (ek, _, share, need) = PR.per_element(k, REF, YARD, FLOOR, 1.0)
    assert (n_bad, first) == (1, 11) and ek == INF and share == INF and need == INF
    # a NaN yardstick fails too: nothing is compared with an undefined bound
    assert not PR.whole(REF, REF, _kernel((0, 0), NAN), FLOOR)[0]
    assert PR.per_group(REF, REF, _kernel((0, 0), NAN), FLOOR)[0].tolist() == [False, True, True]


def test_groups_outside_rows_pass_with_zeros():
    k = _kernel((2, 3), NAN)
    k[0, 1] = 100.0
    rows = torch.tensor([False, True, False])
    ok, ek, bound = PR.per_group(k, REF, YARD, FLOOR, rows=rows)
    assert ok.all() and ek.tolist() == [0.0, 0.0, 0.0] and bound.tolist() == [0.0, GROUP_BOUND[1], 0.0]
    ok, ek, _ = PR.per_group(k, REF, YARD, FLOOR, rows=~rows)
    assert ok.tolist() == [False, True, False] and ek[0].item() == 100.0 and ek[1].item() == 0.0 and math.isnan(ek[2].item())


def test_an_empty_tensor_passes():
    e = torch.zeros((0, 4))
    assert PR.whole(e, e.double(), e, FLOOR) == (True, 0.0, 0.0, 0.0)
    ok, ek, bound = PR.per_group(e, e.double(), e, FLOOR)
    assert ok.shape == ek.shape == bound.shape == (0,)
    assert PR.per_element(e, e.double(), e, FLOOR, 1.0) == (0, -1, (0.0, 0.0, 0.0, 0.0))
    assert PR.share(ek, bound) == 0.0 and PR.need_floor(ek, ek, ek) == 0.0


def test_share_and_its_four_special_values():
    t = lambda *v: torch.tensor(v, dtype=F64)
    assert PR.share(t(0.25, 1.0), t(1.0, 2.0)) == 0.5
    assert PR.share(t(0.25, 1e-300), t(1.0, 0.0)) == INF            # a bound of 0 exceeded
    assert PR.share(t(0.25, NAN), t(1.0, 2.0)) == INF               # a NaN error ...
    assert PR.share(t(0.25, NAN), t(1.0, 0.0)) == INF               # ... over any bound
    assert PR.share(t(0.0, 0.0), t(0.0, 0.0)) == 0.0                # both 0
    assert PR.share(t(), t()) == 0.0                                # empty
    assert (PR.whole_share(0.25, 0.5), PR.whole_share(1e-300, 0.0), PR.whole_share(NAN, 1.0), PR.whole_share(0.0, 0.0)) == (0.5, INF, INF, 0.0)


def test_need_floor():
    t = lambda *v: torch.tensor(v, dtype=F64)
    # (ek - 2 ey) / scale: (1 - 0.5) / 4 = 0.125 and (3 - 2) / 2 = 0.5; never below 0
    assert PR.need_floor(t(1.0, 3.0), t(0.25, 1.0), t(4.0, 2.0)) == 0.5
    assert PR.need_floor(t(1.0), t(1.0), t(4.0)) == 0.0
    assert PR.need_floor(t(1.0, 0.0), t(0.25, 0.0), t(0.0, 0.0)) == INF     # a scale of 0 cannot pay for anything
    assert PR.need_floor(t(0.5, 0.0), t(0.25, 0.0), t(0.0, 0.0)) == 0.0
    assert PR.need_floor(t(NAN, 0.0), t(0.25, 0.0), t(1.0, 1.0)) == INF


def test_the_sum_bound_by_hand():
    ref, yard = torch.tensor([10.0, -3.0], dtype=F64), torch.tensor([10.5, -3.0])
    abs_terms, pre, depth = torch.tensor([3.0, 0.0], dtype=F64), torch.tensor([1.0, -2.0]), 4
    # 2 * 0.5 + 4 * 2^-24 * (3 + 1) = 1 + 2^-20;  0 + 4 * 2^-24 * (0 + 2) = 2^-21
    want = [1.0 + 2.0 ** -20, 2.0 ** -21]
    assert PR.sum_bound(abs_terms, depth, pre, yard, ref).tolist() == want
    # without a pre-fill: 1 + 4 * 2^-24 * 3 = 1 + 3 * 2^-22;  0
    assert PR.sum_bound(abs_terms, depth, None, yard, ref).tolist() == [1.0 + 3 * 2.0 ** -22, 0.0]
    # without a yardstick, and with another unit
    assert PR.sum_bound(abs_terms, depth, pre).tolist() == [2.0 ** -20, 2.0 ** -21]
    assert PR.sum_bound(abs_terms, depth, pre, unit=2.0 ** -23).tolist() == [2.0 ** -19, 2.0 ** -20]
    # an accumulation is compared with pre-fill + reference
    at = torch.tensor([1.0 + 10.0 + want[0], -2.0 - 3.0 - want[1]], dtype=F64)
    ok, err, bound = PR.accept_sum(at, pre, ref, yard, abs_terms, depth)
    assert ok.tolist() == [True, True] and err.tolist() == want and bound.tolist() == want
    above = torch.tensor([_next(11.0 + want[0]), -5.0], dtype=F64)
    assert PR.accept_sum(above, pre, ref, yard, abs_terms, depth)[0].tolist() == [False, True]
    assert PR.accept_sum(ref, pre, ref, yard, abs_terms, depth)[0].tolist() == [True, False]        # overwritten, not added: only where the bound is wider than the pre-fill
    assert PR.accept_sum(torch.tensor([NAN, -5.0]), pre, ref, yard, abs_terms, depth)[0].tolist() == [False, True]


def test_the_statistic_its_line_and_its_merge():
    assert (PR.ratio(1.0, 4.0), PR.ratio(1.0, 0.0), PR.ratio(0.0, 0.0), PR.ratio(0.0, 0.0, INF)) == (0.25, INF, 0.0, INF)
    assert PR.fmt_stat("dx", (1.5e-7, 3e-7, 0.25, 2.0 ** -20)) == "dx 1.50e-07 3.00e-07 0.50 0.25 9.5e-07"
    assert PR.fmt_stat("y", (0.0, 0.0, 0.0, 0.0)) == "y 0.00e+00 0.00e+00 0.00 0.00 0.0e+00"
    assert PR.fmt_stat("y", (1.0, 0.0, INF, INF)) == "y 1.00e+00 0.00e+00 inf inf inf"
    total = {}
    PR.merge_stat(total, "p", (1.0, 5.0, 0.1, 0.0))
    PR.merge_stat(total, "p", (2.0, 3.0, 0.3, 1e-6))
    PR.merge_stat(total, "m", (0.5, 0.5, 0.5, 0.5))
    assert total == {"p": (2.0, 5.0, 0.3, 1e-6), "m": (0.5, 0.5, 0.5, 0.5)}


@pytest.mark.parametrize("dtype,bits", [(torch.bfloat16, torch.int16), (torch.float16, torch.int16), (torch.float32, torch.int32), (torch.float64, torch.int64)])
def test_same_bits(dtype, bits):
    a = torch.tensor([0.0, 1.5, -2.0], dtype=dtype)
    assert PR.same_bits(a, a.clone()) and a[0] == -a[0]
    b = a.clone()
    b[0] = -0.0
    assert not PR.same_bits(a, b), "+0 and -0"
    n = torch.tensor([NAN, 1.0], dtype=dtype)
    assert PR.same_bits(n, n.clone()), "a NaN of the same payload"
    other = n.clone()
    other.view(bits)[0] ^= 1                                       # still a NaN, another payload
    assert bool(torch.isnan(other[0])) and not PR.same_bits(n, other)
    assert not PR.same_bits(a, a[:2]) and not PR.same_bits(a, a.double() if dtype != F64 else a.float())
    assert PR.same_bits(a.view(3, 1).expand(3, 2), a.view(3, 1).repeat(1, 2)), "a view that is not contiguous"
    i = torch.tensor([1, -2, 3])
    assert PR.same_bits(i, i.clone()) and not PR.same_bits(i, i + 1)


def test_rbf_rounds_ties_to_even_and_keeps_the_dtype():
    # bf16 has 7 fraction bits: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 * 2^-8 halfway between
    # 1 + 2^-7 (odd) and 1 + 2^-6 (even)
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8, 0.3])
    want = [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.30078125]
    for dt in (torch.float32, F64):
        r = PR.rbf(x.to(dt))
        assert r.dtype == dt and r.tolist() == want
    assert PR.same_bits(PR.rbf(x.to(torch.bfloat16)), x.to(torch.bfloat16))


def test_gen_hashes_its_key_as_documented():
    assert PR.gen(5).initial_seed() == 5
    assert PR.gen(1, 2).initial_seed() == 1000005
    assert PR.gen("ab").initial_seed() == 97 + 2 * 98
    assert PR.gen(True, start=12345).initial_seed() == 1607618801 == (12345 * 1000003 + 1) % (2 ** 31 - 1)
    assert PR.gen(7, "x", False).initial_seed() == PR.gen(7, "x", 0).initial_seed() != PR.gen(7, "x", 1).initial_seed()
    a, b = torch.rand(4, generator=PR.gen("gae", 3)), torch.rand(4, generator=PR.gen("gae", 3))
    assert torch.equal(a, b) and PR.gen(1).device.type == "cpu"
