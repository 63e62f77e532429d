"""The acceptance rule of the kernel pin suites (tests/test_gpu_*_fp64.py, tests/test_gpu_te_backward.py and the CPU tests of their
reference modules), stated once.  Torch only: no import of the library, of nn_kernels or of another test module; every function takes CPU
or GPU tensors.

A suite has a REFERENCE (the operation in fp64 from the inputs as stored) and a YARDSTICK (the same formulas in fp32, rounded to bf16
exactly where the kernel rounds: what the number formats alone cost against the reference; it is not an oracle).  A kernel output passes when

    |kernel - ref| <= 2 |yardstick - ref| + floor * scale

taken as maxima over a whole tensor (`whole`), over every group of the leading index with the group's own yardstick error and scale
(`per_group`: a row, a sequence, a list), or element by element (`per_element`).  Nothing in a bound comes from the kernel.
  The factor 2 covers a different fp32 summation order (inside an MFMA, across lanes, in atomics), which can turn a rounding at the
  storage precision the other way: the kernel may then be off by the yardstick's error once more, in the other direction.
  The floor is for the cases where the yardstick happens to land exact and the first term vanishes: a share of the output's scale, half
  a bf16 ulp (BF16_FLOOR = 2^-9) where the output is stored as bf16; the fp32 floors are properties of each kernel's arithmetic and live
  in the suites' reference modules.  `scale` is the largest reference magnitude of the tensor or group unless the suite gives its own.
  No element is excluded, and a NaN fails: every comparison is written so that it is false for one.

An accumulated sum (dw, db, dparams: one word that many rows add into, in any order) passes per word when (`sum_bound`, `accept_sum`)

    |kernel - (pre-fill + ref)| <= 2 |yardstick - ref| + depth * 2^-24 * (sum |term| + |pre-fill|)

the any-order bound of a chain of `depth` fp32 additions; the value the accumulator held before is one more addend of that chain.

The figures the suites print come from here too: `share` (the largest part of a bound that was used), `need_floor` (the smallest floor
under which everything would still pass), and the statistic (kernel error, yardstick error, share, needed floor) that `fmt_stat` prints
with the ratio of the two errors and `merge_stat` folds over cases."""
import torch

BF16_FLOOR = 2.0 ** -9
UNIT = 2.0 ** -24                                        # fp32's half-ulp relative to the top of its binade
INF = float("inf")


def _err(t, ref):
    return (t.double() - ref.double()).abs()


def _groups(t):
    """[G, ...] -> [G, n]"""
    return t.flatten(1) if t.dim() > 1 else t.unsqueeze(1)


def group_error(t, ref):
    """[G] fp64: the largest |t - ref| of every group; a NaN in a group makes it NaN (amax propagates it)"""
    return _groups(_err(t, ref)).amax(1)


def group_scale(ref):
    """[G] fp64: the largest reference magnitude of every group"""
    return _groups(ref.double().abs()).amax(1)


# ---------------------------------------------------------------------------------------------------------------------------- rule
def whole_bound(ref, yardstick, floor, scale=None):
    """what `whole` allows a kernel on this tensor, from the reference and the yardstick alone -> (bound, yardstick error)"""
    ey = float(_err(yardstick, ref).max())
    return 2.0 * ey + floor * (float(ref.double().abs().max()) if scale is None else scale), ey


def whole(kernel, ref, yardstick, floor, scale=None):
    """The rule over one tensor -> (ok, kernel error, yardstick error, bound).  scale: the tensor's own largest reference magnitude, or
    the number given.  An empty tensor passes with zeros; a NaN anywhere fails."""
    if ref.numel() == 0:
        return True, 0.0, 0.0, 0.0
    ek = float(_err(kernel, ref).max())
    bound, ey = whole_bound(ref, yardstick, floor, scale)
    return ek <= bound, ek, ey, bound


def per_group(kernel, ref, yardstick, floor, scale=None, rows=None):
    """The rule for every group of the leading index (the trailing dimensions flattened) with ITS yardstick error and ITS scale
    -> (ok [G] bool, kernel error [G], bound [G]).  scale [G]: given instead of the group's largest reference magnitude.  rows [G]
    bool: the groups that are asked about; the others pass with error 0 and bound 0.  A NaN in an asked group fails that group."""
    ek = group_error(kernel, ref)
    bound = 2.0 * group_error(yardstick, ref) + floor * (group_scale(ref) if scale is None else scale.double())
    ok = ek <= bound
    if rows is not None:
        ok = ok | ~rows
        ek, bound = torch.where(rows, ek, torch.zeros_like(ek)), torch.where(rows, bound, torch.zeros_like(bound))
    return ok, ek, bound


def per_element(kernel, ref, yard, floor, scale):
    """The rule for every element -> (number of failures, index of the first or -1, (kernel error, yardstick error, largest share of a
    bound used, the smallest floor under which every element would pass)).  `scale`: a tensor like ref, or a number.  Where the
    reference is not finite the kernel must return that value (inf as inf, NaN as NaN), and a yardstick that left the finite range
    widens nothing."""
    ref = ref.double().reshape(-1)
    k, y = kernel.double().reshape(-1), yard.double().reshape(-1)
    scale = (scale.double().reshape(-1) if isinstance(scale, torch.Tensor) else torch.full_like(ref, float(scale)))
    if ref.numel() == 0:
        return 0, -1, (0.0, 0.0, 0.0, 0.0)
    fin = torch.isfinite(ref)
    zero = torch.zeros_like(ref)
    ek = torch.where(fin, (k - ref).abs(), zero)
    ey = torch.where(fin, (y - ref).abs(), zero)
    ey = torch.where(torch.isfinite(ey), ey, zero)
    bound = 2.0 * ey + floor * scale
    same = (k == ref) | (torch.isnan(k) & torch.isnan(ref))
    ok = torch.where(fin, ek <= bound, same)                               # NaN where the reference is finite: the comparison is false
    n_bad = int((~ok).sum())
    first = int((~ok).nonzero()[0]) if n_bad else -1
    return n_bad, first, (float(_nan_to_inf(ek).max()), float(ey.max()), share(ek, bound), need_floor(ek, ey, scale))


def sum_bound(abs_terms, depth, prefill=None, yardstick=None, ref=None, unit=UNIT):
    """[n] fp64, for one vector (or matrix) of accumulated words: 2 |yardstick - ref| + depth * unit * (abs_terms + |pre-fill|).
    abs_terms = sum |term| per word.  Without a pre-fill the accumulator started at 0; without a yardstick the summation term
    stands alone (a suite whose yardstick of the terms is exact)."""
    chain = depth * unit * (abs_terms.double() if prefill is None else abs_terms.double() + prefill.double().abs())
    return chain if yardstick is None else 2.0 * _err(yardstick, ref) + chain


def accept_sum(kernel, prefill, ref, yardstick, abs_terms, depth, unit=UNIT):
    """an accumulation that ADDED to `prefill` -> (ok [n], error [n], bound [n]); a NaN fails"""
    err = (kernel.double() - (prefill.double() + ref.double())).abs()
    bound = sum_bound(abs_terms, depth, prefill, yardstick, ref, unit)
    return err <= bound, err, bound


# ------------------------------------------------------------------------------------------------------------------------- figures
def _nan_to_inf(t):
    return torch.where(torch.isnan(t), torch.full_like(t, INF), t)


def share(err, bound):
    """the largest err / bound: inf where a bound of 0 is exceeded or the error is NaN, 0 where both are 0, 0 for an empty tensor"""
    if err.numel() == 0:
        return 0.0
    inf = torch.full_like(err, INF)
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), inf))
    return float(_nan_to_inf(r).max())


def whole_share(ek, bound):
    """`share` for the two numbers that `whole` returns"""
    if ek != ek:
        return INF
    return ek / bound if bound > 0 else (INF if ek > 0 else 0.0)


def need_floor(ek, ey, scale):
    """the smallest floor under which everything would still pass: the largest (ek - 2 ey) / scale, 0 where nothing needs one, inf
    where a scale of 0 is exceeded or the error is NaN"""
    if ek.numel() == 0:
        return 0.0
    ek = _nan_to_inf(ek)
    n = torch.where(scale > 0, (ek - 2.0 * ey) / scale, torch.where(ek > 2.0 * ey, torch.full_like(ek, INF), torch.zeros_like(ek)))
    return max(0.0, float(n.max()))


def ratio(ek, ey, both_zero=0.0):
    """kernel error / yardstick error; inf over a yardstick error of 0, `both_zero` where both are 0"""
    return ek / ey if ey > 0 else (INF if ek > 0 else both_zero)


def fmt_stat(name, s):
    """one output of a printed line: kernel error, yardstick error, their ratio, largest share of a bound, the floor needed"""
    ek, ey, sh, need = s
    return f"{name} {ek:.2e} {ey:.2e} {ratio(ek, ey):.2f} {sh:.2f} {need:.1e}"


def merge_stat(total, name, s):
    """total[name] = the element-wise maximum of what it held and s"""
    t = total.get(name, (0.0, 0.0, 0.0, 0.0))
    total[name] = tuple(max(a, b) for a, b in zip(t, s))


# --------------------------------------------------------------------------------------------------------------------------- tools
def rbf(t):
    """round to bf16 and back to t's dtype (fp64 passes through fp32 first)"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def gen(*key, start=0, device="cpu"):
    """a torch.Generator on `device` seeded from the key: s = start, then s = (s * 1000003 + k) mod (2^31 - 1) for every k; a string
    counts as sum (i + 1) ord(ch_i), a bool as 0 / 1"""
    s = start
    for k in key:
        s = (s * 1000003 + (int(k) if isinstance(k, int) else sum(ord(ch) * (i + 1) for i, ch in enumerate(str(k))))) % (2 ** 31 - 1)
    return torch.Generator(device=device).manual_seed(s)


_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def same_bits(a, b):
    """the same shape and the same bits in every element (+0 is not -0; a NaN equals a NaN of the same payload)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        a, b = a.view(_INT[a.element_size()]), b.view(_INT[b.element_size()])
    return torch.equal(a, b)
