"""GPU: the masked-categorical kernels of csrc/catan_nn.hip (k_categorical_fwd / _bwd, k_categorical_bits_fwd / _bwd) row by row against
fp64, through the C ABI (catan_categorical_fwd / _bwd, catan_categorical_bits_fwd / _bwd).

reference = tests/categorical_reference.py (its docstring has the formulas, the rule and the launch table; `judge` is the verdict on one
launch, computed from reference and yardstick alone):
    logp, entropy, lse   per row |kernel - fp64| <= 2 |yardstick - fp64| + 2^-17 max(1, largest legal |logp_all| of the row), and over the case
    dlogits              floor 2^-15; over the case with its largest reference magnitude, per row with max(the row's, |dlogp| + |dent|)
    exact                one legal column: logp = entropy = 0, lse = the logit, dlogits = 0; an illegal given action: -inf; a row without a
                         legal column: NaN logp, lse = -inf (max -inf plus log 0, in the kernel and in the reference alike), entropy 0, a zero
                         gradient row; an illegal column's gradient is 0
    action               given: the given one clamped into [0, K - 1]; arg-max: the reference's lowest-index maximum on every row; sampled:
                         the cdf bracket rule of tests/test_gpu_heads_fp64.py on every row, u = 0 and u = the largest float below 1 planted
                         (only the latter may also give the last legal column)
Regimes, action modes, row counts, K, the two mask pitches, the bits form's segments: categorical_reference's tables.  The backward is
launched on what the forward returned (action, lse, entropy), as nn_kernels does.  The bits form is held to fp64 in the same way on the
mask that a plain unpack of its words gives, and bit for bit to the float kernel on that mask.

Buffers: every float input lies in front of NaN, the float mask in front of (and, as a window of the [rows][325] matrix, between) ones
- a read past a mask row would make an illegal column legal; NaN would only make it illegal again -, the packed rows in front of words
of all ones; every output starts as a sentinel pattern, none of which may be left, in front of guard elements that must be intact.
Every case prints one `CAT` line: per output the kernel's error, the yardstick's error, their ratio, the largest share of a bound
used and the floor its rows would need, the largest over the case's action modes: profiles/categorical_kernel_tests.txt is that output."""
import ctypes as C

import pytest
import torch

import categorical_reference as CR
import guarded as G
from guarded import NAN, ptr as P, stream as _stream
from pin_rule import merge_stat, same_bits

pytestmark = pytest.mark.gpu

GUARD = 512                      # elements behind every buffer
SENTINEL = 0x5A5B5A5B
OUTS = ("action", "logp", "entropy", "lse", "dlogits")


def _check(rc):
    from settlers_of_catan_rl_amd import _lib
    _lib.check(rc)


def _input(t, guard):
    """-> (whole, view): t's elements followed by GUARD elements of `guard`"""
    return G.guarded_input(t, GUARD, guard=guard)


def _output(n, dtype):
    return G.sentinel_output(n, dtype, GUARD, sentinel=SENTINEL)


def _written_and_guarded(whole, view):
    return G.intact(whole, view) and G.written(whole, view, SENTINEL)


def _device(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _finish(name, B, K, outs, bwd):
    torch.cuda.synchronize()
    got = {}
    for n, (whole, view) in outs.items():
        assert _written_and_guarded(whole, view), (name, n, "an element left unwritten, or a write behind the output")
        got[n] = view.clone().view(B, K) if n == "dlogits" else view.clone()
    return got


def _launch(lib, c, mode, window, bwd=True):
    """catan_categorical_fwd (and _bwd on what it returned) on a device case -> {action, logp, entropy, lse[, dlogits]}"""
    B, K = c["B"], c["K"]
    hold = [_input(c["logits"], NAN)]
    if window:
        off = CR.window_off(K)
        full = torch.ones((B + 2, CR.MASK_LD), dtype=torch.float32, device="cuda")
        full[:B, off:off + K] = c["mask"]
        mask_p, ld = P(full, 4 * off), CR.MASK_LD
    else:
        hold.append(_input(c["mask"], 1.0))
        mask_p, ld = P(hold[-1][1]), K
    given = u = None
    if mode.startswith("given"):
        hold.append(_input(c[mode], K + 7))
        given = hold[-1][1]
    elif mode == "sampled":
        hold.append(_input(c["u"], NAN))
        u = hold[-1][1]
    outs = {"action": _output(B, torch.int64), "logp": _output(B, torch.float32), "entropy": _output(B, torch.float32), "lse": _output(B, torch.float32)}
    _check(lib.catan_categorical_fwd(P(hold[0][1]), mask_p, ld, P(given), P(u), P(outs["action"][1]), P(outs["logp"][1]), P(outs["entropy"][1]),
                                     P(outs["lse"][1]), B, K, _stream()))
    if bwd:
        hold += [_input(c["dlogp"], NAN), _input(c["dent"], NAN)]
        outs["dlogits"] = _output(B * K, torch.float32)
        _check(lib.catan_categorical_bwd(P(hold[0][1]), mask_p, ld, P(outs["action"][1]), P(outs["lse"][1]), P(outs["entropy"][1]), P(hold[-2][1]),
                                         P(hold[-1][1]), P(outs["dlogits"][1]), B, K, _stream()))
    return _finish((c["regime"], B, K, mode, window), B, K, outs, bwd)


def _launch_bits(lib, c, mode):
    """catan_categorical_bits_fwd / _bwd on a device bits case (mode: a given_* one, or argmax = no given pointer)"""
    B, K, ld = c["B"], c["K"], c["given_ld"]
    hold = [_input(c["logits"], NAN), _input(c["packed"], -1)]
    idx = None
    if c["rows_idx"] is not None:
        hold.append(_input(c["rows_idx"], 0))
        idx = hold[-1][1]
    segs = (C.c_int32 * 8)(*c["segs"])
    given_p = None
    if mode.startswith("given"):
        col = 3 % ld
        mat = torch.full((B + 2, ld), K + 7, dtype=torch.int64, device="cuda")               # (a column of an action matrix)
        mat[:B, col] = c[mode]
        given_p = P(mat, 8 * col)
    outs = {"action": _output(B, torch.int64), "logp": _output(B, torch.float32), "entropy": _output(B, torch.float32), "lse": _output(B, torch.float32)}
    _check(lib.catan_categorical_bits_fwd(P(hold[0][1]), P(hold[1][1]), CR.PITCH, P(idx), segs, given_p, ld, P(outs["action"][1]), P(outs["logp"][1]),
                                          P(outs["entropy"][1]), P(outs["lse"][1]), B, K, _stream()))
    hold += [_input(c["dlogp"], NAN), _input(c["dent"], NAN)]
    outs["dlogits"] = _output(B * K, torch.float32)
    _check(lib.catan_categorical_bits_bwd(P(hold[0][1]), P(hold[1][1]), CR.PITCH, P(idx), segs, P(outs["action"][1]), P(outs["lse"][1]), P(outs["entropy"][1]),
                                          P(hold[-2][1]), P(hold[-1][1]), P(outs["dlogits"][1]), B, K, _stream()))
    return _finish((c["regime"], B, K, mode, "bits"), B, K, outs, True)


def _merge(total, stats):
    for n, v in stats.items():
        if n == "tau":
            total[n] = max(total.get(n, 0.0), v)
        else:
            merge_stat(total, n, v)


def float_cases(K):
    """-> [(regime, B, window)] of one K: every regime at every row count; both mask pitches in the unit regime and at 257 rows, elsewhere
    the pitch goes round with the case"""
    out = []
    for i, regime in enumerate(CR.REGIMES):
        for j, B in enumerate(CR.ROWS):
            for window in ((False, True) if regime == "unit" or B == 257 else (bool((i + j) % 2),)):
                out.append((regime, B, window))
    return out


def bits_modes(t):
    """the action modes of the t-th bits case: given legal and arg-max always, the illegal and the out-of-range given turn about"""
    return ("given_legal", "argmax", ("given_illegal", "given_oor")[t % 2])


def test_cases_cover_every_path():
    """the case tables reach all five action modes, both mask pitches, every segment layout with and without a row list"""
    for K in CR.KS:
        cases = float_cases(K)
        assert {(r, B) for r, B, _ in cases} == {(r, B) for r in CR.REGIMES for B in CR.ROWS}
        assert {(B, w) for _, B, w in cases} == {(B, w) for B in CR.ROWS for w in (False, True)}
        assert {w for r, _, w in cases if r != "unit"} == {False, True}
        bc = CR.bits_cases(K)
        assert {(nn, wi) for B, nn, wi, _, _ in bc if B == 4097} == {(nn, wi) for nn in CR.seg_layouts(4097) for wi in (False, True)}
        assert {(nn, wi) for B, nn, wi, _, _ in bc if B == 257} == {(nn, wi) for nn in CR.seg_layouts(257) for wi in (False, True)}
        assert {B for B, *_ in bc} == set(CR.ROWS) and {ld for *_, ld, _ in bc} == set(CR.GIVEN_LDS)
        assert {m for t in range(len(bc)) for m in bits_modes(t)} == set(CR.MODES) - {"sampled"}
    assert set(CR.MODES) == {"given_legal", "given_illegal", "given_oor", "argmax", "sampled"}
    assert set(CR.seg_layouts(4097)) == {(0, 0), (0, 4097), (4097, 4097), (255, 257), (256, 256), (1, 4096)}
    assert any(a >= 0 for K in CR.KS for _, a in CR.BITS_SEGS[K]) and all(CR.BITS_SEGS[K][2][0] + K == 32 * CR.PITCH for K in CR.KS)
    assert {r for K in CR.KS for *_, r in CR.bits_cases(K)} == set(CR.BITS_REGIMES)


@pytest.mark.parametrize("K", CR.KS)
def test_categorical_kernel_vs_fp64(hip_lib, K):
    """catan_categorical_fwd / _bwd at one K: every regime, row count and action mode.  See the module docstring for what is asserted.

    Measured on the MI355X: profiles/categorical_kernel_tests.txt."""
    bad = []
    for regime, B, window in float_cases(K):
        c = _device(CR.make_case(regime, B, K))
        total = {}
        for mode in CR.MODES:
            got = _launch(hip_lib, c, mode, window)
            b, stats = CR.judge(c, mode, got)
            bad += [(regime, B, K, window, mode) + x for x in b]
            _merge(total, stats)
        print(f"CAT float K={K} B={B} {regime} ld={CR.MASK_LD if window else K}: " + CR.stats_line(total))
    assert not bad, bad[:12]


@pytest.mark.parametrize("K", CR.KS)
def test_categorical_bits_kernel_vs_fp64(hip_lib, K):
    """catan_categorical_bits_fwd / _bwd at one K: every segment layout with and without a row list, against fp64 on the mask a plain
    unpack gives, and bit for bit against catan_categorical_fwd / _bwd on that mask.

    Measured on the MI355X: profiles/categorical_kernel_tests.txt."""
    bad = []
    for t, (B, n0n1, with_idx, given_ld, regime) in enumerate(CR.bits_cases(K)):
        c = _device(CR.make_bits_case(regime, B, K, n0n1, with_idx, given_ld))
        total = {}
        for mode in bits_modes(t):
            got = _launch_bits(hip_lib, c, mode)
            b, stats = CR.judge(c, mode, got)
            bad += [(regime, B, K, n0n1, with_idx, given_ld, mode) + x for x in b]
            _merge(total, stats)
            flt = _launch(hip_lib, c, mode, False)
            for n in OUTS:
                assert same_bits(got[n], flt[n]), (regime, B, K, n0n1, with_idx, mode, n, "the bits form and the float form differ")
        print(f"CAT bits K={K} B={B} {regime} segs={n0n1} idx={int(with_idx)} given_ld={given_ld}: " + CR.stats_line(total))
    assert not bad, bad[:12]


def _rows_of(c, lo, hi):
    out = {k: (v[lo:hi].contiguous() if isinstance(v, torch.Tensor) and v.shape[0] == c["B"] else v) for k, v in c.items()}
    out["B"] = hi - lo
    return out


@pytest.mark.parametrize("K", CR.KS)
def test_rows_do_not_depend_on_the_grid(hip_lib, K):
    """a row's outputs are the same bits when it is launched alone, inside 257 rows and inside 4097"""
    c = _device(CR.make_case("unit", 4097, K))
    for mode in ("given_legal", "argmax", "sampled"):
        big = _launch(hip_lib, c, mode, True)
        mid = _launch(hip_lib, _rows_of(c, 0, 257), mode, False)
        for n in OUTS:
            assert same_bits(big[n][:257], mid[n]), (K, mode, n, "the first 257 rows depend on the grid")
        for r in (0, 255, 256):
            one = _launch(hip_lib, _rows_of(c, r, r + 1), mode, True)
            for n in OUTS:
                assert same_bits(one[n], mid[n][r:r + 1]), (K, mode, n, r, "a row alone differs from the row in a launch")


def test_abi_refusals_launch_nothing(hip_lib):
    """mask_ld < K, a bit range (or an AND range) past the packed row, n1 < n0: an error code, and every output still the sentinel"""
    B, K = 5, 13
    c = _device(CR.make_bits_case("unit", B, K, (0, 0), False, 1))
    z, m, pk, g = _input(c["logits"], NAN)[1], _input(c["mask"], 1.0)[1], _input(c["packed"], -1)[1], _input(c["given_legal"], 0)[1]
    w = _input(c["dlogp"], NAN)[1]
    outs = {"action": _output(B, torch.int64), "logp": _output(B, torch.float32), "entropy": _output(B, torch.float32), "lse": _output(B, torch.float32),
            "dlogits": _output(B * K, torch.float32)}
    o = {n: P(v[1]) for n, v in outs.items()}
    lse, ent = _input(torch.zeros(B), NAN)[1], _input(torch.zeros(B), NAN)[1]
    assert hip_lib.catan_categorical_fwd(P(z), P(m), K - 1, P(g), None, o["action"], o["logp"], o["entropy"], o["lse"], B, K, _stream()) != 0
    assert hip_lib.catan_categorical_bwd(P(z), P(m), K - 1, P(g), P(lse), P(ent), P(w), P(w), o["dlogits"], B, K, _stream()) != 0
    full = 32 * CR.PITCH
    for segs in ([0, 0, full - K + 1, -1, 0, -1, 0, -1], [0, 0, 0, -1, 0, full - K + 1, 0, -1], [0, 0, 0, -1, 0, -1, full - K + 1, -1],
                 [3, 2, 0, -1, 0, -1, 0, -1], [0, 0, -1, -1, 0, -1, 0, -1]):
        s = (C.c_int32 * 8)(*segs)
        assert hip_lib.catan_categorical_bits_fwd(P(z), P(pk), CR.PITCH, None, s, P(g), 1, o["action"], o["logp"], o["entropy"], o["lse"], B, K, _stream()) != 0, segs
        assert hip_lib.catan_categorical_bits_bwd(P(z), P(pk), CR.PITCH, None, s, P(g), P(lse), P(ent), P(w), P(w), o["dlogits"], B, K, _stream()) != 0, segs
    torch.cuda.synchronize()
    for n, (whole, view) in outs.items():
        assert bool((whole.view(torch.int32) == SENTINEL).all()), (n, "a refused call wrote")
    # the same calls with the last legal arguments are accepted
    s = (C.c_int32 * 8)(0, 0, full - K, -1, 0, full - K, 0, -1)
    _check(hip_lib.catan_categorical_bits_fwd(P(z), P(pk), CR.PITCH, None, s, P(g), 1, o["action"], o["logp"], o["entropy"], o["lse"], B, K, _stream()))
    _check(hip_lib.catan_categorical_fwd(P(z), P(m), K, P(g), None, o["action"], o["logp"], o["entropy"], o["lse"], B, K, _stream()))
    torch.cuda.synchronize()
