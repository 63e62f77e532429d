"""GPU: the LSTM-cell kernels of csrc/catan_nn.hip (k_lstm_cell_fwd<T> / k_lstm_cell_bwd<T>, T = float and bfloat16) row by row against
fp64, through the C ABI (catan_lstm_cell_fwd / catan_lstm_cell_bwd).

reference = tests/lstm_cell_reference.py (its docstring has the formulas, the yardstick's roundings, the rule and the launch table):
    h, c, dc_prev, fp32 dgates   maxabs(kernel - fp64) <= 2 maxabs(yardstick - fp64) + floor maxabs(fp64), floor 2^-17 (h, c) / 2^-15 (gradients),
                                 over the whole case AND for every row with that row's own yardstick error and scale
    bf16 dgates                  the same with floor 2^-9
Nothing in a bound comes from a kernel.  Every case prints one `LSTM` line: per output the kernel's error, the yardstick's error, their
ratio, the largest share of a bound used (by the case or by a single row) and the floor its rows would need:
profiles/lstm_cell_kernel_tests.txt is that output.

Cases (lstm_cell_reference.small_cases / cap_cases): L in 4, 8, 12, 64, 256 x rows in 1, 63, 64, 65, 255, 256, 257 x the regimes unit,
saturated (every output finite), zero (c and h exactly 0: the reference is 0 and so is the bound), masked (the rows with mask 0 carry
c_prev = 1e30: every output equals, bit for bit, the launch with c_prev = 0 there) with and without a mask pointer; and at L = 256 both
sides of the launch cap, 65 536 and 65 537 rows, where fp64 is built for the first and the last 4 096 rows only and those rows are also
compared bit for bit with a 4 096-row launch of their own.

Buffers: 16-byte aligned; every input lies in front of NaN, every output starts as a sentinel pattern, none of which may be left, in
front of guard elements that must be intact."""
import pytest
import torch

import guarded as G
import lstm_cell_reference as LS
from guarded import ptr as P, stream as _stream
from pin_rule import same_bits

pytestmark = pytest.mark.gpu

GUARD = 1024                     # elements behind every buffer
SENTINEL = 0x5A5B5A5B
FWD, BWD = ("h", "c"), ("dgates", "dc_prev")


def _check(rc):
    from settlers_of_catan_rl_amd import _lib
    _lib.check(rc)


def _input(t):
    return G.guarded_input(t, GUARD)


def _output(n, dtype):
    return G.sentinel_output(n, dtype, GUARD, sentinel=SENTINEL)


def _written_and_guarded(whole, view):
    return G.intact(whole, view) and G.written(whole, view, SENTINEL)


def _launch(lib, c, bwd=True):
    """forward, and the backward, on a device case -> {h, c [n, L] fp32; dgates [n, 4 L] of the storage type, dc_prev [n, L]}"""
    n, L = c["n"], c["L"]
    is_bf16 = int(c["gx"].dtype == torch.bfloat16)
    ins = {k: _input(c[k]) for k in ("gx", "gh", "c_prev", "dh", "dc")}
    mask = _input(c["mask"]) if c["mask"] is not None else (None, None)
    outs = {"h": _output(n * L, torch.float32), "c": _output(n * L, torch.float32)}
    _check(lib.catan_lstm_cell_fwd(P(ins["gx"][1]), P(ins["gh"][1]), P(ins["c_prev"][1]), P(mask[1]), P(outs["h"][1]), P(outs["c"][1]), n, L, is_bf16, _stream()))
    if bwd:
        outs["dgates"] = _output(n * 4 * L, c["gx"].dtype)
        outs["dc_prev"] = _output(n * L, torch.float32)
        _check(lib.catan_lstm_cell_bwd(P(ins["gx"][1]), P(ins["gh"][1]), P(ins["c_prev"][1]), P(mask[1]), P(ins["dh"][1]), P(ins["dc"][1]),
                                       P(outs["dgates"][1]), P(outs["dc_prev"][1]), n, L, is_bf16, _stream()))
    torch.cuda.synchronize()
    got = {}
    for k, (whole, view) in outs.items():
        assert _written_and_guarded(whole, view), (c["regime"], n, L, k, "an element left unwritten, or a write behind the output")
        got[k] = view.view(n, -1)
    return got


def _device(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _rows_of(c, lo, hi):
    out = {k: (v[lo:hi].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    out["n"] = hi - lo
    return out


def _args(c):
    return c["gx"], c["gh"], c["c_prev"], c["mask"], c["dh"], c["dc"]


def test_cases_cover_every_path():
    """both storage types, with and without a mask pointer, on both sides of the 16 384-block cap; every regime at every L and row count"""
    caps = LS.cap_cases()
    assert {(dt, LS.launch(n, LS.CAP_L)) for dt, n, _ in caps} == {(dt, g) for dt in LS.DTYPES for g in ((LS.CAP, 1), (LS.CAP, 2))}
    for dt in LS.DTYPES:
        assert {mp for d, _, mp in caps if d == dt} == {False, True}
    small = LS.small_cases()
    assert {(L, n, r) for L, n, r, _ in small} == {(L, n, r) for L in LS.HIDDEN for n in LS.ROWS for r in LS.REGIMES}
    assert {(r, mp) for _, _, r, mp in small if r != "masked"} == {(r, mp) for r in LS.REGIMES if r != "masked" for mp in (False, True)}
    assert all(LS.launch(n, L)[1] == 1 for L, n, _, _ in small) and {LS.launch(n, L)[0] > 1 for L, n, _, _ in small} == {False, True}


@pytest.mark.parametrize("dtype", LS.DTYPES)
@pytest.mark.parametrize("L", LS.HIDDEN)
def test_lstm_cell_kernel_vs_fp64(hip_lib, L, dtype):
    """One width and storage type, forward and backward, at every row count, regime and mask-pointer form of small_cases.  See the module
    docstring for what is asserted.

    Measured on the MI355X: profiles/lstm_cell_kernel_tests.txt."""
    dt = getattr(torch, dtype)
    bf16 = dt == torch.bfloat16
    bad = []
    for _, n, regime, mp in [s for s in LS.small_cases() if s[0] == L]:
        c = _device(LS.make_case(regime, n, L, dt, mp))
        got = _launch(hip_lib, c)
        ref, yard = LS.lstm_ref(*_args(c)), LS.lstm_yardstick(*_args(c))
        b, stats = LS.judge(bf16, got, ref, yard)
        name = f"L={L} {'bf16' if bf16 else 'fp32'} rows={n} {regime} mask={int(mp)}"
        bad += [(name,) + x for x in b]
        print(f"LSTM {name}: " + LS.stats_line(stats))
        assert got["dgates"].dtype == dt
        if regime == "zero":
            assert not bool(got["h"].any()) and not bool(got["c"].any()), (name, "c and h are not exactly 0")
        if regime == "masked":
            c0 = dict(c, c_prev=torch.where(c["masked_rows"][:, None], torch.zeros_like(c["c_prev"]), c["c_prev"]))
            got0 = _launch(hip_lib, c0)
            for k in FWD + BWD:
                assert same_bits(got[k], got0[k]), (name, k, "a masked row's c_prev = 1e30 shows")
            assert not bool(got["dc_prev"][c["masked_rows"]].any()), (name, "dc_prev of a masked row is not 0")
    assert not bad, bad[:12]


@pytest.mark.parametrize("dtype", LS.DTYPES)
@pytest.mark.parametrize("L", [4, 12, 256])
def test_rows_do_not_depend_on_the_grid(hip_lib, L, dtype):
    """a row's outputs are the same bits when it is launched alone, inside 257 rows and inside 4 099.  The largest cases, 65 536 and
    65 537 rows, are held in test_lstm_cell_at_the_launch_cap: their first and last 4 096 rows equal a 4 096-row launch bit for bit."""
    c = _device(LS.make_case("unit", 4099, L, getattr(torch, dtype), True))
    big, mid = _launch(hip_lib, c), _launch(hip_lib, _rows_of(c, 0, 257))
    for k in FWD + BWD:
        assert same_bits(big[k][:257], mid[k]), (L, dtype, k, "the first 257 rows depend on the grid")
    for r in (0, 85, 255, 256):
        one = _launch(hip_lib, _rows_of(c, r, r + 1))
        for k in FWD + BWD:
            assert same_bits(one[k], mid[k][r:r + 1]), (L, dtype, k, r, "a row alone differs from the row in a launch")


@pytest.mark.parametrize("dtype,n,mp", LS.cap_cases(), ids=[f"{dt}-{n}-mask{int(mp)}" for dt, n, mp in LS.cap_cases()])
def test_lstm_cell_at_the_launch_cap(hip_lib, dtype, n, mp):
    """L = 256 at 65 536 rows (exactly 16 384 blocks) and 65 537 (the first launch whose grid-stride loop runs twice): one forward and one
    backward launch; the first and the last 4 096 rows against fp64 and, bit for bit, against a 4 096-row launch of the same rows."""
    dt = getattr(torch, dtype)
    bf16 = dt == torch.bfloat16
    assert LS.launch(n, LS.CAP_L) == (LS.CAP, 1 if n == LS.CAP_ROWS[0] else 2)
    c = LS.make_case("unit", n, LS.CAP_L, dt, mp, device="cuda")
    got = _launch(hip_lib, c)
    bad = []
    for lo, hi in ((0, LS.CAP_SLICE), (n - LS.CAP_SLICE, n)):
        s = _rows_of(c, lo, hi)
        ref, yard = LS.lstm_ref(*_args(s)), LS.lstm_yardstick(*_args(s))
        part = {k: v[lo:hi] for k, v in got.items()}
        b, stats = LS.judge(bf16, part, ref, yard)
        name = f"L={LS.CAP_L} {'bf16' if bf16 else 'fp32'} rows={n} unit mask={int(mp)} [{lo}, {hi})"
        bad += [(name,) + x for x in b]
        print(f"LSTM {name}: " + LS.stats_line(stats))
        own = _launch(hip_lib, s)
        for k in FWD + BWD:
            assert same_bits(part[k], own[k]), (name, k, "the rows differ from a launch of their own")
    assert not bad, bad


def test_abi_refusals_launch_nothing(hip_lib):
    """hidden & 3 and a pointer that is not 16-byte aligned: an error code, and every output still the sentinel"""
    n, L = 5, 8
    c = _device(LS.make_case("unit", n, L, torch.float32, True))
    ins = {k: _input(c[k])[1] for k in ("gx", "gh", "c_prev", "dh", "dc", "mask")}
    outs = {"h": _output(n * L, torch.float32), "c": _output(n * L, torch.float32), "dgates": _output(n * 4 * L, torch.float32),
            "dc_prev": _output(n * L, torch.float32)}
    o = {k: v[1] for k, v in outs.items()}

    def fwd(hidden=L, gx=0, h=0):
        return hip_lib.catan_lstm_cell_fwd(P(ins["gx"], gx), P(ins["gh"]), P(ins["c_prev"]), P(ins["mask"]), P(o["h"], h), P(o["c"]), n, hidden, 0, _stream())

    def bwd(hidden=L, dh=0, dg=0):
        return hip_lib.catan_lstm_cell_bwd(P(ins["gx"]), P(ins["gh"]), P(ins["c_prev"]), P(ins["mask"]), P(ins["dh"], dh), P(ins["dc"]), P(o["dgates"], dg),
                                           P(o["dc_prev"]), n, hidden, 0, _stream())

    for rc in (fwd(hidden=6), fwd(hidden=7), fwd(gx=4), fwd(h=8), bwd(hidden=6), bwd(dh=4), bwd(dg=8)):
        assert rc != 0
    torch.cuda.synchronize()
    for k, (whole, view) in outs.items():
        assert bool((whole.view(torch.int32) == SENTINEL).all()), (k, "a refused call wrote")
    _check(fwd())
    _check(bwd())
    torch.cuda.synchronize()
