"""GPU: the four attention kernels of csrc/catan_nn.hip (k_attn_fwd, k_attn_bwd, k_attn_mfma_fwd, k_attn_mfma_bwd) per sequence against
fp64, on every path of attn_dispatch (csrc/catan_abi_nn_launch.h), through the C ABI (catan_attention_fwd / catan_attention_bwd).

reference = tests/attention_reference.py: attention_ref in fp64 from the inputs as stored; yardstick = attention_yardstick in fp32 with a
bf16 rounding where the kernel of the path rounds (its docstring places them).  Acceptance of an output tensor (out, dq, dk, dv):
    bf16 paths: the rule of tests/pin_rule.py: maxabs(kernel - ref) <= 2 maxabs(yardstick - ref) + 2^-9 maxabs(ref)
    fp32 path : the same rule with the fp32 yardstick and the floor 2^-17 maxabs(ref) for out, 2^-15 maxabs(ref) for the gradients
over the whole case AND for every sequence with that sequence's own yardstick error and scale (a wrong short sequence cannot hide behind
a long one).  Nothing in a bound comes from the kernel.  Per case and output one `ATTN` line is printed (kernel error, yardstick error,
ratio, bound, scale; worst-seq = the largest kernel error / bound of a single sequence): profiles/attention_kernel_tests.txt is that output.

Paths, each asserted from the pointers handed to the library with attn_dispatch's own predicate (`_takes_mfma`):
    mfma       bf16, qkv / out / dout / dqkv 16-byte aligned
    valu_bf16  bf16, every buffer 8 bytes into a larger allocation
    fp32       float32
The launches of attn_dispatch and the cases that reach them (each at both shapes; `lens` / `nolens` = with / without a length vector):
    k_attn_mfma_fwd<19,4,16>, <25,4,4>                       mfma, lens and nolens (the mask is a run-time argument)
    k_attn_mfma_bwd<19,4,16,true>, <25,4,4,true>             mfma lens          k_attn_mfma_bwd<.., false>     mfma nolens
    k_attn_fwd / k_attn_bwd<__hip_bfloat16, 19 | 25, ..>     valu_bf16, lens and nolens
    k_attn_fwd / k_attn_bwd<float, 19 | 25, ..>              fp32, lens and nolens
attn_dispatch<float> also contains the six MFMA launches, which `sizeof(T) == 2` keeps it from ever taking: fourteen kernels can run, and
test_attention_kernel_vs_fp64's parameters (path x shape x mask) are those fourteen, forward and backward in every one.

Batches: the MFMA kernels take 4 sequences per block, the VALU kernels 3 (L = 19) or 2 (L = 25): B = 1, 2, 3, 4, 5, 7, 8, 9 (mfma) /
1 .. 7 (VALU) and 1030 (many blocks, a tail of 2 / 1 / 0).  Every output lies in a buffer filled with a sentinel that is 4 sequences longer
than the result (and, on the valu_bf16 path, begins 8 bytes earlier): both margins must keep the sentinel.  Inputs end in 4 sequences of NaN.
Lengths cycle over attention_reference.length_cycle, continuing through the small batches, so those alone meet every length.
Regimes: unit, saturated (attention_reference.make_case; every output finite) and single = lens 1 everywhere, where out must be V's row 0
to the bit and dq, dk exactly zero (the per-sequence rule has bound 0 there).

The mask: lens[b] >= 1 is the header's contract (no caller can pass 0: policy._MHA is only called without lens by the tile encoder, the
card lists go through catan_card_summary_*), so length 0 is not run.  The mask is a KEY mask: query rows >= len are ordinary queries.
  * K and V rows >= len replaced by +-3e4: out, dq and the rows < len of dk, dv are bit-identical; the rows >= len of dk, dv are == 0.
  * Q rows >= len replaced as well: the outputs of those queries (out and dq rows >= len) legitimately change, and through them dk, dv
    unless their dO is zero - which is how the net uses a masked sequence (the padding's outputs are dropped).  So this rerun zeroes dO's
    rows >= len in both launches and then holds ALL of: out and dq rows < len, dk and dv rows < len bit-identical; dq, dk, dv rows >= len == 0.
  * lens = L everywhere equals the launch without lens bit for bit."""
import pytest
import torch

import attention_reference as A
import guarded as G
import pin_rule as PR
from guarded import ptr as P, stream as _stream
from pin_rule import same_bits

pytestmark = pytest.mark.gpu

GUARD_SEQ = 4
SENTINEL = 0x5A5B


def _takes_mfma(is_bf16, *tensors):
    """attn_dispatch's predicate: bf16 and every pointer it is handed (a missing one counts as 0) 16-byte aligned"""
    return is_bf16 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def _lead(path):
    """the view begins 8 bytes into its allocation on the valu_bf16 path, at its start otherwise"""
    return 4 if path == "valu_bf16" else 0


def _input(path, t):
    """t in front of GUARD_SEQ sequences of NaN"""
    return G.guarded_input(t, GUARD_SEQ * t[0].numel(), _lead(path))


def _output(path, n, seq, dtype):
    """n elements in front of GUARD_SEQ sequences of `seq` sentinel elements"""
    return G.sentinel_output(n, dtype, GUARD_SEQ * seq, _lead(path), SENTINEL)


def _launch(lib, path, qkv, lens, dout):
    """forward and backward of one case on `path` -> {out, dq, dk, dv} as [B, L, D] CPU tensors of the storage dtype"""
    from settlers_of_catan_rl_amd import _lib
    B, L, _, H, HD = qkv.shape
    D = H * HD
    dt = A.path_dtype(path)
    assert qkv.dtype == dt and dout.dtype == dt
    is_bf16 = int(dt == torch.bfloat16)
    hold_q, q_d = _input(path, qkv)
    hold_g, g_d = _input(path, dout)
    lens_d = None if lens is None else lens.to(torch.int32).cuda()
    whole_o, o_d = _output(path, B * L * D, L * D, dt)
    whole_dq, dq_d = _output(path, B * L * 3 * D, L * 3 * D, dt)
    # the path by construction
    assert _takes_mfma(is_bf16, q_d, o_d) == (path == "mfma") and _takes_mfma(is_bf16, q_d, g_d, dq_d) == (path == "mfma"), path
    if path == "valu_bf16":
        assert all(t.data_ptr() % 16 == 8 for t in (q_d, g_d, o_d, dq_d))
    _lib.check(lib.catan_attention_fwd(P(q_d), P(lens_d), P(o_d), B, L, H, HD, is_bf16, _stream()))
    _lib.check(lib.catan_attention_bwd(P(q_d), P(lens_d), P(g_d), P(dq_d), B, L, H, HD, is_bf16, _stream()))
    torch.cuda.synchronize()
    assert G.intact(whole_o, o_d) and G.intact(whole_dq, dq_d), (path, L, B, "a write outside the result")
    dqkv = dq_d.view(B, L, 3, D).cpu()
    return {"out": o_d.view(B, L, D).cpu(), "dq": dqkv[:, :, 0].contiguous(), "dk": dqkv[:, :, 1].contiguous(), "dv": dqkv[:, :, 2].contiguous()}


# ------------------------------------------------------------------------------------------------------------------------ cases
_CASES = {}


def _case(L, H, HD, B, regime, masked, dtype, start=0):
    """inputs and reference of a case: computed once on the CPU, shared, never written.  regime "single": the unit inputs with lens = 1"""
    key = (L, B, regime, masked, dtype, start)
    if key not in _CASES:
        if regime == "single":
            assert masked
            lens = torch.ones(B, dtype=torch.int32)
        else:
            lens = A.case_lens(L, B, start) if masked else None
        c = A.make_case(L, H, HD, B, "unit" if regime == "single" else regime, lens, dtype)
        c["regime"] = regime
        c["ref"] = A.attention_ref(c["qkv"], lens, c["dout"])
        c["yard"] = {}
        _CASES[key] = c
    return _CASES[key]


def _yard(c, path):
    if path not in c["yard"]:
        c["yard"][path] = A.attention_yardstick(c["qkv"], c["lens"], c["dout"], path)
    return c["yard"][path]


def _name(path, c):
    return f"{path} {c['L']} {'nolens' if c['lens'] is None else 'lens'} {c['regime']} B={c['B']}"


def _judge(path, c, got):
    """the rule over the case and per sequence, one ATTN line per output -> the list of failures"""
    ref, yard, bad = c["ref"], _yard(c, path), []
    for o in A.OUTPUTS:
        ok, ek, ey, bound = A.accept(path, o, got[o], ref[o], yard[o])
        oks, eks, bounds = A.per_sequence(path, o, got[o], ref[o], yard[o])
        finite = bool(torch.isfinite(got[o].float()).all())
        print(f"ATTN {_name(path, c)} {o}: kernel {ek:.4e} yardstick {ey:.4e} ratio {PR.ratio(ek, ey, PR.INF):.3f} bound {bound:.4e} "
              f"scale {float(ref[o].abs().max()):.4e} worst-seq {PR.share(eks, bounds):.3f}")
        if not (ok and finite):
            bad.append((_name(path, c), o, "whole", ek, ey, bound, "finite" if finite else "NOT FINITE"))
        if not bool(oks.all()):
            b = int((~oks).nonzero()[0])
            bad.append((_name(path, c), o, f"{int((~oks).sum())} sequences, first {b}", None if c["lens"] is None else int(c["lens"][b]), float(eks[b]), float(bounds[b])))
    return bad


def _rows(c):
    """[B, L, 1] bool: the rows < len"""
    return (torch.arange(c["L"])[None, :] < c["lens"][:, None].long())[:, :, None]


def _mask_checks(lib, path, c, got):
    """the mask properties of the module docstring on a lens case; `got` = the case's own launch"""
    name = _name(path, c)
    keep = _rows(c).expand_as(got["out"])
    for o in ("dk", "dv"):
        assert bool((got[o][~keep] == 0).all()), (name, o, "rows >= len are not zero")
    if bool(keep.all()):
        return
    # K and V behind the mask replaced
    alt = _launch(lib, path, A.replace_masked_rows(c, 1), c["lens"], c["dout"])
    assert same_bits(got["out"], alt["out"]) and same_bits(got["dq"], alt["dq"]), (name, "masked K / V rows reach out or dq")
    for o in ("dk", "dv"):
        assert same_bits(got[o][keep], alt[o][keep]), (name, o, "masked K / V rows reach the rows < len")
        assert bool((alt[o][~keep] == 0).all()), (name, o, "rows >= len are not zero")
    # ... and the Q rows behind it, with the gradient of their outputs zero
    dz = torch.where(keep, c["dout"], torch.zeros((), dtype=c["dout"].dtype))
    base = _launch(lib, path, c["qkv"], c["lens"], dz)
    alt = _launch(lib, path, A.replace_masked_rows(c, 2, ("q", "k", "v")), c["lens"], dz)
    assert same_bits(base["out"], got["out"]), (name, "out depends on dout")
    for o in A.OUTPUTS:
        assert same_bits(base[o][keep], alt[o][keep]), (name, o, "masked Q / K / V rows reach the rows < len")
        if o != "out":
            assert bool((base[o][~keep] == 0).all()) and bool((alt[o][~keep] == 0).all()), (name, o, "rows >= len are not zero")
        assert bool(torch.isfinite(alt[o].float()).all()), (name, o)


PARAMS = [(path, L, H, HD, masked) for path in A.PATHS for (L, H, HD) in A.SHAPES for masked in (False, True)]


@pytest.mark.parametrize("path,L,H,HD,masked", PARAMS, ids=[f"{p}-{L}-{'lens' if m else 'nolens'}" for p, L, H, HD, m in PARAMS])
def test_attention_kernel_vs_fp64(hip_lib, path, L, H, HD, masked):
    """One launch path of attn_dispatch at one shape, with or without lens, forward and backward: unit inputs at every batch size of the
    path, saturated inputs and (lens) single-key sequences at B = 7 and 1030.  See the module docstring for what is asserted.

    Measured on the MI355X: profiles/attention_kernel_tests.txt."""
    dt = A.path_dtype(path)
    bad, start = [], 0
    small = A.MFMA_BS if path == "mfma" else A.VALU_BS
    plan = [("unit", B) for B in small] + [("unit", A.MULTI_B), ("saturated", 7), ("saturated", A.MULTI_B)]
    if masked:
        plan += [("single", 7), ("single", A.MULTI_B)]
    for regime, B in plan:
        c = _case(L, H, HD, B, regime, masked, dt, start if (regime == "unit" and B != A.MULTI_B) else 0)
        if regime == "unit" and B != A.MULTI_B:
            start += B
        got = _launch(hip_lib, path, c["qkv"], c["lens"], c["dout"])
        for o in A.OUTPUTS:
            assert bool(torch.isfinite(got[o].float()).all()), (_name(path, c), o, "not finite")
        bad += _judge(path, c, got)
        if masked:
            _mask_checks(hip_lib, path, c, got)
        elif regime == "unit":
            full = _launch(hip_lib, path, c["qkv"], torch.full((B,), L, dtype=torch.int32), c["dout"])
            for o in A.OUTPUTS:
                assert same_bits(got[o], full[o]), (_name(path, c), o, "lens = L differs from no lens")
        if regime == "single":
            v0 = c["qkv"][:, 0, 2].reshape(B, 1, H * HD).expand(B, L, H * HD)
            assert same_bits(got["out"], v0), (_name(path, c), "one key: out is not V's row 0")
            assert bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all()), (_name(path, c), "one key: dq, dk are not zero")
    assert not bad, bad


@pytest.mark.parametrize("L,H,HD", A.SHAPES)
@pytest.mark.parametrize("masked", [False, True], ids=["nolens", "lens"])
def test_mfma_and_valu_agree_on_bf16(hip_lib, L, H, HD, masked):
    """The same bf16 inputs through the MFMA kernels and through the VALU kernels (unaligned buffers): the two results differ by no more
    than the sum of their two bounds against the reference.  A consistency check between the paths, not a substitute for the reference
    (which test_attention_kernel_vs_fp64 holds each of them to)."""
    for regime, B in (("unit", 7), ("saturated", 7), ("unit", A.MULTI_B), ("saturated", A.MULTI_B)):
        c = _case(L, H, HD, B, regime, masked, torch.bfloat16, 0)
        m = _launch(hip_lib, "mfma", c["qkv"], c["lens"], c["dout"])
        v = _launch(hip_lib, "valu_bf16", c["qkv"], c["lens"], c["dout"])
        for o in A.OUTPUTS:
            bm = A.accept("mfma", o, m[o], c["ref"][o], _yard(c, "mfma")[o])[3]
            bv = A.accept("valu_bf16", o, v[o], c["ref"][o], _yard(c, "valu_bf16")[o])[3]
            d = float((m[o].double() - v[o].double()).abs().max())
            print(f"ATTN-PATHS {L} {'lens' if masked else 'nolens'} {regime} B={B} {o}: mfma - valu_bf16 {d:.4e} bounds {bm:.4e} + {bv:.4e}")
            assert d <= bm + bv, (L, masked, regime, B, o, d, bm, bv)
