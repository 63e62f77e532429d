"""GPU: the tile encoder's training path kernel by kernel against fp64 - catan_ffn_outproj_bwd (k_ffn_bwd_w), catan_qkv_bwd
(k_qkv_bwd_w), the activations catan_tile_encoder_fwd_train stores, and catan_layer_norm_bwd_res at every width it is built for -
called through the C ABI directly.

Acceptance, for every output tensor (te_reference.within_yardstick: the rule of tests/pin_rule.py with the bf16 floor):
    maxabs(kernel - reference) <= 2 * maxabs(yardstick - reference) + 2^-9 * maxabs(reference)
reference = the operation in fp64 from the same bf16 inputs; yardstick = fp32 with a bf16 rounding where the kernel rounds.  The
bound is computed inside the test from those two; nothing in it comes from a kernel's output.  Every case prints one `TE_BWD` line
per output (kernel error, yardstick error, their ratio): profiles/te_backward_kernel_tests.txt is that output.

Rows of the one-pass backward kernels and the blocks they give (te_bwd_grid, csrc/catan_abi_nn_launch.h: stages = ceil(rows / 64) stages of
64 rows; max(1, min(512, stages / 16)) blocks of ceil(stages / blocks) stages each, empty trailing blocks dropped; a wave takes 16 of
a stage's rows):
    1, 15, 16, 17     one stage: less than a wave, a full wave, one row into the second wave
    19                one board: a full wave and three rows
    63, 64, 65        a stage short of one row, exactly full, one row into a second stage
    133               three stages, the last with 5 rows
    1984              31 stages -> 31 / 16 = 1 block: the most stages one block takes
    2047, 2048        32 stages -> 2 blocks of 16 stages (1 024 rows): the second ragged (1 023 rows) / exactly full
    2071 = 19 * 109   33 stages -> 2 blocks of up to 17 stages (1 088 rows): the second holds 983 rows, its last stage 23
    19703 = 19 * 1037 308 stages -> 19 blocks of up to 17 stages: 18 x 1 088 rows, the last block 119 (one full stage and 55 rows)"""
import ctypes as C

import pytest
import torch

import guarded as G
import pin_rule as PR
import te_reference as R
from guarded import ptr as P, stream as _stream

pytestmark = pytest.mark.gpu

EPS = 1e-5
GUARD = 64                       # rows behind every row-major buffer: NaN behind the inputs, a sentinel behind the outputs
SENTINEL = 0x5A5B                # (a bf16 bit pattern no kernel result is likely to equal, and not symmetric in its bytes)
ROWS = [1, 15, 16, 17, 19, 63, 64, 65, 133, 1984, 2047, 2048, 2071, 19703]


def _guarded(t):
    """[rows, W] -> the first `rows` rows of a buffer with GUARD further rows of NaN: a read past `rows` that is used poisons a result"""
    return G.guarded_input(t, GUARD * t.shape[1], device=t.device)[0].view(-1, t.shape[1])


def _out_buffer(rows, W, dtype=torch.bfloat16, guard=GUARD):
    """[rows + guard, W]: an output of `rows` rows followed by `guard` rows of the sentinel (every 16-bit word of the buffer starts as the sentinel)"""
    return G.sentinel_output(rows * W, dtype, guard * W, sentinel=SENTINEL)[0].view(rows + guard, W)


def _guard_intact(buf, rows):
    return G.intact(buf, buf[:rows])


def _check(case, got, ref, yard):
    """every tensor of `got` finite and within the yardstick rule; prints the record line of each and names every failure"""
    bad = []
    for n in ref:
        ok, ek, ey, bound = R.within_yardstick(got[n], ref[n], yard[n])
        finite = bool(torch.isfinite(got[n]).all())
        print(f"TE_BWD {case} {n}: kernel {ek:.4e} yardstick {ey:.4e} ratio {PR.ratio(ek, ey, PR.INF):.3f} bound {bound:.4e} scale {float(ref[n].abs().max()):.4e}")
        if not (ok and finite):
            bad.append((case, n, ek, ey, "finite" if finite else "NOT FINITE"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ (a) inputs
_FFN, _QKV = {}, {}


def _weights(g, *shape):
    return (0.1 * torch.randn(shape, device="cuda", generator=g)).to(torch.bfloat16)


def _rows_x(g, rows):
    """x whose per-row mean and scale vary across the rows, so that the row statistics matter"""
    mean = torch.linspace(-2.0, 3.0, rows, device="cuda")[:, None]
    scale = torch.linspace(0.4, 2.5, rows, device="cuda").flip(0)[:, None]
    return (torch.randn((rows, 64), device="cuda", generator=g) * scale + mean).to(torch.bfloat16)


def _ffn_case(rows):
    """inputs (seeded, asymmetric), reference and yardstick of catan_ffn_outproj_bwd at `rows`: computed once, shared, never written"""
    if rows not in _FFN:
        g = torch.Generator(device="cuda").manual_seed(1000 + rows)
        bf = torch.bfloat16
        i = dict(
            dx=(torch.randn((rows, 64), device="cuda", generator=g) * torch.linspace(0.25, 2.0, 64, device="cuda") + 0.05).to(bf),
            h=torch.relu(torch.randn((rows, 128), device="cuda", generator=g) * torch.linspace(1.5, 0.5, 128, device="cuda")).to(bf),
            x=_rows_x(g, rows),
            o=(torch.randn((rows, 64), device="cuda", generator=g) * torch.linspace(0.5, 1.5, 64, device="cuda") - 0.1).to(bf),
            W2=_weights(g, 64, 128), W1=_weights(g, 128, 64), Wo=_weights(g, 64, 64),
            ln_w=(1.0 + 0.6 * torch.randn(64, device="cuda", generator=g)) * 1.7, ln_b=0.8 * torch.randn(64, device="cuda", generator=g) - 0.4)
        args = (i["dx"], i["h"], i["x"], i["W2"], i["W1"], i["ln_w"], i["ln_b"], EPS, i["o"], i["Wo"])
        _FFN[rows] = (i, R.ffn_outproj_bwd_ref(*args), R.ffn_outproj_bwd_ref(*args, round_bf16=True))
    return _FFN[rows]


def _qkv_case(rows):
    if rows not in _QKV:
        g = torch.Generator(device="cuda").manual_seed(2000 + rows)
        bf = torch.bfloat16
        i = dict(
            dqkv=(torch.randn((rows, 192), device="cuda", generator=g) * torch.linspace(2.0, 0.25, 192, device="cuda") + 0.05).to(bf),
            x=_rows_x(g, rows),
            dres=(torch.randn((rows, 64), device="cuda", generator=g) * torch.linspace(0.3, 1.8, 64, device="cuda") - 0.05).to(bf),
            Wqkv=_weights(g, 192, 64),
            ln_w=(1.0 + 0.6 * torch.randn(64, device="cuda", generator=g)) * 1.7, ln_b=0.8 * torch.randn(64, device="cuda", generator=g) - 0.4)
        args = (i["dqkv"], i["x"], i["dres"], i["Wqkv"], i["ln_w"], i["ln_b"], EPS)
        _QKV[rows] = (i, R.qkv_bwd_ref(*args), R.qkv_bwd_ref(*args, round_bf16=True))
    return _QKV[rows]


_FFN_ACC = (("dw2", (64, 128)), ("db2", (64,)), ("dw1", (128, 64)), ("db1", (128,)), ("dln_w", (64,)), ("dln_b", (64,)), ("dwo", (64, 64)), ("dbo", (64,)))
_QKV_ACC = (("dw", (192, 64)), ("db", (192,)), ("dln_w", (64,)), ("dln_b", (64,)))


def _accumulators(spec, prefill):
    return {n: (G.pattern(torch.Size(s).numel(), k + 1).view(s).contiguous() if prefill else torch.zeros(s, device="cuda")) for k, (n, s) in enumerate(spec)}


def _run_ffn(L, i, rows, prefill=False):
    """catan_ffn_outproj_bwd on the first `rows` rows of the case's inputs -> (outputs minus the pre-fill, dx_out buffer, d_o buffer)"""
    from settlers_of_catan_rl_amd import _lib
    dx, h, x, o = (_guarded(i[k][:rows]) for k in ("dx", "h", "x", "o"))
    w2t, w1t, wot = i["W2"].t().contiguous(), i["W1"].t().contiguous(), i["Wo"].t().contiguous()
    dxo, do = _out_buffer(rows, 64), _out_buffer(rows, 64)
    a = _accumulators(_FFN_ACC, prefill)
    a0 = {n: t.clone() for n, t in a.items()}
    _lib.check(L.catan_ffn_outproj_bwd(P(dx), P(h), P(x), P(w2t), P(w1t), P(i["ln_w"]), P(i["ln_b"]), EPS, P(dxo), P(a["dw2"]), P(a["db2"]), P(a["dw1"]),
                                       P(a["db1"]), P(a["dln_w"]), P(a["dln_b"]), P(o), P(wot), P(do), P(a["dwo"]), P(a["dbo"]), rows, _stream()))
    torch.cuda.synchronize()
    got = {n: a[n].double() - a0[n].double() for n in a}
    got["dx_out"], got["d_o"] = dxo[:rows].float(), do[:rows].float()
    return got, dxo, do


def _run_qkv(L, i, rows, prefill=False):
    from settlers_of_catan_rl_amd import _lib
    dqkv, x, dres = (_guarded(i[k][:rows]) for k in ("dqkv", "x", "dres"))
    wt = i["Wqkv"].t().contiguous()
    dxo = _out_buffer(rows, 64)
    a = _accumulators(_QKV_ACC, prefill)
    a0 = {n: t.clone() for n, t in a.items()}
    _lib.check(L.catan_qkv_bwd(P(dqkv), P(x), P(dres), P(wt), P(i["ln_w"]), P(i["ln_b"]), EPS, P(dxo), P(a["dw"]), P(a["db"]), P(a["dln_w"]), P(a["dln_b"]),
                               rows, _stream()))
    torch.cuda.synchronize()
    got = {n: a[n].double() - a0[n].double() for n in a}
    got["dx_out"] = dxo[:rows].float()
    return got, dxo


# ------------------------------------------------------------------------------------------------ (a) the one-pass backward kernels
@pytest.mark.parametrize("rows", ROWS)
def test_ffn_outproj_bwd_vs_fp64(hip_lib, rows):
    """k_ffn_bwd_w: dx_out, d_o and the eight accumulated gradients against fp64 at every row count of the table above; inputs end
    in NaN rows, outputs in sentinel rows that must come back bit-unchanged."""
    i, ref, yard = _ffn_case(rows)
    assert 0.35 < float((i["h"] == 0).float().mean()) < 0.65            # about half the ReLU mask is off
    got, dxo, do = _run_ffn(hip_lib, i, rows)
    _check(f"ffn_outproj_bwd rows={rows}", got, ref, yard)
    assert _guard_intact(dxo, rows) and _guard_intact(do, rows), rows


@pytest.mark.parametrize("rows", ROWS)
def test_qkv_bwd_vs_fp64(hip_lib, rows):
    """k_qkv_bwd_w: dx_out and the four accumulated gradients against fp64, same row counts and guards."""
    i, ref, yard = _qkv_case(rows)
    got, dxo = _run_qkv(hip_lib, i, rows)
    _check(f"qkv_bwd rows={rows}", got, ref, yard)
    assert _guard_intact(dxo, rows), rows


def test_te_backward_kernels_accumulate(hip_lib):
    """The accumulation contract of the headers ("ACCUMULATED into"): with every accumulator pre-filled with a non-constant pattern,
    what a call at rows = 133 adds is the gradient, to the same bound (the fp32 add of pattern and gradient stays far inside the floor)."""
    rows = 133
    i, ref, yard = _ffn_case(rows)
    _check(f"ffn_outproj_bwd prefilled rows={rows}", _run_ffn(hip_lib, i, rows, prefill=True)[0], ref, yard)
    i, ref, yard = _qkv_case(rows)
    _check(f"qkv_bwd prefilled rows={rows}", _run_qkv(hip_lib, i, rows, prefill=True)[0], ref, yard)


def test_te_backward_rows_do_not_depend_on_the_grid(hip_lib):
    """A row's dx_out / d_o depends on its own inputs only: at rows = 2071 (two blocks, the first of 1 088 rows) the first 1 088 rows
    are bit-equal to those of a call on the first 1 088 rows alone (one block)."""
    i, _, _ = _ffn_case(2071)
    full, one = _run_ffn(hip_lib, i, 2071), _run_ffn(hip_lib, i, 1088)
    assert torch.equal(full[1][:1088].view(torch.int16), one[1][:1088].view(torch.int16))
    assert torch.equal(full[2][:1088].view(torch.int16), one[2][:1088].view(torch.int16))
    i, _, _ = _qkv_case(2071)
    full, one = _run_qkv(hip_lib, i, 2071), _run_qkv(hip_lib, i, 1088)
    assert torch.equal(full[1][:1088].view(torch.int16), one[1][:1088].view(torch.int16))


# ---------------------------------------------------------------------------------------- (b) what the training forward stores
_TE = {}


def _te_setup():
    """the perturbed net, its packed parameters and real tile observations of 17 boards (one env, one rollout, shared)"""
    if not _TE:
        from settlers_of_catan_rl_amd import nn_kernels
        from settlers_of_catan_rl_amd.env import VecCatanEnv
        from settlers_of_catan_rl_amd.policy import CatanPolicy
        torch.manual_seed(0)
        net = CatanPolicy().cuda()
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.05 * torch.randn_like(p))
        te = net.observation_module.tile_encoder
        env = VecCatanEnv(17, seed=3); env.random_rollout(0, 600)
        f, _, _ = env.get_obs()
        tiles = f[:, 18:18 + 1140].reshape(17, 19, 60).to(torch.bfloat16).contiguous()
        wts, vecs = nn_kernels.tile_encoder_pack(te)
        _TE.update(te=te, tiles=tiles, wts=wts, vecs=vecs, refs={})
    return _TE


def _te_refs(B):
    s = _te_setup()
    if B not in s["refs"]:
        with torch.no_grad():
            s["refs"][B] = (R.tile_encoder_ref(s["te"], s["tiles"][:B]), R.tile_encoder_ref(s["te"], s["tiles"][:B], round_bf16=True))
    return s["refs"][B]


def _run_te(L, B, skip=(), pitch=475):
    """catan_tile_encoder_fwd_train on the first B boards with every save pointer set but those named in `skip` -> ({field: buffer
    with 8 sentinel rows behind its B * 19}, out buffer [B + 1, pitch] pre-filled with the sentinel)"""
    from settlers_of_catan_rl_amd import _lib
    s = _te_setup()
    T = B * 19
    bufs = {}
    for n, w in R.TE_FIELDS:
        if n not in skip:
            bufs[n] = _out_buffer(T, w, guard=8)
    ptrs = (C.c_void_p * len(R.TE_FIELDS))(*[bufs[n].data_ptr() if n in bufs else None for n, _ in R.TE_FIELDS])
    out = _out_buffer(B, pitch, guard=1)
    tiles = s["tiles"][:B].contiguous()
    _lib.check(L.catan_tile_encoder_fwd_train(P(tiles), P(s["wts"]), P(s["vecs"]), P(out), pitch, C.cast(ptrs, C.c_void_p), B, _stream()))
    torch.cuda.synchronize()
    return bufs, out


# a workgroup takes TE_G boards (csrc/catan_tile_encoder.hip; 5 as built, 8 in the variant its header comment measured): 1 = one board,
# 5 / 6 and 10 / 11 = the last group exactly full / one board into the next at TE_G = 5, 7, 8, 9 = the same edges at 8, 17 = four groups
@pytest.mark.parametrize("B", [1, 5, 6, 7, 8, 9, 10, 11, 17])
def test_tile_encoder_training_saves_vs_fp64(hip_lib, B):
    """Every activation catan_tile_encoder_fwd_train stores - all eighteen pointers set, n1 and n2 included - and its output against
    the module's own formulas in fp64 (tile_encoder_ref), field by field.  Then: n1 / n2 / h left out change no other bit; out_pitch =
    480 leaves columns 475..479 untouched; tiles64's pad columns are exact zeros; nothing is written behind the B * 19 rows."""
    T = B * 19
    ref, yard = _te_refs(B)
    bufs, out = _run_te(hip_lib, B)
    got = {n: bufs[n][:T].float() for n, _ in R.TE_FIELDS}
    got["out"] = out[:B].float()
    _check(f"tile_encoder_fwd_train B={B}", got, ref, yard)
    for n, _ in R.TE_FIELDS:
        assert _guard_intact(bufs[n], T), n
    assert _guard_intact(out, B)
    assert torch.equal(got["tiles64"][:, :60], _te_setup()["tiles"][:B].reshape(T, 60).float())
    assert bool((bufs["tiles64"][:T, 60:].view(torch.int16) == 0).all())
    # the optional saves left out: everything else bit-equal
    optional = ("n1_0", "n1_1", "n2_0", "n2_1", "h0", "h1")
    bufs2, out2 = _run_te(hip_lib, B, skip=optional)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))
    for n, _ in R.TE_FIELDS:
        if n not in optional:
            assert torch.equal(bufs2[n].view(torch.int16), bufs[n].view(torch.int16)), n
    # a padded output pitch
    _, out3 = _run_te(hip_lib, B, pitch=480)
    assert torch.equal(out3[:B, :475].view(torch.int16), out[:B].view(torch.int16))
    assert bool((out3[:, 475:].view(torch.int16) == SENTINEL).all()) and bool((out3[B:].view(torch.int16) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- (c) catan_layer_norm_bwd_res
@pytest.mark.parametrize("rows", [1, 63, 4099])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_layer_norm_bwd_res_vs_fp64(hip_lib, D, dtype, rows):
    """dx = LayerNorm'(dy) + dres, dw += sum dy * x_hat, db += sum dy at every width the entry point is built for, in both storage
    types, against fp64 from the same inputs; dw / db pre-filled.  bf16: the yardstick rule (the LayerNorm term rounded to bf16 before
    the add, as the header says).  fp32: the bound of test_small_layer_norm_kernel_vs_torch - dx within 8e-5 absolute + relative,
    dw / db within 8e-5 * sqrt(rows) + 2e-2 relative."""
    from settlers_of_catan_rl_amd import _lib
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(D * 7 + rows)
    mean = torch.linspace(-1.0, 2.0, rows, device="cuda")[:, None]
    scale = torch.linspace(2.5, 0.5, rows, device="cuda")[:, None]
    x = (torch.randn((rows, D), device="cuda", generator=g) * scale + mean).to(dt)
    dy = (torch.randn((rows, D), device="cuda", generator=g) * torch.linspace(0.25, 2.0, D, device="cuda") + 0.05).to(dt)
    dres = (torch.randn((rows, D), device="cuda", generator=g) * torch.linspace(1.5, 0.5, D, device="cuda") - 0.05).to(dt)
    w = (1.0 + 0.6 * torch.randn(D, device="cuda", generator=g)) * 1.7
    b = 0.8 * torch.randn(D, device="cuda", generator=g) - 0.4
    xg, dyg, dresg = _guarded(x), _guarded(dy), _guarded(dres)
    dx = _out_buffer(rows, D, dt)
    dw, db = G.pattern(D, 1), G.pattern(D, 2)
    dw0, db0 = dw.clone(), db.clone()
    _lib.check(hip_lib.catan_layer_norm_bwd_res(P(xg), P(w), P(b), P(dyg), P(dresg), P(dx), P(dw), P(db), rows, D, EPS, 0, int(dt == torch.bfloat16), _stream()))
    torch.cuda.synchronize()
    assert _guard_intact(dx, rows), (D, dtype, rows)
    got = {"dx": dx[:rows].float(), "dw": dw.double() - dw0.double(), "db": db.double() - db0.double()}
    ref = R.layer_norm_bwd_res_ref(x, w, dy, dres, EPS)
    case = f"layer_norm_bwd_res D={D} {dtype} rows={rows}"
    if dt == torch.bfloat16:
        _check(case, got, ref, R.layer_norm_bwd_res_ref(x, w, dy, dres, EPS, round_bf16=True))
    else:
        tol = 4 * 2e-5
        for n in ("dx", "dw", "db"):
            err = (got[n].double() - ref[n]).abs()
            print(f"TE_BWD {case} {n}: kernel {float(err.max()):.4e} scale {float(ref[n].abs().max()):.4e}")
        assert bool(torch.isfinite(got["dx"]).all())
        assert bool(((got["dx"].double() - ref["dx"]).abs() <= tol + tol * ref["dx"].abs()).all()), case
        for n in ("dw", "db"):
            assert bool(((got[n] - ref[n]).abs() <= tol * max(1.0, rows ** 0.5) + 2e-2 * ref[n].abs()).all()), (case, n)
