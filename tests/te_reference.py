"""Plain-torch restatements of the tile encoder's training path, one function per hand-written kernel: the two one-pass
backward kernels of csrc/catan_te_bwd.hip (k_ffn_bwd_w, k_qkv_bwd_w) and the training forward of csrc/catan_tile_encoder.hip with
everything it stores.  No call into the library: torch ops only, on the CPU or the GPU, from inputs of any float dtype.

Every function has two modes.
  round_bf16=False  the REFERENCE: fp64 throughout, from the same (bf16-valued) inputs.
  round_bf16=True   the YARDSTICK: fp32, with a round-to-bf16 at exactly the points where the kernels round (named in the kernels'
                    comments and repeated at each function).  It shows what bf16 storage alone costs against the reference; it is
                    not an oracle.
tests/test_te_reference_cpu.py holds the reference against autograd and against the module; tests/test_gpu_te_backward.py holds the
kernels against the reference with `within_yardstick`: the rule of tests/pin_rule.py over a whole tensor, with the bf16 floor."""
import math

import torch

from pin_rule import BF16_FLOOR, whole

# catan_te_saves_t's fields in the struct's order (pointer i of the struct = entry i), with their widths
TE_FIELDS = (("tiles64", 64), ("a0", 64), ("xin0", 64), ("xin1", 64), ("n1_0", 64), ("n1_1", 64), ("qkv0", 192), ("qkv1", 192), ("o0", 64), ("o1", 64),
             ("xmid0", 64), ("xmid1", 64), ("n2_0", 64), ("n2_1", 64), ("h0", 128), ("h1", 128), ("xfin", 64), ("p", 25))


def _modes(round_bf16):
    """-> (working dtype, the rounding applied where a kernel stores or hands on bf16)"""
    if round_bf16:
        return torch.float32, lambda t: t.to(torch.bfloat16).to(torch.float32)
    return torch.float64, lambda t: t


def _ln_stats(x, eps):
    """-> (x_hat, rstd) of LayerNorm over the last dim (biased variance, as nn.LayerNorm)"""
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    rstd = ((c * c).mean(-1, keepdim=True) + eps) ** -0.5
    return c * rstd, rstd


def _ln_backward_term(dn, xhat, rstd, w):
    """the LayerNorm's contribution to the gradient of its input: rstd * (g - mean(g) - x_hat * mean(g * x_hat)), g = dn * w"""
    g = dn * w
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def ffn_outproj_bwd_ref(dx, h, x, W2, W1, ln_w, ln_b, eps, o, Wo, round_bf16=False):
    """catan_ffn_outproj_bwd: the backward of x_out = x + linear2(relu(linear1(LayerNorm(x)))) and of the out-projection
    x = x_in + o Wo^T + bo that produced x.  dx [rows, 64] = d(x_out); h [rows, 128] = relu(linear1(.)); x [rows, 64]; W2 [64, 128] =
    linear2.weight; W1 [128, 64] = linear1.weight; o [rows, 64]; Wo [64, 64] = out_proj.weight (the module's layouts: the kernel takes
    their transposes).
      dH = (dx W2) * [h > 0]      dW2 = dx^T h     db2 = sum dx
      N = LN(x)   dN = dH W1      dW1 = dH^T N     db1 = sum dH
      dln_w = sum dN * x_hat      dln_b = sum dN
      dx' = LN'(dN) + dx          d_o = dx' Wo     dWo = dx'^T o    dbo = sum dx'
    Yardstick roundings (k_ffn_bwd_w): dH and dN; N as the operand of dW1; the LayerNorm term of dx' before the residual add, then
    the sum - dx' is what d_o, dWo and dbo are formed from; d_o itself, a bf16 output like dx_out."""
    wd, r = _modes(round_bf16)
    dx, h, x, W2, W1, ln_w, ln_b, o, Wo = (t.to(wd) for t in (dx, h, x, W2, W1, ln_w, ln_b, o, Wo))
    dH = r((dx @ W2) * (h > 0).to(wd))
    xhat, rstd = _ln_stats(x, eps)
    N = r(xhat * ln_w + ln_b)
    dN = r(dH @ W1)
    dxp = r(r(_ln_backward_term(dN, xhat, rstd, ln_w)) + dx)
    return {"dx_out": dxp, "d_o": r(dxp @ Wo), "dw2": dx.t() @ h, "db2": dx.sum(0), "dw1": dH.t() @ N, "db1": dH.sum(0),
            "dln_w": (dN * xhat).sum(0), "dln_b": dN.sum(0), "dwo": dxp.t() @ o, "dbo": dxp.sum(0)}


def qkv_bwd_ref(dqkv, x, dres, Wqkv, ln_w, ln_b, eps, round_bf16=False):
    """catan_qkv_bwd: the input side of x_mid = x + out_proj(attention(qkv(LayerNorm(x)))).  dqkv [rows, 192]; x [rows, 64]; dres
    [rows, 64] = d(x_mid); Wqkv [192, 64] = the q, k, v weights stacked (the kernel takes the transpose).
      N = LN(x)   dN = dqkv Wqkv   dw = dqkv^T N   db = sum dqkv   dln_w = sum dN * x_hat   dln_b = sum dN   dx_out = LN'(dN) + dres
    Yardstick roundings (k_qkv_bwd_w): dN; N as the operand of dw; the LayerNorm term of dx_out before the residual add, then the sum."""
    wd, r = _modes(round_bf16)
    dqkv, x, dres, Wqkv, ln_w, ln_b = (t.to(wd) for t in (dqkv, x, dres, Wqkv, ln_w, ln_b))
    xhat, rstd = _ln_stats(x, eps)
    N = r(xhat * ln_w + ln_b)
    dN = r(dqkv @ Wqkv)
    return {"dx_out": r(r(_ln_backward_term(dN, xhat, rstd, ln_w)) + dres), "dw": dqkv.t() @ N, "db": dqkv.sum(0),
            "dln_w": (dN * xhat).sum(0), "dln_b": dN.sum(0)}


def layer_norm_bwd_res_ref(x, w, dy, dres, eps, round_bf16=False):
    """catan_layer_norm_bwd_res (no ReLU): dx = LN'(dy) + dres, dw = sum dy * x_hat, db = sum dy.  Yardstick rounding (the header):
    the LayerNorm term to bf16 before the add, then the sum as it is stored."""
    wd, r = _modes(round_bf16)
    x, w, dy, dres = (t.to(wd) for t in (x, w, dy, dres))
    xhat, rstd = _ln_stats(x, eps)
    return {"dx": r(r(_ln_backward_term(dy, xhat, rstd, w)) + dres), "dw": (dy * xhat).sum(0), "db": dy.sum(0)}


def tile_encoder_ref(te, tiles, round_bf16=False):
    """catan_tile_encoder_fwd_train on the parameters of a policy._TileEncoder: tiles [B, 19, 60] -> a dict with every field of
    catan_te_saves_t under TE_FIELDS' names ([B * 19, width] each) and "out" [B, 475], by the formulas of RL/models/tile_encoder.py as
    policy._TileEncoder lays them out:
      a0 = first_layer(tiles)   xin0 = relu(norm_2(a0))
      per layer l:  n1 = norm(xin)  qkv = [q | k | v](n1)  o = softmax(q k^T / sqrt(16)) v per board and head
                    xmid = xin + out_proj_net(o)   n2 = norm(xmid)   h = relu(linear1(n2))   xin' = xmid + linear2(h)
      xfin = the last layer's output   p = out_proj(xfin)   out = relu(norm(p)) as [B, 19 * 25]
    Weights, biases and the tiles are rounded to bf16 first - what bf16 autocast hands to a GEMM - and LayerNorm vectors stay fp32.
    Reference: fp64 from there.  Yardstick: fp32 with every stored activation (and the output) rounded to bf16."""
    wd, r = _modes(round_bf16)
    bf = lambda t: t.detach().to(torch.bfloat16).to(wd)             # a GEMM operand under bf16 autocast
    vec = lambda t: t.detach().to(torch.float32).to(wd)             # a LayerNorm vector

    def ln(m, x):
        return _ln_stats(x, m.eps)[0] * vec(m.weight) + vec(m.bias)

    def lin(x, w, b):
        return x @ bf(w).t() + bf(b)

    B = tiles.shape[0]
    T = B * 19
    out = {}
    t = bf(tiles).reshape(T, 60)
    out["tiles64"] = torch.cat([t, torch.zeros((T, 4), dtype=wd, device=t.device)], 1)
    out["a0"] = r(lin(t, te.first_layer.weight, te.first_layer.bias))
    x = r(torch.relu(ln(te.norm_2, out["a0"])))
    for l, layer in enumerate(te.encoder_layers):
        mha, ffn = layer.multi_headed_attention, layer.pointwise_net
        H, hd = mha.heads, mha.hd
        out[f"xin{l}"] = x
        n1 = out[f"n1_{l}"] = r(ln(layer.sublayers[0].norm, x))
        qkv = out[f"qkv{l}"] = r(lin(n1, torch.cat([n.weight for n in mha.qkv_nets], 0), torch.cat([n.bias for n in mha.qkv_nets], 0)))
        q, k, v = qkv.view(B, 19, 3, H, hd).permute(2, 0, 3, 1, 4)                     # [B, H, 19, hd] each
        prob = torch.softmax(q @ k.transpose(-2, -1) * (1.0 / math.sqrt(hd)), -1)
        o = out[f"o{l}"] = r((prob @ v).transpose(1, 2).reshape(T, H * hd))
        xmid = out[f"xmid{l}"] = r(x + lin(o, mha.out_proj_net.weight, mha.out_proj_net.bias))
        n2 = out[f"n2_{l}"] = r(ln(layer.sublayers[1].norm, xmid))
        h = out[f"h{l}"] = r(torch.relu(lin(n2, ffn.linear1.weight, ffn.linear1.bias)))
        x = r(xmid + lin(h, ffn.linear2.weight, ffn.linear2.bias))
    out["xfin"] = x
    out["p"] = r(lin(x, te.out_proj.weight, te.out_proj.bias))
    out["out"] = r(torch.relu(ln(te.norm, out["p"]))).reshape(B, 19 * te.out_proj.out_features)
    assert set(out) == {n for n, _ in TE_FIELDS} | {"out"}
    return out



def within_yardstick(kernel, ref, yardstick):
    """pin_rule.whole with the floor of a bf16 output, half a bf16 ulp of the tensor's scale -> (ok, kernel error, yardstick error, bound)"""
    return whole(kernel, ref, yardstick, BF16_FLOOR)
