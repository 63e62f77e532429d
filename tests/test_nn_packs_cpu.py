"""The parameter packs of settlers_of_catan_rl_amd/nn_kernels.py on the CPU (the built library is loaded for the `*_elems()` sizes only):
the tile encoder's pack element by element against the layout include/catan_hip_nn.h describes - the offsets below are worked out from
the header's text, not from nn_kernels' table -, the training-side images (_TeImages) against the pack, the one cache helper of the four
packers, and refresh_packs.  Every parameter of the encoder is seeded normal noise, the LayerNorm vectors too: no block is all ones or all
zeros, so a swapped block shows."""
import pytest
import torch

import heads_reference as H
from settlers_of_catan_rl_amd import _lib, nn_kernels

BF = torch.bfloat16
# include/catan_hip_nn.h: weights = first_layer [64][64], per layer qkv [192][64], out_proj [64][64], linear1 [128][64], linear2 [64][128],
# then out_proj [32][64]; vecs = first-layer bias, norm_2 weight, bias [64 each], per layer sublayer-0 norm weight, bias [64], qkv bias
# [192], out_proj bias [64], sublayer-1 norm weight, bias [64], linear1 bias [128], linear2 bias [64], then out_proj bias, norm weight, bias [32 each]
W_FIRST, W_LAYER = 64 * 64, 192 * 64 + 64 * 64 + 128 * 64 + 64 * 128
W_QKV, W_OUT, W_L1, W_L2 = 0, 192 * 64, 192 * 64 + 64 * 64, 192 * 64 + 64 * 64 + 128 * 64          # within a layer
W_TAIL = W_FIRST + 2 * W_LAYER
V_HEAD, V_LAYER = 3 * 64, 64 + 64 + 192 + 64 + 64 + 64 + 128 + 64
V_LN1W, V_LN1B, V_BQKV, V_BO, V_LN2W, V_LN2B, V_B1, V_B2 = 0, 64, 128, 320, 384, 448, 512, 640      # within a layer
V_TAIL = V_HEAD + 2 * V_LAYER


@pytest.fixture(autouse=True)
def _registry_left_empty():
    """the images these tests register are CPU tensors: none stays in the process-wide registry"""
    yield
    nn_kernels.weight_images.clear()


def _encoder(seed=5):
    from settlers_of_catan_rl_amd.policy import _TileEncoder
    te = _TileEncoder()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in te.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return te


def _bits(t):
    return t.view(torch.int16)


def _same_as_pack(im, te):
    wts, vecs = nn_kernels.tile_encoder_pack(te)
    return torch.equal(_bits(im.wts), _bits(wts)) and torch.equal(im.vecs, vecs)


def test_tile_encoder_pack_is_the_headers_layout():
    te = _encoder()
    wts, vecs = nn_kernels.tile_encoder_pack(te)
    L = _lib.lib()
    assert wts.dtype == BF and wts.numel() == L.catan_tile_encoder_weight_elems() == W_TAIL + 32 * 64
    assert vecs.dtype == torch.float32 and vecs.numel() == L.catan_tile_encoder_vec_elems() == V_TAIL + 3 * 32
    l0, l1 = te.encoder_layers
    k1 = l1.multi_headed_attention.qkv_nets[1]
    with torch.no_grad():
        # spot elements
        assert wts[17 * 64 + 41] == te.first_layer.weight[17, 41].to(BF)
        assert wts[W_FIRST + W_LAYER + W_QKV + (64 + 9) * 64 + 33] == k1.weight[9, 33].to(BF)              # layer 1, K's rows of the 192 x 64 block
        assert wts[W_FIRST + W_L2 + 50 * 128 + 101] == l0.pointwise_net.linear2.weight[50, 101].to(BF)      # layer 0, linear2 64 x 128
        assert wts[W_TAIL + 24 * 64 + 63] == te.out_proj.weight[24, 63].to(BF)
        # whole blocks, so that the spot checks are not the only tie
        assert torch.equal(wts[:W_FIRST].view(64, 64)[:, :60], te.first_layer.weight.to(BF))
        assert torch.equal(wts[W_FIRST + W_LAYER + W_L1:W_FIRST + W_LAYER + W_L2].view(128, 64), l1.pointwise_net.linear1.weight.to(BF))
        assert torch.equal(wts[W_FIRST + W_OUT:W_FIRST + W_L1].view(64, 64), l0.multi_headed_attention.out_proj_net.weight.to(BF))
        # the padding is zero
        assert bool((wts[:W_FIRST].view(64, 64)[:, 60:] == 0).all())
        assert bool((wts[W_TAIL:].view(32, 64)[25:] == 0).all())
        for k in range(3):
            assert bool((vecs[V_TAIL + 32 * k + 25:V_TAIL + 32 * k + 32] == 0).all()), k
            assert bool((vecs[V_TAIL + 32 * k:V_TAIL + 32 * k + 25] != 0).all()), k
        # a Linear bias is rounded to bf16, a LayerNorm vector is exact
        b1 = l1.pointwise_net.linear1.bias
        assert bool((b1 != b1.to(BF).float()).any())
        assert torch.equal(vecs[V_HEAD + V_LAYER + V_B1:V_HEAD + V_LAYER + V_B1 + 128], b1.to(BF).float())
        assert torch.equal(vecs[:64], te.first_layer.bias.to(BF).float())
        bqkv = torch.cat([n.bias for n in l0.multi_headed_attention.qkv_nets])
        assert torch.equal(vecs[V_HEAD + V_BQKV:V_HEAD + V_BQKV + 192], bqkv.to(BF).float())
        assert torch.equal(vecs[V_TAIL:V_TAIL + 25], te.out_proj.bias.to(BF).float())
        ln = l1.sublayers[1].norm
        assert bool((ln.weight != ln.weight.to(BF).float()).any())
        assert torch.equal(vecs[V_HEAD + V_LAYER + V_LN2W:V_HEAD + V_LAYER + V_LN2W + 64], ln.weight)
        assert torch.equal(vecs[V_HEAD + V_LAYER + V_LN2B:V_HEAD + V_LAYER + V_LN2B + 64], ln.bias)
        assert torch.equal(vecs[V_HEAD + V_LN1W:V_HEAD + V_LN1W + 64], l0.sublayers[0].norm.weight)
        assert torch.equal(vecs[64:128], te.norm_2.weight) and torch.equal(vecs[128:192], te.norm_2.bias)
        assert torch.equal(vecs[V_TAIL + 32:V_TAIL + 57], te.norm.weight) and torch.equal(vecs[V_TAIL + 64:V_TAIL + 89], te.norm.bias)


def test_te_images_are_the_pack_and_follow_the_parameters():
    te = _encoder()
    im = nn_kernels._TeImages(te).current()
    wts, vecs = nn_kernels.tile_encoder_pack(te)
    assert torch.equal(_bits(im.wts), _bits(wts)) and torch.equal(im.vecs, vecs)

    def transposed(*mods):
        return torch.cat([m.weight.detach() for m in mods], 0).to(BF).t()

    def transposes_hold():
        for l, layer in enumerate(te.encoder_layers):
            mha, ffn = layer.multi_headed_attention, layer.pointwise_net
            for got, want in ((im.w2t[l], transposed(ffn.linear2)), (im.w1t[l], transposed(ffn.linear1)), (im.wot[l], transposed(mha.out_proj_net)),
                              (im.wqt[l], transposed(*mha.qkv_nets))):
                assert got.is_contiguous() and torch.equal(_bits(got), _bits(want.contiguous())), l
        assert torch.equal(_bits(im.wpt), _bits(transposed(te.out_proj).contiguous()))

    transposes_hold()
    ptrs = wts.data_ptr(), vecs.data_ptr()
    before = wts.clone(), vecs.clone()
    changed = (te.encoder_layers[1].pointwise_net.linear2.weight, te.encoder_layers[0].multi_headed_attention.out_proj_net.bias, te.norm.weight)
    with torch.no_grad():
        for p in changed:
            p.mul_(1.25)
    im.current()
    wts2, vecs2 = nn_kernels.tile_encoder_pack(te)
    assert (wts2.data_ptr(), vecs2.data_ptr()) == ptrs and wts2 is wts and vecs2 is vecs
    assert not torch.equal(_bits(wts2), _bits(before[0])) and not torch.equal(vecs2, before[1])
    with torch.no_grad():
        assert torch.equal(wts2[W_FIRST + W_LAYER + W_L2:W_FIRST + 2 * W_LAYER].view(64, 128), changed[0].to(BF))
        assert torch.equal(vecs2[V_HEAD + V_BO:V_HEAD + V_BO + 64], changed[1].to(BF).float())
        assert torch.equal(vecs2[V_TAIL + 32:V_TAIL + 57], changed[2])
    assert torch.equal(_bits(im.wts), _bits(wts2)) and torch.equal(im.vecs, vecs2)
    transposes_hold()


def test_te_images_survive_the_registry_starting_over(monkeypatch):
    """an encoder registers some sixty images: with room for ten the registry starts over several times while they are being registered"""
    monkeypatch.setattr(nn_kernels.weight_images, "MAX_ENTRIES", 10)
    te = _encoder()
    im = nn_kernels._te_images(te)
    assert len(im.entries) > 10 and len(nn_kernels.weight_images.entries) <= 10
    assert _same_as_pack(im, te) and nn_kernels._te_images(te) is im
    nn_kernels.weight_images.clear()
    im2 = nn_kernels._te_images(te)
    assert im2 is not im and im2.wts.data_ptr() != im.wts.data_ptr()
    assert _same_as_pack(im2, te) and torch.equal(_bits(im2.wqt[1]), _bits(im.wqt[1]))


def test_cached_pack_hits_rebuilds_and_keeps_addresses():
    p, q = torch.nn.Parameter(torch.arange(6.0)), torch.nn.Parameter(torch.ones(3))
    calls = []

    def build():
        calls.append(1)
        return p.detach() * 2, q.detach() + 1

    e0 = nn_kernels._cached_pack(None, [p, q], build, extra=(7,))
    assert len(calls) == 1 and len(e0) == 3 and torch.equal(e0[1], torch.arange(6.0) * 2)
    e1 = nn_kernels._cached_pack(e0, [p, q], build, extra=(7,))
    assert e1 is e0 and len(calls) == 1                                   # a hit: the entry itself, the builder not called
    with torch.no_grad():
        q.add_(1)
    e2 = nn_kernels._cached_pack(e1, [p, q], build, extra=(7,))
    assert len(calls) == 2 and e2[0] != e0[0]
    assert e2[1] is e0[1] and e2[2] is e0[2] and torch.equal(e2[2], torch.full((3,), 3.0))     # the same tensors, the new values
    e3 = nn_kernels._cached_pack(e2, [p, q], build, extra=(8,))            # the extra field is part of the stamp
    assert len(calls) == 3 and e3[1] is e0[1]
    assert nn_kernels._cached_pack(e3, [p, q], build, extra=(8,)) is e3 and len(calls) == 3


def test_refresh_packs_refreshes_what_exists_and_builds_nothing():
    ahm = H.chain_heads()
    heads = ahm.action_heads
    nn_kernels.refresh_packs(ahm)
    assert not any(hasattr(m, "_fused_pack") or hasattr(m, "_custom_pack") for m in ahm.modules())
    packed = (1, 7)
    old = {i: nn_kernels.head_pack(heads[i], ahm.D) for i in packed}
    old_custom = nn_kernels.head5_custom_pack(heads[5])
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in ahm.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    for i in packed:                                                      # (stale now)
        assert not torch.equal(_bits(old[i][0]), _bits(H.pack_module(heads[i], ahm.D)[0]))
    nn_kernels.refresh_packs(ahm)
    for i in packed:
        w, v = heads[i]._fused_pack[1:]
        w_ref, v_ref = H.pack_module(heads[i], ahm.D)
        assert w is old[i][0] and v is old[i][1]
        assert torch.equal(_bits(w), _bits(w_ref)) and torch.equal(v, v_ref), i
        assert nn_kernels.head_pack(heads[i], ahm.D)[0] is w
    assert heads[5]._custom_pack[1] is old_custom and torch.equal(old_custom, H.custom_pack_module(heads[5]))
    assert [i for i, h in enumerate(heads) if hasattr(h, "_fused_pack")] == list(packed)
    assert [i for i, h in enumerate(heads) if hasattr(h, "_custom_pack")] == [5]
