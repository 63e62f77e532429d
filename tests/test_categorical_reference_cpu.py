"""CPU: tests/categorical_reference.py itself - the fp64 reference against torch.distributions.Categorical, against the torch formulation
of policy._categorical and against autograd; the bits unpack against rollout.pack_action_masks (the env's packed format); the acceptance
rule against planted errors; the launch tables; and the share of rows on which the sampler's bracket rule could not decide.
tests/test_gpu_categorical_fp64.py holds the kernels to this reference.

Rejection: every planted error (categorical_reference.PLANTS) is computed as the yardstick is - fp32 - so it is what a kernel with that
one error would return, and categorical_reference.judge must refuse it in the case named in REJECTED_IN.  `cdf_ge`, `no_max`,
`argmax_illegal` (wide) and `ent_all` (neginf) are refused at ONE row: those regimes plant what is needed in row 0.  `fall_last` needs a
drawn u above 0.5 (row 0's u is the planted 0) and the three bits plants need a row on the far side of a segment boundary or a mask that
the AND range changes, which the draw produces: they are refused at 255 / 257 rows, the smallest counts of the launch table above 1."""
import pytest
import torch

import categorical_reference as CR


def _logmask(c):
    return c["logits"].double() + torch.log(c["mask"].double())


@pytest.mark.parametrize("regime", ["unit", "wide", "single", "all_legal", "ties", "neginf"])
@pytest.mark.parametrize("K", [1, 2, 13, 73])
def test_reference_matches_torch_categorical_in_double(regime, K):
    c = CR.make_case(regime, 67, K, seed=3)
    d = torch.distributions.Categorical(logits=_logmask(c))
    ref = CR.cat_ref(c["logits"], c["mask"], "given_legal", c["given_legal"])
    assert torch.equal(torch.isinf(ref["logp_all"]), torch.isinf(d.logits))
    fin = torch.isfinite(d.logits)
    assert float((ref["logp_all"][fin] - d.logits[fin]).abs().max()) <= 1e-12 * max(1.0, float(d.logits[fin].abs().max()))
    assert float((ref["p"] - d.probs).abs().max()) <= 1e-14
    assert float((ref["entropy"] - d.entropy()).abs().max()) <= 1e-12
    lp = d.log_prob(c["given_legal"])
    fin = torch.isfinite(lp)                                          # (neginf: a legal column at -inf may be the given one)
    assert torch.equal(ref["logp"][~fin], lp[~fin])
    assert float((ref["logp"][fin] - lp[fin]).abs().max()) <= 1e-12 * max(1.0, float(lp[fin].abs().max()))
    assert float((ref["lse"] - torch.logsumexp(_logmask(c), -1)).abs().max()) <= 1e-12 * max(1.0, float(ref["lse"].abs().max()))
    assert float((ref["cdf"][:, -1] - 1.0).abs().max()) <= 1e-13
    # an illegal given action: -inf
    ref = CR.cat_ref(c["logits"], c["mask"], "given_illegal", c["given_illegal"])
    assert bool((ref["logp"][c["has_illegal"]] == float("-inf")).all())
    if regime == "single":
        ref = CR.cat_ref(c["logits"], c["mask"], "given_legal", c["given_legal"], None, c["dlogp"], c["dent"])
        assert not bool(ref["logp"].any()) and not bool(ref["entropy"].any()) and not bool(ref["dlogits"].any())
        assert torch.equal(ref["lse"], c["logits"].double().gather(1, c["given_legal"][:, None]).squeeze(1))


@pytest.mark.parametrize("regime", ["unit", "all_legal", "ties", "wide"])
@pytest.mark.parametrize("K", [2, 13, 73])
def test_closed_form_gradient_matches_autograd(regime, K):
    c = CR.make_case(regime, 67, K, seed=4)
    z = c["logits"].double().requires_grad_(True)
    lp_all = torch.log_softmax(z + torch.log(c["mask"].double()), -1)
    p = lp_all.exp()
    ent = -(p * torch.where(p > 0, lp_all, torch.zeros_like(lp_all))).sum(-1)
    lp = lp_all.gather(1, c["given_legal"][:, None]).squeeze(1)
    (want,) = torch.autograd.grad((lp * c["dlogp"].double() + ent * c["dent"].double()).sum(), z)
    ref = CR.cat_ref(c["logits"], c["mask"], "given_legal", c["given_legal"], None, c["dlogp"], c["dent"])
    assert float((ref["dlogits"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("regime", ["unit", "ties", "all_legal", "single"])
@pytest.mark.parametrize("K", [1, 5, 54])
def test_reference_matches_the_torch_formulation_of_the_policy(regime, K):
    from settlers_of_catan_rl_amd import policy
    c = CR.make_case(regime, 67, K, seed=5)
    z = c["logits"].double()
    assert not z.is_cuda                                              # (on the CPU policy._categorical takes its torch formulation)
    a, lp, ent = policy._categorical(z, c["mask"].double(), c["given_legal"], False, None)
    ref = CR.cat_ref(c["logits"], c["mask"], "given_legal", c["given_legal"])
    assert torch.equal(a, ref["action"]) and float((lp - ref["logp"]).abs().max()) <= 1e-12 and float((ent - ref["entropy"]).abs().max()) <= 1e-12
    a, lp, ent = policy._categorical(z, c["mask"].double(), None, True, None)
    ref = CR.cat_ref(c["logits"], c["mask"], "argmax")
    assert torch.equal(a, ref["action"]) and float((lp - ref["logp"]).abs().max()) <= 1e-12
    if regime == "ties":
        best = torch.where(c["mask"] > 0, c["logits"], torch.full_like(c["logits"], float("-inf"))).max(1, keepdim=True).values
        tied = ((c["logits"] == best) & (c["mask"] > 0)).sum(1)
        assert float((tied > 1).float().mean()) > 0.3 or K < 5


def test_sampling_rule_of_the_reference():
    """the inverse-CDF pick against a plain loop: the first legal k with cdf_k > u, else the last legal column; u = 0 and the largest
    float below 1 are among the draws"""
    for regime in ("unit", "wide", "neginf", "empty"):
        c = CR.make_case(regime, 67, 13, seed=6)
        o = CR.cat_ref(c["logits"], c["mask"], "sampled", None, c["u"])
        assert bool((c["u"] == 0).any()) and bool((c["u"] == CR.U_TOP).any())
        for r in range(67):
            pick, last, cdf = -1, 0, 0.0
            for k in range(13):
                if c["mask"][r, k] > 0:
                    cdf += float(o["p"][r, k])
                    last = k
                    if pick < 0 and cdf > float(c["u"][r]):
                        pick = k
            assert int(o["action"][r]) == (pick if pick >= 0 else last)
        legal = o["legal"].any(1)
        ok, _ = CR.bracket_ok(o, CR.cat_yardstick(c["logits"], c["mask"], "sampled", None, c["u"]), o["action"], c["u"])
        assert bool(ok[legal].all())
        # u = 0: fp64 resolves probabilities no fp32 evaluation can, so first_ok is asked of the yardstick's pick, not of the reference's
        y = CR.cat_yardstick(c["logits"], c["mask"], "sampled", None, c["u"])
        assert bool(CR.first_ok(o, y["action"])[legal & (c["u"] == 0)].all())


def test_bits_unpack_matches_the_env_packing():
    from settlers_of_catan_rl_amd import rollout, spec
    assert spec.MASK_PACKED_WORDS == CR.PITCH and spec.MASK_WORDS == CR.MASK_LD
    g = torch.Generator().manual_seed(8)
    dense = (torch.rand(41, spec.MASK_WORDS, generator=g) < 0.5).float()
    packed = rollout.pack_action_masks(dense)
    wide = torch.zeros(41, 32 * CR.PITCH)
    wide[:, :spec.MASK_WORDS] = dense
    assert torch.equal(packed, CR.pack_bits(wide))
    idx = torch.randint(0, 41, (90,), generator=g)
    for K in CR.KS:
        (o0, a0), (o1, a1), _ = CR.BITS_SEGS[K]
        if o0 + K > spec.MASK_WORDS or o1 + K > spec.MASK_WORDS or a1 + K > spec.MASK_WORDS:
            continue
        segs = [30, 60, o0, a0, o1, a1, o0, a1]
        m = CR.bits_mask(packed, idx, segs, 90, K)
        want = torch.cat((dense[idx[:30], o0:o0 + K],
                          dense[idx[30:60], o1:o1 + K] * (dense[idx[30:60], a1:a1 + K] if a1 >= 0 else 1.0),
                          dense[idx[60:], o0:o0 + K] * (dense[idx[60:], a1:a1 + K] if a1 >= 0 else 1.0)))
        assert torch.equal(m, want), K
        assert torch.equal(CR.bits_mask(packed, None, [0, 0, 0, -1, 0, -1, o0, -1], 41, K), dense[:, o0:o0 + K])


def test_bits_cases_are_what_they_claim():
    for K in CR.KS:
        segs = CR.BITS_SEGS[K]
        assert segs[2][0] + K == 32 * CR.PITCH and all(o >= 0 and o + K <= 32 * CR.PITCH and a + K <= 32 * CR.PITCH for o, a in segs)
        assert [a >= 0 for _, a in segs] in ([False, True, False], [False, False, False])
        assert segs[0][0] == CR.window_off(K) and CR.window_off(K) + K <= CR.MASK_LD
        cases = CR.bits_cases(K)
        assert {(B, nn, wi) for B, nn, wi, _, _ in cases} == {(B, nn, wi) for B in CR.ROWS for nn in CR.seg_layouts(B) for wi in (False, True)}
        assert {ld for _, _, _, ld, _ in cases} == set(CR.GIVEN_LDS)
    assert any(a >= 0 for K in CR.KS for _, a in CR.BITS_SEGS[K])
    assert (13 >> 5) != ((13 + 54 - 1) >> 5)                           # offset 13 with K = 54 crosses words
    assert {reg for K in CR.KS for *_, reg in CR.bits_cases(K)} == set(CR.BITS_REGIMES)
    assert set(CR.seg_layouts(4097)) == {(0, 0), (0, 4097), (4097, 4097), (255, 257), (256, 256), (1, 4096)}
    c = CR.make_bits_case("unit", 257, 5, (255, 257), True, 18)
    assert c["rows_idx"].unique().numel() < 257 and bool(c["mask"].sum(1).min() >= 1) and c["packed"].shape[1] == CR.PITCH
    c = CR.make_bits_case("empty", 257, 5, (255, 257), False, 1)
    assert not bool(c["mask"][::CR.EMPTY_EVERY].any())


def _planted_got(c, mode, plant, mask=None):
    given = c[mode] if mode.startswith("given") else None
    o = CR.cat_yardstick(c["logits"], c["mask"] if mask is None else mask, mode, given, c["u"], plant=plant)
    a = o["action"]
    o = CR.cat_yardstick(c["logits"], c["mask"] if mask is None else mask, "given", a, None, c["dlogp"], c["dent"], plant=plant)
    return {k: o[k] for k in ("action", "logp", "entropy", "lse", "dlogits")}


# plant -> (regime, mode, row counts, the K it must be refused at, an output that must refuse it)
_K2 = [K for K in CR.KS if K >= 2]
REJECTED_IN = {
    "ent_all": ("neginf", "given_legal", (1, 255, 257), _K2, "entropy"),  # 0 * -inf = NaN (row 0: its last legal logit is -inf)
    "cdf_ge": ("wide", "sampled", (1, 255, 257), _K2, "action"),          # u = 0: a first legal column of probability 0
    "fall_last": ("unit", "sampled", (255, 257), [K for K in CR.KS if K >= 3], "action"),      # drawn u above 0.5: the last legal column
    "argmax_illegal": ("wide", "argmax", (1, 255, 257), [K for K in CR.KS if K >= 3], "action"),  # row 0: the illegal column 1 is the largest
    "no_max": ("wide", "given_legal", (1, 255, 257), CR.KS, "lse"),       # row 0: exp(120 + ..) is inf
}


@pytest.mark.parametrize("plant", sorted(REJECTED_IN))
def test_rule_rejects_planted_error(plant):
    regime, mode, rows, Ks, must = REJECTED_IN[plant]
    for K in Ks:
        for B in rows:
            c = CR.make_case(regime, B, K)
            clean, _ = CR.judge(c, mode, _planted_got(c, mode, None))
            assert not clean, ("the yardstick fails its own rule", regime, B, K, clean)
            bad, _ = CR.judge(c, mode, _planted_got(c, mode, plant))
            refused = sorted({b[0] for b in bad})
            print(f"CAT-PLANT {plant} {regime} {mode} B={B} K={K}: refused on {refused}")
            assert must in refused, (plant, B, K, refused)


# bits plants -> ((n0, n1) layouts at 257 rows, the K it must be refused at)
BITS_REJECTED_IN = {
    "and_ignored": (((0, 257), (255, 257), (1, 256)), [K for K in CR.KS if CR.BITS_SEGS[K][1][1] >= 0]),
    "seg_le": (((255, 257), (256, 256), (1, 256)), [K for K in CR.KS if K >= 5]),
    "bit_off": (((0, 0), (257, 257), (255, 257)), [K for K in CR.KS if K >= 5]),
}


@pytest.mark.parametrize("plant", sorted(BITS_REJECTED_IN))
def test_rule_rejects_planted_bits_error(plant):
    layouts, Ks = BITS_REJECTED_IN[plant]
    for K in Ks:
        for n0n1 in layouts:
            for with_idx in (False, True):
                c = CR.make_bits_case("unit", 257, K, n0n1, with_idx, 1)
                planted = CR.bits_mask(c["packed"], c["rows_idx"], c["segs"], 257, K, plant=plant)
                assert not CR.judge(c, "given_legal", _planted_got(c, "given_legal", None))[0]
                bad, _ = CR.judge(c, "given_legal", _planted_got(c, "given_legal", None, mask=planted))
                print(f"CAT-PLANT {plant} B=257 K={K} {n0n1} idx={with_idx}: refused on {sorted({b[0] for b in bad})}")
                assert bad, (plant, K, n0n1, with_idx)


def test_every_plant_has_a_rejection_case():
    assert set(REJECTED_IN) | set(BITS_REJECTED_IN) == set(CR.PLANTS)


def test_launch_tables():
    """the row counts sit on both sides of the block edge, and the case builders plant what they say"""
    assert CR.BLOCK == 256 and {255, 256, 257} <= set(CR.ROWS) and 1 in CR.ROWS and max(CR.ROWS) == 4097 and 4097 % 256 == 1
    assert [-(-B // CR.BLOCK) for B in CR.ROWS] == [1, 1, 1, 2, 17]
    assert CR.window_off(1) + 1 == CR.MASK_LD and CR.window_off(54) == 13 and CR.window_off(73) == 175
    for K in CR.KS:
        for B in (1, 257):
            for regime in CR.REGIMES:
                c = CR.make_case(regime, B, K)
                n = (c["mask"] > 0).sum(1)
                rows = torch.arange(B)
                if regime == "empty":
                    assert bool((n[rows % CR.EMPTY_EVERY == 0] == 0).all()) and bool((n[rows % CR.EMPTY_EVERY != 0] >= 1).all())
                else:
                    assert bool((n >= 1).all())
                if regime == "single":
                    assert bool((n == 1).all())
                if regime == "all_legal":
                    assert bool((n == K).all())
                if regime == "ties":
                    assert c["logits"].unique().numel() <= 3
                if regime == "neginf":
                    z = torch.where(c["mask"] > 0, c["logits"], torch.zeros_like(c["logits"]))
                    assert bool(torch.isfinite(z).any(1).all()) and (K < 3 or B == 1 or bool(torch.isinf(z).any()))
                legal = c["mask"].gather(1, c["given_legal"][:, None]).squeeze(1) > 0
                assert bool((legal | (n == 0)).all())
                illegal = c["mask"].gather(1, c["given_illegal"][:, None]).squeeze(1) == 0
                assert bool((illegal | ~c["has_illegal"]).all())
                assert bool(((c["given_oor"] < 0) | (c["given_oor"] >= K)).all())
                assert float(c["u"].min()) >= 0.0 and float(c["u"].max()) < 1.0 and float(c["u"][0]) == 0.0
                if regime == "wide" and K >= 2:
                    ref = CR.cat_ref(c["logits"], c["mask"], "argmax")
                    assert float(ref["p"][0, 0]) < CR.P_NEVER and bool(c["mask"][0, 0] > 0)
                    if B > 1:
                        y = CR.cat_yardstick(c["logits"], c["mask"], "argmax")
                        assert float(((y["p"] == 0) & y["legal"]).float().mean()) > 0.01    # p underflows to 0 in fp32


@pytest.mark.parametrize("K", CR.KS)
def test_bracket_rule_is_not_vacuous(K):
    """the share of rows whose u lies within K 2^-20 of an fp64 cdf boundary: under 2 % in the committed cases (0.7 % at most over 20 000
    rows per case when the cases were chosen).  That is the share on which fp32 and fp64 could pick different columns; it is NOT how
    sharply bracket_ok decides - its tau is 2^-9 of cdf mass, wider than many a column at K = 54 or 73."""
    for regime in ("unit", "wide"):
        for B in (257, 4097):
            c = CR.make_case(regime, B, K)
            ref = CR.cat_ref(c["logits"], c["mask"], "sampled", None, c["u"])
            share = CR.near_boundary_share(ref, c["u"])
            print(f"CAT-BRACKET {regime} B={B} K={K}: {share:.4f}")
            assert share < 0.02, (regime, B, K, share)
