"""CPU: tests/card_summary_reference.py against itself and against the package, before tests/test_gpu_card_summary_fp64.py relies on it.
The class form equals the per-token reference; the per-token reference equals policy._card_summary's torch branch in double; the pattern
number, the pattern lists, the launch table, the depths and the hash facts are what csrc/catan_nn.hip and csrc/catan_abi_nn.h say; the
rule refuses every planted error and accepts the yardstick."""
import pytest
import torch

import card_summary_reference as CS
import pin_rule as PR

ROWS = 240
NONE7 = (None,) * 7


def _cases():
    """every regime on every list kind (pitch 25, 32 and 8 in turn) -> (name, params, ids, lens, dout)"""
    out = []
    for i, regime in enumerate(CS.REGIMES):
        p, _ = CS.make_params(regime, seed=i)
        for j, kind in enumerate(CS.LIST_KINDS + ("mixed",)):
            pitch = (25, 32, 8)[(i + j) % 3]
            ids, lens = CS.make_lists(kind, ROWS, pitch, seed=j)
            out.append((f"{regime} {kind} pitch={pitch}", p, ids, lens, CS.make_dout(ROWS, seed=j)))
    ids, lens = CS.pattern_lists(live_padding_seed=5)
    out.append(("unit patterns", CS.make_params("unit", 3)[0], ids.long(), lens.long(), CS.make_dout(CS.PATTERNS, seed=9)))
    return out


@pytest.fixture(scope="module")
def cases():
    res = []
    for name, p, ids, lens, d in _cases():
        res.append({"name": name, "params": p, "ids": ids, "lens": lens, "dout": d,
                    "tok": CS.card_ref_tokens(ids, lens, *NONE7, CS.EPS, d, params=p),
                    "cls": CS.card_ref_classes(ids, lens, p, CS.EPS, d),
                    "yard": CS.card_yardstick(ids, lens, p, CS.EPS, d)})
    return res


def test_class_form_equals_the_token_reference(cases):
    """values and all 544 gradients to 1e-12 relative, on every list kind in every regime"""
    for c in cases:
        t, k = c["tok"], c["cls"]
        for n in ("out", "dparams"):
            scale = float(t[n].abs().max())
            assert float((t[n] - k[n]).abs().max()) <= 1e-12 * scale, (c["name"], n)
        assert bool((k["abs_terms"] >= k["dparams"].abs() * (1 - 1e-12)).all()), c["name"]
        empty = c["lens"] == 0
        assert not bool(t["out"][empty].any()), (c["name"], "an empty list's row is not zero")


def test_empty_lists_have_no_gradient():
    p, _ = CS.make_params("unit", 1)
    ids, _ = CS.make_lists("arbitrary", 50, 25, 2)
    t = CS.card_ref_tokens(ids, torch.zeros(50, dtype=torch.long), *NONE7, CS.EPS, CS.make_dout(50), params=p)
    assert not bool(t["out"].any()) and not bool(t["dparams"].any())


def test_token_reference_equals_the_package_in_double():
    """policy._card_summary's torch branch on a double module; lists of length >= 1 (the net never passes an empty one).  The block
    built from the weights is nn_kernels.card_summary_params' block, and the weights' gradients come through it."""
    from settlers_of_catan_rl_amd import nn_kernels, policy
    torch.manual_seed(3)
    emb = torch.nn.Embedding(CS.VOCAB, CS.WIDTH).double()
    mha = policy._MHA(CS.WIDTH, CS.HEADS).double()
    norm = torch.nn.LayerNorm(CS.WIDTH).double()
    with torch.no_grad():
        for q in list(mha.parameters()) + list(norm.parameters()):
            q.add_(torch.randn_like(q) * 0.1)
    w = (emb.weight, torch.cat([n.weight for n in mha.qkv_nets], 0), torch.cat([n.bias for n in mha.qkv_nets], 0), mha.out_proj_net.weight,
         mha.out_proj_net.bias, norm.weight, norm.bias)
    block = nn_kernels.card_summary_params(emb, mha, norm)
    assert block.shape == (CS.NPAR,)
    assert float((block.detach().double() - CS.params_from_weights(*[t.detach() for t in w])).abs().max()) <= 1e-6     # (card_summary_params is fp32)
    for pitch in (25, 8):
        ids, lens = CS.make_lists("mixed", ROWS, pitch, 4)
        lens = lens.clamp(min=1, max=pitch)
        d = CS.make_dout(ROWS, 4).double()
        for q in list(emb.parameters()) + list(mha.parameters()) + list(norm.parameters()):
            q.grad = None
        out = policy._card_summary(ids, lens, emb, mha, norm)
        assert out.dtype == torch.float64
        (out * d).sum().backward()
        t = CS.card_ref_tokens(ids, lens, *w, norm.eps, d)
        assert float((out.detach() - t["out"]).abs().max()) <= 1e-12 * float(t["out"].abs().max())
        got = [emb.weight.grad, torch.cat([n.weight.grad for n in mha.qkv_nets], 0), torch.cat([n.bias.grad for n in mha.qkv_nets], 0),
               mha.out_proj_net.weight.grad, mha.out_proj_net.bias.grad, norm.weight.grad, norm.bias.grad]
        for a, b in zip(got, t["dweights"]):
            assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


def test_pattern_number_and_lists():
    cnt = CS.pattern_counts()
    k = torch.arange(CS.PATTERNS)
    assert torch.equal(CS.pattern_of(cnt), k)                                   # the header's formula, inverted, on all 4 860
    assert int(cnt.sum(1).max()) == 26 and int((cnt.sum(1) > 25).sum()) == 1
    for i, lim in enumerate(CS.DECK):
        over = cnt.clone()
        over[:, i] = lim + 1
        assert bool((CS.pattern_of(over) == -1).all())
    ids, lens = CS.pattern_lists()
    assert ids.dtype == torch.int8 and lens.dtype == torch.int32 and ids.shape == (CS.PATTERNS, 25)
    back = CS.pattern_of(CS.counts(ids, lens))
    wrong = (back != k).nonzero().flatten().tolist()
    assert wrong == [CS.PATTERNS - 1], wrong                                    # the 26-card pattern, cut to 25 ids, is the one below it in c5
    assert int(back[-1]) == CS.PATTERNS - 1 - 1620 and int(lens[-1]) == 25
    live, lens2 = CS.pattern_lists(live_padding_seed=1)
    assert torch.equal(lens, lens2) and torch.equal(CS.counts(live, lens2), CS.counts(ids, lens))
    valid = torch.arange(25)[None] < lens[:, None]
    assert bool((live[~valid] >= 1).all()) and bool((ids[~valid] == 0).all())
    # the package's own lists
    from settlers_of_catan_rl_amd import nn_kernels
    pid, plen = nn_kernels._pattern_lists(torch.device("cpu"))                  # (asks the built library for the pattern count only)
    assert torch.equal(pid, ids) and torch.equal(plen, lens)


def test_case_lists_keep_live_ids_behind_lens():
    for kind in CS.LIST_KINDS + ("mixed",):
        for pitch in (25, 32, 8):
            ids, lens = CS.make_lists(kind, 600, pitch, 1)
            behind = torch.arange(pitch)[None] >= lens.clamp(max=25)[:, None]
            assert bool((ids[behind] >= 1).all()) and bool((ids <= 5).all()) and bool((ids >= 0).all())
            assert int(lens.max()) <= max(pitch, 30 if pitch >= 25 else pitch)
            if pitch < 25:
                assert int(lens.max()) <= pitch
    ids, lens = CS.make_lists("edge", 600, 32, 1)
    assert set(lens.tolist()) == {0, 1, 2, 24, 25, 30}
    ids, lens = CS.make_lists("deck", 600, 25, 1)
    assert bool((CS.pattern_of(CS.counts(ids, lens)) >= 0).all())
    ids, lens = CS.make_lists("arbitrary", 600, 25, 1)
    assert float((CS.pattern_of(CS.counts(ids, lens)) < 0).float().mean()) > 0.5
    ids, lens = CS.make_lists("single", 600, 25, 1)
    c = CS.counts(ids, lens)
    assert bool(((c > 0).sum(1) == 1).all()) and set(c.max(1).values.tolist()) == set(range(1, 26))


def test_launch_table_and_depths():
    """hand-computed from catan_card_summary_bwd's host rule and k_card_pattern_sum's constants"""
    want = {1: (1, 1, 1, (6, 7), 18), 256: (1, 1, 1, (6, 7), 18), 4860: (1, 19, 19, (114, 7), 126), 65535: (1, 256, 256, (1536, 7), 1548),
            65536: (4, 64, 0, (64, 7), 99), 66561: (4, 66, 0, (66, 7), 101)}
    for rows, (rpl, nb, rb, grid, depth) in want.items():
        la = CS.bwd_launch(rows)
        assert (la["rpl"], la["nb"], la["row_blocks"], la["grid"]) == (rpl, nb, rb, grid), rows
        assert CS.bwd_depth(rows) == depth, rows
    assert (CS.SUM_ROWS, CS.SUM_SLOTS, CS.SUM_PROBES) == (1024, 512, 16)
    for rows, reps, depth in ((1, 1, 2), (256, 1, 257), (4860, 1, 1029), (4860, 3, 1026), (65535, 8, 1032), (65536, 8, 1032), (66561, 8, 1033), (66561, 1, 1090)):
        assert CS.sum_depth(rows, reps) == depth, (rows, reps)
    assert CS.sum_depth(2049, 8, shared=3) == 4
    assert CS.sum_launch(2049, 8)["copy_of"] == [0, 1, 2] and CS.sum_launch(2049, 3)["copy_of"] == [0, 1, 2] and CS.sum_launch(2049, 1)["copy_of"] == [0, 0, 0]


def test_hash_facts():
    assert CS.hash_slot(0) == 0 and CS.hash_slot(1) == 2654435761 >> 23 and CS.hash_slot(3) == ((3 * 2654435761) % 2 ** 32) >> 23
    k = torch.arange(CS.PATTERNS)
    s = CS.hash_slot(k)
    assert int(s.min()) >= 0 and int(s.max()) < CS.SUM_SLOTS
    assert [int(x) for x in s[:5]] == [CS.hash_slot(i) for i in range(5)]
    # 1 024 distinct keys on 512 slots: at least 512 rows of the workgroup go to global memory
    first = torch.arange(1024)
    assert first.unique().numel() == 1024
    assert CS.provable_fallback_rows(first) >= 512
    # keys whose first slot lies in one window of 8 reach 8 + 15 = 23 slots
    w = CS.window_keys(6, 8)
    assert w.numel() == 78 and w.unique().numel() == 78
    assert bool(((s[w] >= 6) & (s[w] < 14)).all())
    assert CS.provable_fallback_rows(w) == 78 - 23
    assert CS.provable_fallback_rows(w.repeat(14)[:1024]) >= (78 - 23) * 13
    # few keys: nothing is provable
    assert CS.provable_fallback_rows(torch.arange(1024) % 5) == 0
    assert CS.provable_fallback_rows(torch.full((1024,), -1)) == 0


def _judged(c, yard):
    """the rules with `yard` in the kernel's place -> accepted?"""
    ok, _, _, _ = CS.accept_out(yard["out"], c["tok"]["out"], c["yard"]["out"])
    oks, _, _ = CS.per_list(yard["out"], c["tok"]["out"], c["yard"]["out"])
    okp, _, _ = PR.accept_sum(yard["dparams"], torch.zeros(CS.NPAR), c["tok"]["dparams"], c["yard"]["dparams"], c["cls"]["abs_terms"],
                                 CS.bwd_depth(c["ids"].shape[0]))
    return ok and bool(oks.all()) and bool(okp.all())


def test_rule_accepts_the_yardstick_and_refuses_every_plant(cases):
    for c in cases:
        assert _judged(c, c["yard"]), c["name"]
    for plant in CS.PLANTS:
        if plant in ("radix_c2_5", "replica_dropped"):
            continue
        refused = [c["name"] for c in cases if not _judged(c, CS.card_yardstick(c["ids"], c["lens"], c["params"], CS.EPS, c["dout"], plant=plant))]
        print(f"CARD-PLANT {plant}: refused on {len(refused)} of {len(cases)} cases")
        assert refused, plant
    # the pattern number: exact comparison
    cnt = CS.pattern_counts()
    assert not torch.equal(CS.pattern_of(cnt, plant="radix_c2_5"), CS.pattern_of(cnt))
    ids, lens = CS.make_lists("deck", 600, 25, 1)
    cnt = CS.counts(ids, lens)
    assert not torch.equal(CS.pattern_of(cnt, plant="radix_c2_5"), CS.pattern_of(cnt))
    # the copies of the pattern sum: exact in the exact regime
    # (an identity where the last copy is empty - fewer workgroups than copies, e.g. 2 049 rows on 8 copies - or the only one: the
    #  GPU file therefore also runs 8 193 rows, nine workgroups, on 8 copies)
    for rows, reps, shows in ((2049, 3, True), (8193, 8, True), (2049, 8, False), (1025, 1, False)):
        keys = torch.arange(rows) % 7
        d = CS.make_dout(rows, 1, exact=True)
        _, good, _, _ = CS.pattern_sum_ref(keys, d, reps)
        _, bad, _, _ = CS.pattern_sum_ref(keys, d, reps, plant="replica_dropped")
        assert torch.equal(good, bad) != shows, (rows, reps)


def test_pattern_sum_reference():
    keys = torch.tensor([0, 5, -1, 5, 4859, -1] * 400)
    d = CS.make_dout(keys.numel(), 3, exact=True)
    copies, total, ab, unk = CS.pattern_sum_ref(keys, d, 8)
    assert unk == 800 and copies.shape == (8, CS.PATTERNS, 16)
    assert not bool(copies[3:].any())                           # 2 400 rows: three workgroups, copies 0..2
    want = torch.zeros(CS.PATTERNS, 16, dtype=torch.float64)
    for r in range(keys.numel()):
        if keys[r] >= 0:
            want[keys[r]] += d[r].double()
    assert torch.equal(total, want)
    assert torch.equal(copies[1].sum(0), d[1024:2048][keys[1024:2048] >= 0].double().sum(0))
