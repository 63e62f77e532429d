"""GPU: the dev-card list kernels of csrc/catan_nn.hip (k_card_summary_fwd, k_card_summary_lookup, k_card_summary_bwd on both grid shapes,
k_card_pattern_sum) list by list against fp64, through the C ABI (catan_card_summary_fwd / _lookup / _bwd, catan_card_pattern_sum); only
the two glue tests at the end go through nn_kernels / policy.

reference = tests/card_summary_reference.py (its docstring has the operation and the yardstick's roundings; the rule is tests/pin_rule.py's):
    out       pin_rule.whole(kernel, fp64 per token, yardstick, 2^-17) over the case AND pin_rule.per_group per list
    dparams   per parameter |kernel - (pre-fill + fp64)| <= 2 |yardstick - fp64| + bwd_depth 2^-24 (abs_terms + |pre-fill|)
    dpat      per word |kernel - fp64| <= sum_depth 2^-24 sum |term|; exact where dout holds small integers times 2^-4
    keys      == pattern_of(counts); lookup == forward bit for bit
Nothing in a bound comes from a kernel.  The backward's sums are made by atomics: no two launches agree to the bit, and nothing here asks
them to, outside the cases that must leave the pre-fill untouched.  Every case prints one `CARD` line: per output the kernel's error, the
yardstick's error, their ratio and the largest share of a bound used (out: by the case or by a single list; dparams: by a parameter);
the pattern-sum lines add the rows that provably went to global memory.  profiles/card_summary_kernel_tests.txt is that output.

Buffers: the ids lie in a wider allocation of LIVE ids 1..5 (in front, behind the last row and in the pitch gap, and every position at or
behind a list's length holds one too: read by mistake they change the counts); float inputs are followed by NaN; out, keys and dpat lie
between sentinel margins; dparams is pre-filled with a non-constant pattern, which the backward must add to."""
import pytest
import torch

import card_summary_reference as CS
import guarded as G
import pin_rule as PR
from guarded import NAN, ptr as P, stream as _stream
from pin_rule import same_bits

pytestmark = pytest.mark.gpu

EPS = CS.EPS
GUARD = 64                       # rows behind (and in front of) every buffer
SENTINEL = 0x5A5B5A5B
NONE7 = (None,) * 7
EINVAL = -1


def _check(rc):
    from settlers_of_catan_rl_amd import _lib
    _lib.check(rc)


def _ids_buffer(ids, dtype, strided=False):
    """ids (int64 [rows, pitch], device) inside a wider allocation of live ids -> (hold, view [rows, pitch] of `dtype`, the pitch to pass)"""
    rows, pitch = ids.shape
    g = torch.Generator(device="cuda").manual_seed(rows * 3 + pitch)
    if strided:                                           # the middle third of a three times wider row
        hold = torch.randint(1, CS.VOCAB, (rows + 2 * GUARD, 3 * pitch), device="cuda", generator=g).to(dtype)
        view = hold[GUARD:GUARD + rows, pitch:2 * pitch]
    else:
        hold = torch.randint(1, CS.VOCAB, (rows + 2 * GUARD, pitch), device="cuda", generator=g).to(dtype)
        view = hold[GUARD:GUARD + rows]
    view.copy_(ids)
    assert view.stride(1) == 1
    return hold, view, view.stride(0)


def _float_input(t):
    """t followed by NaN"""
    hold, view = G.guarded_input(t.float(), GUARD * CS.WIDTH)
    return hold, view.view(t.shape)


def _between_sentinels(shape, dtype, fill=None):
    """`shape` elements of a 32-bit `dtype` with GUARD rows of the sentinel in front and behind -> (hold, view)"""
    hold, view = G.sentinel_output(torch.Size(shape).numel(), dtype, GUARD * CS.WIDTH, GUARD * CS.WIDTH, SENTINEL)
    view = view.view(shape)
    if fill is not None:
        view.fill_(fill)
    return hold, view


class _Lists:
    """the device buffers of one list case in one storage: ids (in its allocation), lens int32, params fp32 (NaN behind)"""

    def __init__(self, ids, lens, params, dtype=torch.int8, strided=False):
        self.rows = ids.shape[0]
        self.hold_ids, self.ids, self.pitch = _ids_buffer(ids.cuda(), dtype, strided)
        self.esz = self.ids.element_size()
        self.lens = lens.to(device="cuda", dtype=torch.int32).contiguous()
        self.hold_p, self.params = _float_input(params.cuda().float())


def _fwd(lib, b, want_keys=True, rows=None):
    rows = b.rows if rows is None else rows
    hold_o, out = _between_sentinels((rows, CS.WIDTH), torch.float32)
    hold_k, keys = _between_sentinels((rows,), torch.int32) if want_keys else (None, None)
    _check(lib.catan_card_summary_fwd(P(b.ids), b.esz, b.pitch, P(b.lens), P(b.params), EPS, P(out), P(keys), rows, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hold_o, out), "a write outside out"
    assert keys is None or G.intact(hold_k, keys), "a write outside keys"
    return out.clone(), None if keys is None else keys.clone()


def _lookup(lib, b, table):
    hold_o, out = _between_sentinels((b.rows, CS.WIDTH), torch.float32)
    hold_t, tab = _float_input(table)
    _check(lib.catan_card_summary_lookup(P(b.ids), b.esz, b.pitch, P(b.lens), P(tab), P(b.params), EPS, P(out), b.rows, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hold_o, out), "a write outside out (lookup)"
    return out.clone()


def _bwd(lib, b, dout, only=None, n_unk=None, k=1, into=None):
    """catan_card_summary_bwd alone into a pre-filled dparams (or on into `into`) -> (dparams, the pre-fill)"""
    hold_d, d = _float_input(dout)
    hold_g, g = _between_sentinels((CS.NPAR,), torch.float32)
    g.copy_(G.pattern(CS.NPAR, k) if into is None else into)
    pre = g.clone()
    _check(lib.catan_card_summary_bwd(P(b.ids), b.esz, b.pitch, P(b.lens), P(b.params), EPS, P(d), P(g), P(only), P(n_unk), b.rows, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hold_g, g), "a write outside dparams"
    return g.clone(), pre


def _pattern_sum(lib, keys, dout, replicas, n_unk):
    rows = keys.numel()
    hold_d, d = _float_input(dout)
    hold_p, dpat = _between_sentinels((replicas, CS.PATTERNS, CS.WIDTH), torch.float32, fill=0.0)
    _check(lib.catan_card_pattern_sum(P(keys), P(d), P(dpat), replicas, P(n_unk), rows, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hold_p, dpat), "a write outside dpat"
    return dpat.clone()


# ------------------------------------------------------------------------------------------------------------------- cases, computed once
_MEMO = {}


def _case(regime, kind, rows, pitch, seed=0, grads=True):
    """one list case with its fp64 reference, class form and yardstick, on the device; computed once and left unchanged"""
    key = (regime, kind, rows, pitch, seed, grads)
    if key not in _MEMO:
        p, _ = CS.make_params(regime, seed)
        if kind == "patterns":
            ids, lens = CS.pattern_lists(live_padding_seed=seed + 1)
            ids, lens = ids.long(), lens.long()
            assert (rows, pitch) == tuple(ids.shape)
        else:
            ids, lens = CS.make_lists(kind, rows, pitch, seed)
        ids, lens, p = ids.cuda(), lens.cuda(), p.cuda()
        d = CS.make_dout(rows, seed).cuda() if grads else None
        c = {"regime": regime, "kind": kind, "rows": rows, "pitch": pitch, "params": p, "ids": ids, "lens": lens, "dout": d}
        c.update(_references(ids, lens, p, d))
        _MEMO[key] = c
    return _MEMO[key]


def _references(ids, lens, p, d):
    tok = CS.card_ref_tokens(ids, lens, *NONE7, EPS, d, params=p)
    yard = CS.card_yardstick(ids, lens, p, EPS, d)
    r = {"out": tok["out"], "yard_out": yard["out"], "cnt": CS.counts(ids, lens)}
    if d is not None:
        cls = CS.card_ref_classes(ids, lens, p, EPS, d)
        assert float((cls["dparams"] - tok["dparams"]).abs().max()) <= 1e-11 * max(1.0, float(tok["dparams"].abs().max()))
        r.update({"dparams": tok["dparams"], "yard_dparams": yard["dparams"], "abs_terms": cls["abs_terms"]})
    return r


def _fmt(n, ek, ey, sh):
    return f"{n} {ek:.2e} {ey:.2e} {PR.ratio(ek, ey):.2f} {sh:.3f}"


def _judge_out(name, out, c, line):
    """the rule for out over the case and per list -> failures"""
    bad = []
    ok, ek, ey, bound = CS.accept_out(out, c["out"], c["yard_out"])
    oks, eks, bnds = CS.per_list(out, c["out"], c["yard_out"])
    finite = bool(torch.isfinite(out).all())
    line.append(_fmt("out", ek, ey, max(PR.whole_share(ek, bound), PR.share(eks, bnds))))
    if not (ok and finite):
        bad.append((name, "out", "whole", ek, ey, bound, "finite" if finite else "NOT FINITE"))
    if not bool(oks.all()):
        r = int((~oks).nonzero()[0])
        bad.append((name, "out", f"{int((~oks).sum())} lists, first {r}", float(eks[r]), float(bnds[r])))
    return bad


def _judge_params(name, g, pre, ref, yard, abs_terms, depth, line, label="dparams"):
    ok, err, bound = PR.accept_sum(g, pre, ref, yard, abs_terms, depth)
    finite = bool(torch.isfinite(g).all())
    line.append(_fmt(label, float(err.max()), float((yard - ref).abs().max()), PR.share(err, bound)) + f" depth {depth}")
    if finite and bool(ok.all()):
        return [], bound
    j = int((~ok).nonzero()[0])
    return [(name, label, f"{int((~ok).sum())} parameters, first {j}", float(err[j]), float(bound[j]), "finite" if finite else "NOT FINITE")], bound


_TABLES = {}


def _table(lib, regime, seed=0):
    """the 4 860-pattern table of a regime, built as nn_kernels.card_summary_table builds it: k_card_summary_fwd on the pattern lists"""
    if (regime, seed) not in _TABLES:
        ids, lens = CS.pattern_lists()
        b = _Lists(ids.long(), lens, CS.make_params(regime, seed)[0])
        _TABLES[(regime, seed)] = _fwd(lib, b, want_keys=False)[0]
    return _TABLES[(regime, seed)]


# (storage, pitch, strided): every id type at every pitch, and int8 as a strided view of a wider tensor
STORAGES = ((torch.int8, 25, False), (torch.int32, 32, False), (torch.int64, 8, False), (torch.int8, 32, True), (torch.int64, 25, False),
            (torch.int32, 8, False), (torch.int8, 8, False), (torch.int64, 32, False), (torch.int32, 25, False), (torch.int8, 8, True))
FWD_ROWS = (1, 255, 256, 257, 513, 4860)


# ------------------------------------------------------------------------------------------------------------------ forward and lookup
@pytest.mark.parametrize("regime", CS.REGIMES)
def test_card_forward_and_lookup_vs_fp64(hip_lib, regime):
    """k_card_summary_fwd and k_card_summary_lookup at every row count, every id type and pitch, with and without keys: out against the
    per-token fp64 reference over the case and per list; keys == pattern_of(counts), -1 outside the deck; lookup == forward bit for bit on
    keyed and on unkeyed lists; the flat regime gives len * ln_b, an empty list a zero row and key 0, to the bit.

    Measured on the MI355X: profiles/card_summary_kernel_tests.txt."""
    bad = []
    table = _table(hip_lib, regime)
    runs = [(rows, STORAGES[(2 * i + j) % len(STORAGES)], "mixed") for i, rows in enumerate(FWD_ROWS) for j in range(2)]
    runs.append((4860, (torch.int8, 25, False), "patterns"))
    for n, (rows, (dtype, pitch, strided), kind) in enumerate(runs):
        c = _case(regime, kind, rows, pitch, grads=False)
        b = _Lists(c["ids"], c["lens"], c["params"], dtype, strided)
        name = f"fwd {regime} {kind} rows={rows} {str(dtype)[6:]} pitch={pitch}{' strided' if strided else ''}"
        out, keys = _fwd(hip_lib, b, want_keys=True)
        out_nokeys, _ = _fwd(hip_lib, b, want_keys=False)
        assert same_bits(out, out_nokeys), (name, "out depends on keys being asked for")
        line = []
        bad += _judge_out(name, out, c, line)
        want_keys = CS.pattern_of(c["cnt"]).to(torch.int32)
        assert torch.equal(keys, want_keys), (name, "keys", int((keys != want_keys).sum()))
        if kind == "patterns":
            k = torch.arange(CS.PATTERNS, device="cuda", dtype=torch.int32)
            assert torch.equal(keys[:-1], k[:-1]) and int(keys[-1]) == CS.PATTERNS - 1 - 1620
            assert same_bits(out, table), (name, "the live padding of the pattern lists changed a row")
        if rows >= 255 and kind == "mixed":
            assert bool((keys >= 0).any()) and bool((keys < 0).any()), name
        looked = _lookup(hip_lib, b, table)
        assert same_bits(looked, out), (name, "lookup differs from forward", int((looked.view(torch.int32) != out.view(torch.int32)).any(1).sum()))
        empty = c["lens"] == 0
        assert not bool(out[empty].view(torch.int32).any()) and not bool(keys[empty].any()), (name, "an empty list")
        if regime == "flat":
            want = c["lens"].clamp(max=25).float()[:, None] * c["params"][CS.OFF_LB:][None, :] + 0.0      # (+ 0.0: an empty list's row is +0)
            assert same_bits(out, want), (name, "flat: out is not len * ln_b to the bit")
        print(f"CARD {name}: " + " | ".join(line) + f" | keyed {int((keys >= 0).sum())} of {rows}")
    assert not bad, bad


def test_card_forward_exact_gates(hip_lib):
    """Bit for bit: permuting a list's valid prefix, or changing the ids at and behind its length, changes nothing; a single-class list of
    count n gives fl32(n * the output of count 1) (the softmax of one class is exactly 1 whatever log n is); the first 257 rows of a
    513-row launch equal a launch over them alone."""
    for regime in ("unit", "saturated"):
        for dtype, pitch, strided in ((torch.int8, 25, False), (torch.int32, 32, False), (torch.int64, 8, False)):
            c = _case(regime, "mixed", 513, pitch, grads=False)
            ids, lens = c["ids"], c["lens"]
            out, keys = _fwd(hip_lib, _Lists(ids, lens, c["params"], dtype, strided))
            n = lens.clamp(max=25)[:, None]
            pos = torch.arange(pitch, device="cuda")[None, :]
            g = torch.Generator(device="cuda").manual_seed(5)
            order = torch.where(pos < n, torch.rand(ids.shape, device="cuda", generator=g), 2.0 + pos).argsort(1)
            shuffled = ids.gather(1, order)
            assert not torch.equal(shuffled, ids) and torch.equal(shuffled[pos.expand_as(ids) >= n], ids[pos.expand_as(ids) >= n])
            out2, keys2 = _fwd(hip_lib, _Lists(shuffled, lens, c["params"], dtype, strided))
            assert same_bits(out, out2) and torch.equal(keys, keys2), (regime, pitch, "a permuted prefix changed the result")
            other = torch.where(pos < n, ids, ids % 5 + 1)                   # another live id at every position behind the length
            assert bool((other != ids).any())
            out3, keys3 = _fwd(hip_lib, _Lists(other, lens, c["params"], dtype, strided))
            assert same_bits(out, out3) and torch.equal(keys, keys3), (regime, pitch, "the ids behind lens are read")
            sub, subk = _fwd(hip_lib, _Lists(ids[:257], lens[:257], c["params"], dtype, strided))
            assert same_bits(sub, out[:257]) and torch.equal(subk, keys[:257]), (regime, pitch, "the first 257 rows depend on the grid")
        # single-class lists
        c = _case(regime, "single", 300, 25, grads=False)
        out, _ = _fwd(hip_lib, _Lists(c["ids"], c["lens"], c["params"]))
        ones = torch.arange(CS.VOCAB, device="cuda")[:, None].expand(CS.VOCAB, 25).contiguous()
        one, _ = _fwd(hip_lib, _Lists(ones, torch.ones(CS.VOCAB, dtype=torch.long), c["params"]))
        cls = c["cnt"].argmax(1)
        want = c["cnt"].amax(1).float()[:, None] * one[cls]
        assert int(c["cnt"].amax(1).max()) == 25
        assert same_bits(out, want), (regime, "a single-class list is not n times its count-1 output")


# ------------------------------------------------------------------------------------------------------------------------ pattern sum
SUM_ROWS = (1, 1023, 1024, 1025, 2049, 8193)


def _key_set(kind, rows, seed):
    g = torch.Generator().manual_seed(seed * 13 + rows)
    r = torch.arange(rows)
    if kind == "few":                                     # 2..5 keys cover every workgroup
        some = torch.randperm(CS.PATTERNS, generator=g)[:2 + seed % 4]
        return some[torch.randint(0, some.numel(), (rows,), generator=g)]
    if kind == "first1024":                               # 1 024 distinct keys in a workgroup of 512 slots
        return r % 1024
    if kind == "window":                                  # 78 keys that reach 23 slots
        w = CS.window_keys(6, 8)
        return w[r % w.numel()]
    keys = torch.randint(0, CS.PATTERNS, (rows,), generator=g)
    if kind == "tenth_unkeyed":
        return torch.where(torch.rand(rows, generator=g) < 0.1, torch.full_like(keys, -1), keys)
    assert kind == "all_unkeyed"
    return torch.full_like(keys, -1)


def _most_shared(keys):
    """the most rows of one workgroup that share a key"""
    most = 0
    for c0 in range(0, keys.numel(), CS.SUM_ROWS):
        k = keys[c0:c0 + CS.SUM_ROWS]
        k = k[k >= 0]
        if k.numel():
            most = max(most, int(torch.unique(k, return_counts=True)[1].max()))
    return most


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_card_pattern_sum_vs_fp64(hip_lib, exact):
    """catan_card_pattern_sum alone at 1 .. 8 193 rows on 1, 3 and 8 copies, on key sets that leave the LDS table almost empty, overfill it
    (1 024 distinct keys on 512 slots) and exhaust the 16 probes in an otherwise empty table (78 keys that reach 23 slots), with 10 % and
    100 % of the keys at -1.  exact: dout = small integers times 2^-4, every copy equals an int64-exact index_add to the bit (so a copy no
    workgroup writes stays zero to the bit) ; real: normal dout, per word |sum of the copies - fp64| <= sum_depth 2^-24 sum |term|.  The
    rows with key -1 hold NaN in dout and are counted into n_unkeyed on top of its previous value."""
    bad = []
    for rows in SUM_ROWS:
        for replicas in (1, 3, 8):
            for i, kind in enumerate(("few", "first1024", "window", "tenth_unkeyed", "all_unkeyed")):
                keys = _key_set(kind, rows, i + replicas)
                d = CS.make_dout(rows, i, exact=exact)
                d[keys < 0] = NAN
                keys_d, d_d = keys.to(device="cuda", dtype=torch.int32), d.cuda()
                n_unk = torch.full((1,), 7, dtype=torch.int32, device="cuda")
                dpat = _pattern_sum(hip_lib, keys_d, d_d, replicas, n_unk)
                copies, total, ab, unkeyed = CS.pattern_sum_ref(keys_d, d_d, replicas)
                name = f"sum {'exact' if exact else 'real'} rows={rows} copies={replicas} {kind}"
                assert int(n_unk) == 7 + unkeyed, (name, int(n_unk), unkeyed)
                assert bool(torch.isfinite(dpat).all()), (name, "a row with key -1 was read")
                used = CS.sum_launch(rows, replicas)["workgroups"]
                assert not bool(dpat[used:].view(torch.int32).any()), (name, "a copy no workgroup writes is not zero")
                fallback = CS.provable_fallback_rows(keys)
                if exact:
                    assert torch.equal(dpat.double(), copies), (name, int((dpat.double() != copies).sum()))
                    print(f"CARD {name}: exact | fallback rows >= {fallback}")
                    continue
                depth = CS.sum_depth(rows, replicas, _most_shared(keys))
                err = (dpat.double().sum(0) - total).abs()
                bound = PR.sum_bound(ab, depth)
                print(f"CARD {name}: dpat {float(err.max()):.2e} share {PR.share(err, bound):.3f} depth {depth} | fallback rows >= {fallback}")
                if not bool((err <= bound).all()):
                    bad.append((name, float(err.max()), PR.share(err, bound)))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------------- backward
BWD_ROWS = (1, 255, 256, 257, 4860, 65535, 65536, 65537, 66561)


def _bwd_case(lib, regime, rows, storage):
    dtype, pitch, strided = storage
    kind = "patterns" if rows == 4860 else "mixed"
    c = _case(regime, kind, rows, pitch)
    b = _Lists(c["ids"], c["lens"], c["params"], dtype, strided)
    g, pre = _bwd(lib, b, c["dout"], k=1 + rows % 5)
    name = f"bwd {regime} {kind} rows={rows} {str(dtype)[6:]} pitch={pitch}{' strided' if strided else ''}"
    line = []
    bad, _ = _judge_params(name, g, pre, c["dparams"], c["yard_dparams"], c["abs_terms"], CS.bwd_depth(rows), line)
    print(f"CARD {name}: " + " | ".join(line))
    return bad


@pytest.mark.parametrize("rows", BWD_ROWS)
def test_card_backward_vs_fp64(hip_lib, rows):
    """catan_card_summary_bwd alone (direct mode) on both sides of the grid-shape switch at 65 536 rows: all 544 parameters, per parameter,
    with the pre-fill as one more addend.  unit at every row count; saturated and flat at 257 and 65 537."""
    storage = (torch.int8, 25, False) if rows == 4860 else STORAGES[BWD_ROWS.index(rows) % len(STORAGES)]
    bad = _bwd_case(hip_lib, "unit", rows, storage)
    if rows in (257, 65537):
        for regime in ("saturated", "flat"):
            bad += _bwd_case(hip_lib, regime, rows, storage)
    assert not bad, bad


@pytest.mark.parametrize("rows", [257, 65537])
def test_card_backward_skips_zero_rows(hip_lib, rows):
    """Rows whose dout is all zero are skipped: with dout zero everywhere the pre-fill stays untouched to the bit, and where only the
    lists of ONE query class have a non-zero dout, S[h][a'][.] for every other a' stays untouched to the bit (and the rest obeys the rule)."""
    c = _case("unit", "single", rows, 25)
    b = _Lists(c["ids"], c["lens"], c["params"])
    g, pre = _bwd(hip_lib, b, torch.zeros_like(c["dout"]), k=2)
    assert same_bits(g, pre), "an all-zero dout changed dparams"
    cls = c["cnt"].argmax(1)
    for a in (0, 4):
        d = torch.where((cls == a)[:, None], c["dout"], torch.zeros_like(c["dout"]))
        g, pre = _bwd(hip_lib, b, d, k=3)
        S, S0 = g[:CS.OFF_V].view(4, 6, 6), pre[:CS.OFF_V].view(4, 6, 6)
        others = [x for x in range(6) if x != a]
        assert same_bits(S[:, others], S0[:, others]), (rows, a, "another query class's rows of dS were written")
        ref = _references(c["ids"], c["lens"], c["params"], d)
        line = []
        bad, _ = _judge_params(f"bwd one-class a={a} rows={rows}", g, pre, ref["dparams"], ref["yard_dparams"], ref["abs_terms"], CS.bwd_depth(rows), line)
        print(f"CARD bwd unit single rows={rows} only class {a}: " + " | ".join(line))
        assert not bad, bad


@pytest.mark.parametrize("rows", [1025, 65536])
def test_card_backward_skip_list(hip_lib, rows):
    """only_unkeyed = the forward's keys: the rows with key >= 0 hold NaN in dout and are not read, the result is the reference over the
    unkeyed rows alone; with *n_unkeyed == 0 the launch leaves dparams untouched to the bit though dout is all NaN; n_unkeyed without
    only_unkeyed is CATAN_EINVAL."""
    c = _case("unit", "mixed", rows, 25)
    b = _Lists(c["ids"], c["lens"], c["params"])
    _, keys = _fwd(hip_lib, b)
    keyed = keys >= 0
    assert 0.2 < float(keyed.float().mean()) < 0.8
    d_ref = torch.where(keyed[:, None], torch.zeros_like(c["dout"]), c["dout"])
    d_nan = torch.where(keyed[:, None], torch.full_like(c["dout"], NAN), c["dout"])
    ref = _references(c["ids"], c["lens"], c["params"], d_ref)
    for n_unk in (None, torch.tensor([int((~keyed).sum())], dtype=torch.int32, device="cuda")):
        g, pre = _bwd(hip_lib, b, d_nan, only=keys, n_unk=n_unk, k=4)
        line = []
        name = f"bwd skip-list rows={rows} n_unkeyed={'NULL' if n_unk is None else int(n_unk)}"
        bad, _ = _judge_params(name, g, pre, ref["dparams"], ref["yard_dparams"], ref["abs_terms"], CS.bwd_depth(rows), line)
        print(f"CARD {name}: " + " | ".join(line))
        assert not bad, bad
    zero = torch.zeros((1,), dtype=torch.int32, device="cuda")
    g, pre = _bwd(hip_lib, b, torch.full_like(c["dout"], NAN), only=keys, n_unk=zero, k=5)
    assert same_bits(g, pre), "*n_unkeyed == 0 did not return at once"
    dp = G.pattern(CS.NPAR, 6)
    rc = hip_lib.catan_card_summary_bwd(P(b.ids), b.esz, b.pitch, P(b.lens), P(b.params), EPS, P(c["dout"]), P(dp), None, P(zero), rows, _stream())
    assert rc == EINVAL and b"bad arguments" in hip_lib.catan_last_error()
    torch.cuda.synchronize()
    assert same_bits(dp, G.pattern(CS.NPAR, 6))


# ------------------------------------------------------------------------------------------------------------------------ composition
def _composition(lib, b, keys, dout, replicas):
    """pattern sum -> backward over the pattern lists -> backward over the unkeyed rows, as nn_kernels._CardSummary.backward chains them
    -> (dparams, the pre-fill)"""
    n_unk = torch.zeros((1,), dtype=torch.int32, device="cuda")
    dpat = _pattern_sum(lib, keys, dout, replicas, n_unk)
    dpat = dpat.sum(0) if replicas > 1 else dpat[0]
    pid, plen = CS.pattern_lists()
    pb = _Lists(pid.long(), plen, b.params[:CS.NPAR])
    g, pre = _bwd(lib, pb, dpat, k=2)
    g, _ = _bwd(lib, b, dout, only=keys, n_unk=n_unk, into=g)
    return g, pre


def composition_depth(rows, replicas):
    """a row's term passes the pattern sum, the sum of the copies, the backward over the 4 860 pattern lists - or the direct backward"""
    return CS.sum_depth(rows, replicas) + replicas + CS.bwd_depth(CS.PATTERNS) + CS.bwd_depth(rows)


@pytest.mark.parametrize("kind", ["mixed", "all_keyed"])
def test_card_backward_composition(hip_lib, kind):
    """The chain of nn_kernels._CardSummary.backward on deck prefixes with 5 % lists outside the deck, and on keyed lists alone: against
    the per-token reference over all rows, and against the direct backward on the same rows within the sum of their bounds."""
    rows = 5003
    p, _ = CS.make_params("unit", 2)
    ids, lens = CS.make_lists("deck", rows, 25, 6)
    if kind == "mixed":
        wild, wlen = CS.make_lists("arbitrary", rows, 25, 7)
        swap = torch.arange(rows) % 20 == 7
        ids, lens = torch.where(swap[:, None], wild, ids), torch.where(swap, wlen, lens)
    ids, lens, p = ids.cuda(), lens.cuda(), p.cuda()
    d = CS.make_dout(rows, 8).cuda()
    ref = _references(ids, lens, p, d)
    b = _Lists(ids, lens, p)
    _, keys = _fwd(hip_lib, b)
    unkeyed = int((keys < 0).sum())
    assert (unkeyed == 0) == (kind == "all_keyed") and unkeyed < rows // 10
    for replicas in (1, 8):
        g, pre = _composition(hip_lib, b, keys, d, replicas)
        line = []
        name = f"composition {kind} rows={rows} copies={replicas}"
        bad, bound_c = _judge_params(name, g, pre, ref["dparams"], ref["yard_dparams"], ref["abs_terms"], composition_depth(rows, replicas), line)
        gd, pred = _bwd(hip_lib, b, d, k=2)
        bad_d, bound_d = _judge_params(name, gd, pred, ref["dparams"], ref["yard_dparams"], ref["abs_terms"], CS.bwd_depth(rows), line, "direct")
        assert same_bits(pre, pred)
        gap = (g.double() - gd.double()).abs()
        print(f"CARD {name}: " + " | ".join(line) + f" | composition - direct share {PR.share(gap, bound_c + bound_d):.3f} | unkeyed {unkeyed}")
        assert not bad and not bad_d, (bad, bad_d)
        assert bool((gap <= bound_c + bound_d).all())


# ------------------------------------------------------------------------------------------------------------------------------- glue
@pytest.mark.parametrize("rows", [32767, 32768])
def test_card_summary_glue_vs_fp64(hip_lib, rows):
    """nn_kernels.card_summary forward and backward on both sides of its `reps` switch (one copy of the pattern table below 32 768 rows,
    eight from there), from the module's own weights: out against the per-token reference built from the weights in double, and the
    weights' gradients against its autograd.  The block the kernel reads is the fp32 expression of nn_kernels.card_summary_params; the
    yardstick reads the same block and pushes its dparams through that expression's fp32 autograd.  Per weight:
    |kernel - fp64| <= 2 |yardstick - fp64| + sum over the block of |d block / d weight| (depth 2^-24 abs_terms)  (the block is a
    function of the weights, so a bound on dparams carries over through the absolute Jacobian)."""
    from settlers_of_catan_rl_amd import nn_kernels
    w = [t.cuda().requires_grad_(True) for t in CS.make_weights(11)]
    ids, lens = CS.make_lists("deck", rows, 25, 12)
    wild, wlen = CS.make_lists("arbitrary", rows, 25, 13)
    swap = torch.arange(rows) % 50 == 9
    ids, lens = torch.where(swap[:, None], wild, ids).cuda(), torch.where(swap, wlen, lens).cuda()
    d = CS.make_dout(rows, 14).cuda()
    block = CS.params_from_weights(*w)
    out = nn_kernels.card_summary(ids.to(torch.int8), lens, block, EPS)
    (out * d).sum().backward()
    got = [t.grad.clone() for t in w]
    ref = CS.card_ref_tokens(ids, lens, *[t.detach() for t in w], EPS, d)
    blk = block.detach()
    yard = CS.card_yardstick(ids, lens, blk, EPS, d)
    cls = CS.card_ref_classes(ids, lens, blk, EPS, d)
    line = []
    c = {"out": ref["out"], "yard_out": yard["out"]}
    name = f"glue rows={rows}"
    bad = _judge_out(name, out.detach(), c, line)
    # the yardstick's weight gradients: its dparams through the fp32 expression
    wy = [t.detach().clone().requires_grad_(True) for t in w]
    CS.params_from_weights(*wy).backward(yard["dparams"].float())
    jac = torch.autograd.functional.jacobian(lambda *a: CS.params_from_weights(*a), tuple(t.detach().double() for t in w))
    reps = 8 if rows >= 32768 else 1
    bound_p = PR.sum_bound(cls["abs_terms"], composition_depth(rows, reps))
    for nme, gk, gr, gy, j in zip(("emb", "wqkv", "bqkv", "wo", "bo", "ln_w", "ln_b"), got, ref["dweights"], [t.grad for t in wy], jac):
        carried = (j.abs() * bound_p.view(-1, *([1] * gr.dim()))).sum(0)
        err = (gk.double() - gr).abs()
        bound = 2.0 * (gy.double() - gr).abs() + carried
        line.append(_fmt(nme, float(err.max()), float((gy.double() - gr).abs().max()), PR.share(err, bound)))
        if not bool((err <= bound).all()):
            bad.append((name, nme, float(err.max()), PR.share(err, bound)))
    print(f"CARD {name}: " + " | ".join(line))
    assert not bad, bad


def test_card_summary_table_is_rebuilt_after_a_weight_change(hip_lib):
    """policy._card_summary under no_grad (the pattern-table look-up) after an in-place weight change equals a fresh forward of the new
    weights bit for bit, and differs from the look-up before the change: the cached table was rebuilt."""
    from settlers_of_catan_rl_amd import policy
    torch.manual_seed(5)
    emb = torch.nn.Embedding(CS.VOCAB, CS.WIDTH).cuda()
    mha = policy._MHA(CS.WIDTH, CS.HEADS).cuda()
    norm = torch.nn.LayerNorm(CS.WIDTH).cuda()
    ids, lens = CS.make_lists("mixed", 1000, 25, 3)
    ids, lens = ids.to(torch.int8).cuda(), lens.clamp(min=1).cuda()
    with torch.no_grad():
        before = policy._card_summary(ids, lens, emb, mha, norm).clone()
        mha.out_proj_net.weight.add_(0.25)
        emb.weight.mul_(1.5)
        after = policy._card_summary(ids, lens, emb, mha, norm).clone()
    fresh = policy._card_summary(ids, lens, emb, mha, norm).detach()
    assert not torch.equal(before, after)
    assert same_bits(after, fresh)
    ref = CS.card_ref_tokens(ids.long(), lens, emb.weight, torch.cat([n.weight for n in mha.qkv_nets], 0), torch.cat([n.bias for n in mha.qkv_nets], 0),
                             mha.out_proj_net.weight, mha.out_proj_net.bias, norm.weight, norm.bias, norm.eps, None)
    from settlers_of_catan_rl_amd import nn_kernels
    yard = CS.card_yardstick(ids.long(), lens, nn_kernels.card_summary_params(emb, mha, norm).detach(), norm.eps, None)
    ok, ek, ey, bound = CS.accept_out(after, ref["out"], yard["out"])
    print(f"CARD glue table rebuilt: {_fmt('out', ek, ey, ek / bound)}")
    assert ok, (ek, ey, bound)
