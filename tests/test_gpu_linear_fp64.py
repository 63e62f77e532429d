"""GPU: the row-split linear kernels of csrc/catan_nn.hip and csrc/catan_wgrad_big.hip element by element against fp64, through the C ABI:
k_linear_rows<KS, NT> (catan_linear_rows / catan_linear_rows_fused, modes 0-3), k_wgrad / k_wgrad_tr<OTW, IT> (catan_linear_wgrad), their
_grouped forms (catan_linear_wgrad_grouped), k_wgrad_big + k_wgrad_big_reduce (catan_linear_wgrad_big).

reference = tests/linear_reference.py (its docstring has the formulas, the yardstick's roundings, the two regimes and the bounds):
    exact regime   y equals the yardstick bit for bit (a zero may carry either sign); dw, db equal pre-fill + fp64 reference exactly
    real regime    per element |y - ref| <= e + 2^-8 (|a| + e), e = (K + 1) 2^-23 S (mode 2: one more rounding), and within_yardstick over the
                   case and per row; |dw - (pre-fill + ref)| <= depth 2^-23 (sum_r |dy x| + |pre-fill|), depth from the launch table
Nothing in a bound comes from a kernel; no element is excluded; a NaN or Inf fails.  The exact regime runs at every row count, the real
regime below 5 000 rows (above, its weight-gradient bound is wider than one row's term).  Every launch is judged on its own; every case
(one shape in one regime, or one problem of the grouped list) prints one `LIN` line per output: the largest kernel error, yardstick error
and share of a per-element bound used (exact regime: 0 or inf) over its launches, and the launch where the share peaked;
profiles/linear_kernel_tests.txt is that output.

The test never reads which kernel ran: the shapes leave the dispatch one choice (linear_reference's launch table, whose coverage of every
instantiation test_cases_cover_every_instantiation asserts).

Buffers: every input lies in front of 64 guard rows of NaN (W and bias: a NaN tail); y, dw, db and the workspace lie between sentinel
margins that must be intact afterwards; dw and db are pre-filled with a non-constant pattern (integer-valued in the exact regime); a
windowed dw is a column window of a wider pre-filled matrix whose other columns must keep their bits."""
import pytest
import torch

import guarded as G
import linear_reference as L
from guarded import NAN, ptr as P, stream as _stream
from pin_rule import same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5B
MARGIN = 512                     # elements of sentinel in front of and behind every output: a multiple of 16 bytes
BF = torch.bfloat16


def _check(rc):
    from settlers_of_catan_rl_amd import _lib
    _lib.check(rc)


def _guarded(t, tail=None):
    """a copy of `t` that is followed by NaN: GUARD rows of it (a matrix) or GUARD elements (a vector) -> (whole, view)"""
    tail = GUARD * (t.shape[-1] if t.dim() == 2 else 1) if tail is None else tail
    return G.guarded_input(t, tail + 8)


def _between_sentinels(n, dtype, fill=None):
    """n elements between two sentinel margins (each a multiple of 16 bytes) -> (whole, view); `fill` [n] is copied in, otherwise the
    view holds the sentinel too (an element the kernel leaves unwritten then shows as 1.5e13)"""
    whole, view = G.sentinel_output(n, dtype, MARGIN, MARGIN, SENTINEL)
    assert view.data_ptr() % 16 == 0
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return whole, view


def _mx(a, b):
    """max that keeps a NaN"""
    return a if (a != a or b <= a) else b


class _Lin:
    """the LIN lines of one test: per (case, output) the largest figures over the case's launches and where the share peaked; `bad`
    collects what the rule refused in any launch"""

    def __init__(self):
        self.acc, self.bad = {}, []

    def add(self, case, out, where, ek, ey, sh, refused=()):
        a = self.acc.setdefault((case, out), [0, 0.0, 0.0, -1.0, ""])
        a[0], a[1], a[2] = a[0] + 1, _mx(a[1], ek), _mx(a[2], ey)
        if not sh <= a[3]:
            a[3], a[4] = sh, where
        self.bad += [(f"{case} {where} {out}", m) for m in refused]

    def done(self):
        for (case, out), (n, ek, ey, sh, where) in self.acc.items():
            print(f"LIN {case}: {out} {ek:.2e} {ey:.2e} {sh:.2f} ({n} launches, at {where})")
        assert not self.bad, self.bad


# ------------------------------------------------------------------------------------------------------------------ forward
class _FwdBuffers:
    def __init__(self, c):
        self.c = c
        self.hold = [_guarded(c[k]) for k in ("x", "W", "b", "aux")]
        self.x, self.W, self.b, self.aux = (v for _, v in self.hold)

    def launch(self, lib, mode, bias, rows=None, plain=False):
        """-> y [rows, N] bf16 (a clone); rows: launch over the first rows only; plain: through catan_linear_rows"""
        c = self.c
        rows = c["rows"] if rows is None else rows
        whole, y = _between_sentinels(rows * c["N"], BF)
        b = P(self.b) if bias else None
        if plain:
            _check(lib.catan_linear_rows(P(self.x), P(self.W), b, P(y), rows, c["K"], c["N"], _stream()))
        else:
            _check(lib.catan_linear_rows_fused(P(self.x), P(self.W), b, P(y), rows, c["K"], c["N"], P(self.aux) if mode >= 2 else None, mode, _stream()))
        torch.cuda.synchronize()
        assert G.intact(whole, y), (c["K"], c["N"], rows, mode, "a write outside y")
        return y.view(rows, c["N"]).clone()


def _forward_case(lib, K, N, rows, regime, lin):
    c = L.make_forward_case(K, N, rows, regime, "cuda")
    buf = _FwdBuffers(c)
    terms = {True: L.linear_terms(c["x"], c["W"], c["b"]), False: L.linear_terms(c["x"], c["W"], None)}
    ys = {}
    for mode, bias in L.fwd_modes(N):
        y = buf.launch(lib, mode, bias, plain=(mode == 0 and not bias))
        ys[(mode, bias)] = y
        b, ek, ey, sh = L.judge_forward(y, c["x"], c["W"], c["b"] if bias else None, c["aux"], mode, regime, terms=terms[bias])
        lin.add(f"rows K={K} N={N} {regime}", "y", f"rows={rows} mode={mode} bias={int(bias)}", ek, ey, sh, b)
    if (2, True) in ys:                    # mode 2 = mode 0 followed by a separate bf16 add
        assert same_bits(ys[(2, True)], ys[(0, True)] + c["aux"]), (K, N, rows, regime, "mode 2 differs from mode 0 + a separate bf16 add")
    if rows == L.FWD_FULL_GRID + 1:        # rows do not depend on the grid
        for mode, bias in L.fwd_modes(N, with_nobias=False):
            assert same_bits(buf.launch(lib, mode, bias, rows=65), ys[(mode, bias)][:65]), (K, N, mode, "the first 65 rows depend on the grid")


@pytest.mark.parametrize("K,N", L.FWD_CASES, ids=[f"K{K}-N{N}" for K, N in L.FWD_CASES])
def test_linear_rows_vs_fp64(hip_lib, K, N):
    """One (KS, NT) instantiation of k_linear_rows: every mode the width admits, with and without bias, at 1 .. 4099 rows in both regimes;
    for a narrow and a wide shape per KS also at 131 072 rows (the grid exactly full), 131 073 (one wave's second pass, a 1-row tile) and
    131 281 (several second passes and a ragged tail) in the exact regime.  Measured on the MI355X: profiles/linear_kernel_tests.txt."""
    assert hip_lib.catan_linear_rows_supported(1, K, N)
    lin = _Lin()
    for rows in L.FWD_ROWS:
        for regime in ("exact", "real"):
            _forward_case(hip_lib, K, N, rows, regime, lin)
    if (K, N) in L.FWD_BIG_CASES:
        for rows in L.FWD_BIG_ROWS:
            assert L.rows_launch(rows, K, N)["passes"] == (1 if rows == L.FWD_FULL_GRID else 2)
            _forward_case(hip_lib, K, N, rows, "exact", lin)
    lin.done()


def test_linear_rows_supported_enumerated(hip_lib):
    """catan_linear_rows_supported equals the Python restatement over the whole (K, N) range, and what it refuses is refused by the launch"""
    for K in range(0, 201):
        for N in range(0, 201):
            assert bool(hip_lib.catan_linear_rows_supported(1, K, N)) == L.rows_supported(1, K, N), (K, N)
    assert not hip_lib.catan_linear_rows_supported(0, 8, 8)
    from settlers_of_catan_rl_amd import _lib
    t = torch.zeros(4096, dtype=BF, device="cuda")
    for K, N in ((96, 192), (136, 72), (192, 128)):                      # 3 x 12, 6 x 8: more than 32 fragments
        with pytest.raises(_lib.CatanHipError, match="<= 32"):
            _lib.check(hip_lib.catan_linear_rows_fused(P(t), P(t), None, P(t), 1, K, N, None, 0, _stream()))


def test_cases_cover_every_instantiation():
    """every instantiation of the launch table is reached by at least one case of this file"""
    assert {(l["KS"], l["NT"]) for l in (L.rows_launch(1, K, N) for K, N in L.FWD_CASES)} == set(L.LINROWS_INSTANCES)
    assert {l["KS"] for l in (L.rows_launch(1, K, N) for K, N in L.FWD_BIG_CASES)} == set(L.LINROWS_KS)
    assert {(l["tr"], l["OTW"], l["IT"]) for I, O in L.WGRAD_CASES for l in L.wgrad_launches(1, I, O)} == set(L.WGRAD_INSTANCES)
    units = [(l["tr"], l["OTW"], l["IT"]) for p in L.grouped_problems() for l in L.wgrad_launches(p["rows"], p["I"], p["O"])]
    assert max(units.count(u) for u in set(units)) > L.WG_MAX_UNITS
    assert {L.big_launch(r, 8, 128)["groups"] for r in L.BIG_ROWS_EXACT} == {8, 16}
    assert {L.wgrad_grid(r, 64, 64)["spb"] for r in L.WGRAD_BIG_ROWS} == {8, 16}


# ------------------------------------------------------------------------------------------------------------ weight gradients
def _wgrad_alone(lib, xv, gv, rows, I, O, dw0, db0):
    """catan_linear_wgrad into a pre-filled dw [O][I] (and db, or NULL) between sentinels -> (dw, db or None)"""
    hw, dw = _between_sentinels(O * I, torch.float32, dw0)
    hb, db = _between_sentinels(O, torch.float32, db0) if db0 is not None else (None, None)
    _check(lib.catan_linear_wgrad(P(xv), P(gv), P(dw), P(db), rows, I, O, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hw, dw), (rows, I, O, "a write outside dw")
    assert db is None or G.intact(hb, db), (rows, I, O, "a write outside db")
    return dw.view(O, I).clone(), None if db is None else db.clone()


def _wgrad_case(lib, I, O, rows, regime, lin, ones=False):
    c = L.make_wgrad_case(I, O, rows, regime, "cuda", ones=ones)
    (hx, xv), (hg, gv) = _guarded(c["x"]), _guarded(c["dy"])
    if ones:
        full = lambda *s: torch.full(s, float(rows), dtype=torch.float64, device="cuda")
        ref = {"dw": full(O, I), "db": full(O), "aw": full(O, I), "ab": full(O)}
    else:
        ref = L.wgrad_ref(c["x"], c["dy"])
    depth = L.wgrad_depth(rows, I, O)
    dw0, db0 = L.prefill((O, I), regime, 1, "cuda"), L.prefill((O,), regime, 2, "cuda")
    yw, yb = L.wgrad_yardstick(c["x"], c["dy"])
    for with_db in (True, False) if not ones else (True,):
        dw, db = _wgrad_alone(lib, xv, gv, rows, I, O, dw0, db0 if with_db else None)
        case, where = f"wgrad I={I} O={O} {'ones' if ones else regime}", f"rows={rows} db={int(with_db)}"
        b, ek, sh = L.judge_wgrad(dw, dw0, ref["dw"], ref["aw"], regime, depth)
        lin.add(case, "dw", where, ek, float((yw.double() - ref["dw"]).abs().max()), sh, b)
        if with_db:
            b, ek, sh = L.judge_wgrad(db, db0, ref["db"], ref["ab"], regime, depth)
            lin.add(case, "db", where, ek, float((yb.double() - ref["db"]).abs().max()), sh, b)


WG_ALL = L.WGRAD_CASES + L.WGRAD_SLICED_CASES


@pytest.mark.parametrize("I,O", WG_ALL, ids=[f"I{I}-O{O}" for I, O in WG_ALL])
def test_linear_wgrad_vs_fp64(hip_lib, I, O):
    """catan_linear_wgrad at one (I, O): one instantiation of k_wgrad / k_wgrad_tr, or the column slices of a wide input; accumulated into a
    pre-filled dw, with a pre-filled db and with db = NULL, at 1 .. 4609 rows in both regimes (for three shapes also 131 071 and 131 073
    rows, exact regime); and the counting case - x and dy all ones: every element is the row count added to the pre-fill, which a row read
    twice or not at all changes.  Measured on the MI355X: profiles/linear_kernel_tests.txt."""
    assert hip_lib.catan_linear_wgrad_supported(1, I, O) and L.wgrad_supported(1, I, O)
    lin = _Lin()
    big = L.WGRAD_BIG_ROWS if (I, O) in L.WGRAD_BIG_ROWS_CASES else ()
    for rows in L.WGRAD_ROWS + big:
        for regime in ("exact", "real") if rows < L.REAL_BELOW else ("exact",):
            _wgrad_case(hip_lib, I, O, rows, regime, lin)
        _wgrad_case(hip_lib, I, O, rows, "exact", lin, ones=True)
    lin.done()


@pytest.mark.parametrize("regime", ["exact", "real"])
def test_linear_wgrad_grouped_vs_fp64(hip_lib, regime):
    """catan_linear_wgrad_grouped over linear_reference.grouped_problems() in one call: every problem against its reference (exact regime:
    exactly, and bit for bit what catan_linear_wgrad leaves when run alone; real regime: the per-element bound), the columns outside every
    dw window untouched to the bit, every margin intact."""
    from settlers_of_catan_rl_amd import _lib
    probs = L.grouped_problems()
    arr = (_lib.CatanWgradProblem * len(probs))()
    keep = []
    for k, p in enumerate(probs):
        I, O, rows, ld = p["I"], p["O"], p["rows"], p["ld"] or p["I"]
        c = L.make_wgrad_case(I, O, rows, regime, "cuda", seed=k + 1)
        (hx, xv), (hg, gv) = _guarded(c["x"]), _guarded(c["dy"])
        dw0, db0 = L.prefill((O, ld), regime, k, "cuda"), L.prefill((O,), regime, k + 1, "cuda") if p["db"] else None
        hw, dw = _between_sentinels(O * ld, torch.float32, dw0)
        hb, db = _between_sentinels(O, torch.float32, db0) if p["db"] else (None, None)
        arr[k] = _lib.CatanWgradProblem(xv.data_ptr(), gv.data_ptr(), dw.data_ptr(), db.data_ptr() if p["db"] else None, rows, I, O, p["ld"], p["col0"])
        keep.append((c, hx, xv, hg, gv, dw0, db0, hw, dw, hb, db))
    _check(hip_lib.catan_linear_wgrad_grouped(arr, len(probs), _stream()))
    torch.cuda.synchronize()
    lin = _Lin()
    for k, p in enumerate(probs):
        c, hx, xv, hg, gv, dw0, db0, hw, dw, hb, db = keep[k]
        I, O, rows, ld, col0 = p["I"], p["O"], p["rows"], p["ld"] or p["I"], p["col0"]
        name = f"grouped #{k} I={I} O={O} ld={p['ld']} col0={col0} {regime}"
        assert G.intact(hw, dw) and (db is None or G.intact(hb, db)), (name, "a write outside dw or db")
        dw = dw.view(O, ld)
        outside = torch.ones(ld, dtype=torch.bool, device="cuda")
        outside[col0:col0 + I] = False
        assert same_bits(dw[:, outside], dw0[:, outside]), (name, "a column outside the window changed")
        ref = L.wgrad_ref(c["x"], c["dy"])
        depth = L.wgrad_depth(rows, I, O)
        yw, yb = L.wgrad_yardstick(c["x"], c["dy"])
        win, win0 = dw[:, col0:col0 + I].contiguous(), dw0[:, col0:col0 + I].contiguous()
        b, ek, sh = L.judge_wgrad(win, win0, ref["dw"], ref["aw"], regime, depth)
        lin.add(name, "dw", f"rows={rows}", ek, float((yw.double() - ref["dw"]).abs().max()), sh, b)
        if db is not None:
            b, ek, sh = L.judge_wgrad(db, db0, ref["db"], ref["ab"], regime, depth)
            lin.add(name, "db", f"rows={rows}", ek, float((yb.double() - ref["db"]).abs().max()), sh, b)
        if regime == "exact":
            aw, ab = _wgrad_alone(hip_lib, xv, gv, rows, I, O, win0, db0)
            assert same_bits(aw, win) and (db is None or same_bits(ab, db)), (name, "grouped differs from catan_linear_wgrad run alone")
    lin.done()


def _big(lib, xv, gv, rows, I, O, ld, dw_fill, db_fill, accumulate):
    """catan_linear_wgrad_big with a NaN-filled workspace of exactly the size the library asks for -> (dw [O][ld], db or None)"""
    need = int(lib.catan_wgrad_big_workspace_floats(rows, I, O))
    assert need == L.big_launch(rows, I, O)["workspace"]
    hs, ws = _between_sentinels(need, torch.float32, torch.full((need,), NAN, device="cuda"))
    hw, dw = _between_sentinels(O * ld, torch.float32, dw_fill)
    hb, db = _between_sentinels(O, torch.float32, db_fill) if db_fill is not None else (None, None)
    _check(lib.catan_linear_wgrad_big(P(xv), P(gv), P(dw), ld, P(db), P(ws), rows, I, O, accumulate, _stream()))
    torch.cuda.synchronize()
    assert G.intact(hs, ws) and G.intact(hw, dw) and (db is None or G.intact(hb, db)), (rows, I, O, "a write outside the workspace, dw or db")
    return dw.view(O, ld).clone(), None if db is None else db.clone()


@pytest.mark.parametrize("I,O", L.BIG_CASES, ids=[f"I{I}-O{O}" for I, O in L.BIG_CASES])
def test_linear_wgrad_big_vs_fp64(hip_lib, I, O):
    """catan_linear_wgrad_big at one (I, O) - at I = 128 and 256 the column of ones that yields db sits alone in a tile of its own - at
    1 .. 4099 rows in both regimes and at 65 535 / 65 536 / 65 537 rows (8 -> 16 row groups) in the exact one.  Every call starts from a
    NaN-filled workspace (the kernel writes every partial tile it later reads).  accumulate = 0 over a NaN-filled dw and db: finite and
    within the rule, and twice the same bits; accumulate = 1 over a pre-fill with dw_ld = I + 8 (the extra columns keep their bits) and
    db = NULL; accumulate = 1 with db.  Measured on the MI355X: profiles/linear_kernel_tests.txt."""
    lin = _Lin()
    for rows in L.BIG_ROWS + L.BIG_ROWS_EXACT:
        for regime in ("exact", "real") if rows < L.REAL_BELOW else ("exact",):
            c = L.make_wgrad_case(I, O, rows, regime, "cuda")
            (hx, xv), (hg, gv) = _guarded(c["x"]), _guarded(c["dy"])
            ref = L.wgrad_ref(c["x"], c["dy"])
            depth = L.big_depth(rows, I, O)
            yw, yb = L.wgrad_yardstick(c["x"], c["dy"])
            ew, eb = float((yw.double() - ref["dw"]).abs().max()), float((yb.double() - ref["db"]).abs().max())
            nan = lambda *s: torch.full(s, NAN, device="cuda")
            zw, zb = torch.zeros((O, I), device="cuda"), torch.zeros(O, device="cuda")
            runs = []
            dw, db = _big(hip_lib, xv, gv, rows, I, O, I, nan(O, I), nan(O), 0)
            dw2, db2 = _big(hip_lib, xv, gv, rows, I, O, I, nan(O, I), nan(O), 0)
            assert same_bits(dw, dw2) and same_bits(db, db2), (I, O, rows, regime, "two runs differ")
            runs.append(("acc=0", dw, zw, db, zb))
            w0 = L.prefill((O, I + 8), regime, 3, "cuda")
            dw, _ = _big(hip_lib, xv, gv, rows, I, O, I + 8, w0, None, 1)
            assert same_bits(dw[:, I:], w0[:, I:]), (I, O, rows, regime, "a column behind the window changed")
            runs.append(("acc=1 ld=I+8 db=NULL", dw[:, :I].contiguous(), w0[:, :I].contiguous(), None, None))
            w0, b0 = L.prefill((O, I), regime, 4, "cuda"), L.prefill((O,), regime, 5, "cuda")
            dw, db = _big(hip_lib, xv, gv, rows, I, O, I, w0, b0, 1)
            runs.append(("acc=1", dw, w0, db, b0))
            for what, dw, w0, db, b0 in runs:
                case, where = f"big I={I} O={O} {regime}", f"rows={rows} {what}"
                b, ek, sh = L.judge_wgrad(dw, w0, ref["dw"], ref["aw"], regime, depth)
                lin.add(case, "dw", where, ek, ew, sh, b)
                if db is not None:
                    b, ek, sh = L.judge_wgrad(db, b0, ref["db"], ref["ab"], regime, depth)
                    lin.add(case, "db", where, ek, eb, sh, b)
    lin.done()
