"""CPU: tests/guarded.py on buffers of a few dozen elements - a single element written outside a view, or left unwritten inside it, is
what the GPU suites rely on these helpers to see."""
import ctypes

import pytest
import torch

import guarded as G

DTYPES = (torch.bfloat16, torch.float32, torch.float64, torch.int64)
SENTINELS = (G.SENTINEL16, G.SENTINEL32)
N, LEAD, TAIL = 24, 4, 12


def _values(n, dtype):
    """n values of `dtype`, none of which holds a sentinel word"""
    return (torch.arange(n) % 7 - 3).to(dtype)


def _words(t, sentinel):
    return t.view(torch.int32 if sentinel == G.SENTINEL32 else torch.int16)


@pytest.mark.parametrize("sentinel", SENTINELS, ids=["s16", "s32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_sentinel_output_intact_and_written(dtype, sentinel):
    for lead in (0, LEAD):
        whole, view = G.sentinel_output(N, dtype, TAIL, lead, sentinel, device="cpu")
        assert whole.numel() == lead + N + TAIL and view.numel() == N and view.data_ptr() == whole.data_ptr() + lead * whole.element_size()
        assert bool((_words(whole, sentinel) == sentinel).all()), "every word of the allocation starts as the sentinel"
        assert G.intact(whole, view) and not G.written(whole, view, sentinel)
        view.copy_(_values(N, dtype))
        assert G.intact(whole, view) and G.written(whole, view, sentinel)
        # one element left unwritten, wherever it lies
        for i in (0, 7, N - 1):
            w2, v2 = G.sentinel_output(N, dtype, TAIL, lead, sentinel, device="cpu")
            keep = torch.arange(N) != i
            v2[keep] = _values(N, dtype)[keep]
            assert G.intact(w2, v2) and not G.written(w2, v2, sentinel), (lead, i)
        # one element written behind the view: the first, and the allocation's last
        for i in (lead + N, lead + N + TAIL - 1):
            w2 = whole.clone()
            w2[i] = 1
            assert not G.intact(w2, w2[lead:lead + N]), (lead, i)
        # ... and in front of it
        for i in range(0, lead, 3):
            w2 = whole.clone()
            w2[i] = 1
            assert not G.intact(w2, w2[lead:lead + N]), (lead, i)
        # a shaped view of the same elements
        assert G.intact(whole, view.view(4, 6)) and G.written(whole, view.view(4, 6), sentinel)
        # a view that ends early: what lies behind it counts as margin, and holds values
        assert not G.intact(whole, view[:N - 1]) and G.written(whole, view[:N - 1], sentinel)


def test_written_sees_half_an_element_under_the_narrow_sentinel_only():
    """an fp32 element whose low half alone equals SENTINEL16: left over under the 16-bit sentinel, written under the 32-bit one"""
    whole, view = G.sentinel_output(8, torch.float32, 8, 0, G.SENTINEL32, device="cpu")
    view.fill_(1.0)
    view.view(torch.int16)[6] = G.SENTINEL16
    assert G.written(whole, view, G.SENTINEL32) and not G.written(whole, view, G.SENTINEL16)
    # a bf16 output under the 32-bit sentinel is looked at element by element
    whole, view = G.sentinel_output(8, torch.bfloat16, 8, 0, G.SENTINEL32, device="cpu")
    view[:5] = 1.0
    view[6:] = 1.0
    assert not G.written(whole, view, G.SENTINEL32)


@pytest.mark.parametrize("dtype,guard", [(torch.bfloat16, G.NAN), (torch.float32, G.NAN), (torch.float64, G.NAN), (torch.int64, 20), (torch.int32, -1)])
def test_guarded_input(dtype, guard):
    t = _values(N, dtype).view(4, 6)
    for lead in (0, 1, LEAD):
        whole, view = G.guarded_input(t, TAIL, lead, guard, device="cpu")
        assert whole.dtype == dtype and whole.numel() == lead + N + TAIL and whole.data_ptr() % 16 == 0
        assert view.data_ptr() == whole.data_ptr() + lead * whole.element_size()
        assert torch.equal(view, t.reshape(-1)), "the view holds the data"
        margins = torch.cat((whole[:lead], whole[lead + N:]))
        assert margins.numel() == lead + TAIL
        assert bool(torch.isnan(margins).all()) if guard != guard else bool((margins == guard).all()), "the margins hold the guard value"
        view.zero_()
        assert bool((t.reshape(-1) == _values(N, dtype)).all()), "a copy, not a view of the input"


def test_ptr_stream_free_helpers():
    t = torch.arange(8, dtype=torch.float32)
    assert G.ptr(None) is None
    assert isinstance(G.ptr(t), ctypes.c_void_p) and G.ptr(t).value == t.data_ptr() and G.ptr(t, 12).value == t.data_ptr() + 12
    assert ctypes.cast(G.ptr(t, 12), ctypes.POINTER(ctypes.c_float))[0] == 3.0


def test_pattern_is_not_constant_and_differs_with_k():
    a, b = G.pattern(16, 1, "cpu"), G.pattern(16, 2, "cpu")
    assert a.dtype == torch.float32 and a.shape == (16,) and a.unique().numel() == 16 and not torch.equal(a, b)
    want = torch.sin(torch.arange(16, dtype=torch.float32) * 0.37 + 1) * 1.5 + 0.25
    assert torch.equal(a, want) and float(a.abs().max()) <= 1.75
