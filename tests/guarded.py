"""The buffers of the kernel pin suites: inputs that end (and may begin) in a guard value, outputs between margins of a sentinel pattern,
and the checks that the margins came back untouched and that every element was written.  Every allocation takes a `device`, so that
tests/test_guarded_cpu.py can hold these helpers to account without a GPU.

Each suite keeps its own numbers - how many rows or elements of margin, which sentinel (SENTINEL16 or SENTINEL32: the same bytes, so a
margin reads the same under either; the width is the word that `written` looks for) - and its own alignment assertions."""
import ctypes as C

import torch

NAN = float("nan")
SENTINEL16 = 0x5A5B              # a bf16 bit pattern (1.5e13) no kernel result is likely to equal, and not symmetric in its bytes
SENTINEL32 = 0x5A5B5A5B
_WORD = {SENTINEL16: torch.int16, SENTINEL32: torch.int32}


def ptr(t, byte_offset=0):
    """the ctypes pointer to t's first element (+ byte_offset); None for None"""
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded_input(t, tail, lead=0, guard=NAN, device="cuda"):
    """t's elements with `lead` elements of `guard` in front and `tail` behind (NaN: a read outside t that is used poisons a result; an
    integer input's guard is the caller's) -> (whole, view), both flat, whole 16-byte aligned"""
    n = t.numel()
    whole = torch.full((lead + n + tail,), guard, dtype=t.dtype, device=device)
    assert whole.data_ptr() % 16 == 0
    view = whole[lead:lead + n]
    view.copy_(t.reshape(-1))
    return whole, view


def sentinel_output(n, dtype, tail, lead=0, sentinel=SENTINEL16, device="cuda"):
    """n elements of `dtype` with `lead` elements in front and `tail` behind, every 16- or 32-bit word of the allocation pre-set to the
    sentinel -> (whole, view), both flat, whole 16-byte aligned"""
    whole = torch.empty(lead + n + tail, dtype=dtype, device=device)
    assert whole.data_ptr() % 16 == 0
    whole.view(_WORD[sentinel]).fill_(sentinel)
    return whole, whole[lead:lead + n]


def _margins(whole, view):
    """-> (the 16-bit words of whole, the first word of the view, the first word behind it)"""
    k = whole.element_size() // 2
    lead = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    return whole.reshape(-1).view(torch.int16), lead * k, (lead + view.numel()) * k


def intact(whole, view):
    """every word in front of the view and behind it still holds the sentinel"""
    w, a, z = _margins(whole, view)
    return bool((w[:a] == SENTINEL16).all()) and bool((w[z:] == SENTINEL16).all())


def written(whole, view, sentinel):
    """no sentinel word is left inside the view: words of the sentinel's width, of the element's where that is narrower (a bf16 output
    under SENTINEL32).  Ask it with a sentinel as wide as the elements or wider: half of an fp32 result may equal SENTINEL16 by chance."""
    w, a, z = _margins(whole, view)
    left = w[a:z] == SENTINEL16
    if sentinel == SENTINEL32 and whole.element_size() >= 4:
        left = left.view(-1, 2).all(1)
    return not bool(left.any())


def pattern(n, k, device="cuda"):
    """a non-constant fp32 pre-fill of an accumulator of n words, another one for every k"""
    return torch.sin(torch.arange(n, device=device, dtype=torch.float32) * 0.37 + k) * 1.5 + 0.25 * k
