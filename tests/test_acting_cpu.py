"""acting.GraphedAct.input_rows: when a producer may write straight into a captured pass's input buffers."""
import torch

from settlers_of_catan_rl_amd.acting import GraphedAct


def _captured(B, obs_dtype=torch.bfloat16, lens_dtype=torch.int32):
    """a GraphedAct whose bucket B holds hand-filled input buffers (no graph: input_rows looks at the buffers only)"""
    ga = GraphedAct(None, buckets=(B,))
    ga.graphs[B] = {"f": torch.zeros((B, 7), dtype=obs_dtype), "lists": torch.zeros((B, 5, 25), dtype=torch.int32),
                    "lens": torch.ones((B, 5), dtype=lens_dtype), "masks": torch.ones((B, 325), dtype=torch.float32)}
    return ga


def test_input_rows_only_of_a_captured_bucket_with_the_producers_dtypes():
    assert GraphedAct(None, buckets=(8,)).input_rows(8, 3, torch.bfloat16) is None            # before the capture
    ga = _captured(8)
    assert ga.input_rows(16, 3, torch.bfloat16) is None                                       # another bucket
    assert ga.input_rows(8, 3, torch.float32) is None                                         # the env would write fp32 observations
    assert _captured(8, lens_dtype=torch.int64).input_rows(8, 3, torch.bfloat16) is None      # the env writes int32 lens
    for n in (1, 3, 8):
        rows = ga.input_rows(8, n, torch.bfloat16)
        assert len(rows) == 4
        for r, k in zip(rows, ("f", "lists", "lens", "masks")):
            buf = ga.graphs[8][k]
            assert r.shape == (n,) + buf.shape[1:] and r.dtype == buf.dtype and r.data_ptr() == buf.data_ptr() and r.is_contiguous()
            r.fill_(5)
            assert bool((buf[:n] == 5).all()) and bool((buf[n:] != 5).all())                 # exactly n rows, aliasing the buffer
            buf.fill_(0)
