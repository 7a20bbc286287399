"""What models/av1_engine.py takes from csrc/include/tv/av1_enc.h through the core library
(tv_av1c_model_constants / tv_av1c_model_q) against independent statements of the same model:
the closed forms the engine used to carry, and the literal CDEF preset lists.  No GPU."""
import numpy as np

from thinvids_amd.models import av1
from thinvids_amd.models import av1_engine as eng


def test_per_q_tables_equal_the_closed_forms():
    assert eng.LF_LEVEL.shape == eng.LR_RATE.shape == eng.CDEF_DAMPING.shape == (256,)
    for q in range(1, 256):
        a = av1.ac_q(q)
        assert eng.LF_LEVEL[q] == min(63, max(0, (a * 20723 + 1015158) >> 18)), q
        assert eng.LR_RATE[q] == ((a * a * 9) >> 10) * 16, q
        assert eng.CDEF_DAMPING[q] == 3 + (q >> 6), q
    assert eng.LR_RATE.dtype == np.int64 and eng.LF_LEVEL.dtype == np.int32  # uploaded as they are


def test_cdef_masks_equal_the_preset_lists():
    mask = lambda pri, sec: sum(1 << (p * 4 + s) for p in pri for s in sec)  # preset = pri * 4 + sec index
    assert eng.CDEF_MASK_Y == mask((0, 1, 2, 3, 5, 7, 10, 13), (0, 2))
    assert eng.CDEF_MASK_UV == mask((0, 2, 4, 7), (0, 2))


def test_constants_and_tool_bits_equal_the_export():
    assert (av1.TOOL_INTRA_IN_INTER, av1.TOOL_CFL) == (eng.TOOL_INTRA_IN_INTER, eng.TOOL_CFL) == (1, 2)
    assert eng.LR_SETS == (4, 10)
    assert eng.MEMO_RECORD_BYTES == 11 * 8 + 1 and eng.IB_PASSES == 7  # av1_enc.h kMvRefineMaxCand, kIbPasses today


def test_out_of_the_filter_ops_is_checked_before_a_launch():
    """ops.av1's `out=`: the wrong shape or dtype is refused, and so is an output that is an
    input of a kernel reading neighbouring tiles (the workspace's aliasing rule)."""
    import pytest
    import torch

    from thinvids_amd.ops import av1 as ops

    a = torch.zeros((2, 8, 8), dtype=torch.uint8)
    good = torch.zeros_like(a)
    assert ops._out(good, a.shape, torch.uint8, a, apart=(a,)) is good
    assert ops._out(None, a.shape, torch.uint8, a).shape == a.shape
    for bad, apart in ((a, (a,)), (torch.zeros((2, 8, 4), dtype=torch.uint8), ()), (good.to(torch.int32), ()),
                       (good.transpose(1, 2), ())):
        with pytest.raises(ValueError):
            ops._out(bad, a.shape, torch.uint8, a, apart=apart)
