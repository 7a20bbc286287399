"""The golden encoder on the pictures of tests/intra_cases.py (no GPU): the precondition of
tests/test_gpu_intra.py.  On exactly those I pictures the golden model alone must code CUs of
all three sizes, a 32x32 CU with luma residual and a 16x16 CU with residual -- so an engine
that equals it there has been through the large TBs of the wave predictor -- and the stream
must decode to the encoder's reconstruction."""
import numpy as np
import pytest

from intra_cases import CASES, frame

from thinvids_amd.models import hevc


@pytest.mark.parametrize("w,h,qp", CASES, ids=[f"{w}x{h}-qp{qp}" for w, h, qp in CASES])
def test_i_picture_reaches_the_large_tbs(w, h, qp):
    enc = hevc.CpuEncoder(w, h, qp=qp)
    stream = enc.encode(frame(w, h), True, 0)
    d = enc.decisions()
    l2, cbf = d["cu_log2"], d["cbf"]
    assert d["intra"].all()
    assert set(np.unique(l2).tolist()) == {3, 4, 5}, np.unique(l2, return_counts=True)
    assert ((l2 == 5) & (cbf & 1 != 0)).any(), "no 32x32 CU with luma residual"
    assert ((l2 == 4) & (cbf != 0)).any(), "no 16x16 CU with residual"
    for got, want in zip(hevc.decode(stream).coded_frames[0], enc.recon()):
        np.testing.assert_array_equal(got, want)
