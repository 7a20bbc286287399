"""k_intra_recon / k_pintra_recon (csrc/gpu/k_intra.hip) through the engine on the pictures of
tests/intra_cases.py, where the golden encoder codes 16x16 and 32x32 intra CUs with residual
(the precondition is tests/test_intra_cpu.py): both segments of a two-segment batch, the
picture and its top-to-bottom mirror, each an I and a P picture, must be byte-equal to the
golden encoder, with and without sign data hiding (both instantiations of the kernels), and
the engine's last reconstruction must be the decoder's."""
import numpy as np
import pytest

from intra_cases import CASES, SEARCH_RANGE, frame, golden

from thinvids_amd.models import hevc


@pytest.mark.gpu
@pytest.mark.parametrize("sign_hiding", [False, True], ids=["plain", "sdh"])
@pytest.mark.parametrize("w,h,qp", CASES, ids=[f"{w}x{h}-qp{qp}" for w, h, qp in CASES])
def test_engine_equals_golden_on_large_intra_cus(w, h, qp, sign_hiding):
    from thinvids_amd.models.gpu_engine import GpuEngine

    eng = GpuEngine(width=w, height=h, qp=qp, batch=2, gop=2, search_range=SEARCH_RANGE, sign_hiding=sign_hiding)
    try:
        segs = eng.encode_frames([[frame(w, h, flip)] * 2 for flip in (False, True)])
        for b, flip in enumerate((False, True)):
            assert segs[b] == golden(w, h, qp, sign_hiding, flip)[0], f"segment {b}: GPU bitstream differs from the golden encoder"
            for got, want in zip(eng.last_recon(b), hevc.decode(segs[b]).coded_frames[-1]):
                np.testing.assert_array_equal(got, want)
    finally:
        eng.close()
