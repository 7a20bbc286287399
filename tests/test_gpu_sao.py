"""k_sao_decide (csrc/gpu/k_frame.hip) on its own, through tv_sao_batch: one workgroup per strip
of four CTBs, one wave per CTB.  The kernel must equal the golden model (tv_sao_picture_cpu)
exactly in the parameters and in all three filtered planes, and its SSE must be the integer
sum over the display area, at every geometry and content of tests/sao_cases.py; the
precondition that those inputs reach every path is tests/test_sao_cpu.py.  One engine-level
case codes a 288x64 sequence (two full strips + one) with B pictures against the golden
encoder."""
import numpy as np
import pytest

from sao_cases import CASES, QPS, display_sse, golden, pictures

from thinvids_amd.models import hevc


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kind", CASES, ids=[f"{w}x{h}-{kind}" for w, h, kind in CASES])
def test_kernel_equals_golden(w, h, kind):
    from thinvids_amd.ops import stage

    src, deb = pictures(w, h, kind)
    params, out, sse = stage.sao_pictures(src, deb, w, h, QPS, "cuda:0")
    for b, (want_params, want_out) in enumerate(golden(w, h, kind)):
        np.testing.assert_array_equal(params[b], want_params, err_msg=f"picture {b} (QP {QPS[b]}): parameters")
        for c in range(3):
            np.testing.assert_array_equal(out[b][c], want_out[c], err_msg=f"picture {b} (QP {QPS[b]}): plane {c}")
        assert sse[b].tolist() == display_sse(w, h, src[b], want_out), f"picture {b} (QP {QPS[b]}): SSE"


@pytest.mark.gpu
def test_engine_equals_golden_with_strips():
    from thinvids_amd.models.gpu_engine import GpuEngine

    w, h, gop, starts = 288, 64, 5, [0, 20]
    opt = dict(qp=27, sao=True, bframes=2)
    eng = GpuEngine(width=w, height=h, batch=2, gop=gop, search_range=64, seed=7, **opt)
    segs = eng.encode_synthetic(starts)
    for b in range(2):
        frames = [hevc.synth_frame(7, starts[b] + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, search_range=64, **opt)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        for got, want in zip(eng.last_recon(b), recons[-1]):
            np.testing.assert_array_equal(got, want)
    eng.close()
