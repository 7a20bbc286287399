"""Rate-distortion quantisation on the GPU (tv/rdq.h): k_inter_recon<kSdh, true> keeps every
coefficient's distance from its dead-zone level and, in the place of RDOQ-lite, chooses the
levels by cost, one thread per coefficient group with per-TB reductions; with sign hiding
on as well (<true, true>) the sign-hiding pass works on the distance from the final level.
Every case compares the bitstream byte for byte and the last reconstruction sample for sample
with the CPU golden encoder: small and odd shapes, dense textured levels in every TB size
with RQT splits, intra-in-P quadrants and bi units, full-swing content that puts the
coefficients and their distances at the ends of their ranges, enough CTBs for the XCD
remap, and both entropy back ends.  Runs only on an MI355X."""
import numpy as np
import pytest

from thinvids_amd.models import hevc

pytestmark = pytest.mark.gpu

TEXTURED = 0x80000000
SDH = pytest.mark.parametrize("sign_hiding", [False, True], ids=["rdq", "rdq+sdh"])


def _engine(**kw):
    from thinvids_amd.models.gpu_engine import GpuEngine
    return GpuEngine(rd_quant=True, **kw)


def _assert_recon(eng, b, want):
    for got, w in zip(eng.last_recon(b), want):
        np.testing.assert_array_equal(got, w)


def _check_synthetic(w, h, qp, gop, seed, starts=(0, 20), rng=16, **kw):
    eng = _engine(width=w, height=h, qp=qp, batch=len(starts), gop=gop, search_range=rng, seed=seed, **kw)
    segs = eng.encode_synthetic(list(starts))
    ckw = {k: v for k, v in kw.items() if k != "entropy"}
    for b, start in enumerate(starts):
        frames = [hevc.synth_frame(seed, start + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=qp, search_range=rng, rd_quant=True, **ckw)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        _assert_recon(eng, b, recons[-1])
    eng.close()
    return segs


@SDH
@pytest.mark.parametrize("w,h,qp,sao,deblock", [(192, 128, 27, False, True), (160, 90, 32, True, True),
                                               (128, 64, 22, False, False)])
def test_small_shapes_equal_golden(w, h, qp, sao, deblock, sign_hiding):
    """160x90 is not a multiple of the CTB."""
    _check_synthetic(w, h, qp, 4, 5, sao=sao, deblock=deblock, sign_hiding=sign_hiding)


@SDH
@pytest.mark.parametrize("bframes,gop", [(1, 4), (2, 5)])
def test_textured_equals_golden(bframes, gop, sign_hiding):
    """Dense levels: every TB size from chroma 4x4 to 32x32, RQT splits, intra-in-P quadrants
    next to inter TBs and (bframes 2) bi-predicted units."""
    _check_synthetic(160, 96, 22, gop, 7 | TEXTURED, rng=32, bframes=bframes, sign_hiding=sign_hiding)


def _checker(cell, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)


@SDH
@pytest.mark.parametrize("name", ["checker1", "checker8"])
def test_full_swing_content_equals_golden(name, sign_hiding):
    """Full-swing luma: the largest coefficients the transform gives."""
    w, h = 96, 64
    c = _checker(1 if name == "checker1" else 8, w, h)
    ys = [c, 255 - c, c] if name == "checker1" else [c, 255 - c, np.full((h, w), 255, np.uint8)]
    chroma = np.full((h // 2, w // 2), 128, np.uint8)
    frames = [(np.ascontiguousarray(y), chroma.copy(), chroma.copy()) for y in ys]
    eng = _engine(width=w, height=h, qp=27, batch=1, gop=3, search_range=16, sign_hiding=sign_hiding)
    seg = eng.encode_frames([frames])[0]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=16, rd_quant=True, sign_hiding=sign_hiding)
    assert seg == cpu_bs, f"{name}: GPU bitstream differs from the golden encoder"
    _assert_recon(eng, 0, recons[-1])
    eng.close()


@SDH
def test_many_ctbs_equal_golden(sign_hiding):
    """640x360: enough CTBs for the XCD remap of the CTB index."""
    _check_synthetic(640, 360, 27, 3, 3, starts=(0,), sign_hiding=sign_hiding)


@SDH
def test_host_and_gpu_entropy_give_the_same_bytes(sign_hiding):
    kw = dict(w=160, h=96, qp=22, gop=4, seed=7 | TEXTURED, rng=32, starts=(0,), sign_hiding=sign_hiding)
    assert _check_synthetic(entropy="host", **kw) == _check_synthetic(entropy="gpu", **kw)


def test_tool_off_is_the_default_stream():
    """The engine without the argument and with rd_quant=False give the same bytes, which are
    the golden encoder's without the tool."""
    from thinvids_amd.models.gpu_engine import GpuEngine

    kw = dict(width=160, height=96, qp=22, batch=1, gop=3, search_range=16, seed=7 | TEXTURED)
    a, b = GpuEngine(**kw), GpuEngine(rd_quant=False, **kw)
    sa, sb = a.encode_synthetic([0])[0], b.encode_synthetic([0])[0]
    a.close()
    b.close()
    frames = [hevc.synth_frame(7 | TEXTURED, f, 160, 96) for f in range(3)]
    assert sa == sb == hevc.encode_sequence_cpu(frames, qp=22, search_range=16)[0]
