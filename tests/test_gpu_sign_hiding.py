"""Sign data hiding on the GPU (tv/sdh.h): k_inter_recon<true> keeps every coefficient's
distance from its level and adjusts one level per coefficient group after RDOQ-lite,
wave_code_tb<true> does the same for the intra recon kernels (I pictures and intra CUs of P
pictures, horizontal / vertical scans included), and the device CABAC coder leaves the hidden
sign bins out.  Everything is checked byte for byte against the CPU golden encoder with the
tool on: small and odd shapes, dense textured levels in every TB size with RQT splits,
intra-in-P quadrants and bi units, an IDR-only segment, full-swing content that puts the
coefficients and their distances at the ends of their ranges, both entropy back ends, and
one 1080p case.  Runs only on an MI355X."""
import numpy as np
import pytest

from thinvids_amd.models import hevc

pytestmark = pytest.mark.gpu

TEXTURED = 0x80000000


def _engine(**kw):
    from thinvids_amd.models.gpu_engine import GpuEngine
    return GpuEngine(sign_hiding=True, **kw)


def _assert_recon(eng, b, want):
    for got, w in zip(eng.last_recon(b), want):
        np.testing.assert_array_equal(got, w)


def _check_synthetic(w, h, qp, gop, seed, starts=(0, 20), rng=16, **kw):
    eng = _engine(width=w, height=h, qp=qp, batch=len(starts), gop=gop, search_range=rng, seed=seed, **kw)
    segs = eng.encode_synthetic(list(starts))
    ckw = {k: v for k, v in kw.items() if k != "entropy"}
    for b, start in enumerate(starts):
        frames = [hevc.synth_frame(seed, start + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=qp, search_range=rng, sign_hiding=True, **ckw)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        _assert_recon(eng, b, recons[-1])
    eng.close()
    return segs


@pytest.mark.parametrize("w,h,qp,sao,deblock", [(192, 128, 27, False, True), (160, 90, 32, True, True),
                                               (128, 64, 22, False, False)])
def test_small_shapes_equal_golden(w, h, qp, sao, deblock):
    """160x90 is not a multiple of the CTB."""
    _check_synthetic(w, h, qp, 4, 5, sao=sao, deblock=deblock)


@pytest.mark.parametrize("bframes,gop", [(1, 4), (2, 5)])
def test_textured_equals_golden(bframes, gop):
    """Dense levels: every TB size from chroma 4x4 to 32x32, RQT splits, intra-in-P quadrants
    and (bframes 2) bi-predicted units."""
    _check_synthetic(160, 96, 22, gop, 7 | TEXTURED, rng=32, bframes=bframes)


def test_idr_only_equals_golden():
    """gop 1: every picture is intra, so wave_code_tb<true> meets the horizontal and vertical
    scans of 8x8 luma and 4x4 chroma TBs."""
    _check_synthetic(160, 96, 22, 1, 7 | TEXTURED, starts=(0, 3))


def _checker(cell, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("name", ["checker1", "checker8"])
def test_full_swing_content_equals_golden(name):
    """Full-swing luma: the largest coefficients the transform gives."""
    w, h = 96, 64
    c = _checker(1 if name == "checker1" else 8, w, h)
    ys = [c, 255 - c, c] if name == "checker1" else [c, 255 - c, np.full((h, w), 255, np.uint8)]
    chroma = np.full((h // 2, w // 2), 128, np.uint8)
    frames = [(np.ascontiguousarray(y), chroma.copy(), chroma.copy()) for y in ys]
    eng = _engine(width=w, height=h, qp=27, batch=1, gop=3, search_range=16)
    seg = eng.encode_frames([frames])[0]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=16, sign_hiding=True)
    assert seg == cpu_bs, f"{name}: GPU bitstream differs from the golden encoder"
    _assert_recon(eng, 0, recons[-1])
    eng.close()


def test_host_and_gpu_entropy_give_the_same_bytes():
    kw = dict(w=160, h=96, qp=22, gop=4, seed=7 | TEXTURED, rng=32)
    assert _check_synthetic(entropy="host", **kw) == _check_synthetic(entropy="gpu", **kw)


def test_tool_off_is_the_default_stream():
    """The engine without the argument and with sign_hiding=False give the same bytes, which
    are the golden encoder's without the tool."""
    from thinvids_amd.models.gpu_engine import GpuEngine

    kw = dict(width=160, height=96, qp=22, batch=1, gop=3, search_range=16, seed=7 | TEXTURED)
    a, b = GpuEngine(**kw), GpuEngine(sign_hiding=False, **kw)
    sa, sb = a.encode_synthetic([0])[0], b.encode_synthetic([0])[0]
    a.close()
    b.close()
    frames = [hevc.synth_frame(7 | TEXTURED, f, 160, 96) for f in range(3)]
    assert sa == sb == hevc.encode_sequence_cpu(frames, qp=22, search_range=16)[0]


def test_full_size_equals_golden():
    w, h, gop, rng, seed, starts = 1920, 1080, 2, 64, 3, [0, 100]
    eng = _engine(width=w, height=h, qp=27, batch=2, gop=gop, search_range=rng, seed=seed)
    segs = eng.encode_synthetic(starts)
    frames = [hevc.synth_frame(seed, starts[1] + f, w, h) for f in range(gop)]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=rng, sign_hiding=True)
    assert segs[1] == cpu_bs, "segment 1: GPU bitstream differs from the golden encoder"
    _assert_recon(eng, 1, recons[-1])
    eng.close()
