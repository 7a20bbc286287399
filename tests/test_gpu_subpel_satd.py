"""The SATD sub-pel decision on the GPU (k_inter_me<true>, csrc/gpu/k_inter.hip): every
(8x8 group, candidate) cell of the half- and quarter-pel rounds goes through two
v_mfma_f32_16x16x16f16 as one of four cells of a 16x16 tile.  Everything is checked byte for
byte against the CPU golden encoder with the tool on: small shapes with clamped border cells,
content at the f16 / f32 bounds of the transform (|Y| = 2040, |Z| = 16320), textured content
whose tiles mix cells of different blocks and candidates (a wrong k order or a cross-cell mix
shows there; a transposed cell would not: SATD(X) = SATD(X^T)), the B path, and one 1080p
case.  Runs only on an MI355X."""
import numpy as np
import pytest

from thinvids_amd.models import hevc

pytestmark = pytest.mark.gpu


def _engine(**kw):
    from thinvids_amd.models.gpu_engine import GpuEngine
    return GpuEngine(subpel_satd=True, **kw)


def _flat(v, w, h):
    return np.full((h, w), v, np.uint8)


def _checker(cell, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)


def _saturating_sequences(w, h):
    c1, c8 = _checker(1, w, h), _checker(8, w, h)
    return {"flat": [_flat(0, w, h), _flat(255, w, h), _flat(0, w, h)],
            "checker1": [c1, 255 - c1, c1],
            "checker8": [c8, 255 - c8, _flat(255, w, h)]}


def _assert_recon(eng, b, want):
    for got, w in zip(eng.last_recon(b), want):
        np.testing.assert_array_equal(got, w)


@pytest.mark.parametrize("name", ["flat", "checker1", "checker8"])
def test_saturating_content_equals_golden(name):
    """Full-swing luma between consecutive frames: every difference is +-255, so the first
    product reaches 2040 and the second 16320 in one coefficient per cell."""
    w, h = 96, 64
    chroma = _flat(128, w // 2, h // 2)
    frames = [(np.ascontiguousarray(y), chroma.copy(), chroma.copy()) for y in _saturating_sequences(w, h)[name]]
    eng = _engine(width=w, height=h, qp=27, batch=1, gop=3, search_range=16)
    seg = eng.encode_frames([frames])[0]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=16, subpel_satd=True)
    assert seg == cpu_bs, f"{name}: GPU bitstream differs from the golden encoder"
    _assert_recon(eng, 0, recons[-1])
    eng.close()


@pytest.mark.parametrize("w,h,qp,sao,deblock", [(192, 128, 27, False, True), (160, 90, 32, True, True),
                                               (128, 64, 22, False, False)])
def test_small_shapes_equal_golden(w, h, qp, sao, deblock):
    """160x90 is not a multiple of the CTB: its bottom cells read the clamped border."""
    gop, rng, seed, starts = 4, 16, 5, [0, 20]
    eng = _engine(width=w, height=h, qp=qp, batch=2, gop=gop, search_range=rng, sao=sao, deblock=deblock, seed=seed)
    segs = eng.encode_synthetic(starts)
    for b, start in enumerate(starts):
        frames = [hevc.synth_frame(seed, start + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=qp, sao=sao, deblock=deblock, search_range=rng,
                                                  subpel_satd=True)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        _assert_recon(eng, b, recons[-1])
    eng.close()


# bframes=2 / gop 5 is the smallest hierarchical-B configuration of tests/test_bframes.py
@pytest.mark.parametrize("bframes,gop", [(1, 4), (2, 5)])
def test_textured_and_b_path_equal_golden(bframes, gop):
    """Distinct vectors per block, so every tile mixes cells of different blocks and
    candidates; with B pictures the per-list results go through CtbMeOut to k_bi_decide."""
    w, h, rng = 160, 96, 32
    seed = 7 | 0x80000000
    eng = _engine(width=w, height=h, qp=27, batch=2, gop=gop, search_range=rng, sao=False, seed=seed, bframes=bframes)
    segs = eng.encode_synthetic([0, 20])
    for b, start in enumerate([0, 20]):
        frames = [hevc.synth_frame(seed, start + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, sao=False, search_range=rng, bframes=bframes,
                                                  subpel_satd=True)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        _assert_recon(eng, b, recons[-1])  # the last display frame is coded as P
    eng.close()


def test_full_size_equals_golden():
    w, h, gop, rng, seed, starts = 1920, 1080, 2, 64, 3, [0, 100]
    eng = _engine(width=w, height=h, qp=27, batch=2, gop=gop, search_range=rng, seed=seed)
    segs = eng.encode_synthetic(starts)
    frames = [hevc.synth_frame(seed, starts[1] + f, w, h) for f in range(gop)]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=rng, subpel_satd=True)
    assert segs[1] == cpu_bs, "segment 1: GPU bitstream differs from the golden encoder"
    _assert_recon(eng, 1, recons[-1])
    eng.close()
