"""Motion-search SADs of the GPU engine (k_coarse_me / k_inter_me, csrc/gpu/k_inter.hip) at
their numeric limits and at picture edges: the coarse search accumulates four positions in
packed 16-bit lanes, so an accumulator carried past one 8x8 block would show on saturating
content first, and the half-pel round takes several candidates' SADs from one patch that is
clamped at the picture border.  Everything is checked byte for byte against the CPU golden
encoder.  Runs only on an MI355X."""
import numpy as np
import pytest

from thinvids_amd.models import hevc

pytestmark = pytest.mark.gpu


def _engine(**kw):
    from thinvids_amd.models.gpu_engine import GpuEngine
    return GpuEngine(**kw)


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


@pytest.mark.parametrize("name", ["flat", "checker1", "checker8"])
def test_saturating_sads_equal_golden(name):
    """Full-swing luma between consecutive frames: in the flat case every 8x8 SAD is 16320
    (the u16 lane limit is 65535), every 16x16 SAD 65280 and every 32x32 SAD 261120."""
    w, h = 96, 64
    chroma = _flat(128, w // 2, h // 2)
    frames = [(np.ascontiguousarray(y), chroma.copy(), chroma.copy()) for y in _saturating_sequences(w, h)[name]]
    eng = _engine(width=w, height=h, qp=27, batch=1, gop=3, search_range=16)
    seg = eng.encode_frames([frames])[0]
    cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, search_range=16)
    assert seg == cpu_bs, f"{name}: GPU bitstream differs from the golden encoder"
    for got, want in zip(eng.last_recon(0), recons[-1]):
        np.testing.assert_array_equal(got, want)
    eng.close()


# bframes=2 / gop 5 is the smallest hierarchical-B configuration of tests/test_bframes.py
@pytest.mark.parametrize("bframes,gop", [(1, 4), (2, 5)])
def test_edges_and_distinct_vectors_equal_golden(bframes, gop):
    """Textured content (distinct vectors per block, candidate windows clamped at every
    picture edge) through the P path and, with B pictures, the per-list search outputs."""
    w, h, rng = 160, 96, 32
    seed = 7 | 0x80000000
    eng = _engine(width=w, height=h, qp=27, batch=2, gop=gop, search_range=rng, sao=False, seed=seed, bframes=bframes)
    segs = eng.encode_synthetic([0, 20])
    for b, start in enumerate([0, 20]):
        frames = [hevc.synth_frame(seed, start + f, w, h) for f in range(gop)]
        cpu_bs, recons = hevc.encode_sequence_cpu(frames, qp=27, sao=False, search_range=rng, bframes=bframes)
        assert segs[b] == cpu_bs, f"segment {b}: GPU bitstream differs from the golden encoder"
        for got, want in zip(eng.last_recon(b), recons[-1]):  # the last display frame is coded as P
            np.testing.assert_array_equal(got, want)
    eng.close()
