"""AV1 GPU engine with intra blocks in inter frames (k_av1e_ib_*) against the golden encoder
with the same tool: mode words, MVs, the candidate / accepted map, CDEF tables and indices,
restoration units, bitstream bytes and the last reconstruction are equal; with the tool off
the engine is the engine it was."""
import numpy as np
import pytest
from av1_ib_cases import CUT_CASES, CUT_IDS, cut_clip, static_clip

from thinvids_amd.models import av1, avif, hevc

pytestmark = pytest.mark.gpu


def engine_vs_golden(w, h, segs, q, intra_in_inter=True, engine_kw=None):
    """Encode the segments (lists of display-size frames, equal lengths) as one batch on the
    engine and one by one with the golden encoder; everything the two decide must be equal.
    Returns (GopHost, [segment streams], [GoldenResult])."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H = av1.coded_size(w, h)
    nframes = len(segs[0])
    kw = {"intra_in_inter": intra_in_inter} if engine_kw is None else engine_kw
    eng = Av1GpuEngine(w, h, batch=len(segs), qindex=q, **kw)
    dev = eng.dev

    def load(t, planes):
        for b, fr in enumerate(segs):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[b].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(dev))

    golds, streams = [], []
    try:
        g = eng.encode_gop(nframes, load)
        futs = eng.submit_entropy(g)
        for b, fr in enumerate(segs):
            gold = av1.golden_encode(fr, w, h, q, intra_in_inter=intra_in_inter)
            golds.append(gold)
            if intra_in_inter:
                np.testing.assert_array_equal(g.ib[:, b], gold.ib, err_msg=f"segment {b}: candidate / accepted map")
            else:
                assert g.ib is None
            np.testing.assert_array_equal(g.mode[:, b], gold.mode, err_msg=f"segment {b}: mode words")
            np.testing.assert_array_equal(g.mv[:, b], gold.mv, err_msg=f"segment {b}: motion vectors")
            np.testing.assert_array_equal(g.tabs[:, b, :8], gold.fparams[:, 9:17])
            np.testing.assert_array_equal(g.tabs[:, b, 8:], gold.fparams[:, 17:25])
            np.testing.assert_array_equal(g.fbidx[:, b], gold.cdef_idx)
            np.testing.assert_array_equal(g.lr[:, b], gold.lr, err_msg=f"segment {b}: restoration units")
            streams.append(b"".join(futs[b].result()))
            assert streams[b] == gold.stream, f"segment {b}: GPU bitstream differs from the golden encoder"
            fin = np.concatenate([x[b].cpu().numpy().reshape(-1) for x in eng.fin])
            np.testing.assert_array_equal(fin, gold.recon[-1], err_msg=f"segment {b}: last reconstruction")
    finally:
        eng.close()
    return g, streams, golds


@pytest.mark.parametrize("w,h,q,kind", CUT_CASES, ids=CUT_IDS)
def test_engine_matches_golden_on_cut_clips(w, h, q, kind):
    g, _, _ = engine_vs_golden(w, h, [cut_clip(w, h, kind)], q)
    assert ((g.mode[2, 0] & 1) == 0).any(), "the cut frame has no intra block"


def test_batch_of_cut_and_static_segments():
    """One segment with the cut, one repeated static frame: no candidate there (a per-segment
    count of zero in every pass) and its skip blocks still merge to 32x32 / 64x64."""
    w, h = 200, 136
    g, _, _ = engine_vs_golden(w, h, [cut_clip(w, h), static_clip(w, h)], 120)
    assert (g.ib[2, 0] >> 1).any()
    assert not g.ib[:, 1].any()
    assert (((g.mode[1:, 1] >> 13) & 3) == 2).any(), "no 64x64 merged block in the static segment"


def test_1080p_key_frame_and_unrelated_frame():
    w, h = 1920, 1080
    fr = [tuple(hevc.synth_frame(7, 0, w, h)), tuple(hevc.synth_frame(23, 41, w, h))]
    g, _, _ = engine_vs_golden(w, h, [fr], 100)
    assert (g.ib[1, 0] >> 1).sum() > 0


def test_engine_cut_stream_decodes_with_dav1d():
    if not avif.dav1d_available():
        pytest.skip("libavif / dav1d (Pillow AVIF plugin) missing")
    from test_av1_conformance import _check as dav1d_check

    w, h = 200, 136
    _, streams, golds = engine_vs_golden(w, h, [cut_clip(w, h)], 100)
    dav1d_check(streams[0], golds[0].tu_sizes, golds[0].recon, w, h)


def test_tool_off_is_the_default_engine():
    w, h, q = 200, 136, 100
    segs = [cut_clip(w, h)]
    a, sa, _ = engine_vs_golden(w, h, segs, q, intra_in_inter=False, engine_kw={})
    b, sb, _ = engine_vs_golden(w, h, segs, q, intra_in_inter=False)
    assert sa == sb
    np.testing.assert_array_equal(a.mode, b.mode)
    assert (a.mode[1:] & 1).all()
