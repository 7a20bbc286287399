"""AV1 GPU engine with chroma from luma (k_av1e_intra<true> / k_av1e_ib_recon<true>) against
the golden encoder with the same tool: mode words including the alpha bits, MVs, CDEF tables and
indices, restoration units, bitstream bytes and the last reconstruction are equal; with the
tool off the engine is the engine it was."""
import numpy as np
import pytest
from av1_cfl_cases import CLIPS, assert_paths, cfl_blocks, golden

from thinvids_amd.models import av1, avif

pytestmark = pytest.mark.gpu


def engine_vs_golden(w, h, cases, q, engine_kw=None, **tools):
    """Encode the segments (`cases`: clip kinds of av1_cfl_cases or lists of frames, equal
    lengths) as one batch on the engine and one by one with the golden encoder (cfl on plus
    `tools`); everything the two decide must be equal.  Returns (GopHost, [segment streams],
    [GoldenResult])."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H = av1.coded_size(w, h)
    segs, golds = [], []
    for c in cases:
        if isinstance(c, tuple):  # (kind, frame count): the shared, cached golden encode
            fr, gold = golden(c[0], w, h, c[1], q, **tools)
        else:
            fr, gold = c, av1.golden_encode(c, w, h, q, cfl=True, **tools)
        segs.append(fr)
        golds.append(gold)
    n = len(segs[0])
    eng = Av1GpuEngine(w, h, batch=len(segs), qindex=q, **({"cfl": True, **tools} if engine_kw is None else engine_kw))
    dev = eng.dev

    def load(t, planes):
        for b, fr in enumerate(segs):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[b].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(dev))

    streams = []
    try:
        g = eng.encode_gop(n, load)
        futs = eng.submit_entropy(g)
        for b, gold in enumerate(golds):
            if tools.get("intra_in_inter"):
                np.testing.assert_array_equal(g.ib[:, b], gold.ib, err_msg=f"segment {b}: candidate / accepted map")
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


# key frames at the smallest geometries: one block (no neighbour, dc 128), one neighbour
# direction each, a partial superblock; then the quantiser's ends
KEY_CASES = [(16, 16, 100), (32, 16, 100), (16, 32, 100), (72, 40, 100), (72, 40, 1), (72, 40, 255)]


@pytest.mark.parametrize("w,h,q", KEY_CASES, ids=[f"{w}x{h}-q{q}" for w, h, q in KEY_CASES])
def test_key_frame_matches_golden(w, h, q):
    g, _, _ = engine_vs_golden(w, h, [("corr", 1)], q)
    assert cfl_blocks(g.mode[:, 0])[0].any(), "no CfL block"
    if (w, h, q) == (72, 40, 100):
        assert_paths("corr", g.mode[:, 0])


@pytest.mark.parametrize("kind", ["saturated", "steep", "one_plane"])
def test_sample_range_and_alpha_edges(kind):
    """Predictions that clip at 0 / 255, |alpha| = 16, and a plane whose alpha symbol is skipped."""
    g, _, _ = engine_vs_golden(72, 40, [(kind, 2 if kind == "saturated" else 1)], 100)
    if kind == "saturated":
        assert cfl_blocks(g.mode[:, 0])[0].any()
    else:
        assert_paths(kind, g.mode[:, 0])


def test_batch_of_correlated_and_flat_segments():
    """A correlated segment beside one with constant luma: den = 0 in every block there, so
    it has no CfL block, whatever its neighbour in the batch does."""
    w, h = 200, 136
    g, _, _ = engine_vs_golden(w, h, [("corr", 2), ("flat", 2)], 100)
    assert_paths("corr", g.mode[:, 0])
    assert_paths("flat", g.mode[:, 1])


def test_cfl_in_intra_blocks_of_inter_frames():
    w, h = 200, 136
    g, _, _ = engine_vs_golden(w, h, [("cut", 4)], 100, intra_in_inter=True)
    assert (g.ib[2, 0] >> 1).any(), "the cut frame has no intra block"
    assert cfl_blocks(g.mode[2, 0])[0].any(), "no intra block of the cut frame uses CfL"


def test_1080p_key_frame_and_inter_frame():
    w, h = 1920, 1080
    g, _, _ = engine_vs_golden(w, h, [CLIPS["corr"](w, h, 2)], 100)
    assert cfl_blocks(g.mode[0, 0])[0].sum() > 100


def test_engine_stream_decodes_with_dav1d():
    if not avif.dav1d_available():
        pytest.skip("libavif / dav1d (Pillow AVIF plugin) missing")
    from test_av1_conformance import _check as dav1d_check

    w, h = 200, 136
    _, streams, golds = engine_vs_golden(w, h, [("corr", 4)], 100)
    dav1d_check(streams[0], golds[0].tu_sizes, golds[0].recon, w, h)


def test_tool_off_is_the_default_engine():
    w, h, q = 200, 136, 100
    fr = CLIPS["corr"](w, h, 2)
    gold = av1.golden_encode(fr, w, h, q)
    out = []
    for kw in ({}, {"cfl": False}):
        import torch

        from thinvids_amd.models.av1_engine import Av1GpuEngine

        W, H = av1.coded_size(w, h)
        eng = Av1GpuEngine(w, h, batch=1, qindex=q, **kw)

        def load(t, planes):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[0].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(eng.dev))

        try:
            g = eng.encode_gop(2, load)
            out.append((g.mode.copy(), b"".join(eng.submit_entropy(g)[0].result())))
        finally:
            eng.close()
    assert out[0][1] == out[1][1] == gold.stream
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][0][:, 0], gold.mode)
    assert not (out[0][0] >> 15).any() and not (((out[0][0] >> 5) & 15) == 13).any()
