"""AV1 GPU engine with the transform split (the TXS instantiation of k_av1e_inter's recon stage, the
split-aware level packing and deblocking info) against the golden encoder with the same tool: mode
words including the split bit and quadrant mask, MVs, CDEF tables and indices, restoration units,
bitstream bytes and the last reconstruction are equal; with the tool off the engine is the engine
it was."""
import numpy as np
import pytest
from av1_tx_cases import CLIPS, PATHS_FRAMES, PATHS_SIZE, assert_paths, golden, split_blocks

from thinvids_amd.models import av1, avif

pytestmark = pytest.mark.gpu
PW, PH = PATHS_SIZE


def _run_engine(w, h, segs, q, **engine_kw):
    """One GOP of the segments (lists of frames, equal lengths) as one batch: (GopHost, [segment
    streams], [last reconstruction per segment])."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H = av1.coded_size(w, h)
    eng = Av1GpuEngine(w, h, batch=len(segs), qindex=q, **engine_kw)

    def load(t, planes):
        for b, fr in enumerate(segs):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[b].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(eng.dev))

    try:
        g = eng.encode_gop(len(segs[0]), load)
        streams = [b"".join(f.result()) for f in eng.submit_entropy(g)]
        fins = [np.concatenate([x[b].cpu().numpy().reshape(-1) for x in eng.fin]) for b in range(len(segs))]
    finally:
        eng.close()
    return g, streams, fins


def engine_vs_golden(w, h, cases, q, **tools):
    """Encode the segments (`cases`: (clip kind of av1_tx_cases, frame count)) as one batch on the
    engine and one by one with the golden encoder (tx_split on plus `tools`); everything the two
    decide must be equal.  Returns (GopHost, [segment streams], [GoldenResult])."""
    pairs = [golden(kind, w, h, n, q, **tools) for kind, n in cases]
    g, streams, fins = _run_engine(w, h, [fr for fr, _ in pairs], q, tx_split=True, **tools)
    golds = [gold for _, gold in pairs]
    for b, gold in enumerate(golds):
        if tools.get("intra_in_inter"):
            np.testing.assert_array_equal(g.ib[:, b], gold.ib, err_msg=f"segment {b}: candidate / accepted map")
        np.testing.assert_array_equal(g.mode[:, b], gold.mode, err_msg=f"segment {b}: mode words")
        np.testing.assert_array_equal(g.mv[:, b], gold.mv, err_msg=f"segment {b}: motion vectors")
        np.testing.assert_array_equal(g.tabs[:, b, :8], gold.fparams[:, 9:17])
        np.testing.assert_array_equal(g.tabs[:, b, 8:], gold.fparams[:, 17:25])
        np.testing.assert_array_equal(g.fbidx[:, b], gold.cdef_idx)
        np.testing.assert_array_equal(g.lr[:, b], gold.lr, err_msg=f"segment {b}: restoration units")
        assert streams[b] == gold.stream, f"segment {b}: GPU bitstream differs from the golden encoder"
        np.testing.assert_array_equal(fins[b], gold.recon[-1], err_msg=f"segment {b}: last reconstruction")
    return g, streams, golds


# the smallest geometries: one block (no neighbour context), one neighbour direction each, a
# partial superblock at the quantiser's ends; then the size whose paths are asserted
CASES = [(16, 16, 100), (32, 16, 100), (16, 32, 100), (72, 40, 1), (72, 40, 100), (72, 40, 255), (PW, PH, 100)]


@pytest.mark.parametrize("w,h,q", CASES, ids=[f"{w}x{h}-q{q}" for w, h, q in CASES])
def test_speckle_matches_golden(w, h, q):
    g, _, _ = engine_vs_golden(w, h, [("speckle", PATHS_FRAMES)], q)
    split, _ = split_blocks(g.mode[:, 0])
    if (w, h) == PATHS_SIZE:
        assert_paths("speckle", g.mode[:, 0])
    elif (w, h) != (16, 16) and q != 255:
        assert split.any(), "no split block"


def test_saturated_stripes():
    g, _, _ = engine_vs_golden(72, 40, [("saturated", 2)], 100)
    assert split_blocks(g.mode[:, 0])[0].any()


def test_batch_of_speckle_and_ramp_segments():
    g, _, _ = engine_vs_golden(PW, PH, [("speckle", 3), ("ramp", 3)], 100)
    assert_paths("speckle", g.mode[:, 0])
    assert_paths("ramp", g.mode[:, 1])


@pytest.mark.parametrize("tools", [{}, {"cfl": True, "dir_intra": True}], ids=["plain", "cfl-dir"])
def test_intra_blocks_of_tx_select_frames(tools):
    g, _, _ = engine_vs_golden(PW, PH, [("cut", 4)], 100, intra_in_inter=True, **tools)
    assert ((g.ib[2, 0] >> 1) & 1).any(), "the cut frame has no accepted intra block"
    assert split_blocks(g.mode[:, 0])[0][2].any(), "no split block next to the intra blocks"


def test_engine_stream_decodes_with_dav1d():
    if not avif.dav1d_available():
        pytest.skip("libavif / dav1d (Pillow AVIF plugin) missing")
    from test_av1_conformance import _check as dav1d_check

    _, streams, golds = engine_vs_golden(PW, PH, [("speckle", PATHS_FRAMES)], 100)
    dav1d_check(streams[0], golds[0].tu_sizes, golds[0].recon, PW, PH)


def test_tool_off_is_the_default_engine():
    w, h, q = PW, PH, 100
    fr = CLIPS["speckle"](w, h, 3)
    gold = av1.golden_encode(fr, w, h, q)
    out = [_run_engine(w, h, [fr], q, **kw) for kw in ({}, {"tx_split": False})]
    for g, streams, fins in out:
        assert streams[0] == gold.stream
        np.testing.assert_array_equal(g.mode[:, 0], gold.mode)
        np.testing.assert_array_equal(fins[0], gold.recon[-1])
        assert not av1.mode_tx(g.mode)[0].any() and not (g.mode >> 15).any(), "a tool bit with the tool off"
    on = _run_engine(w, h, [fr], q, tx_split=True)
    assert on[1][0] != gold.stream and av1.mode_tx(on[0].mode)[0].any()
