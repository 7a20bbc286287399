"""AV1 GPU engine with directional intra (the DIR instantiations of k_av1e_intra /
k_av1e_ib_recon) against the golden encoder with the same tool: mode words including the angle
bits, MVs, CDEF tables and indices, restoration units, bitstream bytes and the last
reconstruction are equal; with the tool off the engine is the engine it was."""
import numpy as np
import pytest
from av1_dir_cases import CLIPS, PATHS_SIZE, assert_paths, dir_blocks, golden

from thinvids_amd.models import av1, avif

pytestmark = pytest.mark.gpu
PW, PH = PATHS_SIZE


def engine_vs_golden(w, h, cases, q, engine_kw=None, **tools):
    """Encode the segments (`cases`: (clip kind of av1_dir_cases, frame count) or lists of frames,
    equal lengths) as one batch on the engine and one by one with the golden encoder (dir_intra on
    plus `tools`); everything the two decide must be equal.  Returns (GopHost, [segment
    streams], [GoldenResult])."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H = av1.coded_size(w, h)
    segs, golds = [], []
    for c in cases:
        if isinstance(c, tuple):  # the shared, cached golden encode
            fr, gold = golden(c[0], w, h, c[1], q, **tools)
        else:
            fr, gold = c, av1.golden_encode(c, w, h, q, dir_intra=True, **tools)
        segs.append(fr)
        golds.append(gold)
    n = len(segs[0])
    eng = Av1GpuEngine(w, h, batch=len(segs), qindex=q,
                       **({"dir_intra": True, **tools} if engine_kw is None else engine_kw))
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


def _angled(mode) -> bool:
    _, yd, _, uvd = av1.mode_angles(mode)
    return bool((yd != 0).any() or (uvd != 0).any())


# key frames at the smallest geometries: one block (no neighbour), one neighbour direction
# each, a partial superblock; then the quantiser's ends; then the size whose paths are asserted
KEY_CASES = [(16, 16, 100), (32, 16, 100), (16, 32, 100), (72, 40, 100), (72, 40, 1), (72, 40, 255), (PW, PH, 100)]


@pytest.mark.parametrize("w,h,q", KEY_CASES, ids=[f"{w}x{h}-q{q}" for w, h, q in KEY_CASES])
def test_key_frame_matches_golden(w, h, q):
    g, _, _ = engine_vs_golden(w, h, [("fan", 1)], q)
    dir_blocks(g.mode[:, 0])
    if (w, h) != (16, 16):
        assert _angled(g.mode[:, 0]), "no angle delta"
    if (w, h) == PATHS_SIZE:
        assert_paths("fan", g.mode[:, 0])


def test_saturated_stripes():
    g, _, _ = engine_vs_golden(72, 40, [("saturated", 2)], 100)
    assert _angled(g.mode[0, 0])


def test_batch_of_fan_and_ramp_segments():
    w, h = 200, 136
    g, _, _ = engine_vs_golden(w, h, [("fan", 2), ("ramp", 2)], 100)
    assert_paths("fan", g.mode[0, 0])
    assert_paths("ramp", g.mode[0, 1])


def _cut_has_directional_intra(g) -> bool:
    acc = ((g.ib[2, 0] >> 1) & 1).astype(bool)
    dy, yd, _, _ = av1.mode_angles(g.mode[2, 0])
    return bool(acc.any() and (dy & acc).any() and ((yd != 0) & acc).any())


@pytest.mark.parametrize("cfl", [False, True], ids=["dir", "dir-cfl"])
def test_directional_intra_blocks_of_inter_frames(cfl):
    w, h = 200, 136
    g, _, _ = engine_vs_golden(w, h, [("cut", 4)], 100, intra_in_inter=True, **({"cfl": True} if cfl else {}))
    assert _cut_has_directional_intra(g), "the cut frame has no directional intra block with a delta"
    if cfl:
        assert av1.mode_cfl(g.mode[:, 0])[0].any(), "no CfL block"


def test_1080p_key_frame_and_inter_frame():
    w, h = 1920, 1080
    g, _, _ = engine_vs_golden(w, h, [CLIPS["fan"](w, h, 2)], 100)
    _, yd, _, uvd = av1.mode_angles(g.mode[0, 0])
    assert (yd != 0).sum() > 100 and (uvd != 0).sum() > 100


def test_engine_stream_decodes_with_dav1d():
    if not avif.dav1d_available():
        pytest.skip("libavif / dav1d (Pillow AVIF plugin) missing")
    from test_av1_conformance import _check as dav1d_check

    w, h = PATHS_SIZE
    _, streams, golds = engine_vs_golden(w, h, [("fan", 4)], 100)
    dav1d_check(streams[0], golds[0].tu_sizes, golds[0].recon, w, h)


def test_tool_off_is_the_default_engine():
    w, h, q = 200, 136, 100
    fr = CLIPS["fan"](w, h, 2)
    gold = av1.golden_encode(fr, w, h, q)
    out = []
    for kw in ({}, {"dir_intra": False}):
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
    assert not (out[0][0] >> 27).any() and not (out[0][0] >> 15).any()
