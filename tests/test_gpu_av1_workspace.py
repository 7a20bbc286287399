"""The AV1 engine's declared workspace (av1_engine.buffers) in use: one engine runs GOP after
GOP on the same buffers, a GOP of fewer segments than the batch runs on leading views of them,
restoration can be switched off and on again between GOPs, and the device memory the engine
holds is what the declaration says, before and during a GOP.

Display 72x40 (coded 80x48): 5x3 blocks, two superblocks of which one is partial, 40x24 chroma,
one restoration unit per plane; 3 frames per GOP (the reference buffer is rewritten twice),
batch 3; with the tools off and with intra blocks in inter frames plus chroma from luma."""
import numpy as np
import pytest
from av1_cfl_cases import corr_clip, cut_corr_clip
from av1_ib_cases import cut_clip, pan_clip

from thinvids_amd.models import av1

pytestmark = pytest.mark.gpu

W_, H_, B_, F_, Q_ = 72, 40, 3, 3, 100
TOOLS = [pytest.param({}, id="tools-off"), pytest.param({"intra_in_inter": True, "cfl": True}, id="ib-cfl")]
_gold = {}


def clips(tools: dict, which: str) -> list:
    """Three segments of F_ frames for GOP `which` ("a" | "b"); with the tools on, segments with
    a cut before the last frame (intra blocks) and chroma that follows luma (CfL)."""
    if tools:
        segs = {"a": [cut_corr_clip(W_, H_, F_, cut=2), cut_clip(W_, H_, "synth", F_, cut=2),
                      corr_clip(W_, H_, F_, seed=5)],
                "b": [cut_clip(W_, H_, "noisy", F_, cut=1), cut_corr_clip(W_, H_, F_, cut=1),
                      corr_clip(W_, H_, F_, seed=9)]}
    else:
        segs = {"a": [pan_clip(W_, H_, F_, seed=s) for s in (7, 11, 13)],
                "b": [pan_clip(W_, H_, F_, seed=s) for s in (17, 19, 23)]}
    return segs[which]


def golden(tools: dict, which: str) -> list:
    """Golden encodes of clips(tools, which), computed once and never modified."""
    key = (tuple(sorted(tools)), which)
    if key not in _gold:
        _gold[key] = [av1.golden_encode(fr, W_, H_, Q_, **tools) for fr in clips(tools, which)]
    return _gold[key]


def loader(eng, segs, hook=None):
    import torch

    W, H = eng.W, eng.H

    def load(t, planes):
        for b, fr in enumerate(segs):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[b].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(eng.dev))
        if hook:
            hook(t)

    return load


def assert_equals_golden(eng, g, golds, tools, what):
    futs = eng.submit_entropy(g)
    assert g.mode.shape[1] == len(golds)
    for b, gold in enumerate(golds):
        msg = f"{what}, segment {b}: "
        if tools.get("intra_in_inter"):
            np.testing.assert_array_equal(g.ib[:, b], gold.ib, err_msg=msg + "candidate / accepted map")
        np.testing.assert_array_equal(g.mode[:, b], gold.mode, err_msg=msg + "mode words")
        np.testing.assert_array_equal(g.mv[:, b], gold.mv, err_msg=msg + "motion vectors")
        np.testing.assert_array_equal(g.tabs[:, b, :8], gold.fparams[:, 9:17], err_msg=msg + "luma CDEF table")
        np.testing.assert_array_equal(g.tabs[:, b, 8:], gold.fparams[:, 17:25], err_msg=msg + "chroma CDEF table")
        np.testing.assert_array_equal(g.fbidx[:, b], gold.cdef_idx, err_msg=msg + "CDEF indices")
        np.testing.assert_array_equal(g.lr[:, b], gold.lr, err_msg=msg + "restoration units")
        assert b"".join(futs[b].result()) == gold.stream, msg + "bitstream"


def fin_of(eng, b):
    return np.concatenate([x[b].cpu().numpy().reshape(-1) for x in eng.fin])


def make_engine(tools):
    from thinvids_amd.models.av1_engine import Av1GpuEngine

    return Av1GpuEngine(W_, H_, batch=B_, qindex=Q_, **tools)


@pytest.mark.parametrize("tools", TOOLS)
def test_two_gops_on_one_engine_the_second_of_fewer_segments(tools):
    """GOP A fills the batch and is collected asynchronously; GOP B, of other content, uses two
    of the three segments on the same workspace.  Both equal the golden encoder."""
    eng = make_engine(tools)
    try:
        fut_a = eng.encode_gop(F_, loader(eng, clips(tools, "a")), nseg=3, async_host=True)
        g_b = eng.encode_gop(F_, loader(eng, clips(tools, "b")[:2]), nseg=2)
        assert_equals_golden(eng, fut_a.result(), golden(tools, "a"), tools, "GOP A")
        assert_equals_golden(eng, g_b, golden(tools, "b")[:2], tools, "GOP B")
        assert len(eng.fin) == 3 and eng.fin[0].shape == (B_, eng.H, eng.W)
        for b, gold in enumerate(golden(tools, "b")[:2]):
            np.testing.assert_array_equal(fin_of(eng, b), gold.recon[-1], err_msg=f"GOP B, segment {b}: last recon")
        if tools:
            assert any((g.ib[-1] >> 1).any() for g in golden(tools, "a")), "no accepted intra block in GOP A"
            assert any(av1.mode_cfl(g.mode)[0].any() for g in golden(tools, "a")), "no CfL block in GOP A"
    finally:
        eng.close()


@pytest.mark.parametrize("tools", TOOLS)
def test_restoration_off_then_on(tools, monkeypatch):
    """Without restoration the CDEF apply writes the reference: every stream decodes and its last
    frame is the engine's, and the decisions and bytes are the golden encoder's without loop
    restoration (TV_AV1_DBG=4); switched on again, the same engine equals the golden encoder."""
    eng = make_engine(tools)
    try:
        eng.lr_enabled = False
        segs = clips(tools, "a")
        g = eng.encode_gop(F_, loader(eng, segs))
        assert (g.lr[..., 0] == -1).all()
        streams = [b"".join(f.result()) for f in eng.submit_entropy(g)]
        for b, s in enumerate(streams):
            d = av1.decode(s)
            assert d.frames.shape[0] == F_
            np.testing.assert_array_equal(d.frames[-1], fin_of(eng, b), err_msg=f"segment {b}: decoded != engine recon")
        monkeypatch.setenv("TV_AV1_DBG", "4")
        for b, fr in enumerate(segs):
            gold = av1.golden_encode(fr, W_, H_, Q_, **tools)
            assert streams[b] == gold.stream, f"segment {b}: bytes differ from the golden encoder without restoration"
            np.testing.assert_array_equal(fin_of(eng, b), gold.recon[-1])
        monkeypatch.delenv("TV_AV1_DBG")
        eng.lr_enabled = True
        g2 = eng.encode_gop(F_, loader(eng, clips(tools, "b")))
        assert_equals_golden(eng, g2, golden(tools, "b"), tools, "restoration on again")
    finally:
        eng.close()


@pytest.mark.parametrize("tools", TOOLS)
def test_ledger_equals_the_declaration_and_the_allocator(tools):
    """footprint() == estimate() once a GOP has run, and what the caching allocator holds for the
    engine is the same at every frame of a later GOP: every declared buffer rounded up to the
    allocator's 512-byte granule (each is under 1 MiB at this shape), and nothing else."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine, buffers

    iii = bool(tools.get("intra_in_inter"))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    eng = make_engine(tools)
    try:
        eng.encode_gop(F_, loader(eng, clips(tools, "a")))
        assert eng.footprint() == Av1GpuEngine.estimate(W_, H_, B_, F_, iii)
        seen = []

        def hook(t):
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated() - base)

        eng.encode_gop(F_, loader(eng, clips(tools, "b"), hook))
        d = buffers(eng.W, eng.H, B_, F_, iii)
        size = lambda shape, dt: int(np.prod(shape)) * np.dtype(dt).itemsize
        assert all(size(*x) < 1 << 20 for g in d.values() for x in g.values())  # the allocator's 512-byte pool
        r512 = lambda g: sum(-(-size(*x) // 512) * 512 for x in g.values())
        declared = r512(d["work"]) + 2 * r512(d["slot"]) + r512(d["upload"])
        print("allocated per frame:", seen, "declared, 512-rounded:", declared, "footprint:", eng.footprint()["dev"])
        assert len(seen) == F_ and len(set(seen)) == 1, seen
        assert seen[0] == declared
    finally:
        eng.close()
