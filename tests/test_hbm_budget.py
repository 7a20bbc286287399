"""HBM-aware engine sizing (verdict r3 item 8): the engines' footprint ledgers (the HEVC
engine's native one, the AV1 engine's buffer declaration) and their no-allocation estimates,
the byte-budgeted EngineCache (LRU eviction by bytes) and the budget-capped auto_batch."""
import pytest

from thinvids_amd.worker.encoder import EncodeSpec, EngineCache, auto_batch, engine_bytes

GiB = 1 << 30


def test_estimate_scales_with_batch_sao_and_dpb():
    from thinvids_amd.models.gpu_engine import estimate_footprint

    a = estimate_footprint(1920, 1080, 24, 64)["dev"]
    b = estimate_footprint(1920, 1080, 48, 64)["dev"]
    assert 1.9 < b / a < 2.05  # per-segment buffers dominate
    assert estimate_footprint(1920, 1080, 48, 64, sao=True)["dev"] > b  # the SAO scratch set
    assert estimate_footprint(1920, 1080, 48, 64, bframes=8)["dev"] > b  # a deeper DPB
    assert 3 * GiB < b < 8 * GiB  # 1080p x 48: the measured order of magnitude
    assert estimate_footprint(3840, 2160, 24, 64)["dev"] > 1.9 * a


def test_av1_estimate_scales_with_batch_tool_and_gop():
    from thinvids_amd.models.av1_engine import Av1GpuEngine

    est = lambda *a, **k: Av1GpuEngine.estimate(*a, **k)["dev"]
    a, b = est(1920, 1080, 16, 64), est(1920, 1080, 32, 64)
    assert 1.9 < b / a < 2.05  # every buffer is per segment
    assert est(1920, 1080, 32, 64, intra_in_inter=True) > b  # the intra-block scratch and the slots' maps
    assert est(1920, 1080, 32, 1) < est(1920, 1080, 32, 2) < est(1920, 1080, 32, 63) < b  # the GOP slots
    assert engine_bytes(EncodeSpec(1920, 1080, gop=64, codec="av1"), 32) > b  # plus the staging buffer


def test_av1_estimate_is_the_sum_of_the_declared_buffers():
    """Display 72x40 -> coded 80x48, batch 3, GOP 3, every buffer of the declaration by hand."""
    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H, B, F = 80, 48, 3, 3
    nb, n8, nfb = 5 * 3, 10 * 6, 2 * 1  # 16x16 blocks, 8x8 blocks, 64x64 filter blocks
    planes = W * H + 2 * (W // 2) * (H // 2)  # one I420 plane set, bytes
    work = (5 * planes  # src, rec, fin, deblocked, CDEF output
            + 4 * ((W // 4) * (H // 4) + 2 * (W // 8) * (H // 8))  # iy, iu, iv words
            + n8 + 4 * n8  # dirs bytes, var words
            + 3 * nfb * 64 * 8  # three CDEF SSE tables
            + 2 * nfb  # py, puv
            + 3 * 1 * 3 * 4  # prm: one restoration unit per plane, three words
            + 8 * (2 + 1 + 1)  # per-unit SSE: 2 luma units (ceil), 1 per chroma plane
            + 4 * nb + 8 + 2 * nb * 89)  # mvtmp, satd, two memo record sets of 11 * 8 + 1 bytes
    ib_work = 4 * nb + nb + 4 * 7 + 4 * 7 * nb  # ibcost, ibcand, ibcnt, iblist (7 passes)
    slot = F * B * (4 * nb + 4 * nb  # mode, mv
                    + 2 * nb * (256 + 64 + 64)  # levels
                    + 16 + nfb + 3 * 8  # tabs, fbidx, sse
                    + 3 * 1 * 3 * 4)  # lr: 3 planes x 1 unit x 3 words
    upload = F * B * (4 + 4 * 4 + 8)  # q-index, four filter levels, restoration rate
    assert Av1GpuEngine.estimate(72, 40, B, F)["dev"] == B * work + 2 * slot + upload == 320442
    assert Av1GpuEngine.estimate(72, 40, B, F, intra_in_inter=True)["dev"] == (
        B * (work + ib_work) + 2 * (slot + F * B * nb) + upload)


class _FakeEngine:
    def __init__(self, spec, batch):
        self.spec, self.batch, self.closed = spec, batch, False
        from thinvids_amd.models.gpu_engine import estimate_footprint

        self._fp = estimate_footprint(spec.width, spec.height, batch, spec.gop, spec.sao)

    def footprint(self):
        return self._fp

    def close(self):
        self.closed = True


def test_engine_cache_evicts_by_bytes(monkeypatch):
    monkeypatch.setenv("TV_ENTROPY", "host")  # footprints without the GPU coder's scratch
    cache = EngineCache(batch=0, max_engines=16, budget=64 * GiB)
    monkeypatch.setattr(cache, "_build", lambda spec, batch: _FakeEngine(spec, batch))
    hd = [EncodeSpec(1920, 1080, qp=q) for q in (22, 25, 27, 30, 32)]
    uhd = EncodeSpec(3840, 2160, qp=27)
    engines = [cache.get(s) for s in hd]  # 5 x ~15 GiB (engine + staging): the oldest go
    assert cache.used_bytes() <= cache.budget
    assert engines[0].closed and not engines[4].closed and cache.evicted == 1
    assert cache.get(hd[1]) is engines[1]  # a hit refreshes the LRU order
    e4 = cache.get(uhd)  # ~30 GiB: evicts the least recently used (2, 3), keeps 1 and 4
    assert cache.used_bytes() <= cache.budget and not e4.closed
    assert engines[2].closed and engines[3].closed and not engines[1].closed and not engines[4].closed
    assert e4.batch == 24 and engines[4].batch == 48  # CU-fill heuristic, inside the budget


def test_engine_cache_refuses_an_engine_over_budget(monkeypatch):
    cache = EngineCache(batch=48, budget=4 * GiB)
    monkeypatch.setattr(cache, "_build", lambda spec, batch: _FakeEngine(spec, batch))
    with pytest.raises(MemoryError):
        cache.get(EncodeSpec(3840, 2160))


def test_auto_batch_is_capped_by_the_budget():
    spec = EncodeSpec(3840, 2160, gop=64)
    assert auto_batch(spec) == 24 and auto_batch(spec, 1000 * GiB) == 24
    small = auto_batch(spec, 24 * GiB)
    assert 1 <= small < 24 and engine_bytes(spec, small) <= 12 * GiB
    assert auto_batch(EncodeSpec(1920, 1080, codec="av1"), 1000 * GiB) == 32
    assert auto_batch(EncodeSpec(3840, 2160, codec="av1"), 1000 * GiB) == 16


# geometries that reach every optional buffer: the minimum size (two CTB columns, the least the
# GPU coder accepts), an uneven 2 + 1 group split, no intra-in-P block, no WPP, a deep DPB with
# the SAO scratch set; each with the GPU coder's scratch and without it
_EDGES = [(64, 64, 1, 2, False, 1, {}), (96, 64, 3, 4, False, 1, {}), (320, 180, 8, 16, False, 1, {"pintra": False}),
          (320, 180, 8, 16, False, 1, {"wpp": False}), (320, 180, 8, 16, True, 8, {})]


def _row(w, h, batch, gop, sao, bframes, kw={}, lanes=None):
    extra = [f"{k}={v}" for k, v in kw.items()] + ([f"lanes={lanes}"] if lanes else [])
    return pytest.param(w, h, batch, gop, sao, bframes, kw, lanes,
                        id="-".join(str(x) for x in (w, h, batch, gop, sao, bframes, *extra)))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,batch,gop,sao,bframes,kw,lanes",
                         [_row(1920, 1080, 48, 64, True, 1), _row(320, 180, 8, 16, False, 8),
                          _row(3840, 2160, 6, 8, True, 1)]
                         + [_row(*e[:6], dict(e[6], entropy=ent)) for e in _EDGES for ent in ("gpu", "host")]
                         + [_row(320, 180, 8, 16, True, 1, {"entropy": "gpu"}, "4")])
def test_native_footprint_equals_estimate(w, h, batch, gop, sao, bframes, kw, lanes, monkeypatch):
    from thinvids_amd.models.gpu_engine import GpuEngine, estimate_footprint

    if lanes:
        monkeypatch.setenv("TV_ENT_LANES", lanes)
    eng = GpuEngine(width=w, height=h, qp=27, batch=batch, gop=gop, sao=sao, bframes=bframes, **kw)
    try:
        assert eng.footprint() == estimate_footprint(w, h, batch, gop, sao, bframes, **kw)
        if "entropy" in kw:
            assert eng.entropy_stats()["gpu"] == (kw["entropy"] == "gpu" and kw.get("wpp", True))
    finally:
        eng.close()


@pytest.mark.gpu
def test_refused_configuration_leaves_the_device_usable():
    """A configuration the constructor refuses is refused before anything is allocated, and an
    engine built right afterwards codes what the golden encoder codes."""
    from thinvids_amd.models import hevc
    from thinvids_amd.models.gpu_engine import GpuEngine

    with pytest.raises(RuntimeError, match="power of 2"):
        GpuEngine(64, 64, batch=1, gop=2, bframes=3)
    with pytest.raises(RuntimeError, match="CRF"):
        GpuEngine(64, 64, batch=1, gop=2, bframes=8, crf=23)
    eng = GpuEngine(64, 64, batch=1, gop=2)
    try:
        seg, = eng.encode_synthetic([0])
    finally:
        eng.close()
    frames = [hevc.synth_frame(1, f, 64, 64) for f in range(2)]  # the engine's default seed
    assert seg == hevc.encode_sequence_cpu(frames)[0]


@pytest.mark.gpu
def test_8k_ladder_and_4k_av1_engine_fit_together():
    """The shipped 8K HDR10 -> 5-rung ladder shape and a concurrent 4K AV1 engine are
    resident on one MI355X at once, each runs a step, and the budget model accounts for
    what the device actually lost."""
    import torch

    from thinvids_amd.models.abr import AbrLadder
    from thinvids_amd.models.av1_engine import Av1GpuEngine
    from thinvids_amd.worker.encoder import device_budget

    free0, total = torch.cuda.mem_get_info(0)
    lad = AbrLadder(7680, 4320, [2160, 1440, 1080, 720, 480], segments=24, gop=64, device=0)
    av = Av1GpuEngine(3840, 2160, batch=16, qindex=100, device=0)
    try:
        lad.prepare_synthetic([64 * b for b in range(24)], slot=0)
        segs = lad.encode_prepared(24, slot=0)
        assert len(segs) == 5 and all(len(r) == 24 for r in segs)

        def load(t, planes):
            for p in planes:
                p.fill_(100 + t)

        g = av.encode_gop(64, load)
        assert g.sse.shape[:2] == (64, 16)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info(0)
        used = free0 - free1
        model = (sum(e.footprint()["dev"] for e in lad.engines)
                 + engine_bytes(EncodeSpec(3840, 2160, gop=64, codec="av1"), 16))
        assert used < device_budget(0), (used / GiB, device_budget(0) / GiB)
        assert model < used * 1.5, (model / GiB, used / GiB)
    finally:
        av.close()
        lad.close()
