"""Every tile path of k_inter_recon (csrc/gpu/k_inter.hip): the kernel codes a CTB as 16x16
MFMA tiles whose operands are f16 fragments -- K = 32 tiles of a 32x32 CU, block-diagonal
composites of 16 / 8 / 4-point DCTs, the Cb|Cr pair tiles, the hi / lo split of both
directions, the per-tile 32-bit quantiser, dequantiser saturation, all-zero tiles that skip the
inverse.  The engine must equal the CPU golden encoder byte for byte, and in its last
reconstruction, on inputs the golden encoder alone shows to contain inter CUs of every size
with and without coded residual, and intra quadrants in P pictures.  GPU cases run only on an
MI355X; the precondition runs anywhere."""
import functools

import numpy as np
import pytest

from thinvids_amd.models import hevc

W, H = 160, 96
TEXTURED = 7 | 0x80000000
SMOOTH = 7
STARTS = [0, 20]


def _rolled(start, n):
    """A textured picture rolled by (+37, -21) pels per frame."""
    y, u, v = hevc.synth_frame(TEXTURED, start, W, H)
    return [(np.ascontiguousarray(np.roll(y, (-21 * t, 37 * t), (0, 1))),
             np.ascontiguousarray(np.roll(u, (-10 * t, 18 * t), (0, 1))),
             np.ascontiguousarray(np.roll(v, (-10 * t, 18 * t), (0, 1)))) for t in range(n)]


# name: (seed or "rolled", gop, coding options shared by the engine and the golden encoder)
CASES = {
    "textured_qp12": (TEXTURED, 4, dict(qp=12)),
    "textured_qp27": (TEXTURED, 4, dict(qp=27)),
    "textured_qp40": (TEXTURED, 4, dict(qp=40)),
    "smooth_qp27": (SMOOTH, 4, dict(qp=27)),
    "rolled": ("rolled", 4, dict(qp=27)),
    "bframes2": (TEXTURED, 5, dict(qp=27, bframes=2)),
    "sao": (TEXTURED, 3, dict(qp=27, sao=True)),
    "no_rqt": (TEXTURED, 4, dict(qp=27, rqt=False)),
    "pintra": (TEXTURED, 4, dict(qp=40, pintra=True)),
}


@functools.lru_cache(maxsize=None)
def _frames(name, b):
    seed, gop, _ = CASES[name]
    if seed == "rolled":
        return _rolled(STARTS[b], gop)
    return [hevc.synth_frame(seed, STARTS[b] + f, W, H) for f in range(gop)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_engine_equals_golden(name):
    from thinvids_amd.models.gpu_engine import GpuEngine

    seed, gop, opt = CASES[name]
    opt = dict(dict(sao=False), **opt)
    eng = GpuEngine(width=W, height=H, batch=2, gop=gop, search_range=64,
                    seed=TEXTURED if seed == "rolled" else seed, **opt)
    if seed == "rolled":
        segs = eng.encode_frames([_frames(name, 0), _frames(name, 1)])
    else:
        segs = eng.encode_synthetic(STARTS)
    for b in range(2):
        cpu_bs, recons = hevc.encode_sequence_cpu(_frames(name, b), search_range=64, **opt)
        assert segs[b] == cpu_bs, f"{name} segment {b}: GPU bitstream differs from the golden encoder"
        for got, want in zip(eng.last_recon(b), recons[-1]):
            np.testing.assert_array_equal(got, want)
    eng.close()


def test_inputs_reach_every_tile_path():
    """The golden encoder alone, on the I P P P cases above: the P pictures hold inter CUs of
    8, 16 and 32 with a coded residual and without one, and intra quadrants."""
    seen, intra = set(), 0
    for name, (_, gop, opt) in CASES.items():
        if opt.get("bframes", 1) > 1:
            continue
        for b in range(2):
            enc = hevc.CpuEncoder(W, H, search_range=64, **dict(dict(sao=False), **opt))
            for i, f in enumerate(_frames(name, b)):
                enc.encode(f, i == 0, i)
                if i == 0:
                    continue
                d = enc.decisions()
                inter = d["intra"] == 0
                for l2 in (3, 4, 5):
                    sized = inter & (d["cu_log2"] == l2)
                    if (sized & (d["cbf"] != 0)).any():
                        seen.add((l2, True))
                    if (sized & (d["cbf"] == 0)).any():
                        seen.add((l2, False))
                intra += int((d["intra"] != 0).sum())
    assert seen == {(l2, c) for l2 in (3, 4, 5) for c in (True, False)}, sorted(seen)
    assert intra > 0
