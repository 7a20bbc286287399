"""The SATD sub-pel decision (tv/me_model.h, SeqConfig::subpel_satd, flag bit 256): half- and
quarter-pel motion vectors chosen by Hadamard SATD + MV rate instead of SAD + MV rate.  An
explicit coding tool, off by default: it enters the engine key and, only when on, tools() and
the checkpoint fingerprint; it is never read from the environment."""
import ctypes as C

import numpy as np
import pytest

from thinvids_amd._native import core_lib
from thinvids_amd.models import hevc
from thinvids_amd.worker.encoder import EncodeSpec

TEXTURED = 1 | (1 << 31)


def _frames(seed, n, w, h):
    return [hevc.synth_frame(seed, t, w, h) for t in range(n)]


def _assert_decodes_to(stream, recons, w, h):
    d = hevc.decode(stream, coded=False)
    assert len(d.frames) == len(recons)
    for a, b in zip(d.frames, recons):
        for p in range(3):
            np.testing.assert_array_equal(a[p], b[p][:h >> (p > 0), :w >> (p > 0)])


@pytest.fixture(scope="module")
def seed3():
    """192x128, seed 3, 4 frames, QP 27, range 32, SAO: (off, on) as (stream, recons)."""
    fr = _frames(3, 4, 192, 128)
    kw = dict(qp=27, search_range=32, sao=True)
    return hevc.encode_sequence_cpu(fr, **kw), hevc.encode_sequence_cpu(fr, subpel_satd=True, **kw)


def test_plumbing():
    assert hevc.codec_flags() == 1 | 4
    assert hevc.codec_flags(subpel_satd=True) == 1 | 4 | 256
    base, on = EncodeSpec(640, 360), EncodeSpec(640, 360, subpel_satd=True)
    assert base.engine_key() != on.engine_key()
    assert base.tools() == {"wpp": True, "rqt": True, "pintra": True, "cascade": True, "rdoq": True}
    assert on.tools() == dict(base.tools(), subpel_satd=True)


def test_job_and_cpu_engine_plumbing():
    from thinvids_amd.models.cpu_engines import CpuHevcEngine
    from thinvids_amd.worker.tasks import encode_spec_for_job

    job = {"source_width": 640, "source_height": 360}
    assert encode_spec_for_job(job, {"tv_gop": "64"}).subpel_satd is False
    assert encode_spec_for_job(dict(job, subpel_satd=True), {"tv_gop": "64"}).subpel_satd is True
    assert encode_spec_for_job(job, {"tv_subpel_satd": "1"}).subpel_satd is True
    assert encode_spec_for_job(job, {"tv_subpel_satd": "0"}).subpel_satd is False
    eng = CpuHevcEngine(64, 64, subpel_satd=True)
    assert eng.tools["subpel_satd"] is True
    eng.close()


def test_seed3_sizes_and_decode(seed3):
    (off, r_off), (on, r_on) = seed3
    assert on != off
    assert (len(on), len(off)) == (4315, 4421)
    _assert_decodes_to(off, r_off, 192, 128)
    _assert_decodes_to(on, r_on, 192, 128)
    for p in range(3):  # the tool never touches an I picture
        np.testing.assert_array_equal(r_on[0][p], r_off[0][p])


def test_textured_differs_and_decodes():
    fr = _frames(TEXTURED, 4, 192, 128)
    kw = dict(qp=22, search_range=32, sao=True)
    off, r_off = hevc.encode_sequence_cpu(fr, **kw)
    on, r_on = hevc.encode_sequence_cpu(fr, subpel_satd=True, **kw)
    assert on != off
    print("textured 192x128 QP 22: off", len(off), "on", len(on))
    _assert_decodes_to(off, r_off, 192, 128)
    _assert_decodes_to(on, r_on, 192, 128)


def test_bframes_differs_decodes_and_keeps_display_order():
    fr = _frames(TEXTURED, 5, 160, 96)
    kw = dict(qp=27, search_range=32, bframes=2, gop=5)
    off, r_off = hevc.encode_sequence_cpu(fr, **kw)
    on, r_on = hevc.encode_sequence_cpu(fr, subpel_satd=True, **kw)
    assert on != off
    _assert_decodes_to(off, r_off, 160, 96)
    _assert_decodes_to(on, r_on, 160, 96)
    plan = hevc.gop_plan(5, 2)
    want = [d - i for i, d in enumerate(plan["disp"])]
    assert list(hevc.display_offsets(on)) == want == list(hevc.display_offsets(off))
    assert any(want)


def test_environment_is_not_read(seed3, monkeypatch):
    (off, _), (on, _) = seed3
    fr = _frames(3, 4, 192, 128)
    kw = dict(qp=27, search_range=32, sao=True)
    monkeypatch.setenv("TV_SUBPEL_SATD", "1")
    assert hevc.encode_sequence_cpu(fr, **kw)[0] == off
    monkeypatch.setenv("TV_SUBPEL_SATD", "0")
    assert hevc.encode_sequence_cpu(fr, subpel_satd=True, **kw)[0] == on
    assert EncodeSpec(640, 360).subpel_satd is False


def _h8():
    h = np.array([[1]])
    for _ in range(3):
        h = np.block([[h, h], [h, -h]])
    return h


def _satd_blocks():
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:8, 0:8]
    chk = np.where((yy + xx) & 1, -255, 255)
    return ([rng.integers(-255, 256, (8, 8)) for _ in range(64)]
            + [np.full((8, 8), 255), np.full((8, 8), -255), chk, -chk])


def test_satd8x8_equals_numpy():
    f = core_lib().tv_satd8x8
    H = _h8()
    for d in _satd_blocks():
        z = H @ d @ H
        buf = np.zeros((8, 12), np.int32)  # a stride wider than the block
        buf[:, :8] = d
        assert f(buf.ctypes.data_as(C.POINTER(C.c_int)), 12) == (int(np.abs(z).sum()) + 2) >> 2
    for d in _satd_blocks()[-4:]:  # the saturating blocks put everything in one coefficient
        z = np.abs(H @ d @ H)
        assert z.max() == 16320 and np.count_nonzero(z) == 1
