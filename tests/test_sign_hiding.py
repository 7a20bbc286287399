"""Sign data hiding (sign_data_hiding_enabled_flag, H.265 7.3.8.11 / 7.4.9.11; tv/sdh.h,
SeqConfig::sign_hiding, flag bit 512): the sign of the first non-zero level of a 4x4
coefficient group whose first and last non-zero scan positions lie more than 3 apart is not
coded; the decoder reads it from the parity of the group's magnitudes.  An explicit coding
tool, off by default: with it off every stream is what it was, with it on the golden encoder
makes the parities fit, the writer refuses levels that do not, and the decoder oracle infers
the hidden signs."""
import numpy as np
import pytest

from thinvids_amd.models import hevc
from thinvids_amd.worker.encoder import EncodeSpec

TEXTURED = 0x80000000


def _frames(seed, n, w, h):
    return [hevc.synth_frame(seed, t, w, h) for t in range(n)]


def _assert_decodes_to(stream, recons):
    d = hevc.decode(stream)
    assert len(d.coded_frames) == len(recons)
    for a, b in zip(d.coded_frames, recons):
        for p in range(3):
            np.testing.assert_array_equal(a[p], b[p])


# ---- the parity rule, from the specification's text alone (nothing of csrc is imported) ----
# 6.5.3 up-right diagonal, 6.5.4 horizontal, 6.5.5 vertical scan of a 4x4 block: (x, y) per position
def _diag4():
    out, x, y = [], 0, 0
    while len(out) < 16:
        while y >= 0:
            if x < 4 and y < 4:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


SCANS = {0: _diag4(), 1: [(i % 4, i // 4) for i in range(16)], 2: [(i // 4, i % 4) for i in range(16)]}


def _scan_idx(intra, log2, cidx, mode):
    """7.4.9.11 scanIdx, 4:2:0: mode dependent for intra 4x4 / 8x8 luma and 4x4 chroma TBs."""
    if intra and (log2 == 2 or (log2 == 3 and cidx == 0)):
        if 6 <= mode <= 14:
            return 2
        if 22 <= mode <= 30:
            return 1
    return 0


def _check_plane(plane, sh, cidx, dec, counts):
    """Every 4x4 group of one level plane: where the sign is hidden (lastSigScanPos -
    firstSigScanPos > 3), sumAbsLevel is odd exactly when the first level is negative."""
    H, W = plane.shape
    for gy in range(0, H, 4):
        for gx in range(0, W, 4):
            g = plane[gy:gy + 4, gx:gx + 4]
            if not g.any():
                continue
            uy, ux = (gy << sh) >> 3, (gx << sh) >> 3
            intra = bool(dec["intra"][uy, ux])
            # TB size: the CU's (intra CUs are one TB; inter TBs scan diagonally whatever their size)
            log2 = int(dec["cu_log2"][uy, ux]) - sh
            scan = _scan_idx(intra, log2, cidx, int(dec["ipm"][uy, ux]))
            lv = [int(g[y, x]) for x, y in SCANS[scan]]
            sig = [n for n in range(16) if lv[n]]
            if sig[-1] - sig[0] <= 3:
                continue
            assert (sum(abs(v) for v in lv) & 1) == (lv[sig[0]] < 0), (cidx, gx, gy, scan, lv)
            counts[(intra, scan)] = counts.get((intra, scan), 0) + 1


def _hidden_sign_counts(sign_hiding):
    w, h = 160, 96
    enc = hevc.CpuEncoder(w, h, qp=22, search_range=32, sign_hiding=sign_hiding)
    counts = {}
    for t, f in enumerate(_frames(1 | TEXTURED, 3, w, h)):
        enc.encode(f, t == 0, t)
        dec, lev = enc.decisions(), enc.levels()
        for cidx in range(3):
            _check_plane(lev[cidx], 1 if cidx else 0, cidx, dec, counts)
    return counts


def test_parity_of_every_hidden_group():
    counts = _hidden_sign_counts(True)
    print("hidden signs (intra, scanIdx):", counts)
    assert counts.get((False, 0), 0) > 0, "no inter diagonal-scan group hides a sign"
    assert counts.get((True, 1), 0) > 0, "no intra horizontal-scan group hides a sign"
    assert counts.get((True, 2), 0) > 0, "no intra vertical-scan group hides a sign"


def test_parity_check_sees_the_tool_off():
    """The same walk over tool-off levels finds groups of the wrong parity: the check above is
    not vacuous."""
    with pytest.raises(AssertionError):
        _hidden_sign_counts(False)


# ---- round trip through the decoder oracle -------------------------------------------------
@pytest.mark.parametrize("w,h", [(160, 96), (160, 90)])
@pytest.mark.parametrize("qp", [22, 27, 37])
@pytest.mark.parametrize("seed", [3, 3 | TEXTURED])
def test_round_trip_ippp(w, h, qp, seed):
    fr = _frames(seed, 4, w, h)
    for sao, wpp in ((False, True), (True, False)):
        on, rec = hevc.encode_sequence_cpu(fr, qp=qp, search_range=32, sao=sao, wpp=wpp, rqt=True, pintra=True,
                                           sign_hiding=True)
        _assert_decodes_to(on, rec)


@pytest.mark.parametrize("w,h", [(160, 96), (160, 90)])
@pytest.mark.parametrize("qp", [22, 27, 37])
@pytest.mark.parametrize("seed", [3, 3 | TEXTURED])
def test_round_trip_bframes(w, h, qp, seed):
    fr = _frames(seed, 5, w, h)
    for sao, wpp in ((True, True), (False, False)):
        on, rec = hevc.encode_sequence_cpu(fr, qp=qp, search_range=32, sao=sao, wpp=wpp, bframes=2, gop=5,
                                           sign_hiding=True)
        _assert_decodes_to(on, rec)


# ---- effect and defaults ----------------------------------------------------------------------
def _pps_sign_hiding_bit(stream: bytes) -> int:
    """sign_data_hiding_enabled_flag: after two ue(v) ids (both 0: one bit each) and five flag
    / count bits, bit 7 of the PPS payload (NAL type 34, two header bytes)."""
    i = stream.find(b"\x00\x00\x01\x44\x01")
    assert i >= 0
    return stream[i + 5] & 1


def test_effect_and_defaults():
    fr = _frames(1 | TEXTURED, 4, 160, 96)
    kw = dict(qp=22, search_range=32)
    plain, _ = hevc.encode_sequence_cpu(fr, **kw)
    off, _ = hevc.encode_sequence_cpu(fr, sign_hiding=False, **kw)
    on, _ = hevc.encode_sequence_cpu(fr, sign_hiding=True, **kw)
    assert off == plain
    assert on != off
    assert _pps_sign_hiding_bit(off) == 0
    assert _pps_sign_hiding_bit(on) == 1
    print("textured 160x96 QP 22: off", len(off), "on", len(on))


def test_decoder_reads_hidden_signs():
    """The stream carries the flag (which the decoder used to refuse) and hides signs: decoding
    it gives the encoder's reconstruction, so every hidden sign was inferred."""
    fr = _frames(2 | TEXTURED, 2, 96, 64)
    on, rec = hevc.encode_sequence_cpu(fr, qp=22, search_range=16, sign_hiding=True)
    assert _pps_sign_hiding_bit(on) == 1
    _assert_decodes_to(on, rec)


# ---- the writer refuses levels of the wrong parity -------------------------------------------
def test_writer_checks_the_parity():
    w, h = 64, 64
    dec = {"cu_log2": np.full((8, 8), 5, np.uint8), "intra": np.ones((8, 8), np.uint8),
           "ipm": np.ones((8, 8), np.uint8), "mv": np.zeros((8, 8, 2), np.int16), "cbf": np.zeros((8, 8), np.uint8)}
    dec["cbf"][:4, :4] = 1  # the first CTB's luma TB
    cy = np.zeros((h, w), np.int16)
    cu = np.zeros((h // 2, w // 2), np.int16)
    # one group, diagonal scan: positions 0 (x 0, y 0) and 15 (x 3, y 3); sum 3 is odd, so the
    # hidden sign reads as negative -- but the first level is positive
    cy[0, 0], cy[3, 3] = 2, 1
    bad = hevc.write_frame(w, h, 27, True, 0, dec, (cy, cu, cu))
    assert hevc.decode(bad).coded_frames  # off: any levels are a valid stream
    with pytest.raises(RuntimeError, match="sign data hiding"):
        hevc.write_frame(w, h, 27, True, 0, dec, (cy, cu, cu), sign_hiding=True)
    cy[0, 0] = -2  # now the parity carries the sign
    good = hevc.write_frame(w, h, 27, True, 0, dec, (cy, cu, cu), sign_hiding=True)
    ref = hevc.write_frame(w, h, 27, True, 0, dec, (cy, cu, cu))
    assert len(good) <= len(ref) and good != ref
    a, b = hevc.decode(good).coded_frames[0], hevc.decode(ref).coded_frames[0]
    for p in range(3):  # same levels, so the same samples, with one sign bin fewer
        np.testing.assert_array_equal(a[p], b[p])


# ---- the 32-bit distance of the GPU quantisers ---------------------------------------------
@pytest.mark.parametrize("intra", [0, 1])
def test_delta_fast_equals_delta(intra):
    """sdh_delta_fast (tv/tb_frag.h) against sdh_delta (tv/sdh.h) over every coefficient the
    forward transform can give (|coef| <= 64548), every TB size and QP, and inside the range
    the byte / 9-bit stores of the GPU paths rely on."""
    import ctypes as C

    from thinvids_amd._native import core_lib

    lib = core_lib()
    coef = np.concatenate([np.arange(-64548, 64549, 7), [-64548, 64548, -1, 0, 1]]).astype(np.int32)
    ref, fast = np.empty_like(coef), np.empty_like(coef)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    for log2n in (2, 3, 4, 5):
        for qp in (0, 5, 17, 22, 27, 32, 37, 46, 51):
            lib.tv_sdh_deltas(ip(coef), int(coef.size), qp, log2n, intra, ip(ref), ip(fast))
            np.testing.assert_array_equal(fast, ref)
            lo, hi = (-86, 171) if intra else (-64, 192)
            assert lo <= ref.min() and ref.max() < hi


# ---- plumbing -------------------------------------------------------------------------------------
def test_plumbing():
    assert hevc.codec_flags() == 1 | 4
    assert hevc.codec_flags(sign_hiding=True) == 1 | 4 | 512
    base, on = EncodeSpec(640, 360), EncodeSpec(640, 360, sign_hiding=True)
    assert base.sign_hiding is False
    assert base.engine_key() != on.engine_key()
    assert base.tools() == {"wpp": True, "rqt": True, "pintra": True, "cascade": True, "rdoq": True}
    assert on.tools() == dict(base.tools(), sign_hiding=True)


def test_default_fingerprint_is_unchanged():
    """The checkpoint fingerprint hashes tools(): the default spec's is the one it was before
    the tool existed, and the tool, when on, moves it."""
    from thinvids_amd.parallel.node_job import Checkpoint

    before = {"wpp": True, "rqt": True, "pintra": True, "cascade": True, "rdoq": True}
    assert Checkpoint.fingerprint(tools=EncodeSpec(1, 1).tools()) == Checkpoint.fingerprint(tools=before)
    assert Checkpoint.fingerprint(tools=EncodeSpec(1, 1, sign_hiding=True).tools()) != Checkpoint.fingerprint(tools=before)


def test_job_and_cpu_engine_plumbing():
    from thinvids_amd.models.cpu_engines import CpuHevcEngine
    from thinvids_amd.worker.tasks import encode_spec_for_job

    job = {"source_width": 640, "source_height": 360}
    assert encode_spec_for_job(job, {"tv_gop": "64"}).sign_hiding is False
    assert encode_spec_for_job(dict(job, sign_hiding=True), {"tv_gop": "64"}).sign_hiding is True
    assert encode_spec_for_job(job, {"tv_sign_hiding": "1"}).sign_hiding is True
    assert encode_spec_for_job(job, {"tv_sign_hiding": "0"}).sign_hiding is False
    eng = CpuHevcEngine(64, 64, sign_hiding=True)
    assert eng.tools["sign_hiding"] is True
    eng.close()
