"""AV1 transform split (av1_enc.h "transform split", tools bit 8): golden encoder -> decoder oracle
round trips, dav1d conformance, the decision against an independent numpy statement, the writer's
refusals, both writer inputs, the key frame of a tool-on stream, tool off against recorded streams."""
import hashlib
import json
import os

import numpy as np
import pytest
from av1_tx_cases import CLIPS, PATHS_FRAMES, PATHS_SIZE, assert_paths, golden, split_blocks

from thinvids_amd.models import av1, avif, hevc

needs_dav1d = pytest.mark.skipif(not avif.dav1d_available(), reason="libavif / dav1d (Pillow AVIF plugin) missing")
PW, PH = PATHS_SIZE
ALL_INTRA_TOOLS = {"intra_in_inter": True, "cfl": True, "dir_intra": True}


def _ids(cases):
    return [f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-q{c[4]}{'-' + '-'.join(c[5]) if c[5] else ''}" for c in cases]


# ---- round trips through the oracle decoder -------------------------------------------------------
ROUND_TRIPS = [("speckle", 16, 16, 3, 100, {}), ("speckle", 32, 16, 3, 100, {}), ("speckle", 16, 32, 3, 100, {}),
               ("speckle", 72, 40, 3, 100, {}), ("speckle", 72, 40, 3, 1, {}), ("speckle", 72, 40, 3, 255, {}),
               ("speckle", PW, PH, PATHS_FRAMES, 100, {}), ("ramp", PW, PH, 3, 100, {}),
               ("saturated", 72, 40, 2, 100, {}), ("cut", PW, PH, 4, 100, {"intra_in_inter": True}),
               ("cut", PW, PH, 4, 100, ALL_INTRA_TOOLS)]


@pytest.mark.parametrize("kind,w,h,n,q,tools", ROUND_TRIPS, ids=_ids(ROUND_TRIPS))
def test_oracle_decodes_split_streams(kind, w, h, n, q, tools):
    _, res = golden(kind, w, h, n, q, **tools)
    split, _ = split_blocks(res.mode)
    if (w, h) == PATHS_SIZE and kind in ("speckle", "ramp"):
        assert_paths(kind, res.mode)
    elif (w, h) != (16, 16) and q != 255:
        assert split.any(), "no split block in the stream"
    if kind == "cut":  # intra blocks of a TX_MODE_SELECT frame code tx_depth
        assert ((res.mode[1:] & 1) == 0).any() and split.any()
    assert (res.fparams[1:, 0] == 2).all() and res.fparams[0, 0] == 1, "tx_mode_select: inter frames only"
    d = av1.decode(res.stream)
    assert len(d.frames) == n
    np.testing.assert_array_equal(np.asarray(d.frames).reshape(n, -1), res.recon.reshape(n, -1))
    mode, mv = av1.decode_modes(res.stream)
    np.testing.assert_array_equal(mode, res.mode, err_msg="mode words do not round-trip")
    np.testing.assert_array_equal(mv, res.mv)


# ---- dav1d ----------------------------------------------------------------------------------------
DAV1D = [("speckle", 72, 40, 3, 1, {}), ("speckle", 72, 40, 3, 100, {}), ("speckle", 72, 40, 3, 255, {}),
         ("speckle", 16, 16, 3, 100, {}), ("speckle", 32, 16, 3, 100, {}), ("speckle", 16, 32, 3, 100, {}),
         ("speckle", PW, PH, PATHS_FRAMES, 100, {}), ("saturated", 72, 40, 2, 100, {}),
         ("cut", PW, PH, 4, 100, {"intra_in_inter": True}), ("cut", PW, PH, 4, 100, ALL_INTRA_TOOLS)]


@needs_dav1d
@pytest.mark.parametrize("kind,w,h,n,q,tools", DAV1D, ids=_ids(DAV1D))
def test_dav1d_decodes_split_streams_exactly(kind, w, h, n, q, tools):
    from test_av1_conformance import _check

    _, res = golden(kind, w, h, n, q, **tools)
    if (w, h) != (16, 16) and q != 255:
        assert split_blocks(res.mode)[0].any(), "no split block in the stream"
    if kind == "cut":
        assert ((res.mode[1:] & 1) == 0).any(), "no intra block in an inter frame"
    _check(res.stream, res.tu_sizes, res.recon, w, h)


# ---- the decision ---------------------------------------------------------------------------------
def _bits16(p: int) -> int:
    return int(np.floor(16 * np.log2(32768 / p) + 0.5))


# Default_Txfm_Split_Cdf (cumulative P(split = 0) * 32768) of the two contexts the model reads
SPLIT_CDF_16, SPLIT_CDF_8 = 26549, 28015


def _tb_bits(lev: np.ndarray) -> int:
    """The rate proxy of one N x N transform block, stated on its zigzag-ordered levels."""
    z = lev.reshape(-1)[av1.zigzag_scan(lev.shape[0])].astype(np.int64)
    nzi = np.nonzero(z)[0]
    if not len(nzi):
        return 8
    eob = int(nzi[-1]) + 1
    a = np.abs(z[nzi])
    lvl = int((40 + 32 * np.floor(np.log2(a)).astype(np.int64)).sum())
    return 24 + 24 * eob.bit_length() + 10 * (eob - len(nzi)) + lvl


def _decision_inputs():
    rng = np.random.default_rng(3)
    i, j = np.mgrid[0:16, 0:16]
    cases = []
    for k in range(24):  # random residuals of growing amplitude on a flat or a gradient prediction
        pred = np.clip(128 + (k % 3) * (i - j) * 2, 0, 255)
        amp = (1, 2, 4, 8, 16, 40, 90, 127)[k % 8]
        cases.append((np.clip(pred + rng.integers(-amp, amp + 1, (16, 16)), 0, 255), pred))
    for k in range(8):  # residual confined to one quadrant
        pred = np.full((16, 16), 100)
        src = pred.copy()
        y0, x0 = (k >> 1 & 1) * 8, (k & 1) * 8
        src[y0:y0 + 8, x0:x0 + 8] += rng.integers(-60, 61, (8, 8))
        cases.append((src, pred))
    full, zero = np.full((16, 16), 255), np.zeros((16, 16), np.int64)
    cases += [(full, zero), (zero, full)]  # +-255 everywhere
    chk = ((i + j) & 1) * 255
    cases += [(chk, 255 - chk)]  # +-255 alternating
    one = np.full((16, 16), 128)
    for v in (255, 0):  # one nonzero sample per quadrant
        s = one.copy()
        s[3, 2] = s[1, 13] = s[12, 5] = s[9, 9] = v
        cases.append((s, one))
    cases.append((one, one))  # nothing to code
    return [(np.asarray(s, np.uint8), np.asarray(p, np.uint8)) for s, p in cases]


@pytest.mark.parametrize("q", [1, 60, 100, 160, 255])
def test_decision_matches_the_numpy_statement(q):
    splits = 0
    for rnd in (43, 21):
        for src, pred in _decision_inputs():
            r = av1.tx_split_decide(src, pred, q, rnd)
            s = src.astype(np.int64)
            sse16 = int(((s - r["rec16"].astype(np.int64)) ** 2).sum())
            sse8 = int(((s - r["rec8"].astype(np.int64)) ** 2).sum())
            bits16 = _tb_bits(r["lev16"])
            bits8 = sum(_tb_bits(r["lev8"][k]) for k in range(4))
            qmask = sum(int(r["lev8"][k].any()) << k for k in range(4))
            lam = (av1.ac_q(q) ** 2 * 9) >> 6
            j16 = (sse16 << 8) + lam * (bits16 + _bits16(SPLIT_CDF_16))
            j8 = (sse8 << 8) + lam * (bits8 + _bits16(32768 - SPLIT_CDF_16) + 4 * _bits16(SPLIT_CDF_8))
            assert (r["sse16"], r["bits16"], r["sse8"], r["bits8"], r["qmask"], r["lam"]) == \
                (sse16, bits16, sse8, bits8, qmask, lam)
            assert r["split"] == int(qmask != 0 and j8 < j16), "ties and all-zero splits keep 16x16"
            splits += r["split"]
    if q < 255:
        assert splits, "no input of the set is split: the decision's split side is not exercised"


def test_zigzag_index_is_the_inverse_scan():
    """The rate proxy's eob needs the scan index of a raster position: a one-hot block per position."""
    for n in (8, 16):
        sc = av1.zigzag_scan(n)
        assert sorted(sc.tolist()) == list(range(n * n))
    pred = np.full((16, 16), 128, np.uint8)
    for y, x in ((0, 0), (5, 9), (15, 15), (8, 7)):  # a strong sample: levels exist, bits consistent
        src = pred.copy()
        src[y, x] = 255
        r = av1.tx_split_decide(src, pred, 60, 43)
        assert r["bits16"] == _tb_bits(r["lev16"]) and r["bits8"] == sum(_tb_bits(r["lev8"][k]) for k in range(4))


# ---- the writer -----------------------------------------------------------------------------------
def _write(w, h, res, k, mode=None, ly=None, packed=0):
    """Frames 0..k of a golden result through the stream writer; frame k with `mode` / `ly`."""
    wr = av1.StreamWriter(w, h)
    out = []
    for t in range(k + 1):
        m = np.ascontiguousarray(res.mode[t] if mode is None or t < k else mode)
        lev = [res.ly[t] if ly is None or t < k else ly, res.lu[t], res.lv[t]]
        if packed == 2:
            lev = [av1.scan_pack(x, m, p) for p, x in enumerate(lev)]
        elif packed == 1:
            lev = [np.ascontiguousarray(x[((m >> (10 + p)) & 1).astype(bool)]) if ((m >> (10 + p)) & 1).any()
                   else np.zeros((1, x.shape[1]), np.int16) for p, x in enumerate(lev)]
        out.append(wr.write(res.fparams[t], m, np.ascontiguousarray(res.mv[t]), *map(np.ascontiguousarray, lev),
                            np.ascontiguousarray(res.cdef_idx[t]), packed=packed, seq_header=(t == 0), lr=res.lr[t]))
    return out


@pytest.mark.parametrize("packed", [0, 1, 2], ids=["raster", "packed", "scan-packed"])
def test_every_writer_input_gives_the_golden_stream(packed):
    w, h = PATHS_SIZE
    _, res = golden("speckle", w, h, PATHS_FRAMES, 100)
    assert split_blocks(res.mode)[0].any()
    assert _write(w, h, res, PATHS_FRAMES - 1, packed=packed) == av1.split_temporal_units(res.stream, res.tu_sizes)


@pytest.mark.parametrize("packed", [0, 2], ids=["raster", "scan-packed"])
def test_writer_refusals(packed):
    w, h = PATHS_SIZE
    _, res = golden("speckle", w, h, PATHS_FRAMES, 100)
    m = res.mode[1].astype(np.int64)
    split, qm = av1.mode_tx(m)
    inter, skip, bsz = (m & 1) == 1, ((m >> 9) & 1) == 1, (m >> 13) & 3
    bit = np.uint32(1 << 30)

    def bad(b, word=None, zero_luma=False, frame=1):
        mode = res.mode[frame].copy()
        mode[b] = mode[b] | bit | np.uint32(1 << 15) if word is None else np.uint32(word)
        ly = res.ly[frame].copy()
        if zero_luma:
            ly[b] = 0
        return _write(w, h, res, frame, mode, ly, packed)

    with pytest.raises(RuntimeError, match="transform split on a skip, intra or merged"):
        bad(int(np.nonzero(inter & skip & (bsz == 0))[0][0]))
    with pytest.raises(RuntimeError, match="transform split on a skip, intra or merged"):
        bad(int(np.nonzero(bsz > 0)[0][0]))
    with pytest.raises(RuntimeError, match="transform split on a skip, intra or merged"):
        bad(0, frame=0)  # an intra block (key frame)
    b = int(np.nonzero(split & (qm != 15))[0][0])
    with pytest.raises(RuntimeError, match="quadrant mask|bad eob"):  # a mask bit without levels
        bad(b, int(m[b]) | (15 << 15))
    b = int(np.nonzero(split & ((qm & (qm - 1)) != 0))[0][0])  # two quadrants or more
    if packed == 0:  # levels without their mask bit (the scan-packed layout is packed by the mask itself)
        with pytest.raises(RuntimeError, match="quadrant mask"):
            bad(b, int(m[b]) & ~(15 << 15) | ((int(qm[b]) & (int(qm[b]) - 1)) << 15))
    with pytest.raises(RuntimeError, match="all-zero quadrants"):
        bad(b, int(m[b]) & ~(15 << 15), zero_luma=True)
    # the tool's bit on a frame that does not signal TX_MODE_SELECT
    off = av1.golden_encode(CLIPS["speckle"](w, h, 2), w, h, 100)
    k = int(np.nonzero(((off.mode[1] & 1) == 1) & (((off.mode[1] >> 9) & 1) == 0))[0][0])
    mode = off.mode[1].copy()
    mode[k] |= bit | np.uint32(1 << 15)
    with pytest.raises(RuntimeError, match="transform split on a skip, intra or merged"):
        _write(w, h, off, 1, mode, None, packed)


# ---- tool off, key frames -------------------------------------------------------------------------
def test_tool_off_streams_equal_the_recorded_ones():
    """sha256 of golden streams recorded before the tool existed (tests/golden)."""
    path = os.path.join(os.path.dirname(__file__), "golden", "av1_tool_off_streams.json")
    cases = json.load(open(path))
    assert len(cases) == 3
    for c in cases:
        fr = CLIPS[c["clip"]](c["width"], c["height"], c["frames"])
        for kw in ({}, {"tx_split": False}):
            res = av1.golden_encode(fr, c["width"], c["height"], c["qindex"], **c["tools"], **kw)
            assert len(res.stream) == c["bytes"] and hashlib.sha256(res.stream).hexdigest() == c["sha256"], c["clip"]
            assert not av1.mode_tx(res.mode)[0].any() and not (res.fparams[:, 0] > 1).any()
            inter = (res.mode & 1) == 1
            assert not ((res.mode >> 15) & 15)[inter].any(), "quadrant bits with the tool off"


@pytest.mark.parametrize("kind,w,h,n,tools", [("speckle", 72, 40, 3, {}), ("speckle", PW, PH, PATHS_FRAMES, {}),
                                              ("cut", PW, PH, 4, {"intra_in_inter": True})],
                         ids=["speckle-72x40", "speckle-paths", "cut"])
def test_key_frame_equals_the_tool_off_key_frame(kind, w, h, n, tools):
    fr, on = golden(kind, w, h, n, 100, **tools)
    off = av1.golden_encode(fr, w, h, 100, **tools)
    assert on.tu_sizes[0] == off.tu_sizes[0]
    assert on.stream[:on.tu_sizes[0]] == off.stream[:off.tu_sizes[0]]
    assert on.stream != off.stream
    np.testing.assert_array_equal(on.mode[0], off.mode[0])
    # the first inter frame searches the same reference: its motion field does not depend on the tool
    np.testing.assert_array_equal(on.mv[1], off.mv[1], err_msg="the motion field depends on the tool")


def test_split_saves_bytes_where_residual_is_local():
    """Not a tuned figure: on the speckle clip the tool must not cost bytes or luma quality."""
    w, h = PATHS_SIZE
    fr, on = golden("speckle", w, h, PATHS_FRAMES, 100)
    off = av1.golden_encode(fr, w, h, 100)
    assert len(on.stream) < len(off.stream)
    W, H = av1.coded_size(w, h)
    src = av1.pack_i420([av1.pad_frame(f, W, H) for f in fr], W, H)[:, :W * H].astype(np.int64)
    sse = lambda r: int(((src - r.recon[:, :W * H].astype(np.int64)) ** 2).sum())  # noqa: E731
    assert sse(on) <= sse(off) * 1.02


# ---- plumbing -------------------------------------------------------------------------------------
def test_plumbing_from_job_to_stream():
    from thinvids_amd.models.cpu_engines import CpuAv1Engine
    from thinvids_amd.parallel.node_job import Checkpoint
    from thinvids_amd.worker.encoder import EncodeSpec, encode_parts
    from thinvids_amd.worker.tasks import encode_spec_for_job

    assert av1.TOOL_TX_SPLIT == 8
    assert av1.TOOL_INTRA_IN_INTER | av1.TOOL_CFL | av1.TOOL_DIR_INTRA | av1.TOOL_TX_SPLIT == 15
    w, h = 72, 40
    job = {"source_width": w, "source_height": h, "codec": "av1", "software_encode": 1}
    st = {"tv_gop": "4", "tv_scenecut": "0"}
    off, on = encode_spec_for_job(job, st), encode_spec_for_job(dict(job, av1_tx_split=1), st)
    assert off.tx_split is False and on.tx_split is True
    assert encode_spec_for_job(job, dict(st, tv_av1_tx_split="1")).tx_split is True
    assert off.engine_key() != on.engine_key()
    assert on.tools() == dict(off.tools(), tx_split=True)
    assert off.tools() == EncodeSpec(1, 1).tools(), "the default fingerprint moved"
    assert Checkpoint.fingerprint(tools=on.tools()) != Checkpoint.fingerprint(tools=off.tools())
    hevc_job = encode_spec_for_job({"source_width": w, "source_height": h, "av1_tx_split": 1}, st)
    assert "tx_split" not in hevc_job.tools(), "an AV1 tool reached the HEVC encoders"
    fr = CLIPS["speckle"](w, h, 3)
    gold = av1.golden_encode(fr, w, h, on.av1_qindex(), cascade=on.cascade, tx_split=True)
    assert av1.mode_tx(gold.mode)[0].any()
    assert encode_parts([fr], on) == [gold.stream]
    assert encode_parts([fr], off) != [gold.stream]
    streams = {}
    for tool in (False, True):  # the CPU rehearsal engine (synthetic source)
        eng = CpuAv1Engine(w, h, batch=1, qindex=100, tx_split=tool)
        g = eng.encode_gop(3, [0])
        streams[tool] = b"".join(eng.submit_entropy(g)[0].result())
        eng.close()
    syn = [hevc.synth_frame(1, t, w, h) for t in range(3)]
    assert streams[True] == av1.golden_encode(syn, w, h, 100, tx_split=True).stream
    assert streams[False] == av1.golden_encode(syn, w, h, 100).stream
