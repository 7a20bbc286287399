"""AV1 chroma from luma (kToolCfl, off by default; csrc/include/tv/av1_enc.h "chroma from
luma"): the new default CDFs against both bundled reference libraries, the alpha fit and
decision against an independent integer transcription, CfL streams through the oracle decoder
and through dav1d (the arbiter of the prediction and the syntax: no specification text was at
hand), the tool off leaving every byte as it was, and the plumbing down from a job."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
from av1_cfl_cases import assert_paths, cfl_blocks, corr_clip, golden

from thinvids_amd.models import av1, avif, hevc

ROOT = Path(__file__).resolve().parents[1]
needs_dav1d = pytest.mark.skipif(not avif.dav1d_available(), reason="libavif / dav1d (Pillow AVIF plugin) missing")


# ---- tables ---------------------------------------------------------------------------------------
def _header_table(name: str) -> list:
    text = (ROOT / "csrc/include/tv/av1_tables.h").read_text()
    m = re.search(r"constexpr uint16_t " + name + r"(?:\[\d+\])+ = \{([^}]*)\}", text)
    return [int(v) for v in m.group(1).split(",") if v.strip()]


@needs_dav1d
def test_cfl_tables_equal_both_libraries_copies():
    """kCflSign / kCflAlpha (cumulative) against the inverse CDFs in the bundled libavif: the
    alpha rows in libaom's layout (stride 17 words, terminal 0 and counter) and in dav1d's
    (stride 16), the sign row in dav1d's (libaom's encoder image does not hold it)."""
    import glob
    import os

    import PIL

    libs = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libavif*.so*")))
    if not libs:
        pytest.skip("bundled libavif not found")
    blob = Path(libs[0]).read_bytes()
    sign, alpha = _header_table("kCflSign"), _header_table("kCflAlpha")
    assert sign == [1418, 2123, 13340, 18405, 26972, 28343, 32294]
    assert len(alpha) == 6 * 15 and alpha[:4] == [7637, 20719, 31401, 32481]
    words = lambda v: np.asarray(v, "<u2").tobytes()  # noqa: E731
    inv = lambda row: [32768 - c for c in row]  # noqa: E731
    assert words(inv(sign) + [0]) in blob
    rows = [alpha[k * 15:(k + 1) * 15] for k in range(6)]
    for r in rows:
        assert r == sorted(r) and 0 < r[0] and r[-1] < 32768
    aom = b"".join(words(inv(r) + [0, 0]) for r in rows)
    dav1d = b"".join(words(inv(r) + [0]) for r in rows)
    assert aom in blob, "kCflAlpha differs from libaom's copy"
    assert dav1d in blob, "kCflAlpha differs from dav1d's copy"


# ---- alpha fit and decision -------------------------------------------------------------------------
def _consts() -> dict:
    text = (ROOT / "csrc/include/tv/av1_enc.h").read_text()
    return {k: int(re.search(k + r" = (-?\d+)", text).group(1))
            for k in ("kCflModeBits16", "kCflZeroBits16", "kCflAlphaBits16", "kCflAlphaStep16")}


_H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=object)


def _satd8(a, b) -> int:
    d = np.array(a, dtype=object).reshape(8, 8) - np.array(b, dtype=object).reshape(8, 8)
    s = 0
    for y in (0, 4):
        for x in (0, 4):
            t = _H4.dot(d[y:y + 4, x:x + 4]).dot(_H4.T)
            s += (sum(abs(int(v)) for v in t.reshape(-1)) + 1) >> 1
    return s


def _model(luma, su, sv, dc, lam, best, K) -> dict:
    """The issue's description transcribed with Python integers (no shared code with csrc)."""
    y = [[int(v) for v in row] for row in np.asarray(luma).reshape(16, 16)]
    L = [(y[2 * i][2 * j] + y[2 * i][2 * j + 1] + y[2 * i + 1][2 * j] + y[2 * i + 1][2 * j + 1]) << 1
         for i in range(8) for j in range(8)]
    avg = (sum(L) + 32) >> 6
    ac = [v - avg for v in L]
    den = sum(a * a for a in ac)
    bits = lambda a: K["kCflAlphaBits16"] + K["kCflAlphaStep16"] * (abs(a) - 1) if a else K["kCflZeroBits16"]  # noqa: E731

    def pred(d, a, c):
        s = a * c
        r = (abs(s) + 32) >> 6
        return min(255, max(0, d + (r if s >= 0 else -r)))

    out = {"den": den}
    chosen, sats = [], []
    for name, src, d in (("u", su, dc[0]), ("v", sv, dc[1])):
        s = [int(v) for v in np.asarray(src).reshape(-1)]
        num = sum(a * (p - d) for a, p in zip(ac, s))
        if den:
            q = Fraction(64 * num, den)
            a0 = int(abs(q) + Fraction(1, 2)) * (1 if q >= 0 else -1)  # nearest, halves away from zero
            a0 = min(16, max(-16, a0))
        else:
            a0 = 0
        bc, ba, bs = None, 0, 0
        for a in (a0, a0 - 1, a0 + 1):
            if not -16 <= a <= 16:
                continue
            sat = _satd8(s, [pred(d, a, c) for c in ac])
            c = sat + ((lam * bits(a)) >> 8)
            if bc is None or c < bc:
                bc, ba, bs = c, a, sat
        out["num_" + name], out["a0_" + name], out["alpha_" + name] = num, a0, ba
        chosen.append(ba)
        sats.append(bs)
    b16 = K["kCflModeBits16"] + bits(chosen[0]) + bits(chosen[1])
    out["bits16"] = b16
    out["win"] = int(any(chosen) and sats[0] + sats[1] + ((lam * b16) >> 8) < best)
    return out


def _half_luma(a: int, b: int) -> np.ndarray:
    """Left half a, right half b: ac = +-4 (a - b), den = 1024 (a - b)^2."""
    y = np.empty((16, 16), np.uint8)
    y[:, :8], y[:, 8:] = a, b
    return y


def _fit_blocks():
    rng = np.random.default_rng(11)
    blocks = []
    for k in range(24):  # seeded: chroma = 128 + k/8 (Y2x2 - 128) + noise for slopes across the range and beyond
        y = rng.integers(0, 256, (16, 16)).astype(np.uint8)
        if k % 3 == 0:  # smooth luma: larger |ac| coherence
            y = np.clip(np.add.outer(np.arange(16) * (k - 8), np.arange(16) * 5) + 100, 0, 255).astype(np.uint8)
        yd = (y[0::2, 0::2].astype(int) + y[0::2, 1::2] + y[1::2, 0::2] + y[1::2, 1::2] + 2) >> 2
        ku, kv = int(rng.integers(-30, 31)), int(rng.integers(-30, 31))
        u = np.clip(128 + ku * (yd - 128) // 8 + rng.integers(-2, 3, yd.shape), 0, 255)
        v = np.clip(128 + kv * (yd - 128) // 8 + rng.integers(-2, 3, yd.shape), 0, 255)
        blocks.append((y, u, v, (int(rng.integers(100, 156)), int(rng.integers(100, 156)))))
    flat = np.full((16, 16), 77, np.uint8)  # den = 0
    blocks.append((flat, rng.integers(0, 256, (8, 8)), rng.integers(0, 256, (8, 8)), (128, 128)))
    # both clamps: chroma 4x steeper than alpha 16 can follow, either sign
    y = _half_luma(100, 140)
    steep = np.where(np.arange(8)[None, :] < 4, 0, 255) * np.ones((8, 1), int)
    blocks.append((y, steep, 255 - steep, (128, 128)))
    # rounding ties: 64 num / den = R / (4 D) with D = a - b = 1 and R = sum_left r - sum_right r
    for R in (2, -2, 6, -6, 10):
        u = np.full((8, 8), 128)
        for k in range(abs(R)):  # the left half is chroma columns 0..3
            u[k // 4, k % 4] += 1 if R > 0 else -1
        blocks.append((_half_luma(121, 120), u, np.full((8, 8), 128), (128, 128)))
    return blocks


def test_alpha_fit_and_decision_match_the_integer_model():
    K = _consts()
    seen = {"den0": 0, "clamp+": 0, "clamp-": 0, "win": 0, "lose": 0}
    ties = []
    for y, u, v, dc in _fit_blocks():
        for lam, best in ((16, 1 << 20), (438, 900), (2000, 300)):
            got = av1.cfl_decide(y, u, v, dc[0], dc[1], lam, best)
            want = _model(y, u, v, dc, lam, best, K)
            assert got == want, (got, want)
        seen["den0"] += got["den"] == 0
        seen["clamp+"] += 16 in (got["a0_u"], got["a0_v"])
        seen["clamp-"] += -16 in (got["a0_u"], got["a0_v"])
        if got["den"] == 1024 and got["num_v"] == 0:
            ties.append((got["num_u"], got["a0_u"]))
        for best in (1 << 20, 0):
            seen["win" if av1.cfl_decide(y, u, v, dc[0], dc[1], 438, best)["win"] else "lose"] += 1
    assert all(seen.values()), seen
    # num = 4 R: 0.5 -> 1, -0.5 -> -1, 1.5 -> 2, -1.5 -> -2, 2.5 -> 3 (halves away from zero)
    assert ties == [(8, 1), (-8, -1), (24, 2), (-24, -2), (40, 3)], ties
    flat = av1.cfl_decide(np.full((16, 16), 9, np.uint8), np.arange(64), np.arange(64), 30, 30, 16, 1 << 20)
    assert (flat["den"], flat["alpha_u"], flat["alpha_v"], flat["win"]) == (0, 0, 0, 0)


# ---- round trips through the oracle decoder -------------------------------------------------------
ROUND_TRIPS = [("corr", 16, 16, 1, 100, {}), ("corr", 72, 40, 1, 100, {}), ("corr", 200, 136, 4, 100, {}),
               ("cut", 200, 136, 4, 100, {"intra_in_inter": True}), ("steep", 72, 40, 1, 100, {}),
               ("one_plane", 72, 40, 1, 100, {}), ("flat", 72, 40, 2, 100, {})]


@pytest.mark.parametrize("kind,w,h,n,q,tools", ROUND_TRIPS, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in ROUND_TRIPS])
def test_oracle_decodes_cfl_streams(kind, w, h, n, q, tools):
    _, res = golden(kind, w, h, n, q, **tools)
    if (w, h) == (16, 16):  # the one block (no neighbour: dc 128)
        assert cfl_blocks(res.mode)[0].all()
    else:
        assert_paths("corr" if kind == "cut" else kind, res.mode)
    if kind == "cut":  # intra blocks of the cut frame take CfL too
        assert (res.ib[2] >> 1).any() and cfl_blocks(res.mode[2])[0].any()
    d = av1.decode(res.stream)
    assert len(d.frames) == n
    np.testing.assert_array_equal(np.asarray(d.frames).reshape(n, -1), res.recon.reshape(n, -1))


def test_writer_refuses_cfl_without_an_alpha():
    """uv mode 13 with both alphas zero cannot be signalled (the joint sign has no such value)."""
    w, h = 16, 16
    _, res = golden("corr", w, h, 1, 100)
    mode = res.mode[0].copy()
    assert cfl_blocks(mode)[0].all()

    def write(m):
        return av1.StreamWriter(w, h).write(res.fparams[0], m, res.mv[0], res.ly[0], res.lu[0], res.lv[0],
                                            res.cdef_idx[0], 0, True, lr=res.lr[0])

    assert write(mode) == res.stream
    bad = (mode & np.uint32(0x7FFF)) | np.uint32((16 << 15) | (16 << 21))
    with pytest.raises(RuntimeError, match="CfL"):
        write(bad)


# ---- dav1d ---------------------------------------------------------------------------------------------
DAV1D = [("corr", 72, 40, 1, 100), ("corr", 200, 136, 4, 100), ("corr", 72, 40, 1, 1), ("corr", 72, 40, 1, 255),
         ("saturated", 72, 40, 2, 100), ("steep", 72, 40, 1, 100), ("one_plane", 72, 40, 1, 100)]


@needs_dav1d
@pytest.mark.parametrize("kind,w,h,n,q", DAV1D, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-q{c[4]}" for c in DAV1D])
def test_dav1d_decodes_cfl_streams_exactly(kind, w, h, n, q):
    from test_av1_conformance import _check

    _, res = golden(kind, w, h, n, q)
    assert cfl_blocks(res.mode)[0].any(), "no CfL block in the stream"
    _check(res.stream, res.tu_sizes, res.recon, w, h)


@needs_dav1d
def test_dav1d_decodes_cfl_intra_blocks_of_inter_frames():
    from test_av1_conformance import _check

    w, h = 200, 136
    _, res = golden("cut", w, h, 4, 100, intra_in_inter=True)
    assert cfl_blocks(res.mode[2])[0].any()
    _check(res.stream, res.tu_sizes, res.recon, w, h)


# ---- tool off -----------------------------------------------------------------------------------------
def test_tool_off_changes_nothing():
    w, h, q = 200, 136, 100
    fr = corr_clip(w, h, 3)
    a, b = av1.golden_encode(fr, w, h, q), av1.golden_encode(fr, w, h, q, cfl=False)
    assert a.stream == b.stream and a.tu_sizes == b.tu_sizes
    np.testing.assert_array_equal(a.mode, b.mode)
    np.testing.assert_array_equal(a.recon, b.recon)
    assert not (((a.mode >> 5) & 15) == 13).any() and not (a.mode >> 15).any()
    _, on = golden("corr", w, h, 4, q)
    assert (on.mode[((on.mode >> 5) & 15) != 13] >> 15 == 0).all(), "alpha bits set on a block that is not CfL"


def test_cfl_saves_bytes_on_correlated_chroma():
    """Not a tuned figure: on chroma that is a linear function of luma the tool must not cost bytes."""
    w, h, q = 200, 136, 100
    fr, on = golden("corr", w, h, 4, q)
    off = av1.golden_encode(fr, w, h, q)
    assert len(on.stream) < len(off.stream)


# ---- plumbing -----------------------------------------------------------------------------------------
def test_plumbing_from_job_to_stream():
    from thinvids_amd.models.cpu_engines import CpuAv1Engine
    from thinvids_amd.parallel.node_job import Checkpoint
    from thinvids_amd.worker.encoder import EncodeSpec, encode_parts
    from thinvids_amd.worker.tasks import encode_spec_for_job

    assert av1.TOOL_CFL == 2 and av1.TOOL_INTRA_IN_INTER | av1.TOOL_CFL == 3
    w, h = 72, 40
    job = {"source_width": w, "source_height": h, "codec": "av1", "software_encode": 1}
    st = {"tv_gop": "4", "tv_scenecut": "0"}
    off, on = encode_spec_for_job(job, st), encode_spec_for_job(dict(job, av1_cfl=1), st)
    assert off.cfl is False and on.cfl is True and encode_spec_for_job(job, dict(st, tv_av1_cfl="1")).cfl is True
    assert (on.width, on.height) == (w, h)
    assert off.engine_key() != on.engine_key()
    assert on.tools() == dict(off.tools(), cfl=True)
    assert off.tools() == EncodeSpec(1, 1).tools(), "the default fingerprint moved"
    assert Checkpoint.fingerprint(tools=on.tools()) != Checkpoint.fingerprint(tools=off.tools())
    hevc_job = encode_spec_for_job({"source_width": w, "source_height": h, "av1_cfl": 1}, st)
    assert "cfl" not in hevc_job.tools(), "an AV1 tool reached the HEVC encoders"
    # the job's software path: the golden encoder with the tool
    fr = corr_clip(w, h, 2)
    gold = av1.golden_encode(fr, w, h, on.av1_qindex(), cascade=on.cascade, cfl=True)
    assert cfl_blocks(gold.mode)[0].any()
    assert encode_parts([fr], on) == [gold.stream]
    assert encode_parts([fr], off) != [gold.stream]
    # the CPU rehearsal engine (synthetic source)
    streams = {}
    for cfl in (False, True):
        eng = CpuAv1Engine(w, h, batch=1, qindex=100, cfl=cfl)
        g = eng.encode_gop(2, [0])
        streams[cfl] = b"".join(eng.submit_entropy(g)[0].result())
        eng.close()
    syn = [hevc.synth_frame(1, t, w, h) for t in range(2)]
    want = av1.golden_encode(syn, w, h, 100, cfl=True)
    assert streams[True] == want.stream and cfl_blocks(want.mode)[0].any()
    assert streams[False] == av1.golden_encode(syn, w, h, 100).stream != streams[True]
