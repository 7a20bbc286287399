"""The MV-rate model (tv/hevc_defs.h mv_bits_est, tv/me_model.h me_pen_index, tv/av1_enc.h
mv_comp_bits) is a closed form on a count-leading-zeros.  It must equal the bit-by-bit loops
it replaced, transcribed here, and the golden encoders must still write the streams they
wrote with the loops (tests/golden/me_rate_parent.json).

    python tests/test_mv_rate.py --record     # rewrite the golden file from the imported build
"""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from thinvids_amd._native import core_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "me_rate_parent.json")


# ---- the former loops, lane by lane over an array (each element runs exactly the loop) -----
def _loop_len(v):
    """n of `while (v > 1) { v >>= 1; ++n; }`"""
    v = v.copy()
    n = np.zeros_like(v)
    while True:
        m = v > 1
        if not m.any():
            return n
        v[m] >>= 1
        n[m] += 1


def old_mv_bits_est(dx, dy):
    bits = np.zeros_like(dx)
    for c in (dx, dy):
        a = np.abs(c)
        bits += np.where(a == 0, 1, 2 * _loop_len(a + 1) + 1)
    return bits


def old_mv_comp_bits(d):
    a = np.abs(d) >> 1
    return np.where(a == 0, 1, 2 * (_loop_len(a) + 1) + 2)  # `while (a) { ++b; a >>= 1; }`: b = n + 1


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _native_rate(dx, dy):
    lib = core_lib()
    dx = np.ascontiguousarray(dx, np.int32)
    dy = np.ascontiguousarray(dy, np.int32)
    est, idx = np.empty_like(dx), np.empty_like(dx)
    lib.tv_mv_rate(_ip(dx), _ip(dy), int(dx.size), _ip(est), _ip(idx))
    return est, idx


def _native_comp_bits(d):
    lib = core_lib()
    d = np.ascontiguousarray(d, np.int32)
    out = np.empty_like(d)
    lib.tv_av1_mv_comp_bits(_ip(d), int(d.size), _ip(out))
    return out


def _check_pairs(dx, dy):
    dx, dy = np.broadcast_arrays(np.asarray(dx, np.int64), np.asarray(dy, np.int64))
    want = old_mv_bits_est(dx, dy)
    est, idx = _native_rate(dx, dy)
    np.testing.assert_array_equal(est, want)
    np.testing.assert_array_equal(idx, np.minimum(63, want))


_EDGES = np.array(sorted({s * ((1 << k) + o) for k in range(31) for o in (-2, -1, 0) for s in (-1, 1)
                          if (1 << k) + o >= 0}), np.int64)


def test_mv_bits_est_dense_range():
    """Every d in [-2^17, 2^17] on one axis, the other at 0, +-1, +-255."""
    d = np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.int64)
    for other in (0, 1, -1, 255, -255):
        _check_pairs(d, other)
        _check_pairs(other, d)


def test_mv_bits_est_power_of_two_edges():
    """d = +-(2^k - 2, 2^k - 1, 2^k) for k <= 30, on both axes and against each other."""
    for other in (0, 1, -1, 255, -255):
        _check_pairs(_EDGES, other)
        _check_pairs(other, _EDGES)
    _check_pairs(_EDGES[:, None], _EDGES[None, :])


def test_me_pen_index_clamps_at_63():
    # 2 * 15 + 1 = 31 bins per component at |d| = 2^15 - 1: the pair is 62, one step on is 64
    dx = np.array([(1 << 15) - 2, (1 << 15) - 1, (1 << 15) - 1, 1 << 30, 0], np.int64)
    dy = np.array([(1 << 15) - 2, (1 << 15) - 2, (1 << 15) - 1, -(1 << 30), 0], np.int64)
    est, idx = _native_rate(dx, dy)
    assert est.tolist() == [58, 60, 62, 122, 2]
    assert idx.tolist() == [58, 60, 62, 63, 2]
    _check_pairs(dx, dy)
    _check_pairs((1 << 16) + np.arange(-3, 4), -(1 << 15) + np.arange(-3, 4)[:, None])


def test_av1_mv_comp_bits():
    d = np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.int64)
    np.testing.assert_array_equal(_native_comp_bits(d), old_mv_comp_bits(d))
    np.testing.assert_array_equal(_native_comp_bits(_EDGES), old_mv_comp_bits(_EDGES))
    both = np.concatenate([_EDGES + 1, _EDGES[np.abs(_EDGES) > 1] - 1])  # odd neighbours of the edges
    np.testing.assert_array_equal(_native_comp_bits(both), old_mv_comp_bits(both))


# ---- golden pin: the golden encoders' streams are the parent commit's -----------------------
W, H = 160, 96
TEXTURED = 7 | 0x80000000


def rolled_frames(n=4):
    """A textured picture rolled by (+37, -21) pels per frame (chroma by (+18, -10)): large,
    growing MVDs against the coarse predictor at the picture edges."""
    from thinvids_amd.models import hevc

    y, u, v = hevc.synth_frame(TEXTURED, 0, W, H)
    return [(np.ascontiguousarray(np.roll(y, (-21 * t, 37 * t), (0, 1))),
             np.ascontiguousarray(np.roll(u, (-10 * t, 18 * t), (0, 1))),
             np.ascontiguousarray(np.roll(v, (-10 * t, 18 * t), (0, 1)))) for t in range(n)]


def _golden_streams():
    from thinvids_amd.models import av1, hevc

    def synth(n, start=0):
        return [hevc.synth_frame(TEXTURED, start + t, W, H) for t in range(n)]

    out = {}
    out["hevc_range64_b1"] = hevc.encode_sequence_cpu(synth(4), qp=27, sao=False, search_range=64, bframes=1)[0]
    out["hevc_range32_b1"] = hevc.encode_sequence_cpu(synth(4), qp=27, sao=False, search_range=32, bframes=1)[0]
    out["hevc_range64_b2_gop5"] = hevc.encode_sequence_cpu(synth(5), qp=27, sao=False, search_range=64, bframes=2)[0]
    out["hevc_range32_b2_gop5"] = hevc.encode_sequence_cpu(synth(5, 20), qp=27, sao=False, search_range=32, bframes=2)[0]
    out["hevc_rolled_range64"] = hevc.encode_sequence_cpu(rolled_frames(4), qp=27, search_range=64)[0]
    out["av1_q100"] = av1.golden_encode(synth(3), W, H, 100).stream
    return {k: {"bytes": len(s), "crc32": zlib.crc32(s) & 0xFFFFFFFF} for k, s in out.items()}


@pytest.fixture(scope="module")
def streams():
    return _golden_streams()


@pytest.mark.parametrize("case", ["hevc_range64_b1", "hevc_range32_b1", "hevc_range64_b2_gop5",
                                  "hevc_range32_b2_gop5", "hevc_rolled_range64", "av1_q100"])
def test_golden_streams_unchanged(streams, case):
    want = json.load(open(GOLDEN))["streams"][case]
    assert streams[case] == want


if __name__ == "__main__":
    import sys

    if "--record" in sys.argv:
        doc = {"how": "python tests/test_mv_rate.py --record, run on the CPU against a build of the commit "
                      "before the closed-form MV rate (bit-by-bit loops in mv_bits_est / mv_comp_bits / bitlen64): "
                      "length and CRC-32 of the golden encoders' bitstreams for the cases of _golden_streams()",
               "streams": _golden_streams()}
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(doc["streams"], indent=1))
