"""AV1 GPU engine against the golden encoder at the edges the synthetic-content tests of
tests/test_av1_codec.py never reach: q-index 1 and 255, saturated / high-contrast content
(levels in the thousands at q 1), content that turns self-guided restoration on (both
candidate sets, weights at the xqd clamps) and planes smaller than one superblock.

The CPU test pins the inputs: the golden encoder is sound on every case (oracle decoder and,
where present, dav1d reproduce its reconstruction) and the cases really reach the edges they
are there for.  The GPU tests are bit-exact comparisons (av1_edge_cases.gpu_vs_golden_segments).

Every geometry the golden encoder accepts runs on the engine too (coded sizes are multiples
of 16, at least 16x16), so no refusal is asserted here; see the README's AV1 section."""
import numpy as np
import pytest
from av1_edge_cases import gpu_vs_golden_segments, segment

from thinvids_amd.models import av1, avif

NFRAMES = 3
# (w, h, q-index, content)
CASES = [
    (200, 120, 1, "checker8"),
    (200, 120, 1, "flatswing"),
    (200, 120, 1, "noise"),
    (200, 120, 255, "binary"),
    (200, 120, 20, "edges"),
    (200, 120, 100, "ramp"),
    (200, 120, 100, "dark"),
    (200, 120, 20, "synth"),
    (72, 40, 100, "noise"),
    (24, 16, 255, "binary"),
    (16, 16, 1, "noise"),
]
_IDS = [f"{w}x{h}-q{q}-{kind}" for w, h, q, kind in CASES]


def _segments(w, h, kind):
    """The batch of two: the second segment has its own seed and starts 5 frames later."""
    return [segment(kind, w, h, NFRAMES, seed=101), segment(kind, w, h, NFRAMES, seed=202, t0=5)]


def _chosen(res, w, h):
    """(set, xqd0, xqd1) rows of the chosen units that exist (av1.lr_real_units)."""
    real = av1.lr_real_units(*av1.coded_size(w, h))
    lr = res.lr[:, real].reshape(-1, 3)
    return lr[lr[:, 0] >= 0]


def test_golden_is_sound_and_cases_reach_their_edges():
    from test_av1_conformance import _check as dav1d_check

    peak_q1 = 0
    for w, h, q, kind in CASES:
        for b, fr in enumerate(_segments(w, h, kind)):
            res = av1.golden_encode(fr, w, h, q)
            dec = av1.decode(res.stream)
            np.testing.assert_array_equal(dec.frames, res.recon, err_msg=f"{w}x{h} q{q} {kind} segment {b}: oracle")
            if avif.dav1d_available():
                dav1d_check(res.stream, res.tu_sizes, res.recon, w, h)
            lev = max(int(np.abs(x.astype(np.int32)).max()) for x in (res.ly, res.lu, res.lv))
            if q == 1:
                peak_q1 = max(peak_q1, lev)
            if b:
                continue
            sel = _chosen(res, w, h)
            if (q, kind) == (20, "synth"):
                assert {4, 10} <= set(sel[:, 0].tolist()), f"synth q 20 chose sets {sorted(set(sel[:, 0].tolist()))}"
            if (q, kind) == (100, "ramp"):
                assert ((sel[:, 1] == 31) | (sel[:, 2] == -32)).any(), "ramp q 100: no unit at an xqd clamp"
    assert peak_q1 >= 2000, f"q-index 1: max |level| {peak_q1}"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,q,kind", CASES, ids=_IDS)
def test_gpu_av1_engine_matches_golden_at_edges(w, h, q, kind):
    gpu_vs_golden_segments(w, h, _segments(w, h, kind), q)
