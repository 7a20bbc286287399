"""Shared inputs of the SAO suites (not a test module): seeded source / deblocked picture pairs
at the geometries where the strip kernel (k_sao_decide: four CTBs per workgroup, a wave per
CTB) can break, and their golden results computed once per case.

Geometries (display size; the pictures are generated at the coded size, so the padding holds
content of its own and the display-area SSE differs from the whole-picture one):

    32x32    1x1 CTBs  all four borders in one CTB, strip of one
    96x64    3x2       only a partial strip
    128x32   4x1       exactly one full strip
    160x96   5x3       full strip + strip of one, interior CTBs
    150x70   5x3       display edge inside a dword (150 % 4 = 2, chroma 75 % 4 = 3); rows 70-95 outside the SSE
    224x96   7x3       partial strip of three with an interior CTB
    288x64   9x2       two full strips + one

Contents: "noise" uniform random deblocked bytes under a source within +-12 of them; "ramp" a
stepped ramp with sparse +-1 extrema whose source lowers the maxima and raises the minima by 9
(offsets saturate at +-7); "rails" a checkerboard of CTBs with deblocked values in {0, 1, 2} or
in {253, 254, 255} under a source at 0 / 255 (filtered samples clip at both ends: an offset of
-2 meets a local maximum of 1); "flat" source = deblocked and constant
(everything off).  Every case has B = 3 pictures with slice QPs 0, 27, 51; sao_lambda16(0) is 0,
so at QP 0 every SSE-reducing offset is taken."""
import functools

import numpy as np

from thinvids_amd.models import hevc

GEOS = [(32, 32), (96, 64), (128, 32), (160, 96), (150, 70), (224, 96), (288, 64)]
CONTENTS = ["noise", "ramp", "rails", "flat"]
QPS = [0, 27, 51]
CASES = [(w, h, kind) for (w, h) in GEOS for kind in CONTENTS]


def _plane(kind, rng, ph, pw, n):
    """(source, deblocked) of one ph x pw plane with CTBs of side n."""
    if kind == "noise":
        deb = rng.integers(0, 256, (ph, pw))
        return np.clip(deb + rng.integers(-12, 13, (ph, pw)), 0, 255), deb
    if kind == "ramp":
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = 60 + xx // 8 + yy // 8
        bump = rng.integers(0, 24, (ph, pw))
        ext = (bump == 0).astype(int) - (bump == 1).astype(int)  # sparse +1 maxima, -1 minima
        return base + ext - 9 * ext, base + ext
    if kind == "rails":
        yy, xx = np.mgrid[0:ph, 0:pw]
        high = ((xx // n + yy // n) & 1).astype(bool)  # checkerboard of low and high CTBs
        low = rng.choice([0, 1, 2], (ph, pw), p=[0.45, 0.1, 0.45])
        deb = np.where(high, 255 - low, low)
        return np.where(high, 255, 0), deb
    v = int(rng.integers(16, 240))
    deb = np.full((ph, pw), v)
    return deb, deb


@functools.lru_cache(maxsize=None)
def pictures(w, h, kind):
    """B = 3 (source, deblocked) picture pairs of one case, each a (Y, U, V) tuple at coded size."""
    cw, ch = hevc.coded_size(w, h)
    src, deb = [], []
    for b in range(len(QPS)):
        rng = np.random.default_rng([w, h, CONTENTS.index(kind), b])
        planes = [_plane(kind, rng, ch >> (c > 0), cw >> (c > 0), 32 >> (c > 0)) for c in range(3)]
        src.append(tuple(np.ascontiguousarray(s, np.uint8) for s, _ in planes))
        deb.append(tuple(np.ascontiguousarray(d, np.uint8) for _, d in planes))
    return src, deb


@functools.lru_cache(maxsize=None)
def golden(w, h, kind):
    """[(params [CTB rows, CTB columns, 3], filtered picture)] of the case's three pictures."""
    src, deb = pictures(w, h, kind)
    return [hevc.sao_picture_cpu(src[b], deb[b], QPS[b]) for b in range(len(QPS))]


def display_sse(w, h, src, out):
    """Integer squared error of the three planes over the display area."""
    return [int(((s[:h >> (c > 0), :w >> (c > 0)].astype(np.int64) - o[:h >> (c > 0), :w >> (c > 0)]) ** 2).sum())
            for c, (s, o) in enumerate(zip(src, out))]


def sao_type(p):
    return p & 3


def sao_class(p):
    return (p >> 2) & 31


def sao_offsets(p):
    return [int((p >> (7 + 4 * i)) & 15) - 8 for i in range(4)]
