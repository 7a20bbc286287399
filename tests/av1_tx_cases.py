"""Shared inputs of the AV1 transform-split suites (not a test module): seeded clips and golden
encodes computed once per case.

SPECKLE is a smooth, slowly panning background on which small high-contrast patches appear anew
in every frame: the inter residual of a block is confined to one or two of its quadrants, which is
what the 8x8 split (av1_enc.h "transform split") is for; patch-free regions stay skip blocks and
merge.  RAMP is a smooth gradient that brightens from frame to frame: a residual that fills the
block, where the 16x16 transform must keep winning.  SATURATED has oblique stripes of 0 and 255
only.  CUT is the fan cut of av1_dir_cases: with `intra_in_inter` the frame after the cut has
intra blocks, which code tx_depth in a TX_MODE_SELECT frame.  `assert_paths` states the coding
paths on mode words: a case that stops exercising its path fails."""
import numpy as np
from av1_dir_cases import cut_clip, saturated_clip

from thinvids_amd.models import av1

PATHS_SIZE = (200, 136)  # the smallest frame (tried from 200x136 up) on which the golden encoder meets assert_paths
PATHS_FRAMES = 3
_cache = {}


def speckle_clip(w: int, h: int, n: int = 3, seed: int = 11) -> list:
    i, j = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        y = np.rint(100 + 50 * np.sin((j + 2 * t) / 37.0) + 30 * np.cos((i + t) / 23.0))
        r = np.random.default_rng(seed * 1000 + t)
        # patches of 2..6 samples at fresh positions in the left three quarters of the frame;
        # the rest stays clean so that skip blocks can merge
        for _ in range(max(3, (w * h) // 700)):
            sz = int(r.integers(2, 7))
            px, py = int(r.integers(0, max(1, (3 * w) // 4 - sz))), int(r.integers(0, max(1, h - sz)))
            y[py:py + sz, px:px + sz] = (20, 235)[int(r.integers(0, 2))]
        out.append(av1.correlated_chroma(np.clip(y, 0, 255).astype(np.uint8), 4, -3, seed=seed * 100 + t, noise=0))
    return out


def ramp_clip(w: int, h: int, n: int = 3, seed: int = 11) -> list:
    i, j = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        y = np.clip(40 + (i * 5 + j * 3) // 8 + 9 * t, 0, 255).astype(np.uint8)
        out.append(av1.correlated_chroma(y, 8, 8, seed=seed * 100 + t, noise=1))
    return out


CLIPS = {"speckle": speckle_clip, "ramp": ramp_clip, "saturated": lambda w, h, n=2: saturated_clip(w, h, n),
         "cut": lambda w, h, n=4: cut_clip(w, h, n)}


def golden(kind: str, w: int, h: int, n: int, q: int, **tools):
    """(frames, GoldenResult with tx_split=True unless `tools` says otherwise) of a case, computed
    once and shared; never modified."""
    key = (kind, w, h, n, q, tuple(sorted(tools.items())))
    if key not in _cache:
        fr = CLIPS[kind](w, h, n)
        _cache[key] = (fr, av1.golden_encode(fr, w, h, q, **{"tx_split": True, **tools}))
    return _cache[key]


def split_blocks(mode):
    """(split mask, quadrant mask) of mode words, after the checks every case must meet: the split
    bit only on non-skip, unmerged inter blocks with the Y bit and a nonzero quadrant mask, and
    never on a key frame (`mode`: (frames, blocks), frame 0 the key frame)."""
    m = np.asarray(mode).astype(np.int64) & 0xFFFFFFFF
    split, qm = av1.mode_tx(m)
    inter, skip, ybit, bsz = (m & 1) == 1, ((m >> 9) & 1) == 1, ((m >> 10) & 1) == 1, (m >> 13) & 3
    ok = inter & ~skip & ybit & (bsz == 0)
    assert not (split & ~ok).any(), "split bit on a skip / intra / merged / Y-less block"
    assert (qm[split] != 0).all(), "split block without a nonzero quadrant"
    assert not ((m >> 15) & 15)[inter & ~split].any(), "quadrant bits on an inter block that is not split"
    if m.ndim == 2:
        assert not split[0].any(), "split block in a key frame"
    return split, qm


def assert_paths(kind: str, mode) -> None:
    """The coding paths the case exists for, read off mode words (frames, blocks)."""
    m = np.asarray(mode).astype(np.int64) & 0xFFFFFFFF
    split, qm = split_blocks(m)
    inter, skip = (m & 1) == 1, ((m >> 9) & 1) == 1
    kept = inter & ~skip & ~split & (((m >> 10) & 1) == 1)
    assert kept.any(), f"{kind}: no kept 16x16 luma transform"
    if kind == "ramp":
        assert not split.any(), "ramp: a block of the gradient was split"
        return
    nq = np.array([bin(int(x)).count("1") for x in qm.reshape(-1)]).reshape(qm.shape)
    assert (split & (nq == 1)).any(), f"{kind}: no split block with exactly one nonzero quadrant"
    assert (split & ((nq == 2) | (nq == 3))).any(), f"{kind}: no split block with 2 or 3 nonzero quadrants"
    assert (split & (nq == 4)).any(), f"{kind}: no split block with four nonzero quadrants"
    assert (inter & skip).any(), f"{kind}: no skip block"
    assert (inter & (((m >> 13) & 3) > 0)).any(), f"{kind}: no merged block"
