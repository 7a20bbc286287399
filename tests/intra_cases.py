"""Shared inputs of the large-TB intra suites (not a test module): deterministic pictures on
which the golden encoder codes 16x16 and 32x32 intra CUs with residual next to 8x8 ones.  The
synthetic source alone never does (its I pictures are all 8x8 CUs), so without these the
second and third gather rounds of the wave predictor (csrc/gpu/wave_intra.h), its 32-wide
smoothing, the 32x32 no-edge-filter case and the 8x8 / 16x16 chroma TBs run in no GPU test.

Per 32x32 CTB column of the luma plane (lx, ly = position within the CTB; bump = 3 in the
13x13 centre of every CTB, else 0):

    column 0     60 + y                   constant rows: exact from the left neighbour
    column 1     60 + y + bump            the same with a residual in the middle of the CTB
    column 2     even CTB rows the synthetic source (8x8 CUs), odd ones a 16x16 checkerboard
    columns 3..  70 + 2 lx + bump         constant columns: exact from the CTB above

Chroma is a slow ramp, Cb with a checkerboard of 8x8 steps.  Cases (width, height, QP):
128x96 is coded as it is; 122x90 is coded at 128x96, so display and coded size differ.  Both
have three CTB rows (above-right available and unavailable in turn), and the picture corners
cover the all-unavailable and the below-left-unavailable references.  Each case is also coded
flipped top to bottom.  tests/test_intra_cpu.py asserts that the golden encoder takes the
large CUs on these pictures; tests/test_gpu_intra.py compares the engine with it."""
import functools

import numpy as np

from thinvids_amd.models import hevc

CASES = [(128, 96, 27), (122, 90, 22)]
SEARCH_RANGE = 16


@functools.lru_cache(maxsize=None)
def frame(w, h, flip=False):
    """The display-size (Y, U, V) picture of a case, or its top-to-bottom mirror."""
    y, x = np.mgrid[0:h, 0:w]
    lx, ly = x % 32, y % 32
    bump = 3 * ((abs(lx - 16) < 7) & (abs(ly - 16) < 7))
    mixed = np.where((y // 32) % 2 == 0, hevc.synth_frame(5, 0, w, h)[0], 90 + 40 * (((x // 16) + (y // 16)) & 1))
    luma = np.select([x // 32 == 0, x // 32 == 1, x // 32 == 2], [60 + y, 60 + y + bump, mixed], 70 + 2 * lx + bump)
    cy2, cx2 = np.mgrid[0:h // 2, 0:w // 2]
    cb = 128 + cx2 // 3 + 6 * (((cx2 // 4) + (cy2 // 4)) & 1)
    cr = 120 + cy2 // 2
    planes = [np.clip(p, 0, 255).astype(np.uint8) for p in (luma, cb, cr)]
    return tuple(np.ascontiguousarray(p[::-1] if flip else p) for p in planes)


@functools.lru_cache(maxsize=None)
def golden(w, h, qp, sign_hiding, flip):
    """(stream, reconstructions) of the golden encoder for the case's segment [frame, frame]."""
    f = frame(w, h, flip)
    return hevc.encode_sequence_cpu([f, f], qp=qp, search_range=SEARCH_RANGE, sign_hiding=sign_hiding)
