"""The tiled form of the synthetic source (csrc/include/tv/synth_tile.h), walked on the host by
tv_synth_frame_tiled, must give the bytes of its definition (tv_synth_frame, tv/synth.h) over
the display area, and replicate the last display column / row into the padding of the coded
planes: at picture edges inside a 4-sample item, odd chroma widths, pictures smaller than a
tile, tile seams inside cells and objects, far pans and both variants."""
import ctypes as C
import functools

import numpy as np
import pytest

from thinvids_amd._native import core_lib
from thinvids_amd.models import hevc

SIZES = [(160, 96), (322, 178), (34, 18), (544, 40)]
TILES = [(256, 16), (256, 32), (32, 8)]  # (256, 32) is the kernel's shape (kSynthTileW x kSynthTileH)
TIMES = [0, 1, 63, 100003]
SEEDS = [1, 5, 11, 7 | 0x80000000]
M32 = 0xFFFFFFFF


def synth_hash(x, y, seed):
    h = (x * 374761393 + y * 668265263 + seed * 2246822519) & M32
    h = ((h ^ (h >> 13)) * 1274126177) & M32
    return h ^ (h >> 16)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


@functools.lru_cache(maxsize=None)
def reference(seed, t, w, h):
    planes = hevc.synth_frame(seed, t, w, h)
    for p in planes:
        p.setflags(write=False)
    return planes


def tiled(seed, t, w, h, tw, th):
    cw, ch = hevc.coded_size(w, h)
    y = np.full((ch, cw), 0xA5, np.uint8)
    u = np.full((ch // 2, cw // 2), 0xA5, np.uint8)
    v = np.full_like(u, 0xA5)
    core_lib().tv_synth_frame_tiled(seed & M32, t, w, h, tw, th, _p(y), _p(u), _p(v))
    return y, u, v


def check_planes(got, ref, what):
    """display area equal to ref, padding equal to the last display column / row"""
    for c, (g, r) in enumerate(zip(got, ref)):
        dh, dw = r.shape
        g = g.reshape(-1, g.shape[-1])
        np.testing.assert_array_equal(g[:dh, :dw], r, err_msg=f"{what} plane {c} display area")
        np.testing.assert_array_equal(g[:dh, dw:], np.repeat(r[:, -1:], g.shape[1] - dw, axis=1),
                                      err_msg=f"{what} plane {c} right padding")
        np.testing.assert_array_equal(g[dh:], np.repeat(g[dh - 1:dh], g.shape[0] - dh, axis=0),
                                      err_msg=f"{what} plane {c} bottom padding")


def test_seeds_cover_both_object_shapes():
    """bit 28 of synth_hash(k, 43, seed) is object k's shape (synth_object): rectangles and
    ellipses both occur, in the smooth seeds and in the textured one"""
    for textured in (False, True):
        seeds = [s for s in SEEDS if bool(s >> 31) == textured]
        assert {(synth_hash(k, 43, s) >> 28) & 1 for s in seeds for k in range(6)} == {0, 1}, textured


@pytest.mark.parametrize("tile", TILES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_tiled_equals_definition(seed, size, tile):
    w, h = size
    for t in TIMES:
        check_planes(tiled(seed, t, w, h, *tile), reference(seed, t, w, h), f"seed {seed:#x} t {t}")

