"""AV1 tool kernels (k_av1.hip: CDEF dir / search / apply, Wiener apply / stats, self-guided
apply / stats) against the C++ golden model (av1_tools.cpp) where tests/test_av1_tools.py
does not look: planes whose last filter block / restoration unit is partial (8 wide, 8 high,
2 x 6), planes smaller than one block, full-range content (noise, 0/255), the CDEF skip flag,
preset mask and checkerboard search the engine uses on every frame, damping 3 and 6, chroma
planes indexed into a wider luma direction array, all 16 self-guided sets and Wiener taps /
self-guided weights at their limits.  Every batch holds B = 3 planes of different content
(a plane-stride error shows).  All comparisons are bit-exact.

The CPU tests pin the golden model itself to the numpy references of tests/test_av1_tools.py
at the same geometries, and the self-guided inputs to content the filter really changes."""
import functools

import numpy as np
import pytest
from av1_edge_cases import luma
from test_av1_tools import _np_cdef_dir, _np_cdef_pixel, _np_wiener_unit

from thinvids_amd.models.av1_engine import CDEF_MASK_UV, CDEF_MASK_Y
from thinvids_amd.ops import av1

LUMA = [(8, 8), (72, 40), (200, 136)]            # (w, h); 200x136: last fb column 8 wide, last row 8 high
CHROMA = [((4, 4), (8, 8)), ((100, 68), (200, 136))]  # (chroma plane, the luma plane its dirs come from)
LR_GEO = LUMA + [(4, 4), (100, 68), (66, 70)]    # 66x70: last unit 2 wide / 6 high (< the 3-pel halo)
SKIP = 0x80                                      # av1_defs.h kCdefSkipBlock
SKIPPED = 1 << 40                                # av1_defs.h kCdefSkipped
_ids = lambda geos: [f"{w}x{h}" for w, h in geos]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _stack(kinds: tuple, w: int, h: int, seed: int) -> np.ndarray:
    """(B, h, w) uint8, plane b of content kinds[b] (its own generator state and frame)."""
    rng = np.random.default_rng(seed)
    out = np.stack([luma(k, b, w, h, rng) for b, k in enumerate(kinds)])
    out.setflags(write=False)
    return out


def _flat(w, h):
    return np.stack([np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), luma("checker1", 1, w, h, None)])


@functools.lru_cache(maxsize=None)
def _cdef_case(w: int, h: int):
    """Luma source / reconstruction stacks (noise, binary, edges) of one geometry, the golden
    directions and variances of the reconstruction, and the directions with the skip flag on
    about a quarter of the blocks."""
    kinds = ("noise", "binary", "edges")
    src, rec = _stack(kinds, w, h, 11), _stack(kinds, w, h, 12)
    dv = [av1.cdef_dirs(p) for p in rec]
    d = np.stack([x[0].ravel() for x in dv])
    v = np.stack([x[1].ravel() for x in dv])
    flag = np.random.default_rng(13).random(d.shape) < 0.25
    if d.shape[1] == 1:
        flag[:] = [[False], [True], [False]]
    ds = (d | (flag * SKIP)).astype(np.uint8)
    for a in (d, v, ds):
        a.setflags(write=False)
    return src, rec, d, v, ds


def _cdef_planes(geo, chroma):
    """(src, rec, flagged dirs, var, luma_w8) of a luma geometry or a (chroma, luma) pair."""
    if not chroma:
        src, rec, _, v, ds = _cdef_case(*geo)
        return src, rec, ds, v, geo[0] // 8
    (cw, ch), (lw, lh) = geo
    _, _, _, v, ds = _cdef_case(lw, lh)
    kinds = ("binary", "edges", "noise")
    return _stack(kinds, cw, ch, 21), _stack(kinds, cw, ch, 22), ds, v, lw // 8


_CDEF_GEOS = [(g, False) for g in LUMA] + [(g, True) for g in CHROMA]
_CDEF_IDS = [f"{'uv' if c else 'y'}{(g[0] if c else g)[0]}x{(g[0] if c else g)[1]}" for g, c in _CDEF_GEOS]
# per-block presets: off, identity, the last preset, primary only (9, 0), secondary only (0, 2)
_PRESETS = [-1, 0, 63, 9 * 4, 2, 17, 40, 5, 15 * 4 + 1, 3]


def _fb_presets(nfb: int, rot: int) -> np.ndarray:
    return np.array([[_PRESETS[(b * 3 + f + rot) % len(_PRESETS)] for f in range(nfb)] for b in range(3)], np.int8)


def _gpu(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached inputs are read-only


# ------------------------------------------------------------------ CPU: golden == numpy ----
def _np_cdef_plane(P, d, v, lw8, fb_preset, chroma, damping):
    h, w = P.shape
    bs, fbs = (4, 32) if chroma else (8, 64)
    nfx = -(-w // fbs)
    out = P.copy()
    for y in range(h):
        for x in range(w):
            p = int(fb_preset[(y // fbs) * nfx + x // fbs])
            d0, var = int(d[(y // bs) * lw8 + x // bs]), int(v[(y // bs) * lw8 + x // bs])
            if p < 0 or d0 & SKIP:
                continue
            pri, sec = p >> 2, (4 if p & 3 == 3 else p & 3)
            if not chroma:
                i = (var >> 6).bit_length() - 1 if var >> 6 else 0
                pri = (pri * (4 + min(i, 12)) + 8) >> 4 if var else 0
            if pri | sec:
                out[y, x] = _np_cdef_pixel(P, x, y, pri, sec, damping - int(chroma), (d0 & 7) if p >> 2 else 0)
    return out


@pytest.mark.parametrize("w,h", LUMA, ids=_ids(LUMA))
def test_golden_cdef_dirs_match_numpy(w, h):
    for stack in (_stack(("noise", "binary", "checker1"), w, h, 3), _flat(w, h)):
        for P in stack:
            d, v = av1.cdef_dirs(P)
            want = [[_np_cdef_dir(P[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]) for bx in range(w // 8)]
                    for by in range(h // 8)]
            np.testing.assert_array_equal(np.stack([d, v], -1), np.array(want).reshape(h // 8, w // 8, 2))


@pytest.mark.parametrize("geo,chroma", [((8, 8), False), ((72, 40), False), (((4, 4), (8, 8)), True),
                                        (((36, 20), (72, 40)), True)], ids=["y8x8", "y72x40", "uv4x4", "uv36x20"])
def test_golden_cdef_apply_matches_numpy_with_skip_flags(geo, chroma):
    """cdef_apply of the golden model against the per-pixel numpy filter: skip-flagged blocks
    and off / identity blocks stay untouched, primary-only and secondary-only presets, the
    direction-0 rule of presets without a primary strength, both ends of the damping range."""
    _, rec, ds, v, lw8 = _cdef_planes(geo, chroma)
    assert (ds & SKIP).any() and not (ds & SKIP).all()
    nfb = av1.n_fb(rec.shape[2], rec.shape[1], chroma)
    for damping, rot in ((3, 2), (6, 3), (6, 6)):
        fbp = _fb_presets(nfb, rot)
        for b in range(3):
            got = av1.cdef_apply(rec[b], ds[b], v[b], fbp[b], chroma, damping, luma_w8=lw8)
            np.testing.assert_array_equal(got, _np_cdef_plane(rec[b], ds[b], v[b], lw8, fbp[b], chroma, damping),
                                          err_msg=f"plane {b} damping {damping} presets {fbp[b].tolist()}")


_TAPS_MIN, _TAPS_MAX, _TAPS_MIX = (-5, -23, -17), (10, 8, 46), (10, -23, 46)
_WIENER = [_TAPS_MIN + _TAPS_MIN, _TAPS_MAX + _TAPS_MAX, _TAPS_MIN + _TAPS_MAX, _TAPS_MAX + _TAPS_MIN,
           _TAPS_MIX + (-5, 8, -17), (-5, 8, -17) + _TAPS_MIX]


@pytest.mark.parametrize("w,h", LR_GEO, ids=_ids(LR_GEO))
def test_golden_wiener_apply_matches_numpy_at_tap_limits(w, h):
    rec = _stack(("binary", "noise", "binary"), w, h, 31)
    nu = av1.n_units(w, h)
    for k, taps in enumerate(_WIENER):
        P = rec[k % 3]
        np.testing.assert_array_equal(av1.wiener_apply(P, np.array([taps] * nu, np.int32)), _np_wiener_unit(P, taps),
                                      err_msg=f"taps {taps}")


_SGR_KINDS = ("bright", "dark", "ramp")
_SGR_W = [(-96, 95), (31, -32), (0, 0)]


def test_sgr_content_is_changed_by_every_set():
    """Input condition of the self-guided tests: with weights (-96, 95) every set changes at
    least 10 % of the samples of each content plane (pure noise would not do: its variance
    drives the guide to the identity)."""
    w, h = 200, 136
    rec = _stack(_SGR_KINDS, w, h, 41)
    nu = av1.n_units(w, h)
    for st in range(16):
        for kind, P in zip(_SGR_KINDS, rec):
            out = av1.sgr_apply(P, np.array([[st, -96, 95]] * nu, np.int32))
            assert (out != P).mean() >= 0.10, f"set {st} leaves {kind} nearly unchanged: {(out != P).mean():.3f}"


# ---------------------------------------------------------------------------- GPU: CDEF ----
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", LUMA, ids=_ids(LUMA))
def test_gpu_cdef_dirs_full_range_content(w, h):
    for stack in (_stack(("noise", "binary", "checker1"), w, h, 3), _flat(w, h)):
        d, v = av1.cdef_dirs(_gpu(stack))
        d, v = d.cpu().numpy(), v.cpu().numpy()
        for b, P in enumerate(stack):
            dc, vc = av1.cdef_dirs(P)
            np.testing.assert_array_equal(d[b], dc.ravel(), err_msg=f"plane {b}: dir")
            np.testing.assert_array_equal(v[b], vc.ravel(), err_msg=f"plane {b}: var")
            want = [_np_cdef_dir(P[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]) for by in range(h // 8)
                    for bx in range(w // 8)]
            np.testing.assert_array_equal(np.stack([d[b], v[b]], -1), np.array(want))


@pytest.mark.gpu
@pytest.mark.parametrize("geo,chroma", _CDEF_GEOS, ids=_CDEF_IDS)
def test_gpu_cdef_search_and_apply_with_skip_flags(geo, chroma):
    src, rec, ds, v, lw8 = _cdef_planes(geo, chroma)
    S, R, D, V = _gpu(src), _gpu(rec), _gpu(ds), _gpu(v)
    nfb = av1.n_fb(rec.shape[2], rec.shape[1], chroma)
    for damping, rot in ((3, 0), (6, 5)):
        sg = av1.cdef_search(S, R, D, V, chroma, damping, luma_w8=lw8).cpu().numpy()
        fbp = _fb_presets(nfb, rot)
        og = av1.cdef_apply(R, D, V, _gpu(fbp), chroma, damping, luma_w8=lw8).cpu().numpy()
        for b in range(3):
            sc = av1.cdef_search(src[b], rec[b], ds[b], v[b], chroma, damping, luma_w8=lw8)
            np.testing.assert_array_equal(sg[b], sc.astype(np.int64), err_msg=f"search plane {b} damping {damping}")
            oc = av1.cdef_apply(rec[b], ds[b], v[b], fbp[b], chroma, damping, luma_w8=lw8)
            np.testing.assert_array_equal(og[b], oc, err_msg=f"apply plane {b} damping {damping}")


_MASK17 = sum(1 << p for p in range(3, 64, 4)) | (1 << 62)  # 17 presets: one more than a 16-preset chunk
assert bin(_MASK17).count("1") == 17


@pytest.mark.gpu
@pytest.mark.parametrize("geo,chroma", _CDEF_GEOS, ids=_CDEF_IDS)
def test_gpu_cdef_search_preset_mask(geo, chroma):
    src, rec, ds, v, lw8 = _cdef_planes(geo, chroma)
    S, R, D, V = _gpu(src), _gpu(rec), _gpu(ds), _gpu(v)
    full = np.stack([av1.cdef_search(src[b], rec[b], ds[b], v[b], chroma, 4, luma_w8=lw8) for b in range(3)])
    full = full.astype(np.int64)
    for mask in (1 << 0, 1 << 63, _MASK17, CDEF_MASK_Y, CDEF_MASK_UV):
        got = av1.cdef_search(S, R, D, V, chroma, 4, luma_w8=lw8, pmask=mask).cpu().numpy()
        sel = np.array([bool(mask >> p & 1) for p in range(64)])
        np.testing.assert_array_equal(got[..., sel], full[..., sel], err_msg=f"mask {mask:#x}: selected presets")
        assert (got[..., ~sel] == SKIPPED).all(), f"mask {mask:#x}: skipped presets"


@pytest.mark.gpu
@pytest.mark.parametrize("geo,chroma", _CDEF_GEOS, ids=_CDEF_IDS)
def test_gpu_cdef_search_checkerboard(geo, chroma):
    """checker=True measures only the 8x8 (chroma 4x4) blocks with (bx + by) even.  The golden
    C API has no such search; the reference is the golden cdef_apply with one preset on every
    filter block and the SSE against the source summed over those blocks."""
    src, rec, ds, v, lw8 = _cdef_planes(geo, chroma)
    h, w = rec.shape[1:]
    bs, fbs = (4, 32) if chroma else (8, 64)
    nfx, nfb = -(-w // fbs), av1.n_fb(w, h, chroma)
    presets = (0, 2, 9 * 4, 27, 63)
    mask = sum(1 << p for p in presets)
    got = av1.cdef_search(_gpu(src), _gpu(rec), _gpu(ds), _gpu(v), chroma, 5, luma_w8=lw8, pmask=mask,
                          checker=True).cpu().numpy()
    yy, xx = np.mgrid[0:h, 0:w]
    even = ((yy // bs + xx // bs) & 1) == 0
    fb = (yy // fbs) * nfx + xx // fbs
    for p in presets:
        for b in range(3):
            out = av1.cdef_apply(rec[b], ds[b], v[b], np.full(nfb, p, np.int8), chroma, 5, luma_w8=lw8)
            e = (out.astype(np.int64) - src[b]) ** 2 * even
            want = np.bincount(fb.ravel(), weights=e.ravel(), minlength=nfb).astype(np.int64)
            np.testing.assert_array_equal(got[b, :, p], want, err_msg=f"preset {p} plane {b}")
    unsel = np.array([p not in presets for p in range(64)])
    assert (got[..., unsel] == SKIPPED).all()


# -------------------------------------------------------------------- GPU: restoration ----
def _unit_table(pool, nu: int, call: int) -> np.ndarray:
    """(3, nu, len(pool[0])): the pool dealt over (call, plane, unit) in order."""
    idx = (call * 3 * nu + np.arange(3 * nu)) % len(pool)
    return np.array(pool, np.int32)[idx].reshape(3, nu, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", LR_GEO, ids=_ids(LR_GEO))
def test_gpu_wiener_apply_taps_at_limits(w, h):
    rec = _stack(("binary", "noise", "binary"), w, h, 31)
    R = _gpu(rec)
    nu = av1.n_units(w, h)
    pool = [list(t) for t in _WIENER] + [[0] * 6]  # all-zero (off) units between active ones
    for call in range(-(-len(pool) // (3 * nu)) + 1):
        coef = _unit_table(pool, nu, call)
        og = av1.wiener_apply(R, coef).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(og[b], av1.wiener_apply(rec[b], coef[b]), err_msg=f"call {call} plane {b}")
    for taps in (_WIENER[0], _WIENER[2]):  # one tap set on every unit: the whole-plane numpy filter
        og = av1.wiener_apply(R, np.array([[taps] * nu] * 3, np.int32)).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(og[b], _np_wiener_unit(rec[b], taps), err_msg=f"taps {taps} plane {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", LR_GEO, ids=_ids(LR_GEO))
def test_gpu_wiener_stats_other_taps_at_limits(w, h):
    kinds = ("binary", "noise", "binary")
    src, rec = _stack(kinds, w, h, 32), _stack(kinds, w, h, 31)
    S, R = _gpu(src), _gpu(rec)
    nu = av1.n_units(w, h)
    pool = [list(_TAPS_MIN), list(_TAPS_MAX), list(_TAPS_MIX), [0, 0, 0]]
    for call in range(-(-len(pool) // (3 * nu)) + 1):
        other = _unit_table(pool, nu, call)
        for dirn in (0, 1):
            sg = av1.wiener_stats(S, R, dirn, other).cpu().numpy()
            for b in range(3):
                np.testing.assert_array_equal(sg[b], av1.wiener_stats(src[b], rec[b], dirn, other[b]),
                                              err_msg=f"call {call} direction {dirn} plane {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", LR_GEO, ids=_ids(LR_GEO))
def test_gpu_sgr_apply_all_sets_weights_at_limits(w, h):
    rec = _stack(_SGR_KINDS, w, h, 41)
    R = _gpu(rec)
    nu = av1.n_units(w, h)
    pool = []
    for st in range(16):  # every (set, weights) pair; an off unit after every fourth set
        pool += [[st, w0, w1] for w0, w1 in _SGR_W]
        if st % 4 == 3:
            pool.append([-1, 0, 0])
    for call in range(-(-len(pool) // (3 * nu))):
        prm = _unit_table(pool, nu, call)
        og = av1.sgr_apply(R, prm).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(og[b], av1.sgr_apply(rec[b], prm[b]),
                                          err_msg=f"call {call} plane {b} params {prm[b].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", LR_GEO, ids=_ids(LR_GEO))
def test_gpu_sgr_stats_all_sets(w, h):
    src, rec = _stack(_SGR_KINDS, w, h, 42), _stack(_SGR_KINDS, w, h, 41)
    S, R = _gpu(src), _gpu(rec)
    for st in range(16):
        sg = av1.sgr_stats(S, R, st).cpu().numpy()
        for b in range(3):
            np.testing.assert_array_equal(sg[b], av1.sgr_stats(src[b], rec[b], st), err_msg=f"set {st} plane {b}")
