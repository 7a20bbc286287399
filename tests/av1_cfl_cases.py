"""Shared inputs of the AV1 chroma-from-luma suites (not a test module): seeded clips whose
chroma follows their luma (av1.correlated_chroma: U = 128 + k_u * (Y2x2 - 128) / 8 + noise), so
the alpha the encoder fits is about k, and golden encodes computed once per case.

Between them the cases make the golden encoder choose a positive and a negative alpha (CORR),
a clamped |alpha| = 16 (STEEP, |k| = 40), a block with exactly one alpha zero (ONE_PLANE, V flat
at 128 and no noise) and blocks where CfL is evaluated and loses (CORR: not every block of the
clip takes it); FLAT has a constant luma plane (den = 0 in every block: CfL cannot be chosen);
SATURATED has every sample at 0 or 255, so predictions clip.  `assert_paths` states those
conditions on the golden mode words: a case that stops exercising its path fails."""
import numpy as np

from thinvids_amd.models import av1, hevc

CORR, STEEP, ONE_PLANE = (6, -5), (40, -40), (5, 0)
_cache = {}


def corr_clip(w: int, h: int, n: int = 1, k=CORR, seed: int = 3, t0: int = 0) -> list:
    """n frames: synthetic luma, chroma following it with slopes k (eighths); +-1 noise
    unless a plane's slope is zero (that plane is then exactly 128)."""
    noise = 0 if 0 in k else 1
    return [av1.correlated_chroma(hevc.synth_frame(seed, t0 + t, w, h)[0], k[0], k[1], seed=seed * 100 + t, noise=noise)
            for t in range(n)]


def flat_clip(w: int, h: int, n: int = 1, seed: int = 3) -> list:
    """Constant luma (128) under the synthetic source's own chroma: den = 0 in every block."""
    out = []
    for t in range(n):
        _, u, v = hevc.synth_frame(seed, t, w, h)
        out.append((np.full((h, w), 128, np.uint8), np.ascontiguousarray(u), np.ascontiguousarray(v)))
    return out


def saturated_clip(w: int, h: int, n: int = 1, seed: int = 3) -> list:
    """Luma thresholded to 0 / 255, chroma equal / opposite to its 2x2-subsampled luma: every
    sample is 0 or 255 and the fitted alphas are large, so CfL predictions clip at both ends."""
    out = []
    for t in range(n):
        y = ((hevc.synth_frame(seed, t, w, h)[0] > 128) * 255).astype(np.uint8)
        _, u, v = av1.correlated_chroma(y, 8, -8, noise=0)
        out.append((y, ((u > 128) * 255).astype(np.uint8), ((v > 128) * 255).astype(np.uint8)))
    return out


def cut_corr_clip(w: int, h: int, n: int = 4, cut: int = 2) -> list:
    """A cut clip (frames from `cut` on are unrelated content) with correlated chroma throughout."""
    a = corr_clip(w, h, n, seed=7)
    b = corr_clip(w, h, n, seed=23, t0=40)
    return a[:cut] + b[cut:]


CLIPS = {"corr": corr_clip, "steep": lambda w, h, n=1: corr_clip(w, h, n, STEEP),
         "one_plane": lambda w, h, n=1: corr_clip(w, h, n, ONE_PLANE), "flat": flat_clip, "saturated": saturated_clip,
         "cut": lambda w, h, n=4: cut_corr_clip(w, h, n)}


def golden(kind: str, w: int, h: int, n: int, q: int, **tools):
    """(frames, GoldenResult with cfl=True) of a case, computed once and shared; never modified."""
    key = (kind, w, h, n, q, tuple(sorted(tools.items())))
    if key not in _cache:
        fr = CLIPS[kind](w, h, n)
        _cache[key] = (fr, av1.golden_encode(fr, w, h, q, cfl=True, **tools))
    return _cache[key]


def cfl_blocks(mode):
    """(CfL mask over intra blocks, alpha_u, alpha_v of the CfL blocks)."""
    is_cfl, au, av_ = av1.mode_cfl(mode)
    assert not (is_cfl & ((np.asarray(mode) & 1) == 1)).any(), "an inter block with uv mode 13"
    return is_cfl, au[is_cfl], av_[is_cfl]


def assert_paths(kind: str, mode) -> None:
    """The coding paths the case exists for, read off the golden mode words."""
    is_cfl, au, av_ = cfl_blocks(mode)
    intra = (np.asarray(mode) & 1) == 0
    if kind == "flat":
        assert not is_cfl.any(), "CfL chosen on flat luma (den = 0)"
        return
    assert is_cfl.any(), f"{kind}: no CfL block"
    assert not ((au == 0) & (av_ == 0)).any(), "a CfL block with both alphas zero"
    if kind == "corr":
        assert (au > 0).any() and (av_ < 0).any(), "no positive / negative alpha"
        assert (intra & ~is_cfl).any(), "CfL never loses"
    elif kind == "steep":
        assert (au == 16).any() and (av_ == -16).any(), "no clamped alpha"
    elif kind == "one_plane":
        assert ((au != 0) & (av_ == 0)).any(), "no block with exactly one alpha zero"
