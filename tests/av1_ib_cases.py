"""Shared inputs of the AV1 intra-in-inter suites (not a test module): cut clips whose last
two frames have nothing to do with the first two, a pan clip without a cut, and the
brute-force acceptance model."""
import numpy as np

from thinvids_amd.models import av1, hevc

SEEDS, STARTS = (7, 23), (0, 40)
# (w, h, q-index, content): "noisy" adds U[-24, 24] to every sample (q 1 codes the noise),
# "binary" thresholds every sample to 0 / 255 (q 255 leaves intra blocks without a level)
CUT_CASES = [(16, 16, 100, "synth"), (72, 40, 100, "synth"), (200, 136, 100, "synth"), (200, 120, 1, "noisy"),
             (200, 120, 255, "binary")]
CUT_IDS = [f"{w}x{h}-q{q}-{kind}" for w, h, q, kind in CUT_CASES]


def cut_clip(w: int, h: int, kind: str = "synth", n: int = 4, cut: int = 2) -> list:
    """Frames [0, cut) from one synthetic seed, frames [cut, n) from an unrelated seed and start."""
    fr = [tuple(hevc.synth_frame(SEEDS[t >= cut], STARTS[t >= cut] + t, w, h)) for t in range(n)]
    if kind == "noisy":
        rng = np.random.default_rng(1)
        fr = [tuple(np.clip(p.astype(np.int32) + rng.integers(-24, 25, p.shape), 0, 255).astype(np.uint8) for p in f)
              for f in fr]
    elif kind == "binary":
        fr = [tuple(((p > 128) * 255).astype(np.uint8) for p in f) for f in fr]
    elif kind != "synth":
        raise ValueError(kind)
    return [tuple(np.ascontiguousarray(p) for p in f) for f in fr]


def pan_clip(w: int, h: int, n: int = 4, seed: int = 7) -> list:
    """Consecutive frames of one synthetic seed (its content pans): no cut."""
    return [tuple(hevc.synth_frame(seed, t, w, h)) for t in range(n)]


def static_clip(w: int, h: int, n: int = 4, seed: int = 5) -> list:
    f0 = tuple(hevc.synth_frame(seed, 0, w, h))
    return [f0] * n


def psnr(res, frames, w: int, h: int) -> float:
    W, H = av1.coded_size(w, h)
    src = av1.pack_i420([av1.pad_frame(f, W, H) for f in frames], W, H)
    return float(10 * np.log10(255.0 ** 2 / np.mean((res.recon.astype(np.float64) - src) ** 2)))


def accept_bruteforce(cand: np.ndarray) -> np.ndarray:
    """The acceptance rule as the recursion it is stated as, with no depth limit: a candidate
    is accepted unless its left, above or above-left neighbour lies in another 64x64
    superblock (4x4 blocks) and is itself accepted."""
    bh, bw = cand.shape
    memo = {}

    def acc(x, y):
        if (x, y) not in memo:
            r = bool(cand[y, x] & 1)
            if r:
                for nx, ny in ((x - 1, y), (x, y - 1), (x - 1, y - 1)):
                    if nx < 0 or ny < 0 or (nx >> 2, ny >> 2) == (x >> 2, y >> 2):
                        continue
                    if acc(nx, ny):
                        r = False
                        break
            memo[(x, y)] = r
        return memo[(x, y)]

    return np.array([[acc(x, y) for x in range(bw)] for y in range(bh)], np.uint8)


def same_sb_dependencies(ib: np.ndarray) -> int:
    """Accepted blocks with an accepted left or above neighbour (necessarily in their superblock)."""
    a = (ib >> 1) & 1
    return int((a[:, 1:] & a[:, :-1]).sum() + (a[1:] & a[:-1]).sum())
