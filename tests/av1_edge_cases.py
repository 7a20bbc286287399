"""Shared inputs of the AV1 edge-case suites (not a test module): deterministic content
generators at the sample-range extremes, and the engine-vs-golden comparison used by
tests/test_av1_codec.py and tests/test_gpu_av1_engine_edges.py."""
import numpy as np

from thinvids_amd.models import av1, hevc

KINDS = ("noise", "binary", "checker1", "checker8", "flatswing", "bright", "dark", "ramp", "edges", "synth")


def luma(kind: str, t: int, w: int, h: int, rng: np.random.Generator) -> np.ndarray:
    """One (h, w) uint8 plane of content `kind` at frame t."""
    y, x = np.mgrid[0:h, 0:w]
    u = lambda a: rng.integers(-a, a + 1, (h, w))  # noqa: E731  U[-a, a]
    if kind == "noise":
        p = rng.integers(0, 256, (h, w))
    elif kind == "binary":
        p = rng.integers(0, 2, (h, w)) * 255
    elif kind == "checker1":
        p = ((x + y + t) & 1) * 255
    elif kind == "checker8":
        p = ((((x - 5 * t) >> 3) + ((y - 3 * t) >> 3)) & 1) * 255
    elif kind == "flatswing":
        p = np.full((h, w), 255 * (t & 1))
    elif kind == "bright":
        p = 246 + u(12)
    elif kind == "dark":
        p = 6 + u(12)
    elif kind == "ramp":
        p = (x + y + 3 * t) * 255 // (w + h) + u(5)
    elif kind == "edges":
        p = (((x - 2 * t) >> 4) & 1) * 255 + u(6)
    elif kind == "synth":
        p = hevc.synth_frame(7, t, w, h)[0]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.clip(p, 0, 255).astype(np.uint8))


def frame(kind: str, t: int, w: int, h: int, rng: np.random.Generator):
    """Display-size I420 (Y, U, V) of content `kind`.  Chroma is the luma decimated by two,
    except noise (independent noise per plane), flatswing (the opposite flat level) and the
    synthetic generator's own chroma."""
    if kind == "synth":
        return tuple(np.ascontiguousarray(p) for p in hevc.synth_frame(7, t, w, h))
    yp = luma(kind, t, w, h, rng)
    if kind == "noise":
        return yp, luma(kind, t, w // 2, h // 2, rng), luma(kind, t, w // 2, h // 2, rng)
    if kind == "flatswing":
        c = np.full((h // 2, w // 2), 255 - int(yp[0, 0]), np.uint8)
        return yp, c, c.copy()
    c = np.ascontiguousarray(yp[::2, ::2][:h // 2, :w // 2])
    return yp, c, c.copy()


def segment(kind: str, w: int, h: int, n: int, seed: int, t0: int = 0) -> list:
    rng = np.random.default_rng(seed)
    return [frame(kind, t0 + t, w, h, rng) for t in range(n)]


def synth_segments(seed, w, h, nframes, starts, static=False):
    segs = [[tuple(hevc.synth_frame(seed, t0 + t, w, h)) for t in range(nframes)] for t0 in starts]
    if static:  # the first frame repeated: skip-block merging to 32x32 / 64x64
        segs = [[s[0]] * nframes for s in segs]
    return segs


def gpu_vs_golden_segments(w, h, segs, q):
    """Encode the segments (lists of display-size frames, equal lengths) as one batch on the
    GPU engine and with the golden encoder, default cascade on both sides: mode words, MVs,
    CDEF tables and indices, restoration units, bitstream bytes and the last reconstruction
    must be equal.  Returns (GopHost, engine, [GoldenResult])."""
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine

    W, H = av1.coded_size(w, h)
    nframes = len(segs[0])
    eng = Av1GpuEngine(w, h, batch=len(segs), qindex=q)
    dev = eng.dev

    def load(t, planes):
        for b, fr in enumerate(segs):
            for dst, x in zip(planes, av1.pad_frame(fr[t], W, H)):
                dst[b].copy_(torch.from_numpy(np.ascontiguousarray(x)).to(dev))

    g = eng.encode_gop(nframes, load)
    futs = eng.submit_entropy(g)
    golds = []
    try:
        for b, fr in enumerate(segs):
            gold = av1.golden_encode(fr, w, h, q)
            golds.append(gold)
            np.testing.assert_array_equal(g.mode[:, b], gold.mode, err_msg=f"segment {b}: mode words")
            np.testing.assert_array_equal(g.mv[:, b], gold.mv, err_msg=f"segment {b}: motion vectors")
            np.testing.assert_array_equal(g.tabs[:, b, :8], gold.fparams[:, 9:17])
            np.testing.assert_array_equal(g.tabs[:, b, 8:], gold.fparams[:, 17:25])
            np.testing.assert_array_equal(g.fbidx[:, b], gold.cdef_idx)
            np.testing.assert_array_equal(g.lr[:, b], gold.lr, err_msg=f"segment {b}: restoration units")
            tus = futs[b].result()
            assert b"".join(tus) == gold.stream, f"segment {b}: GPU bitstream differs from the golden encoder"
            last = gold.recon[-1]
            fin = np.concatenate([x[b].cpu().numpy().reshape(-1) for x in eng.fin])
            np.testing.assert_array_equal(fin, last, err_msg=f"segment {b}: last reconstruction")
    finally:
        eng.close()
    return g, eng, golds


def gpu_vs_golden(w, h, starts, nframes, q, static=False, seed=11):
    g, eng, _ = gpu_vs_golden_segments(w, h, synth_segments(seed, w, h, nframes, starts, static), q)
    return g, eng
