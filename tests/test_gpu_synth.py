"""The generator kernel (k_synth, csrc/gpu/k_frame.hip) through stage.synth_frames against the
definition of the source (hevc.synth_frame): every byte of the display area of the three
planes, the replicated padding of the coded planes, several frame times in one launch (the
per-segment context travels as kernel arguments), more frames than one launch takes, smooth and
textured.  Sizes, seeds and times are those of tests/test_synth_tiles.py, which checks the same
arithmetic on the host."""
import numpy as np
import pytest

from thinvids_amd.models import hevc

SIZES = [(160, 96), (322, 178), (34, 18), (544, 40)]
TIMES = [0, 1, 63, 100003]
SEEDS = [1, 5, 11, 7 | 0x80000000]
MAX_BATCH = 64  # kMaxBatch (csrc/gpu/k_encode.h): frames per launch


def device_frames(seed, w, h, ts):
    """[frame][plane] coded-size planes of one stage.synth_frames call"""
    import torch

    from thinvids_amd.ops import stage

    d = stage.synth_frames(seed, w, h, ts, torch.device("cuda", 0))
    torch.cuda.synchronize()
    buf = d.buf.cpu().numpy()
    ch = hevc.coded_size(w, h)[1]
    out = []
    for f in range(len(ts)):
        planes = []
        for c, (off, _, _, stride, fs) in enumerate(d.planes):
            rows = ch if c == 0 else ch // 2
            assert fs == rows * stride
            planes.append(buf[off + f * fs:off + (f + 1) * fs].reshape(rows, stride))
        out.append(planes)
    return out


def check_frame(got, ref, what):
    for c, (g, r) in enumerate(zip(got, ref)):
        dh, dw = r.shape
        np.testing.assert_array_equal(g[:dh, :dw], r, err_msg=f"{what} plane {c} display area")
        np.testing.assert_array_equal(g[:dh, dw:], np.repeat(r[:, -1:], g.shape[1] - dw, axis=1),
                                      err_msg=f"{what} plane {c} right padding")
        np.testing.assert_array_equal(g[dh:], np.repeat(g[dh - 1:dh], g.shape[0] - dh, axis=0),
                                      err_msg=f"{what} plane {c} bottom padding")


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_kernel_equals_definition(seed, size):
    w, h = size
    got = device_frames(seed, w, h, TIMES)  # one launch, a different t per segment
    for f, t in enumerate(TIMES):
        check_frame(got[f], hevc.synth_frame(seed, t, w, h), f"seed {seed:#x} t {t}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 7 | 0x80000000], ids=hex)
def test_more_frames_than_one_launch(seed):
    w, h = 34, 18
    ts = list(range(MAX_BATCH)) + [100003]
    got = device_frames(seed, w, h, ts)
    for f, t in enumerate(ts):
        check_frame(got[f], hevc.synth_frame(seed, t, w, h), f"seed {seed:#x} frame {f} t {t}")
