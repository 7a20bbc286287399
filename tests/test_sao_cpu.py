"""The golden SAO model on the inputs of tests/test_gpu_sao.py (no GPU): the precondition of
the GPU cases.  On exactly those pictures the golden model alone must choose every luma EO
class, chroma EO, "off", offsets of +7 and -7, clip filtered samples at 0 and at 255, switch
SAO on in a CTB on each picture border and in an interior CTB, and choose different classes
in neighbouring CTBs of one four-CTB strip -- so a kernel that equals the model there has been
through every one of those paths.  tv_sao_picture_cpu is checked against a numpy filter."""
import numpy as np

from sao_cases import CASES, QPS, golden, pictures, sao_class, sao_offsets, sao_type

DIRS = {0: (-1, 0), 1: (0, -1), 2: (-1, -1), 3: (1, -1)}  # (dx, dy) of neighbour a; b is the mirror


def _unclipped(deb, params, n):
    """deb + the EO offset of every sample's category (before clipping) of one plane; params
    [CTB rows, CTB columns] of that component, CTB side n."""
    h, w = deb.shape
    d = deb.astype(np.int64)
    pad = np.full((h + 2, w + 2), -1, np.int64)  # -1: outside the picture
    pad[1:-1, 1:-1] = d
    out = d.copy()
    for cy in range(params.shape[0]):
        for cx in range(params.shape[1]):
            p = int(params[cy, cx])
            if sao_type(p) != 2:
                assert sao_type(p) == 0, "band offsets are never chosen"
                continue
            dx, dy = DIRS[sao_class(p)]
            ys, xs = slice(cy * n, (cy + 1) * n), slice(cx * n, (cx + 1) * n)
            v = d[ys, xs]
            a = pad[cy * n + 1 + dy:(cy + 1) * n + 1 + dy, cx * n + 1 + dx:(cx + 1) * n + 1 + dx]
            b = pad[cy * n + 1 - dy:(cy + 1) * n + 1 - dy, cx * n + 1 - dx:(cx + 1) * n + 1 - dx]
            e = np.sign(v - a) + np.sign(v - b)
            e[(a < 0) | (b < 0)] = 0
            off = np.array([0] + sao_offsets(p))  # by category
            cat = np.select([e == -2, e == -1, e == 1, e == 2], [1, 2, 3, 4], 0)
            out[ys, xs] = v + off[cat]
    return out


def test_model_filter_equals_numpy():
    for w, h, kind in CASES:
        _, deb = pictures(w, h, kind)
        for b, (params, out) in enumerate(golden(w, h, kind)):
            for c in range(3):
                want = np.clip(_unclipped(deb[b][c], params[:, :, c], 16 if c else 32), 0, 255)
                np.testing.assert_array_equal(out[c], want, err_msg=f"{w}x{h} {kind} picture {b} plane {c}")


def test_inputs_reach_every_path():
    luma_classes, offsets, borders = set(), set(), set()
    chroma_eo = off = clip0 = clip255 = interior = strip_neighbours_differ = 0
    for w, h, kind in CASES:
        _, deb = pictures(w, h, kind)
        for b, (params, out) in enumerate(golden(w, h, kind)):
            hc, wc = params.shape[:2]
            ty, cl = sao_type(params), sao_class(params)
            luma_classes |= set(cl[:, :, 0][ty[:, :, 0] == 2].tolist())
            both = (ty[:, :, 1] == 2) & (ty[:, :, 2] == 2)
            assert ((ty[:, :, 1] == 2) == (ty[:, :, 2] == 2)).all(), "Cb and Cr share the type"
            assert (cl[:, :, 1][both] == cl[:, :, 2][both]).all(), "Cb and Cr share the EO class"
            chroma_eo += int(both.sum())
            off += int((ty == 0).sum())
            for p in params[ty == 2].reshape(-1).tolist():
                offsets |= set(sao_offsets(p))
            on = (ty == 2).any(axis=2)
            borders |= {name for name, m in (("top", on[0]), ("bottom", on[-1]), ("left", on[:, 0]), ("right", on[:, -1]))
                        if m.any()}
            interior += int(on[1:-1, 1:-1].sum())
            for cx in range(wc - 1):
                if cx // 4 == (cx + 1) // 4:  # the two CTBs are waves of one workgroup
                    pair = (ty[:, cx, 0] == 2) & (ty[:, cx + 1, 0] == 2) & (cl[:, cx, 0] != cl[:, cx + 1, 0])
                    strip_neighbours_differ += int(pair.sum())
            for c in range(3):
                u = _unclipped(deb[b][c], params[:, :, c], 16 if c else 32)
                clip0 += int((u < 0).sum())
                clip255 += int((u > 255).sum())
    assert luma_classes == {0, 1, 2, 3}, luma_classes
    assert chroma_eo > 0 and off > 0
    assert 7 in offsets and -7 in offsets, sorted(offsets)
    assert clip0 > 0 and clip255 > 0, (clip0, clip255)
    assert borders == {"top", "bottom", "left", "right"}, borders
    assert interior > 0 and strip_neighbours_differ > 0, (interior, strip_neighbours_differ)


def test_flat_is_off_and_qp0_takes_every_gain():
    for w, h, kind in CASES:
        src, deb = pictures(w, h, kind)
        res = golden(w, h, kind)
        if kind == "flat":
            for b, (params, out) in enumerate(res):
                assert (sao_type(params) == 0).all()
                for c in range(3):
                    np.testing.assert_array_equal(out[c], deb[b][c])
        if kind == "noise":  # lambda 0: the filtered picture is never worse than the deblocked one
            assert QPS[0] == 0
            for c in range(3):
                before = ((src[0][c].astype(np.int64) - deb[0][c]) ** 2).sum()
                after = ((src[0][c].astype(np.int64) - res[0][1][c]) ** 2).sum()
                assert after < before
