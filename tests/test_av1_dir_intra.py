"""AV1 directional intra (kToolDirIntra, off by default; csrc/include/tv/av1_enc.h "directional
intra"): the derivative table against the bundled decoder libraries' copies, the generated rate
tables against their big-integer definition, the predictor and the 34-candidate decision against
independent Python transcriptions, streams through the oracle decoder and through dav1d (the
arbiter), the tool off leaving every byte as it was, and the plumbing down from a job."""
import re
from pathlib import Path

import numpy as np
import pytest
from av1_dir_cases import ANGLES, PATHS_SIZE, assert_paths, dir_blocks, fan_clip, golden

from thinvids_amd.models import av1, avif, hevc

ROOT = Path(__file__).resolve().parents[1]
needs_dav1d = pytest.mark.skipif(not avif.dav1d_available(), reason="libavif / dav1d (Pillow AVIF plugin) missing")

DC, V, H, D135, D113, D157, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH = 0, 1, 2, 4, 5, 6, 9, 10, 11, 12
BASE = {V: 90, H: 180, D135: 135, D113: 113, D157: 157}
# the issue's search order, written out
ORDER = ([(m, 0) for m in (DC, V, H, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH)] + [(V, d) for d in (1, 2, 3)] +
         [(H, d) for d in (-1, -2, -3)] + [(m, d) for m in (D135, D113, D157) for d in (0, -1, 1, -2, 2, -3, 3)])
PAIRS = [p for p in ORDER[7:] if p[1] or p[0] in (D135, D113, D157)]  # the 27 angled (mode, delta) pairs
# the issue's Dr_Intra_Derivative table
DR = dict(zip((3, 6, 9, 14, 17, 20, 23, 26, 29, 32, 36, 39, 42, 45, 48, 51, 54, 58, 61, 64, 67, 70, 73, 76, 81, 84, 87),
              (1023, 547, 372, 273, 215, 178, 151, 132, 116, 102, 90, 80, 71, 64, 57, 51, 45, 40, 35, 31, 27, 23, 19, 15,
               11, 7, 3)))
INTRA_MODE_CTX = [0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0]


def lam_of(q: int) -> int:
    return max(16, (av1.ac_q(q) * 16 * 3) // 32)


# ---- tables ---------------------------------------------------------------------------------------
def test_search_order_and_pairs():
    assert av1.dir_cands() == ORDER and len(ORDER) == av1.NUM_DIR_CAND == 34 and len(PAIRS) == 27
    assert sorted({BASE[m] + 3 * d for m, d in PAIRS} | {90, 180}) == sorted(ANGLES)
    assert all(90 < BASE[m] + 3 * d < 180 for m, d in PAIRS)


def test_derivative_table_is_the_issues():
    d = av1.dir_tables()["deriv"]
    assert {a: int(v) for a, v in enumerate(d) if v} == DR


@needs_dav1d
def test_derivative_table_equals_both_libraries_copies():
    """The model's table in dav1d's layout (uint16 [44], indexed by angle >> 1) and in libaom's
    (int16 [90], indexed by angle) inside the bundled libavif."""
    import glob
    import os

    import PIL

    libs = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libavif*.so*")))
    if not libs:
        pytest.skip("bundled libavif not found")
    blob = Path(libs[0]).read_bytes()
    d = av1.dir_tables()["deriv"]
    d44 = np.zeros(44, "<u2")
    for a in range(88):
        if d[a]:
            assert d44[a >> 1] == 0
            d44[a >> 1] = d[a]
    assert d44.tobytes() in blob, "derivative table differs from dav1d's copy"
    aom = np.zeros(90, "<i2")
    aom[:88] = d
    assert aom.tobytes() in blob, "derivative table differs from libaom's copy"


def _header_cdf(name: str, nsym: int) -> list:
    text = (ROOT / "csrc/include/tv/av1_tables.h").read_text()
    m = re.search(r"constexpr uint16_t " + name + r"(?:\[\d+\])+ = \{([^}]*)\}", text)
    v = [int(x) for x in m.group(1).split(",") if x.strip()]
    return [v[k:k + nsym - 1] for k in range(0, len(v), nsym - 1)]


def _bits16(p: int) -> int:
    """The n with 2^(2n - 1) <= (32768 / p)^32 < 2^(2n + 1), in Python integers."""
    assert 0 < p <= 32768
    big, pp = 2 ** 481, p ** 32  # both sides doubled: 2^(2n) p^32 <= 2^481 < 2^(2n + 2) p^32
    n = 0
    while not (2 ** (2 * n) * pp <= big < 2 ** (2 * n + 2) * pp):
        n += 1
    return n


def _rates(rows, nsym) -> np.ndarray:
    out = []
    for r in rows:
        c = [0] + r + [32768]
        out.append([_bits16(c[k + 1] - c[k]) for k in range(nsym)])
    return np.array(out)


def _py_tables() -> dict:
    return {"kf_y": _rates(_header_cdf("kKfYMode", 13), 13).reshape(5, 5, 13),
            "y_mode": _rates(_header_cdf("kYMode", 13), 13)[2],
            "uv": _rates(_header_cdf("kUvMode1", 14), 14), "angle": _rates(_header_cdf("kAngleDelta", 7), 7)}


def test_rate_tables_equal_the_big_integer_definition():
    assert [_bits16(p) for p in (32768, 16384, 23170, 23171, 1)] == [0, 16, 8, 8, 240]
    got, want = av1.dir_tables(), _py_tables()
    for k, w in want.items():
        assert got[k].shape == w.shape
        np.testing.assert_array_equal(got[k], w, err_msg=k)
    # the committed header constants are those numbers too
    text = (ROOT / "csrc/include/tv/av1_tables.h").read_text()
    for name, k in (("kKfYModeBits16", "kf_y"), ("kYModeBits16", "y_mode"), ("kUvMode1Bits16", "uv"),
                    ("kAngleDeltaBits16", "angle")):
        m = re.search(r"constexpr uint8_t " + name + r"(?:\[\d+\])+ = \{([^}]*)\}", text)
        assert [int(x) for x in m.group(1).split(",") if x.strip()] == want[k].reshape(-1).tolist(), name


# ---- predictor ------------------------------------------------------------------------------------
SM = {8: [255, 197, 146, 105, 73, 50, 37, 32],
      16: [255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16]}


def _edges(rng, n: int, have_a: bool, have_l: bool, sat: bool = False):
    """(above, left, tl) as the specification's edge preparation leaves them for a block whose
    above row / left column / corner hold random samples (0 / 255 only with `sat`)."""
    draw = (lambda k: rng.integers(0, 2, k) * 255) if sat else (lambda k: rng.integers(0, 256, k))
    a, le, tl = [int(v) for v in draw(n)], [int(v) for v in draw(n)], int(draw(1)[0])
    if have_a and have_l:
        return a, le, tl
    if have_a:
        return a, [a[0]] * n, a[0]
    if have_l:
        return [le[0]] * n, le, le[0]
    return [127] * n, [129] * n, 128


def _dir_px(a, le, tl, i, j, dx, dy, idx_seen=None):
    """7.11.2.4 for 90 < pAngle < 180 without edge filter / upsampling; AboveRow[-1] = LeftCol[-1]
    = the corner."""
    A, L = (lambda k: tl if k == -1 else a[k]), (lambda k: tl if k == -1 else le[k])
    idx = (j << 6) - (i + 1) * dx
    base = idx >> 6
    if base >= -1:
        shift = (idx >> 1) & 0x1F
        if idx_seen is not None:
            idx_seen.append(("a", base))
        return (A(base) * (32 - shift) + A(base + 1) * shift + 16) >> 5
    idx = (i << 6) - (j + 1) * dy
    base = idx >> 6
    shift = (idx >> 1) & 0x1F
    if idx_seen is not None:
        idx_seen.append(("l", base))
    return (L(base) * (32 - shift) + L(base + 1) * shift + 16) >> 5


def _dc(a, le, n, have_a, have_l):
    lg = 3 if n == 8 else 4
    if have_a and have_l:
        return (sum(a) + sum(le) + n) >> (lg + 1)
    if have_a:
        return (sum(a) + (n >> 1)) >> lg
    if have_l:
        return (sum(le) + (n >> 1)) >> lg
    return 128


def _pred(mode, delta, a, le, tl, n, have_a=True, have_l=True) -> np.ndarray:
    out = np.zeros((n, n), np.int64)
    w = SM[n]
    ang = BASE.get(mode, 0) + 3 * delta
    for i in range(n):
        for j in range(n):
            if mode in BASE and ang not in (90, 180):
                p = _dir_px(a, le, tl, i, j, DR[180 - ang], DR[ang - 90])
            elif mode == V:
                p = a[j]
            elif mode == H:
                p = le[i]
            elif mode == SMOOTH:
                p = (w[i] * a[j] + (256 - w[i]) * le[n - 1] + w[j] * le[i] + (256 - w[j]) * a[n - 1] + 256) >> 9
            elif mode == SMOOTH_V:
                p = (w[i] * a[j] + (256 - w[i]) * le[n - 1] + 128) >> 8
            elif mode == SMOOTH_H:
                p = (w[j] * le[i] + (256 - w[j]) * a[n - 1] + 128) >> 8
            elif mode == PAETH:
                b = a[j] + le[i] - tl
                pl, pa, pt = abs(b - le[i]), abs(b - a[j]), abs(b - tl)
                p = le[i] if pl <= pa and pl <= pt else (a[j] if pa <= pt else tl)
            else:
                p = _dc(a, le, n, have_a, have_l)
            out[i, j] = p
    return out


@pytest.mark.parametrize("n", [8, 16])
def test_predictor_matches_the_transcription(n):
    rng = np.random.default_rng(n)
    for have_a in (True, False):
        for have_l in (True, False):
            for sat in (False, True):
                a, le, tl = _edges(rng, n, have_a, have_l, sat)
                for mode, delta in ORDER:
                    got = av1.dir_predict(n, a, le, tl, mode, delta, have_a, have_l)
                    np.testing.assert_array_equal(got, _pred(mode, delta, a, le, tl, n, have_a, have_l),
                                                  err_msg=f"mode {mode} delta {delta} N {n} above {have_a} left {have_l}")
    for mode, delta in ((V, -1), (H, 1), (3, 0), (7, 0), (8, 0), (DC, 1)):
        with pytest.raises(RuntimeError, match="subset"):
            av1.dir_predict(n, [1] * n, [1] * n, 1, mode, delta)


@pytest.mark.parametrize("n", [8, 16])
def test_every_read_stays_inside_the_edges(n):
    """All 27 angles, every (i, j): base >= -1 and base + 1 <= N - 1 in whichever edge is read,
    so nothing right of above[N-1] or below left[N-1] (the wavefront's condition)."""
    a = le = list(range(n))
    for mode, delta in PAIRS:
        ang = BASE[mode] + 3 * delta
        seen = []
        for i in range(n):
            for j in range(n):
                _dir_px(a, le, 0, i, j, DR[180 - ang], DR[ang - 90], seen)
        assert len(seen) == n * n
        assert all(-1 <= base <= n - 2 for _, base in seen), (mode, delta, n)


# ---- decision -------------------------------------------------------------------------------------
_H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)


def _satd(a, b, n) -> int:
    d = np.asarray(a, np.int64).reshape(n, n) - np.asarray(b, np.int64).reshape(n, n)
    s = 0
    for y in range(0, n, 4):
        for x in range(0, n, 4):
            s += (int(np.abs(_H4 @ d[y:y + 4, x:x + 4] @ _H4.T).sum()) + 1) >> 1
    return s


def _decide(T, srcs, edges, n, lam, kf, above, left, ym):
    costs = []
    for mode, delta in ORDER:
        c = sum(_satd(s, _pred(mode, delta, *e, n), n) for s, e in zip(srcs, edges))
        if n == 16:
            bits = int(T["kf_y"][INTRA_MODE_CTX[above]][INTRA_MODE_CTX[left]][mode]) if kf else int(T["y_mode"][mode])
        else:
            bits = int(T["uv"][ym][mode])
        if 1 <= mode <= 8:
            bits += int(T["angle"][mode - 1][delta + 3])
        costs.append(c + ((lam * bits) >> 8))
    win = min(range(34), key=lambda k: (costs[k], k))  # the first strict minimum
    return costs, win


def _oriented_block(rng, n):
    t = np.deg2rad(float(rng.choice(ANGLES)) - 90)
    i, j = np.mgrid[-1:n, -1:n]
    u = j * np.cos(t) - i * np.sin(t) + rng.uniform(0, 8)
    img = np.clip(128 + 90 * np.sign(np.sin(2 * np.pi * u / float(rng.uniform(6, 20)))) + rng.integers(-3, 4, u.shape), 0, 255)
    img = img.astype(np.uint8)
    return img[1:, 1:], (img[0, 1:].tolist(), img[1:, 0].tolist(), int(img[0, 0]))


def test_decision_matches_the_python_model():
    T = _py_tables()
    rng = np.random.default_rng(34)
    winners = set()
    modes13 = [0, 1, 2, 4, 5, 6, 9, 10, 11, 12]
    ctx_modes = [0, 1, 2, 3, 4]  # one neighbour y mode per context (3: D45, which only a neighbour could have)
    assert [INTRA_MODE_CTX[m] for m in ctx_modes] == [0, 1, 2, 3, 4]
    ctxs = [(ctx_modes[a], ctx_modes[b]) for a in range(5) for b in range(5)]
    for k in range(25):
        src, e = _oriented_block(rng, 16)
        above, left = ctxs[k]  # all 25 key-frame contexts
        for q in (1, 100, 255):
            lam = lam_of(q)
            got = av1.dir_decide(src, e, lam, kf=True, above=above, left=left)
            assert got == _decide(T, [src], [e], 16, lam, True, above, left, 0), (k, q)
            winners.add(ORDER[got[1]])
        got = av1.dir_decide(src, e, lam_of(100), kf=False)  # the inter-frame table
        assert got == _decide(T, [src], [e], 16, lam_of(100), False, 0, 0, 0), k
        su, eu = _oriented_block(rng, 8)
        sv, ev = _oriented_block(rng, 8)
        ym = modes13[k % len(modes13)]
        got = av1.dir_decide((su, sv), (eu, ev), lam_of(100), ym=ym)
        assert got == _decide(T, [su, sv], [eu, ev], 8, lam_of(100), False, 0, 0, ym), k
    assert len({m for m, _ in winners}) >= 4 and any(d for _, d in winners), winners
    # constructed ties: a flat block between flat edges has SATD 0 under every candidate but DC_PRED
    # (no neighbour is "available", so its value is 128), and at lam 16 the rate term is bits >> 4,
    # which candidates share: in every context where the minimum is shared the earliest must win
    flat, fe = np.full((16, 16), 100, np.uint8), ([100] * 16, [100] * 16, 100)
    ties = 0
    for above, left in ctxs:
        costs, win = av1.dir_decide(flat, fe, 16, kf=True, above=above, left=left, have_above=False, have_left=False)
        sats = [_satd(flat, _pred(m, d, *fe, 16, False, False), 16) for m, d in ORDER]
        assert sats[0] > 0 and not any(sats[1:])
        bits = [int(T["kf_y"][above][left][m]) + (int(T["angle"][m - 1][d + 3]) if 1 <= m <= 8 else 0) for m, d in ORDER]
        assert costs == [s_ + ((16 * b) >> 8) for s_, b in zip(sats, bits)]
        assert win == costs.index(min(costs))
        ties += costs.count(min(costs)) > 1
    assert ties, "no context with a shared minimum: the tie rule is not exercised"


# ---- round trips through the oracle decoder -------------------------------------------------------
PW, PH = PATHS_SIZE
ROUND_TRIPS = [("fan", 16, 16, 1, {}), ("fan", 32, 16, 1, {}), ("fan", 16, 32, 1, {}), ("fan", 72, 40, 1, {}),
               ("fan", PW, PH, 4, {}), ("cut", PW, PH, 4, {"intra_in_inter": True}), ("fan", PW, PH, 2, {"cfl": True})]


def _cut_has_directional_intra(res) -> bool:
    acc = ((res.ib[2] >> 1) & 1).astype(bool)
    dy, yd, _, _ = av1.mode_angles(res.mode[2])
    return bool(acc.any() and (dy & acc).any() and ((yd != 0) & acc).any())


@pytest.mark.parametrize("kind,w,h,n,tools", ROUND_TRIPS,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}{'-' + '-'.join(c[4]) if c[4] else ''}" for c in ROUND_TRIPS])
def test_oracle_decodes_directional_streams(kind, w, h, n, tools):
    _, res = golden(kind, w, h, n, 100, **tools)
    dir_blocks(res.mode)
    if (w, h) == PATHS_SIZE and kind == "fan":
        assert_paths("fan", res.mode[0])
    if kind == "cut":
        assert _cut_has_directional_intra(res), "the cut frame has no directional intra block with a delta"
    if tools.get("cfl"):
        assert av1.mode_cfl(res.mode)[0].any() and (av1.mode_angles(res.mode)[3] != 0).any()
    d = av1.decode(res.stream)
    assert len(d.frames) == n
    np.testing.assert_array_equal(np.asarray(d.frames).reshape(n, -1), res.recon.reshape(n, -1))


def test_ramp_keeps_the_non_directional_modes():
    _, res = golden("ramp", PW, PH, 1, 100)
    assert_paths("ramp", res.mode)
    ym = dir_blocks(res.mode)[0]
    assert np.isin(ym, (0, 9, 10, 11, 12)).mean() > 0.9


def test_writer_refuses_angles_outside_the_subset():
    w, h = 72, 40
    _, res = golden("fan", w, h, 1, 100)
    mode = res.mode[0].copy()

    def write(m):
        return av1.StreamWriter(w, h).write(res.fparams[0], m, res.mv[0], res.ly[0], res.lu[0], res.lv[0],
                                            res.cdef_idx[0], 0, True, lr=res.lr[0])

    assert write(mode) == res.stream
    keep = np.uint32(~((15 << 1) | (7 << 27)) & 0xFFFFFFFF)
    for ym, delta in ((V, -1), (H, 1), (DC, 2)):
        bad = mode.copy()
        bad[0] = (bad[0] & keep) | np.uint32((ym << 1) | ((delta & 7) << 27))
        with pytest.raises(RuntimeError, match="angle delta"):
            write(bad)
    keep_uv = np.uint32(~((15 << 5) | (4095 << 15)) & 0xFFFFFFFF)
    for uvm, delta in ((V, -2), (H, 3)):
        bad = mode.copy()
        bad[0] = (bad[0] & keep_uv) | np.uint32((uvm << 5) | ((delta & 7) << 15))
        with pytest.raises(RuntimeError, match="angle delta"):
            write(bad)


# ---- dav1d ----------------------------------------------------------------------------------------
DAV1D = [("fan", PW, PH, 4, 100, {}), ("fan", 72, 40, 1, 1, {}), ("fan", 72, 40, 1, 255, {}),
         ("saturated", 72, 40, 2, 100, {}), ("cut", PW, PH, 4, 100, {"intra_in_inter": True}),
         ("fan", PW, PH, 2, 100, {"cfl": True})]


@needs_dav1d
@pytest.mark.parametrize("kind,w,h,n,q,tools", DAV1D,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-q{c[4]}{'-' + '-'.join(c[5]) if c[5] else ''}" for c in DAV1D])
def test_dav1d_decodes_directional_streams_exactly(kind, w, h, n, q, tools):
    from test_av1_conformance import _check

    _, res = golden(kind, w, h, n, q, **tools)
    _, yd, _, uvd = av1.mode_angles(res.mode)
    assert (yd != 0).any() and (uvd != 0).any(), "no angle delta in the stream"
    if kind == "cut":
        assert _cut_has_directional_intra(res)
    _check(res.stream, res.tu_sizes, res.recon, w, h)


# ---- tool off -------------------------------------------------------------------------------------
def test_tool_off_changes_nothing():
    w, h, q = PW, PH, 100
    fr = fan_clip(w, h, 3)
    a, b = av1.golden_encode(fr, w, h, q), av1.golden_encode(fr, w, h, q, dir_intra=False)
    assert a.stream == b.stream and a.tu_sizes == b.tu_sizes
    np.testing.assert_array_equal(a.mode, b.mode)
    np.testing.assert_array_equal(a.recon, b.recon)
    assert not (a.mode >> 15).any(), "angle bits set with the tool off"
    assert np.isin((a.mode[0] >> 1) & 15, (0, 1, 2, 9, 10, 11, 12)).all()
    on = av1.golden_encode(fr, w, h, q, dir_intra=True)
    assert on.stream != a.stream


def test_tool_saves_bytes_on_oriented_content():
    """Not a tuned figure: on gratings along the tool's own angles it must not cost bytes."""
    w, h, q = PW, PH, 100
    fr, on = golden("fan", w, h, 4, q)
    off = av1.golden_encode(fr, w, h, q)
    assert len(on.stream) < len(off.stream)


# ---- plumbing -------------------------------------------------------------------------------------
def test_plumbing_from_job_to_stream():
    from thinvids_amd.models.cpu_engines import CpuAv1Engine
    from thinvids_amd.parallel.node_job import Checkpoint
    from thinvids_amd.worker.encoder import EncodeSpec, encode_parts
    from thinvids_amd.worker.tasks import encode_spec_for_job

    assert av1.TOOL_DIR_INTRA == 4 and av1.TOOL_INTRA_IN_INTER | av1.TOOL_CFL | av1.TOOL_DIR_INTRA == 7
    w, h = 72, 40
    job = {"source_width": w, "source_height": h, "codec": "av1", "software_encode": 1}
    st = {"tv_gop": "4", "tv_scenecut": "0"}
    off, on = encode_spec_for_job(job, st), encode_spec_for_job(dict(job, av1_dir_intra=1), st)
    assert off.dir_intra is False and on.dir_intra is True
    assert encode_spec_for_job(job, dict(st, tv_av1_dir_intra="1")).dir_intra is True
    assert (on.width, on.height) == (w, h)
    assert off.engine_key() != on.engine_key()
    assert on.tools() == dict(off.tools(), dir_intra=True)
    assert off.tools() == EncodeSpec(1, 1).tools(), "the default fingerprint moved"
    assert Checkpoint.fingerprint(tools=on.tools()) != Checkpoint.fingerprint(tools=off.tools())
    hevc_job = encode_spec_for_job({"source_width": w, "source_height": h, "av1_dir_intra": 1}, st)
    assert "dir_intra" not in hevc_job.tools(), "an AV1 tool reached the HEVC encoders"
    # the job's software path: the golden encoder with the tool
    fr = fan_clip(w, h, 2)
    gold = av1.golden_encode(fr, w, h, on.av1_qindex(), cascade=on.cascade, dir_intra=True)
    assert (av1.mode_angles(gold.mode)[1] != 0).any()
    assert encode_parts([fr], on) == [gold.stream]
    assert encode_parts([fr], off) != [gold.stream]
    # the CPU rehearsal engine (synthetic source)
    streams = {}
    for tool in (False, True):
        eng = CpuAv1Engine(w, h, batch=1, qindex=100, dir_intra=tool)
        g = eng.encode_gop(2, [0])
        streams[tool] = b"".join(eng.submit_entropy(g)[0].result())
        eng.close()
    syn = [hevc.synth_frame(1, t, w, h) for t in range(2)]
    want = av1.golden_encode(syn, w, h, 100, dir_intra=True)
    assert streams[True] == want.stream
    assert streams[False] == av1.golden_encode(syn, w, h, 100).stream != streams[True]
