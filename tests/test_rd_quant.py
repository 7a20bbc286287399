"""Rate-distortion quantisation of inter TBs (tv/rdq.h, SeqConfig::rd_quant, tool bit 1024): the
golden encoder chooses the levels of inter TBs by J = D + lambda R with a static rate model,
in three stages that need one thread per 4x4 coefficient group plus reductions.  The model
is checked against a transcription written here from the header's text (it shares only the
generated rate values, parsed from tv/rdq_tables.h), its J against the dead zone's and
RDOQ-lite's, the generator against the committed table, the streams against the decoder
oracle, and the switch through every layer.  An explicit coding tool, off by default."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from thinvids_amd.models import hevc
from thinvids_amd.worker.encoder import EncodeSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "csrc", "include", "tv", "rdq_tables.h")
TEXTURED = 0x80000000
QPS = (0, 22, 27, 37, 51)


# ---- the model, transcribed ------------------------------------------------------------------
def _tables():
    txt, out = open(TABLES).read(), {}
    for name, dims in re.findall(r"constexpr unsigned short (\w+)((?:\[\d+\])+) = ", txt):
        body = re.search(name + r"(?:\[\d+\])+ = (\{.*?\});", txt, re.S).group(1)
        out[name] = np.array([int(v) for v in re.findall(r"\d+", body)]).reshape([int(d) for d in re.findall(r"\d+", dims)])
    return out


T = _tables()
SCALE = (26214, 23302, 20560, 18396, 16384, 14564)
RATE_CAP = 511


def _diag_scan(s):
    """6.5.3 up-right diagonal scan of an s x s array: (x, y) per position."""
    out, x, y = [], 0, 0
    while len(out) < s * s:
        while y >= 0:
            if x < s and y < s:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


SCAN4 = _diag_scan(4)


def _l0_and_d(coef, qp, log2n):
    """Inter dead-zone level magnitude (rounding 1/4) and the distance of |coef| from it in
    1/256 step, rounded down."""
    qbits = 14 + qp // 6 + 7 - log2n
    a = np.abs(coef.astype(np.int64)) * SCALE[qp % 6]
    l0 = np.minimum((a + (128 << (qbits - 9))) >> qbits, 32767)
    return l0, (a - (l0 << qbits)) >> (qbits - 8)


def _rate(a, c, dc, cls):
    """Excess rate of magnitude a > 0 in 1/16 bit."""
    r = max(0, int(T["kRdqSig"][c, dc, cls, 1]) - int(T["kRdqSig"][c, dc, cls, 0])) + 16
    if a == 1:
        r += int(T["kRdqG1"][c, dc, 0])
    elif a == 2:
        r += int(T["kRdqG1"][c, dc, 1]) + int(T["kRdqG2"][c, dc, 0])
    else:
        v = a - 3
        r += int(T["kRdqG1"][c, dc, 1]) + int(T["kRdqG2"][c, dc, 1]) + 16 * (v + 1 if v < 4 else 4 + 2 * ((v - 2).bit_length() - 1))
    return min(r, RATE_CAP)


def _sig_class(right, below, x, y):
    if not right and not below:
        return 2 if x + y == 0 else (1 if x + y < 3 else 0)
    if right and below:
        return 2
    t = y if right else x
    return 2 if t == 0 else (1 if t == 1 else 0)


class Model:
    """Stages 1 to 3 on one TB, group by group in coding order, with plain Python integers."""

    def __init__(self, coef, qp, log2n, c, lam):
        self.n, self.s, self.c, self.lam = 1 << log2n, max(1, (1 << log2n) >> 2), c, lam
        self.neg = coef < 0
        self.l0, self.d = _l0_and_d(coef, qp, log2n)
        self.groups = _diag_scan(self.s)  # coding order
        nz = self.l0.reshape(self.s, 4, self.s, 4).any(axis=(1, 3))  # [gy, gx]
        self.right = {(gx, gy): gx + 1 < self.s and bool(nz[gy, gx + 1]) for gx, gy in self.groups}
        self.below = {(gx, gy): gy + 1 < self.s and bool(nz[gy + 1, gx]) for gx, gy in self.groups}

    def pos(self, g, n):
        return g[1] * 4 + SCAN4[n][1], g[0] * 4 + SCAN4[n][0]  # (row, column)

    def coef_j(self, g, n, a):
        """D + lambda Rx of coding position n of group g as magnitude a."""
        y, x = self.pos(g, n)
        e = int(self.d[y, x]) + 256 * (int(self.l0[y, x]) - a)
        cls = _sig_class(self.right[g], self.below[g], *SCAN4[n])
        return e * e + (self.lam * _rate(a, self.c, int(g == (0, 0)), cls) if a else 0)

    def cost(self, mag):
        """The model's J of the magnitudes `mag`."""
        live = [k for k, g in enumerate(self.groups) if mag[g[1] * 4:g[1] * 4 + 4, g[0] * 4:g[0] * 4 + 4].any()]
        J = 0
        for k, g in enumerate(self.groups):
            sub = mag[g[1] * 4:g[1] * 4 + 4, g[0] * 4:g[0] * 4 + 4]
            J += sum(self.coef_j(g, n, int(mag[self.pos(g, n)])) for n in range(16))
            if live and 0 < k < live[-1] and sub.any():
                cx = T["kRdqCsbf"][self.c, int(self.right[g] or self.below[g])]
                J += self.lam * max(0, int(cx[1]) - int(cx[0]))
            if live and k == live[-1]:
                J += self.lam * int(T["kRdqLast"][self.c, g[0] + g[1]])
        return J

    def run(self):
        """-> (final magnitudes, [J after stage 1, 2, 3])."""
        mag = self.l0.copy()
        info = []
        for k, g in enumerate(self.groups):
            l0 = [int(self.l0[self.pos(g, n)]) for n in range(16)]
            last0 = max([n for n in range(16) if l0[n]], default=-1)
            zero_d = []
            for n in range(16):
                y, x = self.pos(g, n)
                d, a0 = int(self.d[y, x]), l0[n]
                zero_d.append((d + 256 * min(a0, 3)) ** 2)
                other = a0 + 1 if d >= 0 else a0 - 1
                if a0 == 0:
                    continue  # a zero stays zero
                if self.coef_j(g, n, other) < self.coef_j(g, n, a0):
                    mag[y, x] = other
            a1 = [int(mag[self.pos(g, n)]) for n in range(16)]
            eligible = max(a1) <= 2
            # J minus the all-zero distortion of ending the group after position n (n non-zero)
            run, ends = 0, {}
            for n in range(16):
                run += (self.coef_j(g, n, a1[n]) if n <= last0 else zero_d[n]) - zero_d[n]
                if a1[n]:
                    ends[n] = run
            full = 0
            if ends:
                cx = T["kRdqCsbf"][self.c, int(self.right[g] or self.below[g])]
                full = run + (self.lam * max(0, int(cx[1]) - int(cx[0])) if k else 0)
            emptied = bool(k and eligible and full > 0)
            if not ends:
                nlast, glast = -1, 0
            elif eligible:
                glast = min(ends.values())
                nlast = max(n for n, v in ends.items() if v == glast)
            else:
                nlast = max(ends)
                glast = ends[nlast]
            info.append(dict(g=g, eligible=eligible, full=0 if emptied else full, emptied=emptied, nlast=nlast, glast=glast))
        J = [self.cost(mag)]
        m2 = mag.copy()
        for i in info:
            if i["emptied"]:
                m2[i["g"][1] * 4:i["g"][1] * 4 + 4, i["g"][0] * 4:i["g"][0] * 4 + 4] = 0
        J.append(self.cost(m2))
        kmin = max([k for k, i in enumerate(info) if not i["eligible"]], default=0)
        best, kend, before = None, 0, 0
        for k, i in enumerate(info):
            if (i["nlast"] >= 0 or k == 0) and k >= kmin:
                e = before if i["nlast"] < 0 else before + i["glast"] + self.lam * int(T["kRdqLast"][self.c, i["g"][0] + i["g"][1]])
                if best is None or e <= best:
                    best, kend = e, k
            before += i["full"]
        for k, i in enumerate(info):
            keep = -1 if k > kend else (i["nlast"] if k == kend else (-1 if i["emptied"] else 15))
            for n in range(keep + 1, 16):
                mag[self.pos(i["g"], n)] = 0
        J.append(self.cost(mag))
        return mag, J


def _rdoq_lite(l0, mode=2):
    """RDOQ-lite (tv code_tb): trailing groups whose only level is a lone 1 are dropped, walking
    the groups backwards to the first one that holds anything else; the DC group and, in the
    default mode, the groups before the TB's anti-diagonal stay."""
    mag, s = l0.copy(), l0.shape[0] // 4
    if s < 2:
        return mag
    dmin = 1 if mode == 1 else (max(1, s - 1) if mode == 2 else s)
    for gx, gy in reversed(_diag_scan(s)):
        if gx + gy < dmin:
            break
        t = int(mag[gy * 4:gy * 4 + 4, gx * 4:gx * 4 + 4].sum())
        if t == 0:
            continue
        if t != 1:
            break
        mag[gy * 4:gy * 4 + 4, gx * 4:gx * 4 + 4] = 0
    return mag


def _native(coef, qp, log2n, c, lam=0):
    from thinvids_amd._native import core_lib

    coef = np.ascontiguousarray(coef, np.int32)
    lev, J = np.empty(coef.shape, np.int16), (C.c_longlong * 3)()
    shipped = core_lib().tv_rdq_tb(coef.ctypes.data_as(C.POINTER(C.c_int32)), qp, log2n, c, lam,
                                   lev.ctypes.data_as(C.POINTER(C.c_int16)), J)
    return lev, list(J), shipped


def _step(qp, log2n):
    return 2.0 ** (14 + qp // 6 + 7 - log2n) / SCALE[qp % 6]


def _from_levels(x, qp, log2n):
    """Coefficients that lie at `x` quantiser steps (fractions allowed), clamped to the
    forward transform's range."""
    return np.clip(np.round(np.asarray(x, float) * _step(qp, log2n)), -64548, 64548).astype(np.int32)


def _cases(qp, log2n, rng):
    n = 1 << log2n
    out = {}
    sparse = np.where(rng.random((n, n)) < 0.08, rng.normal(0, 1.5, (n, n)), rng.normal(0, 0.3, (n, n)))
    out["sparse"] = _from_levels(sparse, qp, log2n)
    fall = 1.0 / (1 + np.add.outer(np.arange(n), np.arange(n)) / 3.0)
    out["dense"] = _from_levels(rng.normal(0, 6, (n, n)) * fall + rng.normal(0, 0.6, (n, n)), qp, log2n)
    ext = rng.choice([-64548, 64548, 0, 0], (n, n)).astype(np.int32)
    ext[0, 0] = 64548
    out["extreme"] = ext
    # a few solid low-frequency levels, then lone +-1 levels (0.77 of a step) in trailing groups
    t = np.zeros((n, n))
    t[0, 0], t[0, 1], t[1, 0] = 7.1, -3.2, 2.1
    # (isolated groups: with a coded neighbour the static contexts make a level cheap to keep)
    t[n - 1, n - 1] = 0.77
    if n >= 16:
        t[n - 9, n - 1], t[n - 1, n - 9] = -0.78, 0.77
    out["trailing"] = _from_levels(t, qp, log2n)
    # levels just under the next integer, where the dead zone rounds down and the cost up
    r = np.zeros((n, n))
    r[0, 0], r[0, 1], r[1, 0], r[1, 1], r[0, 2] = 5.74, -2.74, 3.73, 1.74, -4.72
    out["raise"] = _from_levels(r, qp, log2n)
    # an interior group of weak levels between a strong DC group and a strong last group
    e = np.zeros((n, n))
    e[0, 0], e[1, 0] = 9.0, -4.0
    if n >= 8:
        e[1, 5], e[2, 6] = 0.8, -0.79    # each cheaper as zero: stage 1 empties the group
        e[5, 1], e[6, 2] = 0.86, -0.87   # each kept, the group with its coded_sub_block_flag is not
        e[n - 4, n - 4], e[n - 3, n - 4], e[n - 4, n - 3] = 6.0, -5.0, 4.0
    out["interior"] = _from_levels(e, qp, log2n)
    return out


ALL = [(qp, log2n, c) for qp in QPS for log2n in (2, 3, 4, 5) for c in (0, 1)]


@pytest.fixture(scope="module")
def results():
    """Every case once: native levels and J, the transcription's, and the events seen."""
    rng = np.random.default_rng(7)
    out = []
    lam = _native(np.zeros((4, 4), np.int32), 27, 2, 0)[2]
    for qp, log2n, c in ALL:
        for name, coef in _cases(qp, log2n, rng).items():
            lev, J, _ = _native(coef, qp, log2n, c)
            m = Model(coef, qp, log2n, c, lam)
            mag, Jm = m.run()
            out.append(dict(qp=qp, log2n=log2n, c=c, name=name, coef=coef, lev=lev, J=J, model=m, mag=mag, Jm=Jm))
    return out


def test_model_equals_transcription(results):
    for r in results:
        tag = (r["name"], r["qp"], r["log2n"], r["c"])
        want = np.where(r["model"].neg, -r["mag"], r["mag"])
        np.testing.assert_array_equal(r["lev"], want, err_msg=str(tag))
        assert r["J"] == r["Jm"], tag


def test_j_is_no_worse_than_dead_zone_and_rdoq_lite(results):
    for r in results:
        m, tag = r["model"], (r["name"], r["qp"], r["log2n"], r["c"])
        j_out = m.cost(np.abs(r["lev"].astype(np.int64)))
        assert j_out == r["J"][2], tag
        assert j_out <= m.cost(m.l0), tag
        for mode in (1, 2, 3):
            assert j_out <= m.cost(_rdoq_lite(m.l0, mode)), (tag, mode)
        assert np.all(m.l0 - np.abs(r["lev"]) <= 3) and np.all(np.abs(r["lev"]) - m.l0 <= 1), tag


def test_the_three_events_occur(results):
    """Stage 1 raises a level, stage 2 empties an interior group, and on the trailing-group TB
    the tool ends the TB no later than RDOQ-lite does (which itself drops groups there)."""
    raised = emptied = trimmed = 0
    stage2 = sum(r["J"][1] < r["J"][0] for r in results)
    for r in results:
        m, mag = r["model"], np.abs(r["lev"].astype(np.int64))
        if r["name"] == "raise":
            raised += int((mag > m.l0).any())
        live = lambda a: [k for k, g in enumerate(m.groups) if a[g[1] * 4:g[1] * 4 + 4, g[0] * 4:g[0] * 4 + 4].any()]  # noqa: E731
        if r["name"] == "interior" and r["log2n"] >= 3:
            was, now = live(m.l0), live(mag)
            emptied += int(any(0 < k < now[-1] and k not in now for k in was))
        if r["name"] == "trailing" and r["log2n"] >= 3:
            lite = live(_rdoq_lite(m.l0))
            assert lite[-1] < live(m.l0)[-1], "RDOQ-lite drops nothing on this TB"
            assert live(mag)[-1] <= lite[-1], (r["qp"], r["log2n"], r["c"])
            trimmed += 1
    print("raised", raised, "interior groups emptied", emptied, "of them by stage 2", stage2, "trailing TBs", trimmed)
    assert raised > 0 and emptied > 0 and stage2 > 0 and trimmed == len(QPS) * 3 * 2


def test_generator_reproduces_the_table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hevc_rate_tables_gen.py"), "--stdout"],
                         check=True, capture_output=True, text=True).stdout
    assert out == open(TABLES).read()


# ---- streams ---------------------------------------------------------------------------------
def _frames(seed, n, w, h):
    return [hevc.synth_frame(seed, t, w, h) for t in range(n)]


def _assert_decodes_to(stream, recons):
    d = hevc.decode(stream)
    assert len(d.coded_frames) == len(recons)
    for a, b in zip(d.coded_frames, recons):
        for p in range(3):
            np.testing.assert_array_equal(a[p], b[p])


@pytest.mark.parametrize("sign_hiding", [False, True], ids=["alone", "sdh"])
@pytest.mark.parametrize("w,h", [(160, 96), (160, 90)])
@pytest.mark.parametrize("qp", [22, 27, 37])
@pytest.mark.parametrize("seed", [3, 3 | TEXTURED])
def test_round_trip_ippp(w, h, qp, seed, sign_hiding):
    """With sign hiding on, the host writer's parity check runs on every group it codes."""
    fr = _frames(seed, 4, w, h)
    for sao, wpp in ((False, True), (True, False)):
        on, rec = hevc.encode_sequence_cpu(fr, qp=qp, search_range=32, sao=sao, wpp=wpp, rqt=True, pintra=True,
                                           rd_quant=True, sign_hiding=sign_hiding)
        _assert_decodes_to(on, rec)


@pytest.mark.parametrize("sign_hiding", [False, True], ids=["alone", "sdh"])
@pytest.mark.parametrize("w,h", [(160, 96), (160, 90)])
@pytest.mark.parametrize("qp", [22, 27, 37])
@pytest.mark.parametrize("seed", [3, 3 | TEXTURED])
def test_round_trip_bframes(w, h, qp, seed, sign_hiding):
    fr = _frames(seed, 5, w, h)
    for sao, wpp in ((True, True), (False, False)):
        on, rec = hevc.encode_sequence_cpu(fr, qp=qp, search_range=32, sao=sao, wpp=wpp, bframes=2, gop=5,
                                           rd_quant=True, sign_hiding=sign_hiding)
        _assert_decodes_to(on, rec)


def test_the_tool_acts_on_every_tb_size():
    """First P picture of the textured clip (its reference, the IDR, is the same either way):
    the tool changes levels in inter TBs of every size.  Without the residual quadtree a TB is
    its CU, so the decisions give every TB's size."""
    w, h = 160, 96
    fr = _frames(7 | TEXTURED, 2, w, h)
    got = []
    for on in (False, True):
        enc = hevc.CpuEncoder(w, h, qp=22, search_range=32, rqt=False, rd_quant=on)
        for t, f in enumerate(fr):
            enc.encode(f, t == 0, t)
        got.append((enc.decisions(), enc.levels()))
    (dec, off), (dec_on, on) = got
    for k in ("cu_log2", "intra", "mv"):
        np.testing.assert_array_equal(dec[k], dec_on[k])
    changed = {}
    for uy in range(h // 8):
        for ux in range(w // 8):
            if dec["intra"][uy, ux]:
                continue
            for c in range(3):
                sh = 1 if c else 0
                a = off[c][(uy * 8) >> sh:(uy * 8 + 8) >> sh, (ux * 8) >> sh:(ux * 8 + 8) >> sh]
                b = on[c][(uy * 8) >> sh:(uy * 8 + 8) >> sh, (ux * 8) >> sh:(ux * 8 + 8) >> sh]
                if (a != b).any():
                    key = ("chroma" if c else "luma", int(dec["cu_log2"][uy, ux]) - sh)
                    changed[key] = changed.get(key, 0) + 1
    print("8x8 units with changed levels by TB size:", changed)
    assert set(changed) == {("luma", 3), ("luma", 4), ("luma", 5), ("chroma", 2), ("chroma", 3), ("chroma", 4)}


def test_effect_and_defaults():
    fr = _frames(7 | TEXTURED, 4, 160, 96)
    kw = dict(qp=22, search_range=32)
    plain, _ = hevc.encode_sequence_cpu(fr, **kw)
    off, _ = hevc.encode_sequence_cpu(fr, rd_quant=False, **kw)
    on, _ = hevc.encode_sequence_cpu(fr, rd_quant=True, **kw)
    print("textured 160x96 QP 22: off", len(off), "on", len(on))
    assert off == plain
    assert len(on) < len(off)
    # with the tool on the RDOQ-lite pass does not run, whatever `rdoq` says
    assert hevc.encode_sequence_cpu(fr, rd_quant=True, rdoq=False, **kw)[0] == on


# ---- plumbing --------------------------------------------------------------------------------
def test_tool_bit_matches_the_native_header():
    txt = open(os.path.join(ROOT, "csrc", "include", "tv", "rdq.h")).read()
    native = {n: int(v) for n, v in re.findall(r"constexpr int (kTool\w+) = (\d+);", txt)}
    assert native == {"kToolRdQuant": hevc.TOOL_RD_QUANT} and hevc.TOOL_RD_QUANT == 1024
    py = {n for n in dir(hevc) if n.startswith("TOOL_")}
    assert py == {"TOOL_RD_QUANT"}
    flags = [getattr(hevc, n) for n in dir(hevc) if n.startswith("FLAG_")]
    assert all(hevc.TOOL_RD_QUANT & f == 0 for f in flags)
    assert _native(np.zeros((4, 4), np.int32), 27, 2, 0)[2] == int(re.search(r"kRdqLambda = (\d+);", txt).group(1))


def test_plumbing():
    assert hevc.codec_flags() == 1 | 4
    assert hevc.codec_flags(rd_quant=True) == 1 | 4 | 1024
    base, on = EncodeSpec(640, 360), EncodeSpec(640, 360, rd_quant=True)
    assert base.rd_quant is False
    assert base.engine_key() != on.engine_key()
    assert base.tools() == {"wpp": True, "rqt": True, "pintra": True, "cascade": True, "rdoq": True}
    assert on.tools() == dict(base.tools(), rd_quant=True)


def test_default_fingerprint_is_unchanged():
    from thinvids_amd.parallel.node_job import Checkpoint

    before = {"wpp": True, "rqt": True, "pintra": True, "cascade": True, "rdoq": True}
    assert Checkpoint.fingerprint(tools=EncodeSpec(1, 1).tools()) == Checkpoint.fingerprint(tools=before)
    assert Checkpoint.fingerprint(tools=EncodeSpec(1, 1, rd_quant=True).tools()) != Checkpoint.fingerprint(tools=before)


def test_job_and_cpu_engine_plumbing():
    from thinvids_amd.models.cpu_engines import CpuHevcEngine
    from thinvids_amd.worker.tasks import encode_spec_for_job

    job = {"source_width": 640, "source_height": 360}
    assert encode_spec_for_job(job, {"tv_gop": "64"}).rd_quant is False
    assert encode_spec_for_job(dict(job, rd_quant=True), {"tv_gop": "64"}).rd_quant is True
    assert encode_spec_for_job(job, {"tv_rd_quant": "1"}).rd_quant is True
    assert encode_spec_for_job(job, {"tv_rd_quant": "0"}).rd_quant is False
    eng = CpuHevcEngine(64, 64, rd_quant=True)
    assert eng.tools["rd_quant"] is True
    eng.close()
