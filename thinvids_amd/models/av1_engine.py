"""GPU AV1 encode engine (BASELINE config #4) for one MI355X.

Encodes a BATCH of B independent GOP-aligned segments in lock-step: frame t of every
segment is one launch of each kernel (grid = blocks x segments).  Per frame, on the
current HIP stream:

    key frame   k_av1e_intra (anti-diagonal wavefront of 16x16 blocks)
    P frame     k_av1e_inter (full-pel +-16 LDS search, quarter-pel refine, recon)
                [intra_in_inter: k_av1e_ib_analyse -> k_av1e_ib_select -> 7 x k_av1e_ib_recon]
                [cfl: the <CFL = true> instantiations of k_av1e_intra / k_av1e_ib_recon, whose block
                 coder also tries chroma from luma]
                [dir_intra: their <DIR = true> instantiations, whose mode searches run over 34
                 (mode, angle delta) candidates with rates from the default CDFs]
                [tx_split: the <TXS = true> instantiation of k_av1e_inter's recon stage, which codes
                 the luma residual as one 16x16 and as four 8x8 transforms and keeps the cheaper]
    both        k_av1e_lfinfo -> k_deblock (Y, U, V) -> k_cdef_dir -> k_av1e_cdef_skip ->
                k_cdef_search (Y, U, V) -> k_av1e_cdef_choose -> k_cdef_apply -> next reference

Decisions (mode / MV words, quantised levels, CDEF tables and indices) of the whole GOP
stay resident in HBM; at the end of the GOP the nonzero transform blocks are compacted on
the device and copied to the host once, and a CPU thread pool writes every segment's OBU
temporal units (range coder) while the GPU moves on to the next GOP.

Device memory: `buffers()` below names every device buffer of an engine once; the
constructor and `_alloc_gop` allocate from it, `Av1GpuEngine.estimate` sums it without a GPU
(the worker's byte budget, worker/encoder.py engine_bytes) and `footprint()` sums what was
allocated.  A frame allocates nothing.  The encoder model's constants and per-q-index values
(av1_enc.h) are read from the core library, not restated here.

Bit-exact with the C++ golden encoder (``av1.golden_encode``), whose streams decode
bit-exactly with dav1d (tests/test_av1_conformance.py), and with the decoder oracle
(``av1.decode``): tests/test_av1_codec.py.
"""
from __future__ import annotations

import concurrent.futures as cf
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from .._native import core_lib as _core, dptr as _p, gpu_lib as _gpu, ok, stream
from . import av1 as av1m


def _model():
    """The encoder model of csrc/include/tv/av1_enc.h, read from the core library once:
    constants, and the per-q-index tables of q = 0..255."""
    lib = _core()
    c = (C.c_int64 * 16)()
    nsets = lib.tv_av1c_model_constants(c)
    q = np.zeros((256, 3), np.int64)
    for i in range(256):
        lib.tv_av1c_model_q(i, q[i].ctypes.data_as(C.POINTER(C.c_int64)))
    assert c[6 + nsets] == av1m.TOOL_DIR_INTRA  # appended after the lr sets (kToolDirIntra)
    assert c[7 + nsets] == av1m.TOOL_TX_SPLIT  # then kToolTxSplit
    return list(c[:6]) + [tuple(c[6:6 + nsets])], q


(CDEF_MASK_Y, CDEF_MASK_UV, MEMO_RECORD_BYTES, IB_PASSES, TOOL_INTRA_IN_INTER, TOOL_CFL, LR_SETS), _Q = _model()
LF_LEVEL = _Q[:, 0].astype(np.int32)  # frame loop-filter level of a q-index
LR_RATE = _Q[:, 1].copy()  # rate of a restored unit in SSE units
CDEF_DAMPING = _Q[:, 2].astype(np.int32)  # of a stream, from its base q-index


def _ok(rc: int):
    ok(rc, _gpu(), "tv_av1e_last_error")


def lr_grid(size: int) -> int:
    """Restoration units along a plane dimension (av1_defs.h lr_count_units, 64-px units)."""
    return max(1, (size + 32) // 64)


def buffers(W: int, H: int, B: int, F: int, intra_in_inter: bool = False) -> dict:
    """Every device buffer of an engine of coded size W x H, B segments and GOPs of up to F
    frames, as group -> name -> (shape, dtype name):

    * ``work``: the frame workspace, allocated by the constructor.  Kernels run on the
      ``[:nseg]`` leading views of these full-batch buffers.
    * ``slot``: one GOP decision slot; the engine holds two (_alloc_gop).
    * ``upload``: the per-GOP q-index / filter-level / restoration-rate uploads.

    Aliasing: k_deblock, k_cdef_apply and k_sgr_select read neighbouring tiles of their
    inputs, so an output buffer is never one of that launch's inputs (rec -> dbk -> cdf ->
    fin).  The reference (`fin` of frame t-1) is read by k_av1e_inter and the refine / unify
    kernels of frame t and by nothing later, so the last filter of frame t (the restoration,
    or the CDEF apply without it) writes `fin` in the same stream.  The copy stream reads GOP
    slots only, never the workspace."""
    bw, bh = W // 16, H // 16
    nb, n8, nfb = bw * bh, (W // 8) * (H // 8), -(-W // 64) * -(-H // 64)
    planes = (("y", H, W), ("u", H // 2, W // 2), ("v", H // 2, W // 2))
    work = {f"{s}_{c}": ((B, h, w), "uint8") for s in ("src", "rec", "fin", "dbk", "cdf") for c, h, w in planes}
    work.update({
        "iy": ((B, H // 4, W // 4), "int32"),
        "iu": ((B, H // 8, W // 8), "int32"), "iv": ((B, H // 8, W // 8), "int32"),
        "dirs": ((B, n8), "uint8"), "var": ((B, n8), "int32"),
        "se_y": ((B, nfb, 64), "int64"), "se_u": ((B, nfb, 64), "int64"), "se_v": ((B, nfb, 64), "int64"),
        "py": ((B, nfb), "int8"), "puv": ((B, nfb), "int8"),
    })
    for c, h, w in planes:
        work[f"prm_{c}"] = ((B, lr_grid(w) * lr_grid(h), 3), "int32")
        work[f"sse_{c}"] = ((B, -(-h // 64) * -(-w // 64)), "int64")
    # inter frames: the motion field's second buffer, per-segment frame SATD, two [B][nb] memo record sets
    work.update({"mvtmp": ((B, nb), "int32"), "satd": ((B,), "int64"),
                 "memo": ((2 * B * nb * MEMO_RECORD_BYTES,), "uint8")})
    if intra_in_inter:  # scratch of the intra-block passes
        work.update({"ibcost": ((B, nb), "int32"), "ibcand": ((B, nb), "uint8"), "ibcnt": ((B, IB_PASSES), "int32"),
                     "iblist": ((B, IB_PASSES, nb), "int32")})
    slot = {
        "mode": ((F, B, nb), "int32"), "mv": ((F, B, nb), "int32"),
        "ly": ((F, B, nb, 256), "int16"), "lu": ((F, B, nb, 64), "int16"), "lv": ((F, B, nb, 64), "int16"),
        "tabs": ((F, B, 16), "uint8"), "fbidx": ((F, B, nfb), "int8"), "sse": ((F, B, 3), "int64"),
        "lr": ((F, B, 3, av1m.lr_units(W, H), 3), "int32"),
    }
    if intra_in_inter:
        slot["ib"] = ((F, B, nb), "uint8")
    upload = {"q": ((F, B), "int32"), "lf": ((F, B, 4), "int32"), "lr_rate": ((F, B), "int64")}
    return {"work": work, "slot": slot, "upload": upload}


def _nbytes(group: dict) -> int:
    return sum(int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in group.values())


@dataclass
class GopHost:
    """Host copy of one GOP's decisions for the entropy stage."""
    nframes: int
    mode: np.ndarray     # (F, B, nb) uint32
    mv: np.ndarray
    tabs: np.ndarray     # (F, B, 16) uint8
    fbidx: np.ndarray    # (F, B, nfb) int8
    packed: list         # per plane: (eob-truncated scan-order TBs int16, start offsets (F, B) int64)
    sse: np.ndarray      # (F, B, 3) int64
    key: list            # per frame
    qm: np.ndarray = None  # (F, B) q-index per frame and segment
    lr: np.ndarray = None  # (F, B, 3, nu, 3) restoration units (set | -1, xqd0, xqd1)
    ib: np.ndarray = None  # (F, B, nb) uint8: bit 0 intra candidate, bit 1 accepted (intra_in_inter engines)


class Av1GpuEngine:
    """B segments x one GOP per call on one GPU; see module docstring."""

    def __init__(self, width: int, height: int, batch: int, qindex: int = 100, device: int = 0,
                 threads: int | None = None, cascade: bool = True, intra_in_inter: bool = False,
                 cfl: bool = False, dir_intra: bool = False, tx_split: bool = False):
        """`intra_in_inter` (off by default): 16x16 blocks of inter frames may be coded as intra
        blocks (av1_enc.h "intra blocks in inter frames"; k_av1e_ib_*), as the golden encoder
        does with the same flag.  `cfl` (off by default): intra blocks may predict chroma from
        their reconstructed luma (av1_enc.h "chroma from luma"; the CFL instantiations of
        k_av1e_intra / k_av1e_ib_recon).  `dir_intra` (off by default): the intra mode searches run
        over every directional angle strictly between 90 and 180 degrees with CDF-based rates
        (av1_enc.h "directional intra"; the DIR instantiations of the same kernels).  `tx_split`
        (off by default): non-skip inter blocks may code their luma as four 8x8 transforms
        (av1_enc.h "transform split"; the TXS instantiation of k_av1e_inter)."""
        import torch

        self.intra_in_inter = bool(intra_in_inter)
        self.cfl = bool(cfl)
        self.dir_intra = bool(dir_intra)
        self.tx_split = bool(tx_split)
        # the kernels' tools word (intra_in_inter is a launch of its own)
        self.tools = ((TOOL_CFL if self.cfl else 0) | (av1m.TOOL_DIR_INTRA if self.dir_intra else 0) |
                      (av1m.TOOL_TX_SPLIT if self.tx_split else 0))
        self.cascade = bool(cascade)  # constant q: the low-delay q cascade (av1.cascade_qmap)
        self.torch = torch
        self.w, self.h, self.B, self.q = width, height, batch, int(qindex)
        self.W, self.H = av1m.coded_size(width, height)
        self.dev = torch.device("cuda", device)
        self.lr_enabled = True
        self.damping = int(CDEF_DAMPING[self.q])
        self._ws = self._alloc(buffers(self.W, self.H, batch, 0, self.intra_in_inter)["work"])
        self.src, self.rec, self.fin, self._dbk, self._cdf = (
            tuple(self._ws[f"{s}_{c}"] for c in "yuv") for s in ("src", "rec", "fin", "dbk", "cdf"))
        self.pool = cf.ThreadPoolExecutor(max_workers=threads or min(32, os.cpu_count() or 8))
        self._gop_cap = 0
        self._slots = []
        self._keep = ()
        self.lock = None  # set by the worker's engine cache
        self.staging = None
        self._copy_stream = torch.cuda.Stream(self.dev)
        self._copy_pool = cf.ThreadPoolExecutor(max_workers=1)

    def _alloc(self, group: dict) -> dict:
        return {n: self.torch.zeros(shape, dtype=getattr(self.torch, dt), device=self.dev)
                for n, (shape, dt) in group.items()}

    @staticmethod
    def estimate(width: int, height: int, batch: int, gop: int, intra_in_inter: bool = False) -> dict:
        """{"dev": bytes} of an engine that has run a GOP of `gop` frames: the sum over
        buffers() (workspace, two slots, one GOP's uploads); needs no GPU.  _collect's packing
        buffers depend on the data (the nonzero levels of the GOP), live only during the copy
        and are not counted."""
        d = buffers(*av1m.coded_size(width, height), batch, gop, intra_in_inter)
        return {"dev": _nbytes(d["work"]) + 2 * _nbytes(d["slot"]) + _nbytes(d["upload"])}

    def footprint(self) -> dict:
        """{"dev": bytes} of the device tensors the engine holds now (estimate()'s terms)."""
        held = [*self._ws.values(), *(x for S in self._slots for x in S.values()), *self._keep]
        return {"dev": sum(x.numel() * x.element_size() for x in held)}

    def _alloc_gop(self, F: int):
        """Two GOP decision buffers (slots): the GPU fills one while the previous GOP's is
        compacted and copied to the host on the copy stream (encode_gop(async_host=True))."""
        if F <= self._gop_cap:
            return
        slot = buffers(self.W, self.H, self.B, F, self.intra_in_inter)["slot"]
        self._slots = [self._alloc(slot) for _ in range(2)]
        self._slot_busy = [None, None]
        self._slot = 0
        self._gop_cap = F

    def _use_slot(self):
        s = self._slot
        self._slot ^= 1
        if self._slot_busy[s] is not None:  # the previous GOP in this slot is still being collected
            self._slot_busy[s].result()
            self._slot_busy[s] = None
        return s

    # ------------------------------------------------------------------ one frame ----
    def _frame(self, G: dict, t: int, key: bool, B: int, qarr, lvl, q_rate):
        """Frame t of the first B segments into GOP slot G: launches on [:B] views of the
        workspace (buffers() has the aliasing rules), no allocation."""
        from ..ops import av1 as ops

        lib = _gpu()
        st = stream(self.dev)
        W, H, w, h, dmp = self.W, self.H, self.w, self.h, self.damping
        ws = {n: x[:B] for n, x in self._ws.items() if n != "memo"}
        src, rec, fin, dbk, cdf = ([x[:B] for x in s] for s in (self.src, self.rec, self.fin, self._dbk, self._cdf))
        mode, mv = G["mode"][t, :B], G["mv"][t, :B]
        lev = [G[k][t, :B] for k in ("ly", "lu", "lv")]
        if key:
            if self.intra_in_inter:
                G["ib"][t, :B].zero_()
            _ok(lib.tv_av1e_intra(*map(_p, src), *map(_p, rec), _p(mode), _p(mv), *map(_p, lev), W, H, B, _p(qarr),
                                  self.tools, st))
        else:
            icost = ws["ibcost"] if self.intra_in_inter else None
            _ok(lib.tv_av1e_inter_tools(*map(_p, src), *map(_p, fin), *map(_p, rec), _p(mode), _p(mv),
                                        _p(ws["mvtmp"]), _p(ws["satd"]), _p(self._ws["memo"]), *map(_p, lev),
                                        None if icost is None else _p(icost), W, H, B, _p(qarr), self.tools, st))
            if self.intra_in_inter:
                _ok(lib.tv_av1e_iblocks(*map(_p, src), *map(_p, rec), _p(mode), _p(mv), *map(_p, lev), _p(icost),
                                        _p(ws["ibcand"]), _p(G["ib"][t, :B]), _p(ws["ibcnt"]), _p(ws["iblist"]), W, H,
                                        B, _p(qarr), self.tools, st))
            _ok(lib.tv_av1e_merge(_p(mode), _p(mv), W, H, B, st))
        info = (ws["iy"], ws["iu"], ws["iv"])
        _ok(lib.tv_av1e_lfinfo(_p(mode), W, H, B, _p(lvl), *map(_p, info), st))
        # every transform / block edge of the encoder's planes is on the 16 (luma) / 8
        # (chroma) grid: blocks are 16x16 or merged 32 / 64 with one TX per plane; the luma of a
        # transform-split block has 8x8 transforms
        for c in range(3):
            ops.deblock(rec[c], info[c], c > 0, 0, estep=8 if c or self.tx_split else 16, out=dbk[c])
        dirs, var = ops.cdef_dirs(dbk[0], out=(ws["dirs"], ws["var"]))
        _ok(lib.tv_av1e_cdef_skip(_p(mode), _p(dirs), W, H, B, st))  # skip blocks are not filtered
        se = [ops.cdef_search(src[c], dbk[c], dirs, var, c > 0, dmp, luma_w8=W // 8,
                              pmask=CDEF_MASK_UV if c else CDEF_MASK_Y, checker=True, out=ws["se_" + "yuv"[c]])
              for c in range(3)]
        py, puv = ws["py"], ws["puv"]
        _ok(lib.tv_av1e_cdef_choose(*map(_p, se), _p(mode), W, H, B, _p(G["tabs"][t, :B]), _p(G["fbidx"][t, :B]),
                                    _p(py), _p(puv), st))
        flt = cdf if self.lr_enabled else fin  # the last filter of the frame writes the next reference
        for c in range(3):
            ops.cdef_apply(dbk[c], dirs, var, puv if c else py, c > 0, dmp, luma_w8=W // 8, out=flt[c])
        if self.lr_enabled:
            # Normative self-guided restoration search + apply on the CDEF output (7.17 unit grid
            # and stripes, whose edges read the deblocked planes): the golden encoder's per-unit
            # off / set-4 / set-10 choice (SSE + rate, first minimum), one fused launch per plane
            for c in range(3):
                _, prm = ops.sgr_select(src[c], cdf[c], dbk[c], c > 0, q_rate, out=fin[c], prm=ws["prm_" + "yuv"[c]])
                G["lr"][t, :B, c, :prm.shape[1]] = prm
        for c in range(3):  # per-64x64-unit SSE over the display region, summed per segment
            u = ws["sse_" + "yuv"[c]]
            _ok(lib.tv_av1e_unit_sse(_p(src[c]), _p(fin[c]), W >> (c > 0), H >> (c > 0), w >> (c > 0), h >> (c > 0), B,
                                     _p(u), st))
            self.torch.sum(u, dim=1, out=G["sse"][t, :B, c])

    def encode_gop(self, nframes: int, load_frame, nseg: int | None = None, qmap=None, async_host: bool = False):
        """Run the GPU part of one GOP for all B segments.  load_frame(t, (Y, U, V)) fills
        the coded-size source planes [B, H, W] of frame t (device tensors).  `qmap`
        (optional (nframes, nseg) ints): per-frame, per-segment q-index from rate control
        (2-pass / CRF plans); None = the engine's constant q-index.  Returns the host copy
        of the decisions (one device->host transfer of compacted levels).  async_host=True
        returns a Future of it instead: the copy runs on a copy stream / thread behind the next
        GOP's kernels (double-buffered decision slots)."""
        torch = self.torch
        nseg = nseg or self.B
        if not 1 <= nseg <= self.B:
            raise ValueError(f"nseg {nseg} outside 1..{self.B}")
        self._alloc_gop(nframes)
        slot = self._use_slot()
        if qmap is None:
            col = av1m.cascade_qmap(self.q, nframes) if self.cascade else [self.q] * nframes
            qm = np.repeat(np.asarray(col, np.int32)[:, None], nseg, axis=1)
        else:
            qm = np.clip(np.asarray(qmap, np.int32).reshape(nframes, nseg), 1, 255)
        lv = np.repeat(LF_LEVEL[qm][:, :, None], 4, axis=2)
        # pinned + non_blocking: a pageable upload would block the host on the previous
        # GOP's kernels (the stream drains before this GOP's first launch)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(self.dev, non_blocking=True)
        qd = up(qm)
        ld = up(lv)
        rd = up(LR_RATE[qm])
        self._keep = (qd, ld, rd)
        S = self._slots[slot]
        if not self.lr_enabled:
            S["lr"][:nframes, :nseg, :, :, 0] = -1
        for t in range(nframes):
            load_frame(t, self.src)
            self._frame(S, t, t == 0, nseg, qd[t], ld[t], rd[t])
        self.nseg = nseg
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        if not async_host:
            return self._collect(S, ev, nframes, nseg, qm)
        fut = self._copy_pool.submit(self._collect, S, ev, nframes, nseg, qm)
        self._slot_busy[slot] = fut
        return fut

    def _collect(self, S: dict, ev, F: int, nseg: int, qm) -> GopHost:
        """Pack the nonzero TBs of a GOP slot eob-truncated in scan order on the copy stream
        (after `ev`: k_av1e_tb_len -> cumsum -> k_av1e_tb_pack) and copy every decision
        array to the host."""
        torch = self.torch
        torch.cuda.set_device(self.dev)
        cs = self._copy_stream
        lib = _gpu()
        Bmax, nb = S["mode"].shape[1], S["mode"].shape[2]
        ntb = F * nseg * nb
        with torch.cuda.stream(cs):
            cs.wait_event(ev)
            st = cs.cuda_stream
            lens, ends = [], []
            for p, k in enumerate(("ly", "lu", "lv")):
                ln = torch.empty(ntb, dtype=torch.int32, device=self.dev)
                _ok(lib.tv_av1e_tb_len(_p(S[k]), _p(S["mode"]), ntb, nb, nseg, Bmax, p, _p(ln), st))
                lens.append(ln)
                ends.append(torch.cumsum(ln, 0, dtype=torch.int64))
            totals = torch.stack([e[-1] for e in ends]).cpu().tolist()
            outs = []
            for p, k in enumerate(("ly", "lu", "lv")):
                o = torch.empty(max(1, totals[p]), dtype=torch.int16, device=self.dev)
                _ok(lib.tv_av1e_tb_pack(_p(S[k]), _p(S["mode"]), _p(lens[p]), _p(ends[p]), ntb, nb, nseg, Bmax, p, _p(o),
                                        st))
                outs.append((o, (ends[p] - lens[p]).view(F, nseg, nb)[:, :, 0]))
            host = GopHost(
                nframes=F,
                mode=S["mode"][:F, :nseg].cpu().numpy().view(np.uint32),
                mv=S["mv"][:F, :nseg].cpu().numpy().view(np.uint32),
                tabs=S["tabs"][:F, :nseg].cpu().numpy(),
                fbidx=S["fbidx"][:F, :nseg].cpu().numpy(),
                packed=[(o[:max(1, t)].cpu().numpy(), off.cpu().numpy().astype(np.int64))
                        for (o, off), t in zip(outs, totals)],
                sse=S["sse"][:F, :nseg].cpu().numpy(),
                key=[t == 0 for t in range(F)],
                qm=qm,
                lr=S["lr"][:F, :nseg].cpu().numpy(),
                ib=S["ib"][:F, :nseg].cpu().numpy() if "ib" in S else None,
            )
        return host

    # ------------------------------------------------------------------ entropy ------
    def write_segment(self, g: GopHost, b: int) -> list:
        """Temporal units of segment b of a GOP (runs on a pool thread; the native writer
        releases the GIL)."""
        tus = []
        wr = av1m.StreamWriter(self.w, self.h)
        for t in range(g.nframes):
            tabs = g.tabs[t, b]
            q = int(g.qm[t, b])
            fp = av1m.frame_params(g.key[t], q, [int(LF_LEVEL[q])] * 4, 0, self.damping, tabs[:8], tabs[8:],
                                   tx_select=self.tx_split)
            lev = [pk[0][pk[1][t, b]:] for pk in g.packed]  # eob-truncated scan-order TBs
            tus.append(wr.write(fp, np.ascontiguousarray(g.mode[t, b]), np.ascontiguousarray(g.mv[t, b]), lev[0],
                                lev[1], lev[2], np.ascontiguousarray(g.fbidx[t, b]), packed=2, seq_header=g.key[t],
                                lr=np.ascontiguousarray(g.lr[t, b])))
        return tus

    def submit_entropy(self, g: GopHost) -> list:
        return [self.pool.submit(self.write_segment, g, b) for b in range(g.mode.shape[1])]

    def psnr(self, g: GopHost) -> dict:
        n = g.sse.shape[0] * g.sse.shape[1]
        px = [self.w * self.h, (self.w // 2) * (self.h // 2), (self.w // 2) * (self.h // 2)]
        out = {}
        for c, k in enumerate("yuv"):
            mse = g.sse[:, :, c].sum() / (n * px[c])
            out[k] = float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))
        mse = g.sse.sum() / (n * sum(px))
        out["yuv"] = float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))
        return out

    def close(self):
        self._copy_pool.shutdown(wait=True)
        self.pool.shutdown(wait=True)
