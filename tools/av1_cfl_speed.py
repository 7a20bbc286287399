"""AV1 engine speed, bytes and PSNR with an opt-in intra tool off and on: chroma from luma (--name
cfl, the default), directional intra (--name dir_intra) or the transform split (--name tx_split);
all in tv/av1_enc.h.

    python tools/av1_cfl_speed.py [--res 1920x1080] [--qindex 100] [--gop 64] [--batch 8] [--textured]
                                  [--intra-in-inter] [--rounds 3] [--steps 2] [--warmup 1] [--out FILE]
    python tools/av1_cfl_speed.py --gop 2            # key-frame heavy: every second frame is a key frame
    python tools/av1_cfl_speed.py --name dir_intra   # the same for directional intra
    python tools/av1_cfl_speed.py --name tx_split    # the same for the transform split
    python tools/av1_cfl_speed.py --tool on --once   # one untimed step of one engine, for a kernel profiler

Both engines (tool off, tool on) live in this one process and take turns, off / on / off / on ...,
so drift of the machine shows up in both alike: `batch` segments x `gop` synthetic frames (the
bench's content) per step through Av1GpuEngine.encode_gop + the OBU writer pool.  Prints one
JSON line per timed run (frames/s, bytes, PSNR of the last step, blocks of the last step that use
the tool: CfL blocks, or blocks with a non-zero angle delta) and
a summary with the medians.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", choices=("cfl", "dir_intra", "tx_split"), default="cfl", help="the tool that is switched")
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--gop", type=int, default=64, help="frames per segment (2: key-frame heavy; 64: the bench's GOP)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--intra-in-inter", action="store_true", help="both engines also code intra blocks in inter frames")
    ap.add_argument("--rounds", type=int, default=3, help="off / on pairs")
    ap.add_argument("--steps", type=int, default=2, help="GOP batches per timed run")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tool", choices=("off", "on"), default=None, help="only this engine")
    ap.add_argument("--once", action="store_true", help="with --tool: one untimed step (for a profiler)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from thinvids_amd.models import av1
    from thinvids_amd.models.av1_engine import Av1GpuEngine
    from thinvids_amd.ops import stage

    w, h = map(int, a.res.split("x"))
    seed = 1 | ((1 << 31) if a.textured else 0)
    states = [a.tool] if a.tool else ["off", "on"]
    engs = {s: Av1GpuEngine(w, h, batch=a.batch, qindex=a.qindex, intra_in_inter=a.intra_in_inter, **{a.name: s == "on"})
            for s in states}
    lib = stage._lib()

    def step(eng, i: int):
        dev, W, H = eng.dev, eng.W, eng.H

        def load(t, planes):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ts = [(i * a.batch + b) * a.gop + t for b in range(a.batch)]
            src = stage.synth_frames(seed, w, h, ts, dev)
            for c, dst in enumerate(planes):
                off, pw, ph, stride, fs = src.planes[c]
                cw, chh = (W, H) if c == 0 else (W // 2, H // 2)
                stage._ok(lib.tv_pad_batch(C.c_void_p(src.ptr(c)), pw, ph, stride, fs, C.c_void_p(dst.data_ptr()),
                                           cw, chh, cw, cw * chh, a.batch, st))

        g = eng.encode_gop(a.gop, load)
        return g, [b"".join(f.result()) for f in eng.submit_entropy(g)]

    def tool_blocks(mode) -> int:
        if a.name == "cfl":
            return int(av1.mode_cfl(mode)[0].sum())
        if a.name == "tx_split":
            return int(av1.mode_tx(mode)[0].sum())
        _, yd, _, uvd = av1.mode_angles(mode)
        return int(((yd != 0) | (uvd != 0)).sum())

    def timed(state: str, first: int) -> dict:
        eng = engs[state]
        torch.cuda.synchronize(eng.dev)
        t0 = time.perf_counter()
        for i in range(a.steps):
            g, segs = step(eng, first + i)
        dt = time.perf_counter() - t0
        ps = eng.psnr(g)
        return {"tool": state, "frames_per_s": round(a.steps * a.batch * a.gop / dt, 1),
                "last_step_bytes": sum(len(s) for s in segs), "last_step_psnr": {k: round(v, 4) for k, v in ps.items()},
                {"cfl": "last_step_cfl_blocks", "tx_split": "last_step_split_blocks"}.get(
                    a.name, "last_step_angled_blocks"): tool_blocks(g.mode),
                "last_step_intra_blocks": int(((np.asarray(g.mode) & 1) == 0).sum())}

    try:
        if a.once:
            step(engs[states[0]], 0)
            return
        for s in states:
            for i in range(a.warmup):
                step(engs[s], i)
        runs = []
        for _ in range(a.rounds):
            for s in states:  # every run of both engines codes the same frames
                runs.append(timed(s, a.warmup))
                print(json.dumps(runs[-1]), flush=True)
    finally:
        for e in engs.values():
            e.close()
    med = {s: statistics.median(r["frames_per_s"] for r in runs if r["tool"] == s) for s in states}
    summary = dict(med)
    if len(states) == 2:
        summary["on_over_off"] = round(med["on"] / med["off"], 4)
    print(json.dumps(summary), flush=True)
    if a.out:
        cfg = {k: getattr(a, k) for k in ("name", "res", "qindex", "gop", "batch", "textured", "intra_in_inter", "steps", "warmup")}
        with open(a.out, "w") as f:
            json.dump({"config": cfg, "runs": runs, "median_frames_per_s": med}, f, indent=1)


if __name__ == "__main__":
    main()
