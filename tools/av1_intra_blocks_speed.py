"""AV1 engine speed, bytes and PSNR with intra blocks in inter frames (intra_in_inter,
tv/av1_enc.h) off and on.

    python tools/av1_intra_blocks_speed.py [--res 1920x1080] [--qindex 100] [--gop 16] [--batch 8] [--cut 8]
                                           [--textured] [--rounds 3] [--steps 3] [--warmup 1] [--out FILE]
    python tools/av1_intra_blocks_speed.py --tool on --once     # one untimed step, for a kernel profiler

Every measurement runs in a fresh child process (one process owns the GPU at a time), off and
on alternately: `batch` segments x `gop` synthetic frames per step through
Av1GpuEngine.encode_gop + the OBU writer pool.  --cut N: frames N.. of every segment come from
an unrelated seed and start (a cut that stays a P frame); 0: the bench's content, no cut.
Prints one JSON line per child (frames/s, bytes, PSNR-Y and accepted intra blocks of the last
step) and a summary with the medians.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a) -> None:
    import numpy as np
    import torch

    from thinvids_amd.models.av1_engine import Av1GpuEngine
    from thinvids_amd.ops import stage

    w, h = map(int, a.res.split("x"))
    on = a.tool == "on"
    seed = 1 | ((1 << 31) if a.textured else 0)
    eng = Av1GpuEngine(w, h, batch=a.batch, qindex=a.qindex, intra_in_inter=on)
    dev, W, H, lib = eng.dev, eng.W, eng.H, stage._lib()

    def loader(i: int):
        def load(t, planes):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            cut = a.cut and t >= a.cut
            ts = [(i * a.batch + b) * a.gop + t + (40 if cut else 0) for b in range(a.batch)]
            src = stage.synth_frames(seed + (16 if cut else 0), w, h, ts, dev)
            for c, dst in enumerate(planes):
                off, pw, ph, stride, fs = src.planes[c]
                cw, chh = (W, H) if c == 0 else (W // 2, H // 2)
                stage._ok(lib.tv_pad_batch(C.c_void_p(src.ptr(c)), pw, ph, stride, fs, C.c_void_p(dst.data_ptr()),
                                           cw, chh, cw, cw * chh, a.batch, st))
        return load

    def step(i: int):
        g = eng.encode_gop(a.gop, loader(i))
        return g, [b"".join(f.result()) for f in eng.submit_entropy(g)]

    if a.once:
        step(0)
        eng.close()
        return
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(a.steps):
        g, segs = step(a.warmup + i)
    dt = time.perf_counter() - t0
    out = {"tool": a.tool, "frames_per_s": round(a.steps * a.batch * a.gop / dt, 1),
           "last_step_bytes": sum(len(s) for s in segs), "last_step_psnr_y": round(eng.psnr(g)["y"], 4),
           "last_step_accepted": int((g.ib >> 1).sum()) if g.ib is not None else 0,
           "last_step_blocks": int(np.prod(g.mode.shape))}
    eng.close()
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--qindex", type=int, default=100)
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cut", type=int, default=0, help="frames from this index on are unrelated content (0: no cut)")
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--rounds", type=int, default=3, help="off / on pairs")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tool", choices=("off", "on"), default=None, help="run one measurement in this process")
    ap.add_argument("--once", action="store_true", help="with --tool: one untimed step (for a profiler)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.tool:
        child(a)
        return
    common = [sys.executable, os.path.abspath(__file__), "--res", a.res, "--qindex", str(a.qindex), "--gop", str(a.gop),
              "--batch", str(a.batch), "--cut", str(a.cut), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    common += ["--textured"] if a.textured else []
    runs = []
    for _ in range(a.rounds):
        for state in ("off", "on"):
            p = subprocess.run(common + ["--tool", state], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:  # a failed child ends the measurement: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"child ({state}) exited with {p.returncode}")
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), flush=True)
    med = {t: statistics.median(r["frames_per_s"] for r in runs if r["tool"] == t) for t in ("off", "on")}
    res = {"config": {k: getattr(a, k) for k in ("res", "qindex", "gop", "batch", "cut", "textured", "steps", "warmup")},
           "runs": runs, "median_frames_per_s": med, "on_over_off": round(med["on"] / med["off"], 4)}
    print(json.dumps(res["median_frames_per_s"] | {"on_over_off": res["on_over_off"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
