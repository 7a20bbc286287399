"""Engine speed with the SATD sub-pel decision (subpel_satd) off and on.

    python tools/subpel_satd_speed.py [--rounds 3] [--steps 3] [--warmup 1] [--out FILE]

Runs the bench's 1080p engine configuration (QP 27, GOP 64, range 64, SAO, the auto batch)
through GpuEngine.encode_synthetic, off and on alternately, every measurement in a fresh child
process (one process owns the GPU at a time).  Prints one JSON line per child and a summary
(median frames/s of both, bytes and PSNR-Y of the last step).  With --once the process runs a
single untimed step of --tool and exits: the command to put under a kernel profiler.

main(tool, script) measures any opt-in GpuEngine / EncodeSpec switch the same way
(tools/sign_hiding_speed.py).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a, tool: str) -> None:
    from thinvids_amd.models.gpu_engine import GpuEngine
    from thinvids_amd.worker.encoder import EncodeSpec, auto_batch, device_budget

    w, h = map(int, a.res.split("x"))
    on = a.tool == "on"
    spec = EncodeSpec(w, h, qp=a.qp, gop=a.gop, sao=True, **{tool: on})
    batch = a.batch or auto_batch(spec, device_budget(0))
    seed = 1 | ((1 << 31) if a.textured else 0)
    eng = GpuEngine(width=w, height=h, qp=a.qp, batch=batch, gop=a.gop, search_range=64, sao=True, seed=seed,
                    **{tool: on})
    starts = lambda i: [(i * batch + b) * a.gop for b in range(batch)]  # noqa: E731
    if a.once:
        eng.encode_synthetic(starts(0))
        eng.close()
        return
    for i in range(a.warmup):
        eng.encode_synthetic(starts(i))
    t0 = time.perf_counter()
    for i in range(a.steps):
        segs = eng.encode_synthetic(starts(a.warmup + i))
    dt = time.perf_counter() - t0
    out = {"tool": a.tool, "batch": batch, "frames_per_s": round(a.steps * batch * a.gop / dt, 1),
           "last_step_bytes": sum(len(s) for s in segs), "last_step_psnr_y": round(eng.psnr(0)["y"], 4),
           "last_step_gpu_ms": round(eng.timing()["gpu_ms"], 1)}
    eng.close()
    print(json.dumps(out), flush=True)


def main(tool: str = "subpel_satd", script: str = os.path.abspath(__file__)) -> None:
    """`tool`: the switch to alternate; `script`: the file the children run (it calls this)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--gop", type=int, default=64)
    ap.add_argument("--batch", type=int, default=0, help="segments per step (0: the bench's auto batch)")
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--rounds", type=int, default=3, help="off / on pairs")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tool", choices=("off", "on"), default=None, help="run one measurement in this process")
    ap.add_argument("--once", action="store_true", help="with --tool: one untimed step (for a profiler)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.tool:
        child(a, tool)
        return
    common = [sys.executable, script, "--res", a.res, "--qp", str(a.qp), "--gop", str(a.gop),
              "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup)] + (["--textured"] if a.textured else [])
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
    res = {"config": {"tool": tool, "res": a.res, "qp": a.qp, "gop": a.gop, "textured": a.textured, "steps": a.steps, "warmup": a.warmup},
           "runs": runs, "median_frames_per_s": med, "on_over_off": round(med["on"] / med["off"], 4)}
    print(json.dumps(res["median_frames_per_s"] | {"on_over_off": res["on_over_off"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
