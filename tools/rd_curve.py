"""Rate-distortion curve of the golden HEVC encoder on the bench's synthetic content.

    python tools/rd_curve.py --res 640x360 --frames 32 --qps 22,27,32,37 [--cascade 1,3,2,3] [--textured]

Prints one JSON line per QP (kbps per 30 fps stream, PSNR-Y / YUV over the whole clip) and,
with --anchor FILE (a previous run's output), the BD-rate against it.  The GPU engine is bit-
exact with this encoder, so the curve is the engine's curve too; --engine gpu runs the points on
the GPU engine itself (its own synthetic source and SSE), which is what makes 1080p practical.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_point(args):
    qp, a = args
    from thinvids_amd.models import hevc

    w, h = map(int, a["res"].split("x"))
    seed = a["seed"] | (1 << 31 if a["textured"] else 0)
    frames = [hevc.synth_frame(seed, t, w, h) for t in range(a["frames"])]
    if a.get("cut"):  # frames from `cut` on come from an unrelated seed and start: a cut inside the GOP
        frames[a["cut"]:] = [hevc.synth_frame(seed + 16, 40 + t, w, h) for t in range(a["cut"], a["frames"])]
    if a.get("fan"):  # oriented gratings stepping through the directional angles, e.g. for --dir-intra
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from av1_dir_cases import cut_clip, fan_clip

        frames = cut_clip(w, h, a["frames"], a["cut"]) if a.get("cut") else fan_clip(w, h, a["frames"])
    if a.get("chroma_k"):  # chroma that follows luma (av1.correlated_chroma), e.g. for --cfl
        from thinvids_amd.models import av1 as _av1

        ku, kv = a["chroma_k"]
        frames = [_av1.correlated_chroma(f[0], ku, kv, seed=a["seed"] * 1000 + t) for t, f in enumerate(frames)]
    cascade = a["cascade"]
    fq = None
    if cascade:
        fq, k = [], 0
        for i in range(len(frames)):
            idr = i % a["gop"] == 0
            fq.append(max(0, min(51, qp + (a["iqp"] if idr else cascade[(i % a["gop"] - 1) % len(cascade)]))))
    import numpy as np

    uv_mse = []
    kw = dict(sao=a["sao"], rqt=a["rqt"], pintra=a["pintra"], wpp=a["wpp"], cascade=a["ippp_cascade"], rdoq=a["rdoq"],
              subpel_satd=a["subpel_satd"], sign_hiding=a.get("sign_hiding", False),
              rd_quant=a.get("rd_quant", False))
    if a.get("engine") == "gpu":
        return run_point_gpu(qp, a, w, h, seed, fq, kw)
    if a.get("codec") == "av1":
        from thinvids_amd.models import av1

        q = av1.qindex_for_hevc_qp(qp)
        W, H = av1.coded_size(w, h)
        stream, ys = b"", []
        for s0 in range(0, len(frames), a["gop"]):
            n = min(a["gop"], len(frames) - s0)
            qm = None
            if fq is not None:  # a QP cascade in HEVC QP units, mapped to q-indices
                qm = [av1.qindex_for_hevc_qp(x) for x in fq[s0:s0 + n]]
            r = av1.golden_encode(frames[s0:s0 + a["gop"]], w, h, q, qmap=qm,
                                  intra_in_inter=a.get("intra_in_inter", False), cfl=a.get("cfl", False),
                                  dir_intra=a.get("dir_intra", False), tx_split=a.get("tx_split", False))
            stream += r.stream
            ys += [hevc.psnr(f[0], rec[:W * H].reshape(H, W)[:h, :w]) for f, rec in zip(frames[s0:], r.recon)]
            for f, rec in zip(frames[s0:], r.recon):  # chroma MSE for the 6:1:1 PSNR-YUV
                c = rec[W * H:].reshape(2, H // 2, W // 2)[:, :(h + 1) // 2, :(w + 1) // 2].astype(np.float64)
                uv_mse.append([float(np.mean((c[k] - f[1 + k]) ** 2)) for k in range(2)])
    else:
        stream, recons = hevc.encode_sequence_cpu(frames, qp=qp, gop=a["gop"], frame_qps=fq, bframes=a["bframes"], **kw)
        ys = [hevc.psnr(f[0], r[0][:h, :w]) for f, r in zip(frames, recons)]

    mse_y = np.mean([10 ** (-p / 10) for p in ys])
    py = -10 * np.log10(mse_y)
    kbps = len(stream) * 8 * 30 / len(frames) / 1000
    pt = {"qp": qp, "kbps": round(kbps, 2), "psnr_y": round(float(py), 4), "frames": len(frames)}
    if uv_mse:  # av1: PSNR of the 6:1:1 weighted MSE (chroma tools move chroma quality, not luma)
        mu, mv = np.mean(uv_mse, axis=0) / 255.0 ** 2
        pt["psnr_yuv"] = round(float(-10 * np.log10(max((6 * mse_y + mu + mv) / 8, 1e-12))), 4)
    return pt


def run_point_gpu(qp, a, w, h, seed, fq, kw):
    """The same point on the GPU engine: one segment per GOP, PSNR-Y from the engine's SSE."""
    import numpy as np

    from thinvids_amd.models.gpu_engine import GpuEngine

    if a.get("codec") == "av1":
        raise SystemExit("--engine gpu is the HEVC engine")
    n, gop = a["frames"], min(a["gop"], a["frames"])
    if n % gop:
        raise SystemExit("--engine gpu: --frames must be a multiple of --gop")
    starts = list(range(0, n, gop))
    eng = GpuEngine(w, h, qp=qp, batch=len(starts), gop=gop, seed=seed, bframes=a["bframes"], **kw)
    try:
        segs = eng.encode_synthetic(starts, gop, qp=None if fq is None else [fq[s:s + gop] for s in starts])
        sse_y = sum(eng.sse(b)[0] for b in range(len(starts)))
    finally:
        eng.close()
    py = float("inf") if sse_y == 0 else 10 * np.log10(255.0 ** 2 * w * h * n / sse_y)
    kbps = sum(len(s) for s in segs) * 8 * 30 / n / 1000
    return {"qp": qp, "kbps": round(kbps, 2), "psnr_y": round(float(py), 4), "frames": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="640x360")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--gop", type=int, default=64)
    ap.add_argument("--qps", default="22,27,32,37")
    ap.add_argument("--cascade", default="", help="P-frame QP offsets repeating over the GOP, e.g. 3,2,3,1")
    ap.add_argument("--iqp", type=int, default=0, help="I-frame QP offset (with --cascade)")
    ap.add_argument("--sao", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--bframes", type=int, default=1, help="hierarchical-B mini-GOP size (1 = IPPP)")
    ap.add_argument("--codec", choices=("hevc", "av1"), default="hevc",
                    help="av1: the golden AV1 encoder at the q-index matched to each QP")
    # coding tools: explicit flags; this tool alone also honours TV_RQT=0 / TV_PINTRA=0 / TV_WPP=0
    # (A/B sweeps), nothing else in the framework reads them from the environment
    env_on = lambda k: os.environ.get(k, "1") != "0"
    ap.add_argument("--rqt", type=int, default=int(env_on("TV_RQT")))
    ap.add_argument("--ippp-cascade", type=int, default=1, help="built-in constant-QP I P P P QP cascade (tv/gop.h)")
    ap.add_argument("--pintra", type=int, default=int(env_on("TV_PINTRA")))
    ap.add_argument("--wpp", type=int, default=int(env_on("TV_WPP")))
    ap.add_argument("--rdoq", type=int, default=1, help="RDOQ-lite coefficient-group trimming")
    ap.add_argument("--subpel-satd", type=int, default=0, help="sub-pel vectors chosen by SATD + MV rate (tv/me_model.h)")
    ap.add_argument("--sign-hiding", type=int, default=0, help="sign data hiding (tv/sdh.h)")
    ap.add_argument("--rd-quant", type=int, default=0, help="rate-distortion quantisation of inter TBs (tv/rdq.h)")
    ap.add_argument("--intra-in-inter", type=int, default=0, help="av1: intra blocks in inter frames (tv/av1_enc.h)")
    ap.add_argument("--cfl", type=int, default=0, help="av1: chroma from luma (tv/av1_enc.h)")
    ap.add_argument("--dir-intra", type=int, default=0, help="av1: directional intra angles, CDF-based mode rates (tv/av1_enc.h)")
    ap.add_argument("--tx-split", type=int, default=0, help="av1: 8x8 transform split of the luma of inter blocks (tv/av1_enc.h)")
    ap.add_argument("--fan", type=int, default=0, help="av1: replace the clip by the oriented-grating clip of tests/av1_dir_cases.py")
    ap.add_argument("--chroma-k", default="", help="KU,KV: replace the clip's chroma by one that follows its luma "
                    "(U = 128 + KU * (Y2x2 - 128) / 8 + noise; models/av1.py correlated_chroma)")
    ap.add_argument("--metric", choices=("y", "yuv"), default="y", help="BD-rate on PSNR-Y or (av1) on the 6:1:1 PSNR-YUV")
    ap.add_argument("--cut", type=int, default=0, help="frames from this index on are unrelated content (a cut that stays a P frame)")
    ap.add_argument("--engine", choices=("cpu", "gpu"), default="cpu", help="gpu: run the points on the GPU engine, one after another")
    ap.add_argument("--anchor", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = dict(res=a.res, frames=a.frames, gop=a.gop, sao=bool(a.sao), seed=a.seed, textured=a.textured,
               cascade=[int(x) for x in a.cascade.split(",")] if a.cascade else [], iqp=a.iqp,
               bframes=a.bframes, codec=a.codec, rqt=bool(a.rqt), pintra=bool(a.pintra), wpp=bool(a.wpp),
               ippp_cascade=bool(a.ippp_cascade), rdoq=bool(a.rdoq), subpel_satd=bool(a.subpel_satd),
               sign_hiding=bool(a.sign_hiding), rd_quant=bool(a.rd_quant), intra_in_inter=bool(a.intra_in_inter), cut=a.cut,
               engine=a.engine, cfl=bool(a.cfl), dir_intra=bool(a.dir_intra), tx_split=bool(a.tx_split), fan=bool(a.fan), chroma_k=[int(x) for x in a.chroma_k.split(",")] if a.chroma_k else [])
    qps = [int(q) for q in a.qps.split(",")]
    if a.engine == "gpu":
        pts = [run_point((q, cfg)) for q in qps]
    else:
        with ProcessPoolExecutor(len(qps)) as ex:
            pts = list(ex.map(run_point, [(q, cfg) for q in qps]))
    for p in pts:
        print(json.dumps(p))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(pts, f)
    if a.anchor:
        from thinvids_amd.utils.bdrate import bd_rate

        with open(a.anchor) as f:
            anc = json.load(f)
        m = "psnr_yuv" if a.metric == "yuv" else "psnr_y"
        print(json.dumps({"bd_rate_pct": round(bd_rate([p["kbps"] for p in anc], [p[m] for p in anc],
                                                        [p["kbps"] for p in pts], [p[m] for p in pts]), 2), "metric": m}))


if __name__ == "__main__":
    main()
