"""Byte counts of estimate_footprint over the engine-layout table (README.md).  One line per
(environment, size, entropy): `env | WxH entropy | dev host sha`, where dev / host are summed
over the 64 (batch, sao, bframes, pintra, wpp) combinations and sha is the first 12 hex digits
of the sha256 of those 64 rows' individual numbers; --full prints the rows themselves.
Every environment setting runs in a fresh process (TV_SLOTS is cached per process).  No GPU.

    python profiles/engine_layout/estimate_table.py OUT.txt [--full]
"""
import hashlib
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [(64, 64), (96, 64), (320, 180), (1920, 1080), (3840, 2160)]
BATCHES = [1, 3, 8, 48]
# (environment, entropy modes): the coder's own knobs only matter with entropy="gpu"
ENVS = [({}, ("host", "gpu")),
        ({"TV_ENGINE_GROUPS": "1"}, ("host", "gpu")),
        ({"TV_ENGINE_GROUPS": "3"}, ("host", "gpu")),
        ({"TV_SLOTS": "2"}, ("host", "gpu")),
        ({"TV_SLOTS": "8"}, ("host", "gpu")),
        ({"TV_ENT_LANES": "1"}, ("gpu",)),
        ({"TV_ENT_LANES": "2"}, ("gpu",)),
        ({"TV_ENT_LANES": "4"}, ("gpu",)),
        ({"TV_ENT_TOKENS_PER_PX": "0.25"}, ("gpu",)),
        ({"TV_ENT_LANES": "4", "TV_ENT_TOKENS_PER_PX": "0.25", "TV_ENGINE_GROUPS": "3", "TV_SLOTS": "8"}, ("gpu",)),
        ({"TV_ENT_DEBUG": "1"}, ("gpu",))]
KNOBS = ("TV_ENGINE_GROUPS", "TV_SLOTS", "TV_ENT_LANES", "TV_ENT_TOKENS_PER_PX", "TV_ENT_DEBUG", "TV_ENTROPY")


def rows(tag, modes, full):
    sys.path.insert(0, ROOT)
    from thinvids_amd.models.gpu_engine import estimate_footprint

    for (w, h), ent in itertools.product(SIZES, modes):
        dev = host = 0
        sha = hashlib.sha256()
        for batch, sao, bf, pintra, wpp in itertools.product(BATCHES, (0, 1), (1, 8), (1, 0), (1, 0)):
            fp = estimate_footprint(w, h, batch, 16, sao=bool(sao), bframes=bf, pintra=bool(pintra), wpp=bool(wpp),
                                    entropy=ent)
            dev, host = dev + fp["dev"], host + fp["host"]
            sha.update(f"{fp['dev']} {fp['host']}\n".encode())
            if full:
                print(f"{tag} | {w}x{h} {batch} {sao} {bf} {pintra} {wpp} {ent} | {fp['dev']} {fp['host']}")
        if not full:
            print(f"{tag} | {w}x{h} {ent} | {dev} {host} {sha.hexdigest()[:12]}")


if __name__ == "__main__":
    if sys.argv[1] == "--rows":
        rows(sys.argv[2], sys.argv[3].split(","), sys.argv[4] == "full")
    else:
        with open(sys.argv[1], "w") as out:
            for env, modes in ENVS:
                tag = " ".join(f"{k}={v}" for k, v in env.items()) or "default"
                base = {k: v for k, v in os.environ.items() if k not in KNOBS}
                cmd = [sys.executable, __file__, "--rows", tag, ",".join(modes), "full" if "--full" in sys.argv else "sum"]
                out.write(subprocess.run(cmd, check=True, env={**base, **env}, capture_output=True, text=True).stdout)
