"""engine_bytes(spec, batch) of the tree in the current directory for the AV1 configurations of
profiles/av1_workspace/README.md, and the HBM budgets at which auto_batch first gives each
batch size (it lowers the batch until engine_bytes <= budget // 2).  No GPU.

    python profiles/av1_workspace/bytes_table.py"""
import os
import sys

sys.path.insert(0, os.getcwd())
from thinvids_amd.worker.encoder import EncodeSpec, auto_batch, engine_bytes  # noqa: E402

for w, h, batch in ((1920, 1080, 32), (3840, 2160, 16), (640, 360, 8)):
    for on in (False, True):
        spec = EncodeSpec(w, h, gop=64, codec="av1", intra_in_inter=on)
        print(f"engine_bytes {w}x{h} x{batch} gop 64 intra_in_inter={int(on)}: {engine_bytes(spec, batch)}")
for w, h in ((1920, 1080), (3840, 2160)):
    spec = EncodeSpec(w, h, gop=64, codec="av1")
    b, steps = auto_batch(spec), []
    while True:
        steps.append((b, 2 * engine_bytes(spec, b)))
        if b == 1:
            break
        b = max(1, b * 3 // 4)
    print(f"auto_batch {w}x{h}: " + ", ".join(f"{b} from budget {need}" for b, need in steps))
