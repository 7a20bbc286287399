"""Engine speed with rate-distortion quantisation (rd_quant, tv/rdq.h) off and on: the
measurement of tools/subpel_satd_speed.py (the bench's 1080p configuration, off and on
alternately, every measurement in a fresh child process) with this switch.

    python tools/rd_quant_speed.py [--rounds 3] [--steps 3] [--warmup 1] [--textured] [--qp 27] [--out FILE]
    python tools/rd_quant_speed.py --tool on --once      # one untimed step, for a kernel profiler
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from subpel_satd_speed import main  # noqa: E402

if __name__ == "__main__":
    main("rd_quant", os.path.abspath(__file__))
