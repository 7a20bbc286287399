"""Generate csrc/include/tv/rdq_tables.h: the static bin rates of the rate-distortion
quantiser (tv/rdq.h), in 1/16 bit.

Nothing is typed by hand.  The context-initialisation values are read out of
csrc/include/tv/cabac.h (the tables the encoder and the decoder oracle initialise their
contexts from) and the LPS ranges out of csrc/core/hevc_writer.cpp (kRangeTabLps, the table
the arithmetic coder codes with).  A context is taken in the state 9.3.2.2 gives it for a P
slice (initType 1) at slice QP `QP`; the probability of its LPS is the mean over the four
range quarters of kRangeTabLps[state][q] / (288 + 64 q), the middle of the quarter; the rate
of a bin is -log2 of its probability.  Where the rate model (tv/rdq.h) merges several
contexts into one class the class takes the mean of their rates.

    python tools/hevc_rate_tables_gen.py            # rewrite the header
    python tools/hevc_rate_tables_gen.py --stdout   # print it instead
"""
from __future__ import annotations

import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "csrc", "include", "tv", "rdq_tables.h")
QP = 27        # the slice QP the states are taken at
INIT_TYPE = 1  # P slices


def _ints(s: str) -> list:
    return [int(v) for v in re.findall(r"\d+", s)]


def _read_tables():
    cabac = open(os.path.join(ROOT, "csrc", "include", "tv", "cabac.h")).read()
    writer = open(os.path.join(ROOT, "csrc", "core", "hevc_writer.cpp")).read()
    init = {}
    for name in ("CTX_CSBF", "CTX_SIG", "CTX_G1", "CTX_G2"):
        m = re.search(r"set\(" + name + r",\s*\d+,\s*\{([^}]*)\},\s*\{([^}]*)\},\s*\{([^}]*)\}\)", cabac)
        init[name] = _ints(m.group(1 + INIT_TYPE))
    init["CTX_LAST"] = _ints(re.search(r"last%d = \{([^}]*)\}" % INIT_TYPE, cabac).group(1))
    lps = _ints(re.search(r"kRangeTabLps\[64\]\[4\] = \{(.*?)\};", writer, re.S).group(1))
    assert len(lps) == 256 and len(init["CTX_SIG"]) == 44 and len(init["CTX_G1"]) == 24
    return init, [lps[4 * s:4 * s + 4] for s in range(64)]


INIT, LPS = _read_tables()


def state_of(init_value: int):
    """9.3.2.2: (pStateIdx, valMps) of a context at slice QP `QP`."""
    m, n = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
    pre = min(126, max(1, ((m * min(51, max(0, QP))) >> 4) + n))
    return (63 - pre, 0) if pre <= 63 else (pre - 64, 1)


def bits(init_value: int, b: int) -> float:
    s, mps = state_of(init_value)
    p = sum(LPS[s][q] / (288 + 64 * q) for q in range(4)) / 4
    return -math.log2(1 - p if b == mps else p)


def q16(x: float) -> int:
    return max(1, int(round(16 * x)))


def mean_rate(name: str, ctxs, b: int) -> int:
    return q16(sum(bits(INIT[name][c], b) for c in ctxs) / len(ctxs))


# prefix of last_sig_coeff_{x,y}_prefix per position (9.3.3.x groupIdx)
GROUP_IDX = [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7] + [8] * 8 + [9] * 8


def last_bits(pos: int, log2n: int, cidx: int) -> float:
    prefix = GROUP_IDX[pos]
    if cidx == 0:
        off, shift = 3 * (log2n - 2) + ((log2n - 1) >> 2), (log2n + 1) >> 2
    else:
        off, shift = 15, log2n - 2
    r = sum(bits(INIT["CTX_LAST"][off + (i >> shift)], 1) for i in range(prefix))
    if prefix < 2 * log2n - 1:
        r += bits(INIT["CTX_LAST"][off + (prefix >> shift)], 0)
    return r + ((prefix >> 1) - 1 if prefix > 3 else 0)


def tables():
    t = {}
    # sig_coeff_flag [component][DC group][pattern class 0..2][bin]: luma 8x8 (sizeOff 9) and
    # 16x16 / 32x32 (21) TBs, + 3 outside the DC group; chroma (+27) 8x8 (9) and 16x16 (12)
    t["kRdqSig"] = [[[[mean_rate("CTX_SIG", ([9 + o + v, 21 + o + v] if c == 0 else [27 + 9 + v, 27 + 12 + v]), b)
                       for b in range(2)] for v in range(3)] for o in (3, 0)] for c in range(2)]  # o = 0: the DC group
    # coeff_abs_level_greater1 [component][DC group][bin]: the four greater1Ctx of the ctxSet
    sets = lambda c, dc: 0 if (c or dc) else 2  # noqa: E731
    t["kRdqG1"] = [[[mean_rate("CTX_G1", [4 * sets(c, dc) + 16 * c + k for k in range(4)], b) for b in range(2)]
                    for dc in range(2)] for c in range(2)]
    t["kRdqG2"] = [[[mean_rate("CTX_G2", [sets(c, dc) + 4 * c], b) for b in range(2)] for dc in range(2)] for c in range(2)]
    # coded_sub_block_flag [component][right | below coded][bin]
    t["kRdqCsbf"] = [[[mean_rate("CTX_CSBF", [k + 2 * c], b) for b in range(2)] for k in range(2)] for c in range(2)]
    # last significant position by group diagonal: the position in the middle of the groups'
    # diagonal, (2 d + 1, 2 d + 2), of a 32x32 luma / 16x16 chroma TB; non-decreasing (rdq.h)
    last = []
    for c in range(2):
        row, log2n = [], 5 - c
        for d in range(15):
            m = (1 << log2n) - 1
            v = q16(last_bits(min(m, 2 * d + 1), log2n, c) + last_bits(min(m, 2 * d + 2), log2n, c))
            row.append(max(v, row[-1]) if row else v)
        last.append(row)
    t["kRdqLast"] = last
    return t


def _fmt(v) -> str:
    return "{" + ", ".join(_fmt(x) for x in v) + "}" if isinstance(v, list) else str(v)


def render() -> str:
    dims = {"kRdqSig": "[2][2][3][2]", "kRdqG1": "[2][2][2]", "kRdqG2": "[2][2][2]", "kRdqCsbf": "[2][2][2]",
            "kRdqLast": "[2][15]"}
    doc = {"kRdqSig": "sig_coeff_flag [component][DC group][sigCtx pattern class][bin]",
           "kRdqG1": "coeff_abs_level_greater1_flag [component][DC group][bin]",
           "kRdqG2": "coeff_abs_level_greater2_flag [component][DC group][bin]",
           "kRdqCsbf": "coded_sub_block_flag [component][right or lower group coded][bin]",
           "kRdqLast": "last_sig_coeff x + y, prefix and suffix, [component][group diagonal]; non-decreasing"}
    out = ["// rdq_tables.h -- static bin rates of tv/rdq.h in 1/16 bit.  Generated by",
           "// tools/hevc_rate_tables_gen.py from the context-initialisation values of tv/cabac.h and",
           "// kRangeTabLps (hevc_writer.cpp): P-slice contexts at slice QP %d.  Do not edit." % QP,
           "#pragma once", "", "namespace tv {", "", "constexpr int kRdqTableQp = %d;" % QP]
    for k, v in tables().items():
        out.append("// " + doc[k])
        out.append("constexpr unsigned short %s%s = %s;" % (k, dims[k], _fmt(v)))
    out += ["", "}  // namespace tv", ""]
    return "\n".join(out)


if __name__ == "__main__":
    if "--stdout" in sys.argv:
        sys.stdout.write(render())
    else:
        with open(OUT, "w") as f:
            f.write(render())
