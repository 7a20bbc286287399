"""Constants of the matrix-core TB path of k_inter_recon (csrc/include/tv/tb_frag.h): the f16
fragment tables, expanded back to integer matrices by the core library, must be the HEVC DCT,
its row-subsampled 16 / 8 / 4-point matrices as 16x16 block-diagonal composites, and their
transposes; and the 32-bit quantiser with hoisted parameters must equal tv::quant_level for
every QP, every TB size and every |coef| below 2^17, the range the header's proof covers (the
forward transform of 8-bit video keeps |coef| <= 64548)."""
import ctypes as C

import numpy as np
import pytest

from thinvids_amd._native import core_lib

# H.265 (8.6.4.2): the 33 magnitudes of transMatrix indexed by ((2n + 1) k mod 128) folded to [0, 32]
MAG = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64,
       61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0]


def dct32():
    t = np.zeros((32, 32), np.int32)
    for k in range(32):
        for n in range(32):
            m = ((2 * n + 1) * k) % 128
            t[k, n] = MAG[m] if m <= 32 else -MAG[64 - m] if m < 64 else -MAG[m - 64] if m <= 96 else MAG[128 - m]
    return t


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def expand(which):
    lib = core_lib()
    out = np.full(1024, 12345, np.int32)
    side = lib.tv_tb_frag_expand(int(which), _ip(out))
    return side, out[:side * side].reshape(side, side)


def test_dct32_is_the_standard_matrix():
    t = dct32()
    assert t[0].tolist() == [64] * 32 and t[1, 0] == 90 and t[1, 31] == -90 and t[16, 0] == 64 and t[16, 1] == -64
    assert t[4, :4].tolist() == [89, 75, 50, 18] and t[2, :8].tolist() == [90, 87, 80, 70, 57, 43, 25, 9]
    assert t[8, :2].tolist() == [83, 36]


def test_t32_tables():
    t = dct32()
    side, a = expand(0)
    assert side == 32
    np.testing.assert_array_equal(a, t)
    side, b = expand(1)
    assert side == 32
    np.testing.assert_array_equal(b, t.T)


@pytest.mark.parametrize("s", [0, 1, 2])
def test_composites(s):
    n = 16 >> s
    tn = dct32()[::32 // n, :n]  # the N-point DCT: rows k * 32 / N, first N columns
    comp = np.zeros((16, 16), np.int32)
    for blk in range(16 // n):
        comp[blk * n:(blk + 1) * n, blk * n:(blk + 1) * n] = tn
    side, a = expand(2 + 2 * s)
    assert side == 16
    np.testing.assert_array_equal(a, comp)
    side, b = expand(3 + 2 * s)
    assert side == 16
    np.testing.assert_array_equal(b, comp.T)


def test_bad_table_index():
    assert expand(8)[0] == 0 and expand(-1)[0] == 0


@pytest.mark.parametrize("log2n", [2, 3, 4, 5])
def test_quant_fast_equals_quant_level(log2n):
    lib = core_lib()
    lim = (1 << 17) - 1
    assert lim >= 64548
    coef = np.arange(-lim, lim + 1, dtype=np.int32)
    ref, fast = np.empty_like(coef), np.empty_like(coef)
    for qp in range(52):
        lib.tv_quant_levels(_ip(coef), int(coef.size), qp, log2n, _ip(ref), _ip(fast))
        bad = np.nonzero(ref != fast)[0]
        assert bad.size == 0, f"qp {qp} log2N {log2n}: coef {coef[bad[0]]} -> {fast[bad[0]]}, want {ref[bad[0]]}"
        # the reference itself: a deadzone quantiser, odd-symmetric and monotonic
        assert ref[lim] == 0 and np.array_equal(ref, -ref[::-1]) and (np.diff(ref) >= 0).all()
