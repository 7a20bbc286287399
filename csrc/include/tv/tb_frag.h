// tb_frag.h — constants of the matrix-core TB path of k_inter_recon (csrc/gpu/k_inter.hip):
// the DCT operands as ready f16 MFMA fragments, and the quantiser with its per-TB-size
// parameters hoisted out of the per-coefficient code.  Generated from kDct32 at compile time;
// shared with the host so tests can expand the tables again (capi.cpp).
#pragma once
#include <cstdint>

#include "hevc_defs.h"

namespace tv {

// IEEE binary16 bit pattern of an integer |v| < 2048 (exact), and back.
constexpr uint16_t f16_bits_of_int(int v) {
  if (v == 0) return 0;
  const unsigned s = v < 0 ? 0x8000u : 0u, a = (unsigned)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0) ++e;
  return (uint16_t)(s | (unsigned)(e + 15) << 10 | ((a << (10 - e)) & 0x3ffu));
}
constexpr int int_of_f16_bits(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 0x3ff;
  if (e == 0) return 0;  // the tables hold no subnormals
  const int a = e >= 25 ? (0x400 | m) << (e - 25) : (0x400 | m) >> (25 - e);
  return (h & 0x8000) ? -a : a;
}

// A lane of v_mfma_f32_16x16x32_f16 (16x16x16f16) holds, of the row (A) or column (B) n =
// lane & 15 of its operand, the K-run 8 * (lane >> 4) .. + 7 (4 * (lane >> 4) .. + 3).  Each
// table below is indexed [n][k], so that run is one aligned 16-byte (8-byte) read:
//   t32[0][n][k] = T32[n][k]    A of the forward stage 1 (T * R), B of stage 2 (A * T^T)
//   t32[1][n][k] = T32[k][n]    A of the inverse stage 1 (T^T * D), B of stage 2 (G * T)
//   c16[s][o]                   the same pair for the 16x16 block-diagonal composite of
//                               16 >> s point DCTs (s = 0, 1, 2: TB size 16, 8, 4)
struct TbFragTables {
  uint16_t t32[2][32][32];
  uint16_t c16[3][2][16][16];
};
constexpr int tb_comp16(int log2N, int r, int k) {
  const int m = (1 << log2N) - 1;
  return (r >> log2N) == (k >> log2N) ? kDct32.m[(r & m) << (5 - log2N)][k & m] : 0;
}
constexpr TbFragTables make_tb_frag() {
  TbFragTables t{};
  for (int n = 0; n < 32; ++n)
    for (int k = 0; k < 32; ++k) {
      t.t32[0][n][k] = f16_bits_of_int(kDct32.m[n][k]);
      t.t32[1][n][k] = f16_bits_of_int(kDct32.m[k][n]);
    }
  for (int s = 0; s < 3; ++s)
    for (int n = 0; n < 16; ++n)
      for (int k = 0; k < 16; ++k) {
        t.c16[s][0][n][k] = f16_bits_of_int(tb_comp16(4 - s, n, k));
        t.c16[s][1][n][k] = f16_bits_of_int(tb_comp16(4 - s, k, n));
      }
  return t;
}
static_assert(sizeof(TbFragTables) == 7168 && sizeof(TbFragTables) % 16 == 0, "fragment tables: 16-byte chunks");

// tv::quant_level (inter rounding) with everything that depends only on (qp, log2N) computed
// once, and the product in 32 bits.  The forward transform bounds its own output: residuals
// are |r| <= 255 and |T| <= 90, so stage 1 gives |tmp| <= 90 * N * 255 >> (log2N - 1) = 45900
// and stage 2 |coef| <= (90 * N * 45900 >> (log2N + 6)) + 1 = 64548 for every N.  For any
// |coef| < 2^17: |coef| * scale <= 131071 * 26214 < 3.44e9 and add = 128 << (qbits - 9) <=
// 2^25 (qbits <= 14 + 8 + 5), so the sum is < 2^32: the unsigned 32-bit form equals the
// 64-bit one (tests/test_dct_fragments.py compares them over that whole range).
struct QuantParams {
  uint32_t scale, add;
  int qbits;
};
TV_HD QuantParams quant_params(int qp, int log2N) {
  QuantParams q;
  q.qbits = 14 + qp / 6 + (15 - 8 - log2N);
  q.add = 128u << (q.qbits - 9);
  q.scale = (uint32_t)quant_scale(qp);
  return q;
}
TV_HD int quant_fast(int coef, const QuantParams& q) {
  int l = (int)(((uint32_t)tv_abs(coef) * q.scale + q.add) >> q.qbits);
  if (l > 32767) l = 32767;
  return coef < 0 ? -l : l;
}
// tv::sdh_delta (tv/sdh.h) of the level quant_fast or quant_level gave, in 32 bits: the level is
// not clamped (|coef| <= 64548 gives at most 25819), so |coef| * scale - (|level| << qbits)
// lies in [-add, 2^qbits - add), |.| < 2^27, and the wrapped unsigned difference is that value
// (-64 <= d < 192 with the inter rounding, -86 <= d < 171 with the intra one;
// tests/test_sign_hiding.py compares the two forms).
TV_HD int sdh_delta_fast(int coef, int level, const QuantParams& q) {
  const uint32_t e = (uint32_t)tv_abs(coef) * q.scale - ((uint32_t)tv_abs(level) << q.qbits);
  return (int)e >> (q.qbits - 8);
}

}  // namespace tv
