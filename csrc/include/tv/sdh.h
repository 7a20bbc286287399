// sdh.h — sign data hiding (sign_data_hiding_enabled_flag, H.265 7.3.8.11 / 7.4.9.11), the
// encoder side: SeqConfig::sign_hiding, flag bit 512, off by default.  One definition for the
// golden encoder (cpu_encoder.cpp code_tb) and both GPU quantisers (wave_tb.h, k_inter_recon).
//
// A 4x4 coefficient group (CG) whose first and last non-zero levels in the TB's own 4x4 scan
// lie more than 3 positions apart codes no sign for the first one: the decoder takes it from
// the parity of the group's sum of magnitudes (odd = negative).  The encoder makes the parity
// fit by changing one magnitude of the group by one, the change that costs the least
// distortion (the HM's rule without its rate terms).  It runs on final levels: after
// quantisation, RDOQ-lite trimming and the lone-level TB drop, and nothing is dropped after it.
// A hidden group holds at least two levels and a -1 never touches a first level of 1, so no
// group empties, no cbf changes and no group becomes non-zero that was zero.
#pragma once
#include "tv/hevc_defs.h"

namespace tv {

// Distance of |coef| from the reconstruction point of |level| in 1/256 of a quantiser step
// (rounded down): > 0 the coefficient lies above the level.  The quantiser's rounding offset
// does not enter.  quant_level rounds by 171/512 (intra) or 1/4 (inter) of a step, so an
// unclamped level gives -86 <= d < 171 (intra) and -64 <= d < 192 (inter).
TV_HD int sdh_delta(int coef, int level, int qp, int log2N) {
  const int qbits = 14 + qp / 6 + (15 - 8 - log2N);
  const long long e = (long long)tv_abs(coef) * quant_scale(qp) - ((long long)tv_abs(level) << qbits);
  return (int)(e >> (qbits - 8));
}

// x | y << 2 of scan position n of a 4x4 group (coef_pos_in_sb), from the scan packed four
// bits per position: device code reads no table
constexpr unsigned long long sdh_pack_scan(const uint8_t (&s)[16]) {
  unsigned long long v = 0;
  for (int n = 0; n < 16; ++n) v |= (unsigned long long)s[n] << (4 * n);
  return v;
}
constexpr unsigned long long kSdhScanDiag = sdh_pack_scan(kScanDiag4x4), kSdhScanHor = sdh_pack_scan(kScanHor4x4),
                             kSdhScanVer = sdh_pack_scan(kScanVer4x4);
TV_HD int sdh_scan_pos(int scanIdx, int n) {
  const unsigned long long k = scanIdx == 0 ? kSdhScanDiag : (scanIdx == 1 ? kSdhScanHor : kSdhScanVer);
  return (int)(k >> (4 * n)) & 15;
}

// One CG.  level(n) / delta(n) / cneg(n): the level, sdh_delta and "coefficient < 0" of scan
// position n (0..15, the TB's true scan: diagonal / horizontal / vertical).  Returns false if
// nothing changes (no sign hidden, or the parity already fits); otherwise position `pos`
// takes the value `value`.
template <class Lv, class Dl, class Ng>
TV_HD bool sdh_adjust(Lv level, Dl delta, Ng cneg, int& pos, int& value) {
  int first = -1, last = -1, sum = 0;
  for (int n = 0; n < 16; ++n) {
    const int l = level(n);
    if (!l) continue;
    if (first < 0) first = n;
    last = n;
    sum += tv_abs(l);
  }
  if (first < 0 || last - first <= 3) return false;
  const bool neg = level(first) < 0;
  if (((sum & 1) != 0) == neg) return false;
  int best = 0x7fffffff, bchg = 0;
  pos = -1;
  for (int n = last; n >= 0; --n) {  // ties: the highest n
    const int l = level(n), d = delta(n);
    int cost, chg;
    if (l != 0) {
      if (d > 0) {
        cost = -d;
        chg = 1;
      } else {
        if (n == first && tv_abs(l) == 1) continue;  // would move the first position
        cost = d;
        chg = -1;
      }
    } else {
      if (n < first && cneg(n) != neg) continue;  // a new first level must carry the hidden sign
      cost = -d;
      chg = 1;
    }
    if (cost < best) {
      best = cost;
      bchg = chg;
      pos = n;
    }
  }
  const int l = level(pos);
  int a = tv_abs(l);
  a += a == 32767 ? -1 : bchg;
  value = l != 0 ? (l < 0 ? -a : a) : (cneg(pos) ? -1 : 1);
  return true;
}

// Does the sign of the first non-zero level of a CG with significance mask m (bit n = scan
// position n, m != 0) go uncoded?
TV_HD bool sdh_hidden(unsigned m) { return (31 - __builtin_clz(m)) - __builtin_ctz(m) > 3; }

}  // namespace tv
