// rdq.h — rate-distortion quantisation of inter TBs (SeqConfig::rd_quant, tool bit 1024, off by
// default).  One definition for the golden encoder (cpu_encoder.cpp code_tb) and the GPU
// quantiser (k_inter_recon<kSdh, true>).  The tool changes no syntax: it only chooses other
// levels than the dead-zone quantiser, by J = D + lambda * R with a static rate model.
//
// Everything is a function of a TB's forward-transform coefficients, QP, log2 size and
// component, and every decision needs one thread per 4x4 coefficient group (CG) plus
// reductions over the TB's groups: nothing depends on another coefficient's decided level,
// only on the initial dead-zone levels l0 = quant_level(coef, inter) and on position.
//
// Units.  Distortion is in (1/256 quantiser step)^2, from d = sdh_delta(coef, l0) alone
// (-64 <= d < 192): a coefficient coded as magnitude a is off by d + 256 (|l0| - a).  Rates
// are in 1/16 bit (tv/rdq_tables.h, generated: P-slice contexts at slice QP kRdqTableQp).
// Lambda: the usual 0.57 * 2^((QP - 12) / 3) per bit of squared sample error, over step^2 = 2^((QP - 4) / 3), is 0.57 * 2^(-8/3) = 0.08977
// step^2 per bit whatever the QP; times 256^2 that is 5883 distortion units per bit, 367.7
// per 1/16 bit: 368.  The static rates are those of freshly initialised contexts and of
// excesses only, which underrate a real stream's; of x0.5 / x1 / x2 of the derived value the
// 640x360 sweep (profiles/rd_quant/README.md) is best at x2, so kRdqLambda = 736.
//
// Rate model: excess rates, all >= 0.  A zero level costs nothing; a magnitude a > 0 costs
//   Rx(a) = max(0, sig(1) - sig(0)) + 16 (sign) + greater1 / greater2 / remainder(a),
// sig by (component, DC group or not, the position's sigCtx pattern class 0..2 of H.265
// 9.3.4.2.5 with the coded flags of the right and lower groups taken from l0), the
// remainder the Rice-0 binarisation's length in closed form, Rx capped at kRdqRateCap.  A
// non-empty group strictly between the DC group and the last one costs
//   Cx = max(0, csbf(1) - csbf(0)) (context: right or lower group non-empty in l0),
// and a TB that ends in the group on group diagonal g costs kRdqLast[g], which does not
// decrease with g.  Because every term is an excess over "zero / empty / ends earlier" and
// the last term is monotone, lowering levels never raises a structural term: the model's J
// of the result is <= J of the dead-zone levels and of RDOQ-lite's (tests/test_rd_quant.py).
//
// Stage 1, per coefficient: the two integers bracketing |coef| / step are |l0| and, by the
//   sign of d, |l0| + 1 or |l0| - 1; the cheaper D + lambda Rx wins, ties keep l0.  A zero
//   stays zero: the tool makes no coefficient significant, so no group and no last
//   position appears that l0 did not have (raising zeros below a group's last level gave
//   more BD-rate but a larger stream at low QP; profiles/rd_quant/README.md).
// Stage 2, per CG other than the DC group: if all stage-1 magnitudes are <= 2 (eligible) and
//   the group as coded (+ Cx) costs more than all zero, it is emptied -- tentatively: that
//   holds if the group ends up before the TB's last group.
// Stage 3, per TB: the TB ends in the group k, in coding order, that minimises
//   sum over groups before k of their stage-2 J + the J of k as last group + lambda kRdqLast,
//   ties to the later k; groups after k are zeroed, and only eligible groups can be: k is not
//   before the last ineligible group.  Group k is taken as stage 1 left it, and its thread
//   ends it after the non-zero position that minimises its J (ties: the later one); an
//   ineligible group ends at its last non-zero level.  The DC group is never emptied.
// A final level therefore lies at most 3 below and 1 above l0.
//
// 32-bit ranges.  Per coefficient the error is at most 192 + 3 * 256 = 960 (the zeroing
// distortion of an ineligible group's coefficient is taken at min(|l0|, 3): such a group is
// never zeroed, the value only has to be the same wherever it cancels), so D <= 921600, and
// lambda * Rx <= kRdqLambda * kRdqRateCap; the static_assert below keeps a coefficient's
// D + lambda Rx under 2^21, so a sum over a TB's 1024 coefficients, any difference of two
// such sums, and those plus the group and last-position terms (64 * 255 + 65535 rate units)
// stay inside int32.  The cap applies to every candidate alike.
#pragma once
#include "tv/rdq_tables.h"
#include "tv/sdh.h"

namespace tv {

constexpr int kToolRdQuant = 1024;  // the tool's bit in the flags word (SeqConfig::set_flags)
constexpr int kRdqLambda = 736;     // distortion units per 1/16 bit
constexpr int kRdqRateCap = 511;    // 1/16 bit
static_assert(960 * 960 + kRdqLambda * kRdqRateCap < (1 << 21), "rdq: a coefficient's J fits 21 bits");

// ---- the rate table as packed constants: device code selects, it loads nothing
constexpr int rdq_excess(int one, int zero) { return one > zero ? one - zero : 0; }
constexpr uint32_t rdq_pack_sigx(int c, int dc) {  // byte v: class v
  uint32_t r = 0;
  for (int v = 0; v < 3; ++v) r |= (uint32_t)rdq_excess(kRdqSig[c][dc][v][1], kRdqSig[c][dc][v][0]) << (8 * v);
  return r;
}
constexpr uint32_t rdq_pack_levx(int c, int dc) {  // 10 bits each: magnitude 1, 2, >= 3 (without the remainder)
  return (uint32_t)kRdqG1[c][dc][0] | (uint32_t)(kRdqG1[c][dc][1] + kRdqG2[c][dc][0]) << 10 |
         (uint32_t)(kRdqG1[c][dc][1] + kRdqG2[c][dc][1]) << 20;
}
constexpr uint32_t rdq_pack_cx() {  // byte 2 c + ctx
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= (uint32_t)rdq_excess(kRdqCsbf[i >> 1][i & 1][1], kRdqCsbf[i >> 1][i & 1][0]) << (8 * i);
  return r;
}
constexpr unsigned long long rdq_pack_last(int c, int q) {  // 16 bits each: diagonals 4 q .. 4 q + 3
  unsigned long long r = 0;
  for (int i = 0; i < 4; ++i)
    if (4 * q + i < 15) r |= (unsigned long long)kRdqLast[c][4 * q + i] << (16 * i);
  return r;
}
constexpr uint32_t kRdqSigX00 = rdq_pack_sigx(0, 0), kRdqSigX01 = rdq_pack_sigx(0, 1), kRdqSigX10 = rdq_pack_sigx(1, 0),
                   kRdqSigX11 = rdq_pack_sigx(1, 1);
constexpr uint32_t kRdqLevX00 = rdq_pack_levx(0, 0), kRdqLevX01 = rdq_pack_levx(0, 1), kRdqLevX10 = rdq_pack_levx(1, 0),
                   kRdqLevX11 = rdq_pack_levx(1, 1);
constexpr uint32_t kRdqCx = rdq_pack_cx();
constexpr unsigned long long kRdqLast00 = rdq_pack_last(0, 0), kRdqLast01 = rdq_pack_last(0, 1), kRdqLast02 = rdq_pack_last(0, 2),
                             kRdqLast03 = rdq_pack_last(0, 3), kRdqLast10 = rdq_pack_last(1, 0), kRdqLast11 = rdq_pack_last(1, 1),
                             kRdqLast12 = rdq_pack_last(1, 2), kRdqLast13 = rdq_pack_last(1, 3);

TV_HD uint32_t rdq_sigx(int c, bool dc) { return c ? (dc ? kRdqSigX11 : kRdqSigX10) : (dc ? kRdqSigX01 : kRdqSigX00); }
TV_HD uint32_t rdq_levx(int c, bool dc) { return c ? (dc ? kRdqLevX11 : kRdqLevX10) : (dc ? kRdqLevX01 : kRdqLevX00); }
TV_HD int rdq_cx(int c, int ctx) { return (int)(kRdqCx >> (8 * (2 * c + ctx))) & 255; }
TV_HD int rdq_last_rate(int c, int diag) {
  const int q = diag >> 2;
  const unsigned long long k = c ? (q == 0 ? kRdqLast10 : q == 1 ? kRdqLast11 : q == 2 ? kRdqLast12 : kRdqLast13)
                                 : (q == 0 ? kRdqLast00 : q == 1 ? kRdqLast01 : q == 2 ? kRdqLast02 : kRdqLast03);
  return (int)(k >> (16 * (diag & 3))) & 0xffff;
}

// sigCtx pattern class (9.3.4.2.5) of position (x, y) of a group, pc = right + 2 * below
TV_HD int rdq_sig_class(int pc, int x, int y) {
  if (pc == 0) return x + y == 0 ? 2 : (x + y < 3 ? 1 : 0);
  if (pc == 1) return y == 0 ? 2 : (y == 1 ? 1 : 0);
  if (pc == 2) return x == 0 ? 2 : (x == 1 ? 1 : 0);
  return 2;
}
// excess rate of magnitude a > 0; sx = the class's sig excess, levx = rdq_levx
TV_HD int rdq_rate(int a, int sx, uint32_t levx) {
  int r = sx + 16 + (int)((levx >> (a >= 3 ? 20 : 10 * (a - 1))) & 1023);
  if (a >= 3) {  // coeff_abs_level_remaining of a - 3, Rice parameter 0: v + 1 bits below 4, else 4 + 2 floor(log2(v - 2))
    const int v = a - 3;
    r += 16 * (v < 4 ? v + 1 : 4 + 2 * (31 - __builtin_clz((unsigned)(v - 2))));
  }
  return tv_min(r, kRdqRateCap);
}
// position of group (gx, gy) in the up-right diagonal scan of s x s groups (coding order)
TV_HD int rdq_rank(int gx, int gy, int s) {
  const int d = gx + gy;
  if (d < s) return d * (d + 1) / 2 + gx;
  return s * s - (2 * s - 1 - d) * (2 * s - d) / 2 + gx - (d - s + 1);
}

// One coefficient, stage 1: a0 = |l0|, d its distance.  a1 the chosen magnitude, jc its
// D + lambda Rx, dz the distortion of zeroing it (at min(a0, 3)).
TV_HD void rdq_coef(int a0, int d, int sx, uint32_t levx, int lambda, int& a1, int& jc, int& dz) {
  const int j0 = d * d + (a0 ? lambda * rdq_rate(a0, sx, levx) : 0);
  a1 = a0, jc = j0;
  if (a0 > 0) {
    const int a = d >= 0 ? a0 + 1 : a0 - 1, e = d >= 0 ? d - 256 : d + 256;
    const int j = e * e + (a ? lambda * rdq_rate(a, sx, levx) : 0);
    if (j < j0) a1 = a, jc = j;
  }
  const int ez = d + 256 * tv_min(a0, 3);
  dz = ez * ez;
}

struct RdqGroup {
  int gfull;      // stage 2: J of the group before the last one, minus its all-zero distortion (0: empty or emptied)
  int glast;      // the same as the TB's last group, ended after scan position nlast
  int nlast;      // -1: the group is empty
  int maxmag;     // largest stage-1 magnitude (eligible: <= 2)
  bool emptied;   // stage 2 empties it if it is not the last group
};
// One group, stages 1 and 2 and the group's own part of stage 3.  mag0(n) / delta(n): |l0| and
// d of scan position n (diagonal scan); store(n, a): the stage-1 magnitude of a position that
// changes.  c: 0 luma, 1 chroma; dc: the TB's DC group; right / below: those groups hold
// a non-zero l0 (0 outside the TB).
template <class Mg, class Dl, class St>
TV_HD RdqGroup rdq_group(Mg mag0, Dl delta, St store, int c, bool dc, int right, int below, int lambda) {
  const uint32_t sigx = rdq_sigx(c, dc), levx = rdq_levx(c, dc);
  const int pc = right + 2 * below;
  int last0 = -1;
  for (int n = 0; n < 16; ++n)
    if (mag0(n)) last0 = n;
  RdqGroup g;
  g.nlast = -1, g.maxmag = 0, g.glast = 0, g.emptied = false;
  int acc = 0, best = 0x7fffffff, bestn = -1, lastn = -1, acclast = 0;
  for (int n = 0; n <= last0; ++n) {  // beyond last0 everything is and stays zero: J = the zeroing distortion
    const int p = sdh_scan_pos(0, n), a0 = mag0(n);
    const int sx = (int)(sigx >> (8 * rdq_sig_class(pc, p & 3, p >> 2))) & 255;
    int a1, jc, dz;
    rdq_coef(a0, delta(n), sx, levx, lambda, a1, jc, dz);
    if (a1 != a0) store(n, a1);
    acc += jc - dz;
    if (a1) {
      g.maxmag = tv_max(g.maxmag, a1);
      lastn = n, acclast = acc;
      if (acc <= best) best = acc, bestn = n;
    }
  }
  const bool eligible = g.maxmag <= 2;
  if (lastn >= 0) {
    g.nlast = eligible ? bestn : lastn;
    g.glast = eligible ? best : acclast;
  }
  g.gfull = lastn >= 0 ? acc + (dc ? 0 : lambda * rdq_cx(c, right | below)) : 0;
  if (!dc && eligible && g.gfull > 0) g.emptied = true, g.gfull = 0;
  return g;
}
// stage 3: J (minus the TB's all-zero distortion) of ending the TB in this group, `before`
// the sum of gfull over the groups before it
TV_HD int rdq_end_cost(const RdqGroup& g, int before, int c, int diag, int lambda) {
  return g.nlast < 0 ? before : before + g.glast + lambda * rdq_last_rate(c, diag);
}

// ---- the model on one TB, scalar (the golden encoder; the kernel spreads the same calls
// over one thread per group).  coef: N x N row-major; lev (pitch ls) receives the levels.
// The model's J of any levels for this TB, in 64 bits (the tests' yardstick; sums are exact)
inline long long rdq_cost(const int* coef, const int16_t* lev, int ls, int qp, int log2N, int c, int lambda = kRdqLambda) {
  const int N = 1 << log2N, s = N >> 2;
  bool f0[8][8] = {}, f[8][8] = {};
  int klast = -1;
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x) {
      if (quant_level(coef[y * N + x], qp, log2N, false)) f0[y >> 2][x >> 2] = true;
      if (lev[y * ls + x]) f[y >> 2][x >> 2] = true;
    }
  for (int gy = 0; gy < s; ++gy)
    for (int gx = 0; gx < s; ++gx)
      if (f[gy][gx]) klast = tv_max(klast, rdq_rank(gx, gy, s));
  long long J = 0;
  for (int gy = 0; gy < s; ++gy)
    for (int gx = 0; gx < s; ++gx) {
      const int rank = rdq_rank(gx, gy, s), right = gx + 1 < s && f0[gy][gx + 1], below = gy + 1 < s && f0[gy + 1][gx];
      const bool dc = rank == 0;
      for (int n = 0; n < 16; ++n) {
        const int p = sdh_scan_pos(0, n), i = (gy * 4 + (p >> 2)) * N + gx * 4 + (p & 3);
        const int l0 = quant_level(coef[i], qp, log2N, false), a = tv_abs(lev[(i >> log2N) * ls + (i & (N - 1))]);
        const long long e = sdh_delta(coef[i], l0, qp, log2N) + 256LL * (tv_abs(l0) - a);
        J += e * e;
        if (a) J += (long long)lambda * rdq_rate(a, (int)(rdq_sigx(c, dc) >> (8 * rdq_sig_class(right + 2 * below, p & 3, p >> 2))) & 255, rdq_levx(c, dc));
      }
      if (f[gy][gx] && rank > 0 && rank < klast) J += (long long)lambda * rdq_cx(c, right | below);
      if (rank == klast) J += (long long)lambda * rdq_last_rate(c, gx + gy);
    }
  return J;
}

// J, if given, receives the model's J after each of the three stages.
inline void rdq_tb(const int* coef, int qp, int log2N, int c, int16_t* lev, int ls, long long* J = nullptr,
                   int lambda = kRdqLambda) {
  const int N = 1 << log2N, s = N >> 2;
  int a0[32 * 32], dl[32 * 32];
  bool f0[8][8] = {};
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x) {
      const int l = quant_level(coef[y * N + x], qp, log2N, false);
      lev[y * ls + x] = (int16_t)l;
      a0[y * N + x] = tv_abs(l);
      dl[y * N + x] = sdh_delta(coef[y * N + x], l, qp, log2N);
      if (l) f0[y >> 2][x >> 2] = true;
    }
  RdqGroup G[64];
  int gxy[64];
  auto at = [&](int gx, int gy, int n) {
    const int p = sdh_scan_pos(0, n);
    return (gy * 4 + (p >> 2)) * N + gx * 4 + (p & 3);
  };
  auto put = [&](int i, int a) { lev[(i >> log2N) * ls + (i & (N - 1))] = (int16_t)(coef[i] < 0 ? -a : a); };
  for (int gy = 0; gy < s; ++gy)
    for (int gx = 0; gx < s; ++gx) {
      const int rank = rdq_rank(gx, gy, s);
      gxy[rank] = gx | gy << 3;
      G[rank] = rdq_group([&](int n) { return a0[at(gx, gy, n)]; }, [&](int n) { return dl[at(gx, gy, n)]; },
                          [&](int n, int a) { put(at(gx, gy, n), a); }, c, rank == 0, gx + 1 < s && f0[gy][gx + 1],
                          gy + 1 < s && f0[gy + 1][gx], lambda);
    }
  if (J) {
    J[0] = rdq_cost(coef, lev, ls, qp, log2N, c, lambda);
    int16_t t[32 * 32];
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) {
        const RdqGroup& g = G[rdq_rank(x >> 2, y >> 2, s)];
        t[y * N + x] = g.emptied ? (int16_t)0 : lev[y * ls + x];
      }
    J[1] = rdq_cost(coef, t, N, qp, log2N, c, lambda);
  }
  int kmin = 0, before = 0, best = 0x7fffffff, k = 0;
  for (int r = 0; r < s * s; ++r)
    if (G[r].maxmag > 2) kmin = r;
  for (int r = 0; r < s * s; ++r) {
    if ((G[r].nlast >= 0 || r == 0) && r >= kmin) {
      const int e = rdq_end_cost(G[r], before, c, (gxy[r] & 7) + (gxy[r] >> 3), lambda);
      if (e <= best) best = e, k = r;
    }
    before += G[r].gfull;
  }
  for (int r = 0; r < s * s; ++r) {
    const int gx = gxy[r] & 7, gy = gxy[r] >> 3;
    const int keep = r > k ? -1 : (r == k ? G[r].nlast : (G[r].emptied ? -1 : 15));  // last scan position kept
    for (int n = keep + 1; n < 16; ++n) put(at(gx, gy, n), 0);
  }
  if (J) J[2] = rdq_cost(coef, lev, ls, qp, log2N, c, lambda);
}

}  // namespace tv
