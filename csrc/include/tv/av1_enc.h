// av1_enc.h — AV1 encoder primitives shared (TV_HD) by the C++ golden encoder / decoder
// oracle (csrc/core/av1_codec.cpp) and the gfx950 encode kernels (csrc/gpu/k_av1_enc.hip),
// so GPU and CPU reconstructions are identical bit for bit (BASELINE
// config #4 "4K60 AV1 with CDEF + loop-restoration HIP kernels").
//
// Coding structure (a GPU-friendly subset of AV1 Main, 8-bit 4:2:0):
//   * 64x64 superblocks, coded size padded to a multiple of 16 (render_size = display size);
//     every superblock splits to 16x16 coding blocks (PARTITION_SPLIT / split_or_* at edges);
//   * TX_MODE_LARGEST: one 16x16 luma and two 8x8 chroma transforms per block, reduced_tx_set;
//     opt-in (kToolTxSplit, off by default): inter frames signal TX_MODE_SELECT and a non-skip
//     inter block may code its luma as four 8x8 transforms ("transform split" below);
//   * key frames: intra modes DC / V / H / SMOOTH / SMOOTH_V / SMOOTH_H / PAETH searched (D113 /
//     D135 / D157 predicted and decodable too); all read no above-right / below-left samples,
//     so the I-frame wavefront is a plain diagonal; angle delta 0; intra edge filter / filter
//     intra / palette off; opt-in (kToolCfl, off by default): chroma from luma as an eighth
//     chroma mode of every intra block ("chroma from luma" below), which reads only the
//     block's own reconstructed luma, so the wavefront is unchanged; opt-in (kToolDirIntra,
//     off by default): every directional angle strictly between 90 and 180 degrees (V / H /
//     D113 / D135 / D157 with angle deltas, 34 (mode, delta) candidates for luma and for
//     chroma) searched with mode rates read from the default CDFs ("directional intra"
//     below); those angles read nothing right of above[N-1] or below left[N-1], so the
//     wavefront is unchanged;
//   * inter frames: one reference (LAST = previous frame), quarter-pel motion, EIGHTTAP
//     (regular) filters; the NEWMV / NEARESTMV / NEARMV / GLOBALMV choice is made by the
//     syntax writer from the spatial MV stack (the mode does not change the reconstruction);
//     opt-in (kToolIntraInInter, off by default): 16x16 intra blocks where the reference has
//     no match ("intra blocks in inter frames" below);
//   * deblocking with frame levels, CDEF (8 presets per frame, 64x64 cdef_idx).
//
// Every normative table (q lookup, default CDFs) is the specification's (tv/av1_tables.h)
// and the inverse transforms are the specification's (tv/av1_itx.h): streams decode with
// any conformant AV1 decoder (tests/test_av1_conformance.py decodes them with dav1d).
#pragma once
#include <cstdint>

#include "tv/av1_tables.h"
#include "tv/hevc_defs.h"  // TV_HD, clip3, tv_abs

namespace tv {
namespace av1 {

constexpr int kBlk = 16;   // coding block (luma)
constexpr int kCBlk = 8;   // chroma block
constexpr int kSb = 64;    // superblock
constexpr int kMaxPresets = 8;

// intra modes (AV1 numbering)
enum : int { DC_PRED = 0, V_PRED = 1, H_PRED = 2, D135_PRED = 4, D113_PRED = 5, D157_PRED = 6, SMOOTH_PRED = 9,
             SMOOTH_V_PRED = 10, SMOOTH_H_PRED = 11, PAETH_PRED = 12 };
// inter modes (YModes of inter blocks)
enum : int { NEARESTMV = 13, NEARMV = 14, GLOBALMV = 15, NEWMV = 16 };
// Mode search candidates.  D113 / D135 / D157 are predicted exactly (intra_dir_px; dav1d
// decodes them bit-exactly) but the SATD-driven search picked them where they cost more than
// they saved: key-frame-only clips at QP 27 +1.0 % bytes at -0.09 dB even with a 10-bit mode
// penalty (profiles/README.md, round 4), so the search keeps the seven non-directional-delta
// modes; the opt-in rate-aware decision is "directional intra" below (kToolDirIntra).
constexpr int kNumIntraCand = 7;
TV_HD int intra_cand(int i) {
  constexpr int8_t m[kNumIntraCand] = {DC_PRED, V_PRED, H_PRED, SMOOTH_PRED, SMOOTH_V_PRED, SMOOTH_H_PRED, PAETH_PRED};
  return m[i];
}
// 1-D transform types (av1_txfm.h: 0 DCT, 1 ADST) of the chroma intra transform
// (Mode_To_Txfm: V -> ADST_DCT, H -> DCT_ADST, SMOOTH / PAETH -> ADST_ADST, ...): vertical
// (column) type in bit 0, horizontal (row) type in bit 1.
TV_HD int uv_txtype(int uv_mode) {
  switch (uv_mode) {
    case V_PRED: case D113_PRED: case SMOOTH_V_PRED: return 1;      // ADST_DCT
    case H_PRED: case D157_PRED: case SMOOTH_H_PRED: return 2;      // DCT_ADST
    case D135_PRED: case SMOOTH_PRED: case PAETH_PRED: return 3;    // ADST_ADST
    default: return 0;                                      // DCT_DCT (DC_PRED, UV_CFL_PRED)
  }
}

// ---------------------------------------------------------------- quantizer ------------
// Dc_Qlookup / Ac_Qlookup (8-bit) of the specification (tv/av1_tables.h)
TV_HD int ac_q(int q) { return tab::kAcQLookup[clip3(0, 255, q)]; }
TV_HD int dc_q(int q) { return tab::kDcQLookup[clip3(0, 255, q)]; }
// encoder quantisation rounding (1/128 of the step): 1/3 for intra blocks; inter frames
// choose per frame (inter_rounding).  With the refined motion field a clean source leaves a
// small, coherent residual that is worth keeping (1/3: -2.3 % BD-rate against 1/6 on the
// smooth bench content), while sensor grain is not (1/6: -5.5 % on the textured variant).
// The frame's mean luma SATD per pixel at its final MVs tells them apart: 1.8-3.5 on the
// smooth content, 6.3-10 on the textured one at QP 22..37 (tools/rd_curve.py --codec av1).
constexpr int kRndIntra = 43, kRndInter = 43, kRndInterNoisy = 21;
constexpr int kNoisySatdPerPx = 5;
TV_HD int inter_rounding(long long satd_sum, int W, int H) {
  return satd_sum > (long long)kNoisySatdPerPx * W * H ? kRndInterNoisy : kRndInter;
}
TV_HD int quant(int c, int q, int rnd) {
  const int a = c < 0 ? -c : c;
  const int l = (a + ((q * rnd) >> 7)) / q;
  return c < 0 ? -l : l;
}
// AV1 dequantisation (7.12.3, dqDenom 0 for <= 16x16): |l * q| & 0xFFFFFF, clamp to int16
TV_HD int dequant(int l, int q) {
  if (!l) return 0;
  const long long a = ((long long)(l < 0 ? -l : l) * q) & 0xFFFFFF;
  const int v = (int)(l < 0 ? -a : a);
  return clip3(-32768, 32767, v);
}
// frame loop-filter level from the AC step (libaom-style linear guess), 0..63
TV_HD int lf_level_for_q(int q) {
  const long long v = ((long long)ac_q(q) * 20723 + 1015158) >> 18;
  return (int)clip3(0LL, 63LL, v);
}
// lambda for SAD/SATD-domain decisions (bits -> distortion units, x16)
TV_HD int lambda16(int q) { return tv_max(16, (ac_q(q) * 16 * 3) / 32); }

// Coefficient scan (zigzag over anti-diagonals, odd diagonals top-down): raster position of
// scan index k for N x N, written to out[0..N*N).  The syntax writer's scan and the order
// of the GPU's eob-truncated level packing (k_av1e_tb_pack).
TV_HD void zigzag_scan(int N, int16_t* out) {
  int k = 0;
  for (int s = 0; s <= 2 * N - 2; ++s) {
    const int lo = s - N + 1 > 0 ? s - N + 1 : 0, hi = s < N - 1 ? s : N - 1;
    if (s & 1)
      for (int r = lo; r <= hi; ++r) out[k++] = (int16_t)(r * N + (s - r));
    else
      for (int r = hi; r >= lo; --r) out[k++] = (int16_t)(r * N + (s - r));
  }
}

// ------------------------------------------------------------------ intra prediction ----
// Smooth weights (Sm_Weights_Tx_*)
TV_HD int sm_weight(int N, int i) {
  constexpr uint8_t w8[8] = {255, 197, 146, 105, 73, 50, 37, 32};
  constexpr uint8_t w16[16] = {255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16};
  return N == 8 ? w8[i] : w16[i];
}

// Edge samples of an N x N block at (x, y) of a plane (7.11.2 without the intra edge
// filter): above[0..N-1], left[0..N-1], top-left.  get(x, y) reads reconstructed samples.
struct IntraEdge {
  int above[16], left[16], tl;
  bool have_a, have_l;
};
template <class G>
TV_HD void intra_edges(G get, int x, int y, int N, IntraEdge& e) {
  e.have_a = y > 0;
  e.have_l = x > 0;
  for (int i = 0; i < N; ++i) {
    if (e.have_a) e.above[i] = get(x + i, y - 1);
    else if (e.have_l) e.above[i] = get(x - 1, y);
    else e.above[i] = 127;
    if (e.have_l) e.left[i] = get(x - 1, y + i);
    else if (e.have_a) e.left[i] = get(x, y - 1);
    else e.left[i] = 129;
  }
  if (e.have_a && e.have_l) e.tl = get(x - 1, y - 1);
  else if (e.have_a) e.tl = get(x, y - 1);
  else if (e.have_l) e.tl = get(x - 1, y);
  else e.tl = 128;
}

TV_HD int intra_dc(const IntraEdge& e, int N) {
  const int lg = N == 8 ? 3 : 4;
  int s = 0;
  if (e.have_a && e.have_l) {
    for (int i = 0; i < N; ++i) s += e.above[i] + e.left[i];
    return (s + N) >> (lg + 1);
  }
  if (e.have_a) {
    for (int i = 0; i < N; ++i) s += e.above[i];
    return (s + (N >> 1)) >> lg;
  }
  if (e.have_l) {
    for (int i = 0; i < N; ++i) s += e.left[i];
    return (s + (N >> 1)) >> lg;
  }
  return 128;
}

// Directional prediction for 90 < pAngle < 180 (7.11.2.4; no edge filter, no upsampling):
// the above row at x = j - (i + 1) * dx / 64 while that lands at or right of the corner
// (index -1 = top-left), else the left column at y = i - (j + 1) * dy / 64; linear
// interpolation in 1/32 steps.  dx = Dr_Intra_Derivative[180 - pAngle], dy = [pAngle - 90].
// Every read is inside above[-1 .. N-1] / left[-1 .. N-1]: no above-right, no below-left.
TV_HD int intra_dir_px(const IntraEdge& e, int i, int j, int dx, int dy) {
  int idx = (j << 6) - (i + 1) * dx;
  int base = idx >> 6;
  if (base >= -1) {
    const int shift = (idx >> 1) & 0x1f;
    const int a0 = base < 0 ? e.tl : e.above[base], a1 = e.above[base + 1];
    return (a0 * (32 - shift) + a1 * shift + 16) >> 5;
  }
  idx = (i << 6) - (j + 1) * dy;
  base = idx >> 6;
  const int shift = (idx >> 1) & 0x1f;
  const int l0 = base < 0 ? e.tl : e.left[base], l1 = e.left[base + 1];
  return (l0 * (32 - shift) + l1 * shift + 16) >> 5;
}

// predicted sample (row i, col j); dc = intra_dc(e, N) precomputed for DC_PRED
TV_HD int intra_pred_px(int mode, const IntraEdge& e, int N, int i, int j, int dc) {
  switch (mode) {
    case D113_PRED: return intra_dir_px(e, i, j, 27, 151);  // Dr_Intra_Derivative[67], [23]
    case D135_PRED: return intra_dir_px(e, i, j, 64, 64);   // [45], [45]
    case D157_PRED: return intra_dir_px(e, i, j, 151, 27);  // [23], [67]
    case V_PRED: return e.above[j];
    case H_PRED: return e.left[i];
    case SMOOTH_PRED: {
      const int wy = sm_weight(N, i), wx = sm_weight(N, j);
      const int s = wy * e.above[j] + (256 - wy) * e.left[N - 1] + wx * e.left[i] + (256 - wx) * e.above[N - 1];
      return (s + 256) >> 9;
    }
    case SMOOTH_V_PRED: {
      const int wy = sm_weight(N, i);
      return (wy * e.above[j] + (256 - wy) * e.left[N - 1] + 128) >> 8;
    }
    case SMOOTH_H_PRED: {
      const int wx = sm_weight(N, j);
      return (wx * e.left[i] + (256 - wx) * e.above[N - 1] + 128) >> 8;
    }
    case PAETH_PRED: {
      const int base = e.above[j] + e.left[i] - e.tl;
      const int pl = tv_abs(base - e.left[i]), pa = tv_abs(base - e.above[j]), pt = tv_abs(base - e.tl);
      if (pl <= pa && pl <= pt) return e.left[i];
      if (pa <= pt) return e.above[j];
      return e.tl;
    }
    default: return dc;
  }
}

// ------------------------------------------------------------------ inter prediction ----
// EIGHTTAP (regular) sub-pixel filters, 1/16 positions.
TV_HD int subpel_tap(int f, int t) {
  constexpr int16_t k[16][8] = {
      {0, 0, 0, 128, 0, 0, 0, 0},      {0, 2, -6, 126, 8, -2, 0, 0},    {0, 2, -10, 122, 18, -4, 0, 0},
      {0, 2, -12, 116, 28, -8, 2, 0},  {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -14, 102, 48, -12, 2, 0},
      {0, 2, -16, 94, 58, -12, 2, 0},  {0, 2, -14, 84, 66, -12, 2, 0},  {0, 2, -14, 76, 76, -14, 2, 0},
      {0, 2, -12, 66, 84, -14, 2, 0},  {0, 2, -12, 58, 94, -16, 2, 0},  {0, 2, -12, 48, 102, -14, 2, 0},
      {0, 2, -10, 38, 110, -14, 2, 0}, {0, 2, -8, 28, 116, -12, 2, 0},  {0, 0, -4, 18, 122, -10, 2, 0},
      {0, 0, -2, 8, 126, -6, 2, 0}};
  return k[f][t];
}
constexpr int kInterRound0 = 3, kInterRound1 = 11;

// Predicted sample at integer position (x, y) of a block displaced by (ix + fx/16, iy +
// fy/16); get(x, y) reads the reference with coordinates clamped to the plane (7.11.3.3).
template <class G>
TV_HD int inter_pred_px(G get, int x, int y, int fx, int fy) {
  if (!fx && !fy) return get(x, y);
  int col[8];
  for (int r = 0; r < 8; ++r) {
    int s = 0;
    for (int t = 0; t < 8; ++t) s += subpel_tap(fx, t) * get(x + t - 3, y + r - 3);
    col[r] = (s + (1 << (kInterRound0 - 1))) >> kInterRound0;
  }
  int s = 0;
  for (int t = 0; t < 8; ++t) s += subpel_tap(fy, t) * col[t];
  return clip_pixel((s + (1 << (kInterRound1 - 1))) >> kInterRound1);
}
// Motion vectors are (row, col) in 1/8 luma samples, always even (quarter-pel, no hp).
// Luma: integer mv >> 3, phase (mv & 7) * 2; chroma (4:2:0): integer mv >> 4, phase mv & 15.
TV_HD int mv_int(int mv, bool chroma) { return chroma ? (mv >> 4) : (mv >> 3); }
TV_HD int mv_frac(int mv, bool chroma) { return chroma ? (mv & 15) : ((mv & 7) << 1); }

// ------------------------------------------------------------------------- costs --------
// 4x4 Hadamard SATD of a difference block d[16] (row-major)
TV_HD int satd4(const int* d) {
  int m[16];
  for (int i = 0; i < 4; ++i) {
    const int a0 = d[i * 4] + d[i * 4 + 3], a1 = d[i * 4 + 1] + d[i * 4 + 2];
    const int a2 = d[i * 4 + 1] - d[i * 4 + 2], a3 = d[i * 4] - d[i * 4 + 3];
    m[i * 4] = a0 + a1;
    m[i * 4 + 1] = a3 + a2;
    m[i * 4 + 2] = a0 - a1;
    m[i * 4 + 3] = a3 - a2;
  }
  int s = 0;
  for (int j = 0; j < 4; ++j) {
    const int a0 = m[j] + m[12 + j], a1 = m[4 + j] + m[8 + j];
    const int a2 = m[4 + j] - m[8 + j], a3 = m[j] - m[12 + j];
    s += tv_abs(a0 + a1) + tv_abs(a3 + a2) + tv_abs(a0 - a1) + tv_abs(a3 - a2);
  }
  return (s + 1) >> 1;
}
// approximate bits of one MV component difference (1/8 units, even)
TV_HD int mv_comp_bits(int d) {
  const int a = tv_abs(d) >> 1;  // quarter-pel units
  return a ? 2 * tv_bitlen((unsigned)a) + 2 : 1;
}
// approximate mode bits of the key-frame intra candidates (x16)
TV_HD int intra_mode_bits16(int m) {
  switch (m) {
    case DC_PRED: return 32;
    case V_PRED: case H_PRED: return 48;
    case SMOOTH_PRED: return 40;
    case PAETH_PRED: return 48;
    default: return 56;
  }
}

// CDEF presets the encoder evaluates (preset = pri * 4 + sec_idx): luma primary strengths
// {0,1,2,3,5,7,10,13} x secondary {0, 2}; chroma {0,2,4,7} x {0, 2} (a libaom-style fast
// strength subset: 16 / 8 of the 64 presets, 4x / 8x less CDEF search work).
constexpr uint64_t cdef_mask(const int* pri, int npri, const int* sec, int nsec) {
  uint64_t m = 0;
  for (int i = 0; i < npri; ++i)
    for (int j = 0; j < nsec; ++j) m |= 1ull << (pri[i] * 4 + sec[j]);
  return m;
}
constexpr int kCdefPriY[8] = {0, 1, 2, 3, 5, 7, 10, 13}, kCdefPriUV[4] = {0, 2, 4, 7}, kCdefSec[2] = {0, 2};
constexpr uint64_t kCdefMaskY = cdef_mask(kCdefPriY, 8, kCdefSec, 2);
constexpr uint64_t kCdefMaskUV = cdef_mask(kCdefPriUV, 4, kCdefSec, 2);
// cdef_damping of a stream, from its base q-index (3..6)
TV_HD int cdef_damping_for_q(int q) { return 3 + (q >> 6); }

// ---------------------------------------------------------------- loop restoration ------
// Self-guided restoration (SGRPROJ) per 64x64 unit of each plane: candidate parameter sets
// (Sgr_Params rows), projection weights by an integer least-squares solve, unit on/off by
// SSE + rate.  xqd ranges / reference mid of the AV1 syntax (Sgrproj_Xqd_Min/Max/Mid).
constexpr int kNumLrSets = 2;
TV_HD int lr_set(int i) { return i == 0 ? 4 : 10; }
constexpr int kXqdMin0 = -96, kXqdMax0 = 31, kXqdMin1 = -32, kXqdMax1 = 95, kXqdMid0 = -32, kXqdMid1 = 31;
TV_HD int bitlen64(unsigned long long v) { return tv_bitlen64(v); }
TV_HD long long div_round(long long n, long long d) { return n >= 0 ? (n + d / 2) / d : -((-n + d / 2) / d); }
// Coded weights (xqd0, xqd1) of a unit from its sgr_stats (H00 H01 H11 c0 c1: normal
// equations of the weights a, b of F0 - u and F1 - u, 1/128 units).  The decoder applies
// a to F0, 128 - xqd0 - xqd1 to F1 and xqd1 to u (sgr_project_xqd), so xqd0 = a and
// xqd1 = 128 - a - b, each clamped to its coded range (one weight clamped, the other
// re-solved given it); radius-0 passes get the syntax's implied values.  Stats are scaled
// below 2^30 so the 2x2 Cramer solve stays in 64 bits.
TV_HD void sgr_solve(const long long* st, int r0, int r1, int* xqd0, int* xqd1) {
  unsigned long long m = 0;
  for (int i = 0; i < 5; ++i) {
    const unsigned long long a = (unsigned long long)(st[i] < 0 ? -st[i] : st[i]);
    m = a > m ? a : m;
  }
  const int sh = tv_max(0, bitlen64(m) - 30);
  const long long H00 = (st[0] >> sh) + 1, H01 = st[1] >> sh, H11 = (st[2] >> sh) + 1, c0 = st[3] >> sh,
                  c1 = st[4] >> sh;
  long long a = 0, b = 0;
  if (r0 && r1) {
    const long long det = H00 * H11 - H01 * H01;
    if (det > 0) {
      a = div_round(c0 * H11 - c1 * H01, det);
      b = div_round(H00 * c1 - H01 * c0, det);
    }
    if (a < kXqdMin0 || a > kXqdMax0) {
      a = clip3((long long)kXqdMin0, (long long)kXqdMax0, a);
      b = div_round(c1 - H01 * a, H11);
    } else if (b < 128 - kXqdMax1 - a || b > 128 - kXqdMin1 - a) {
      b = clip3(128 - kXqdMax1 - a, 128 - kXqdMin1 - a, b);
      a = clip3((long long)kXqdMin0, (long long)kXqdMax0, div_round(c0 - H01 * b, H00));
    }
    *xqd0 = (int)a;
    *xqd1 = (int)clip3((long long)kXqdMin1, (long long)kXqdMax1, 128 - a - b);
  } else if (r0) {
    *xqd0 = (int)clip3((long long)kXqdMin0, (long long)kXqdMax0, div_round(c0, H00));
    *xqd1 = clip3(kXqdMin1, kXqdMax1, 128 - *xqd0);
  } else {
    *xqd0 = 0;
    *xqd1 = (int)clip3((long long)kXqdMin1, (long long)kXqdMax1, 128 - div_round(c1, H11));
  }
}
// rate of a restored unit (~16 bits) in SSE units
TV_HD long long lr_rate_cost(int q) {
  const long long a = ac_q(q);
  return ((a * a * 9) >> 10) * 16;
}

// ------------------------------------------------------------------ motion search -------
// Full-pel search of +-kMeRange around the co-located block on a 2-pel grid (17 x 17), then
// the 8 full-pel neighbours of the best grid point, then 8 half-pel and 8 quarter-pel
// refinements (SAD / SATD + lambda * mv bits, first minimum wins at every stage).
constexpr int kMeRange = 16;
constexpr int kMeGrid = kMeRange + 1;  // grid points per axis (step 2)
constexpr int kMeSide = 2 * kMeRange + 1;
TV_HD int me_cand_dx(int k) { return 2 * (k % kMeGrid) - kMeRange; }
TV_HD int me_cand_dy(int k) { return 2 * (k / kMeGrid) - kMeRange; }
TV_HD int me_ring_dx(int k) { constexpr int8_t t[8] = {-1, 0, 1, -1, 1, -1, 0, 1}; return t[k]; }
TV_HD int me_ring_dy(int k) { constexpr int8_t t[8] = {-1, -1, -1, 0, 0, 1, 1, 1}; return t[k]; }

// Motion-field refinement (inter frames): after the per-block search, kMvRefineRounds
// Jacobi rounds in which every 16x16 block re-chooses, by luma SATD alone (first minimum
// wins, its own MV first), among the current MVs of its neighbours.  The field becomes
// coherent (the writer codes most blocks as NEARESTMV / NEARMV, and skip blocks merge)
// and the search's local minima are escaped: on the bench content -31 % BD-rate against
// the independent per-block search (tools/rd_curve.py --codec av1, profiles/README.md).
constexpr int kMvRefineRounds = 3;
constexpr int kMvRefineMaxCand = 11;
// bytes of one block's record in the GPU's refinement memo: kMvRefineMaxCand MV words and as
// many SATDs, and a count
constexpr int kMvMemoRecordBytes = kMvRefineMaxCand * 8 + 1;
// candidate list of block (bx, by) from the current field `cur` (bw x bh blocks):
// own, left, above, above-right, right, below, zero, then the distance-2 neighbours
// (left, above, right, below); duplicates dropped.  Returns the count.
TV_HD int mv_refine_cands(const uint32_t* cur, int bw, int bh, int bx, int by, uint32_t* out) {
  const int b = by * bw + bx;
  uint32_t c[kMvRefineMaxCand];
  int n = 0;
  c[n++] = cur[b];
  if (bx) c[n++] = cur[b - 1];
  if (by) c[n++] = cur[b - bw];
  if (by && bx + 1 < bw) c[n++] = cur[b - bw + 1];
  if (bx + 1 < bw) c[n++] = cur[b + 1];
  if (by + 1 < bh) c[n++] = cur[b + bw];
  c[n++] = 0u;
  if (bx > 1) c[n++] = cur[b - 2];
  if (by > 1) c[n++] = cur[b - 2 * bw];
  if (bx + 2 < bw) c[n++] = cur[b + 2];
  if (by + 2 < bh) c[n++] = cur[b + 2 * bw];
  int m = 0;
  for (int i = 0; i < n; ++i) {
    bool dup = false;
    for (int j = 0; j < m; ++j) dup |= out[j] == c[i];
    if (!dup) out[m++] = c[i];
  }
  return m;
}

// MV unification after the refinement: a complete 32x32 quad (blocks k = 0..3 in raster
// order, sat[k][c] = SATD of block k at member c's MV) takes the member MV of least total
// SATD when that is at most kQuadUnifyBits' worth (lambda) above its blocks' own MVs; then
// a complete 64x64 superblock likewise takes one of its quads' (top-left block) MVs
// (own = its 16 blocks at their MVs, tot[c] = at quad c's).  Same-MV skip blocks merge into
// 32x32 / 64x64 blocks: -5 % BD-rate on the bench content (tools/rd_curve.py --codec av1).
constexpr int kQuadUnifyBits = 6, kSbUnifyBits = 16;
TV_HD int quad_unify(const int (*sat)[4], int lam) {
  const int own = sat[0][0] + sat[1][1] + sat[2][2] + sat[3][3];
  int bc = 1 << 30, bi = 0;
  for (int c = 0; c < 4; ++c) {
    const int t = sat[0][c] + sat[1][c] + sat[2][c] + sat[3][c];
    if (t < bc) bc = t, bi = c;
  }
  return bc <= own + ((lam * kQuadUnifyBits) >> 4) ? bi : -1;
}
TV_HD int sb_unify(int own, const int* tot, int lam) {
  int bc = tot[0], bi = 0;
  for (int c = 1; c < 4; ++c)
    if (tot[c] < bc) bc = tot[c], bi = c;
  return bc <= own + ((lam * kSbUnifyBits) >> 4) ? bi : -1;
}

// ------------------------------------------------------------------ per-block record ----
// One 32-bit word per 16x16 block: bit 0 inter, 1-4 y mode, 5-8 uv mode, 9 skip (no
// nonzero level in any plane), 10-12 nonzero mask (Y, U, V); mv word: row (low 16, signed)
// and col (high 16).
TV_HD uint32_t pack_mode(int inter, int ym, int uvm, int skip, int nzmask) {
  return (uint32_t)(inter & 1) | ((uint32_t)(ym & 15) << 1) | ((uint32_t)(uvm & 15) << 5) |
         ((uint32_t)(skip & 1) << 9) | ((uint32_t)(nzmask & 7) << 10);
}
TV_HD int mode_inter(uint32_t m) { return m & 1; }
TV_HD int mode_y(uint32_t m) { return (m >> 1) & 15; }
TV_HD int mode_uv(uint32_t m) { return (m >> 5) & 15; }
TV_HD int mode_skip(uint32_t m) { return (m >> 9) & 1; }
TV_HD int mode_nz(uint32_t m) { return (m >> 10) & 7; }
// bits 13-14: size of the (merged) block covering this 16x16 cell: 0 = 16x16, 1 = 32x32, 2 = 64x64
TV_HD int mode_bsz(uint32_t m) { return (m >> 13) & 3; }
TV_HD uint32_t with_bsz(uint32_t m, int s) { return (m & ~(3u << 13)) | ((uint32_t)(s & 3) << 13); }

// Skip-block merging of inter frames (one 64x64 superblock at sb (sx, sy)): a fully inside
// 32x32 quad whose four 16x16 blocks are all inter + skip with one motion vector becomes one
// 32x32 block; four such quads with one motion vector become one 64x64 block.  Prediction is
// unchanged (same MV), only the block size seen by the syntax and the deblocking differs.
TV_HD void merge_sb(uint32_t* mode, const uint32_t* mv, int bw, int bh, int sx, int sy) {
  bool q_ok[4];
  int nq = 0;
  for (int q = 0; q < 4; ++q) {
    const int qx = sx * 4 + (q & 1) * 2, qy = sy * 4 + (q >> 1) * 2;
    bool ok = qx + 1 < bw && qy + 1 < bh;
    if (ok) {
      const uint32_t v0 = mv[qy * bw + qx];
      for (int k = 0; k < 4 && ok; ++k) {
        const int c = (qy + (k >> 1)) * bw + qx + (k & 1);
        ok = mode_inter(mode[c]) && mode_skip(mode[c]) && mv[c] == v0;
      }
    }
    q_ok[q] = ok;
    nq += ok;
  }
  const int x0 = sx * 4, y0 = sy * 4;
  bool sb = nq == 4;
  if (sb) {
    const uint32_t v0 = mv[y0 * bw + x0];
    for (int q = 1; q < 4 && sb; ++q) sb = mv[(y0 + (q >> 1) * 2) * bw + x0 + (q & 1) * 2] == v0;
  }
  for (int q = 0; q < 4; ++q) {
    if (!q_ok[q]) continue;
    const int qx = x0 + (q & 1) * 2, qy = y0 + (q >> 1) * 2;
    for (int k = 0; k < 4; ++k) {
      const int c = (qy + (k >> 1)) * bw + qx + (k & 1);
      mode[c] = with_bsz(mode[c], sb ? 2 : 1);
    }
  }
}
TV_HD uint32_t pack_mv(int row, int col) { return (uint32_t)(row & 0xFFFF) | ((uint32_t)(col & 0xFFFF) << 16); }
TV_HD int mv_row(uint32_t v) { return (int)(int16_t)(v & 0xFFFF); }
TV_HD int mv_col(uint32_t v) { return (int)(int16_t)(v >> 16); }

// --------------------------------------------------- intra blocks in inter frames -------
// Opt-in tool (kToolIntraInInter, off by default): 16x16 blocks of an inter frame whose
// content has no match in the reference (a cut the scene detector missed, uncovered
// background, motion beyond +-kMeRange) are coded as intra blocks.  The model runs per inter
// frame once the motion field is final and every block has been coded as inter, before
// merge_sb.
//   inter cost   luma 16x16 SATD of the source against the inter prediction at the final MV;
//   gate         only blocks with inter cost > kIbGate * 256 are analysed;
//   candidate    the seven intra_cand modes predicted from SOURCE neighbours (intra_edges on
//                the source frame, so every block is analysed independently), mode cost =
//                SATD + ((lam * intra_mode_bits16(m)) >> 8), first minimum; the block is a
//                candidate when ib_cost(best, lam) < inter cost;
//   acceptance   ib_accepted(): a pure function of the candidate flags of a bounded
//                neighbourhood (below);
//   recon        accepted blocks are re-coded exactly as key-frame blocks are (luma and chroma
//                mode search on RECONSTRUCTED neighbours, kRndIntra, uv_txtype) and overwrite
//                the block's reconstruction, levels, mode word (pack_mode(0, ym, uvm, skip,
//                nz), block size 0) and MV word (0).
// Acceptance is a wavefront local to each 64x64 superblock: with lx = bx & 3, ly = by & 3,
// block b belongs to pass d = lx + ly (0..6), and pass d of every superblock of the frame
// runs before pass d + 1.  An intra block reads its left, above and above-left neighbours
// (no above-right, no below-left sample).  Those inside b's superblock belong to passes d - 1
// and d - 2: final when b runs.  Those in another superblock have lx = 3 or ly = 3 while b
// has lx = 0 or ly = 0 there, so they belong to a LATER pass (left of an lx = 0 block: pass
// 3 + ly > ly; likewise above and above-left); b may only read them if they stay inter, so a
// candidate is accepted unless one of its outside neighbours is itself accepted.  An outside
// neighbour of an edge block is either interior (lx > 0 && ly > 0: no outside neighbour,
// accepted whenever candidate) or an edge block whose own outside neighbours are all
// interior, so the recursion ends after two steps (ib_accepted<2>).  Blocks on the picture's
// left / top edge have no neighbour there.
// Order independence: an accepted block reads only samples that are final when it runs -
// inter blocks that are never re-coded, and accepted blocks of earlier passes, which are also
// earlier in raster order.  So re-coding the accepted blocks in raster order (golden encoder,
// the decoder's order) and in pass order (GPU) gives the same reconstruction by induction.
// No rule that accepts more and stays a bounded pure function was found: letting an edge
// block win against its outside neighbour needs a tie-break that propagates along a row
// of superblocks.
// Constants: BD-rate of the tool against off with the golden encoder (tools/rd_curve.py --codec
// av1 --intra-in-inter 1, QP 22..37 = q 60..160; 320x192 x 8 frames with --cut 4 smooth /
// textured, the same without a cut ("pan"), 640x360 x 16 frames of the bench content smooth /
// textured; profiles/av1_intra_blocks/README.md):
//   s * 5/4, gate 4, 16 bits (the start)   -8.79  -3.89   0.00  +0.06  -0.24
//   s * 3/2, gate 4, 16 bits               -7.34  -2.00   0.00  +0.08  +0.05
//   s * 5/4, gate 4,  8 bits               -8.99  -4.28   0.00  +0.10  -0.29
//   s * 5/4, gate 2, 16 bits               -8.79  -3.89   0.00  +0.06  -0.24  (= gate 4)
//   s * 5/4, gate 8, 16 bits               -8.12  -3.89   0.00  -0.16  -0.24
//   s * 9/8, gate 4, 24 bits               -8.93  -4.99  -0.06  +0.02  -0.26
//   s * 1,   gate 4, 32 bits               -9.27  -6.26  -0.62  -0.09  -0.65
//   s * 1,   gate 4, 16 bits               -9.75  -7.38  -0.54  -0.26  -1.24
//   s * 1,   gate 4,  8 bits              -10.17  -7.75  -0.80  -1.08  -1.31
//   s * 7/8, gate 4, 32 bits               -9.97  -8.31  -0.73  -0.54  -1.46
//   s * 7/8, gate 4, 16 bits (kept)       -10.16  -8.74  -0.21  -0.93  -1.70
//   s * 3/4, gate 4, 16 bits              -10.43  -9.38  -0.58  -0.83  -1.39
// Weights below 1 keep gaining although source neighbours flatter the intra SATD; why was not
// investigated.  The curve is flat between 1 and 3/4; 7/8 is the best on the textured bench
// content and touches the pan clip least of the three.
constexpr int kToolIntraInInter = 1;  // bit of the encoders' tools word
constexpr int kIbGate = 4;            // inter SATD per luma sample below which a block is not analysed
constexpr int kIbPenBits = 16;
TV_HD bool ib_gated(int inter_cost) { return inter_cost > kIbGate * 256; }
TV_HD int ib_cost(int s, int lam) { return s * 7 / 8 + ((lam * kIbPenBits) >> 4); }
// Luma mode decision of one block from the edges `e` (source neighbours for the analysis):
// sat(mode) -> 16x16 SATD of the source against the mode's prediction.  Returns the least
// cost (first minimum over intra_cand order).
template <class F>
TV_HD int ib_best_cost(F sat, int lam) {
  int best = 1 << 30;
  for (int k = 0; k < kNumIntraCand; ++k) {
    const int c = sat(intra_cand(k)) + ((lam * intra_mode_bits16(intra_cand(k))) >> 8);
    if (c < best) best = c;
  }
  return best;
}
TV_HD bool ib_candidate(int inter_cost, int best_intra, int lam) {
  return ib_gated(inter_cost) && ib_cost(best_intra, lam) < inter_cost;
}
TV_HD int ib_pass(int bx, int by) { return (bx & 3) + (by & 3); }
constexpr int kIbPasses = 7;
// cand [bh][bw]: bit 0 = candidate.  D = remaining recursion depth (callers use 2).
template <int D>
TV_HD bool ib_accepted_d(const uint8_t* cand, int bw, int bx, int by) {
  if (!(cand[by * bw + bx] & 1)) return false;
  if constexpr (D > 0) {
    for (int k = 0; k < 3; ++k) {  // left, above, above-left
      const int nx = bx - (k != 1), ny = by - (k != 0);
      if (nx < 0 || ny < 0) continue;
      if ((nx >> 2) == (bx >> 2) && (ny >> 2) == (by >> 2)) continue;
      if (ib_accepted_d<D - 1>(cand, bw, nx, ny)) return false;
    }
  }
  return true;
}
TV_HD bool ib_accepted(const uint8_t* cand, int bw, int bx, int by) { return ib_accepted_d<2>(cand, bw, bx, by); }

// ------------------------------------------------------------- chroma from luma ---------
// Opt-in tool (kToolCfl, off by default): UV_CFL_PRED as an eighth chroma mode of every intra
// block (key frames and the intra blocks of inter frames).  4:2:0, 8x8 chroma of a 16x16 luma
// block; the coded size is a multiple of 16, so every luma sample of the block is in the frame.
//   prediction  L[i][j] = (the four reconstructed - before deblocking - luma samples at rows
//               2i..2i+1, cols 2j..2j+1, summed) << 1; avg = (sum of L + 32) >> 6; ac = L - avg
//               (|ac| <= 2040); pred = clip_pixel(dc + Round2Signed(alpha * ac, 6)) with dc the
//               plane's DC_PRED value (intra_dc, missing-neighbour variants included) and
//               alpha in -16..16 (eighths); transform type DCT_DCT (uv_txtype).
//   decision    per plane, r = src - dc: num = sum ac * r, den = sum ac^2 (int32; 64 * num in 64
//               bits), a0 = cfl_fit(num, den); candidates a0, a0 - 1, a0 + 1 inside -16..16,
//               cost = 8x8 SATD + alpha rate, first strict minimum in that order (cfl_pick);
//               both alphas zero cannot be signalled: no candidate.  CfL is compared last
//               against the best of the seven regular modes and wins only when strictly
//               cheaper (cfl_decide), so every tie keeps the regular mode.
//   mode word   uv mode 13, alpha_u + 16 in bits 15-20, alpha_v + 16 in bits 21-26 (zero for
//               every other block).
// No specification text was at hand: the above (AV1 7.11.5, the cfl_alpha_signs / cfl_alpha_u
// / cfl_alpha_v syntax and contexts in av1_codec.cpp) is written from memory and dav1d is the
// arbiter - where dav1d and this description disagree, dav1d wins (tests/test_av1_cfl.py
// decodes CfL streams with dav1d sample for sample).
// Rate constants (1/16 bit, the units of intra_mode_bits16; cfl_bits16 = mode + plane(alpha_u) +
// plane(alpha_v), plane(0) = zero, plane(a) = base + step * (|a| - 1)): BD-rate of the tool
// against off with the golden encoder (tools/rd_curve.py --codec av1 --cfl 1, QP 22..37, PSNR-Y /
// 6:1:1 PSNR-YUV; 640x360: 8 frames with chroma = 128 + k/8 (Y2x2 - 128) + noise, k = 6 / -5
// ("corr"), 16 frames of the bench content smooth / textured at GOP 64, 4 key frames of the
// same; profiles/av1_cfl/README.md):
//   mode zero base step    corr           smooth       textured     key smooth   key textured
//   40   16   40   8 (kept) -17.36/-25.14  +0.24/+0.12  +0.12/+0.11  -0.29/-0.37  -0.00/+0.01
//   72   16   48   8        -16.65/-24.01  +0.26/+0.16  +0.13/+0.14  -0.32/-0.38  -0.01/+0.00
//   24   16   32   8        -17.40/-25.44  +0.27/+0.13  +0.12/+0.12  -0.31/-0.39  -0.03/-0.02
//   56   16   48   8        -17.02/-24.49  +0.26/+0.16  +0.14/+0.14  -0.31/-0.38  -0.00/+0.01
//   40    8   24   8        -17.45/-25.47  +0.34/+0.21  +0.12/+0.12  -0.30/-0.38  -0.03/-0.02
// Flat in the constants; the start has the best bench-content figures.  The bench content's
// chroma does not follow its luma (0.2 % of its key-frame blocks take CfL) and the tool loses
// 0.1 .. 0.25 % there at GOP 64, which is one reason it ships off.
constexpr int kToolCfl = 2;  // bit of the encoders' tools word
constexpr int UV_CFL_PRED = 13;
constexpr int kCflModeBits16 = 40, kCflZeroBits16 = 16, kCflAlphaBits16 = 40, kCflAlphaStep16 = 8;
TV_HD int cfl_alpha_bits16(int a) { return a ? kCflAlphaBits16 + kCflAlphaStep16 * (tv_abs(a) - 1) : kCflZeroBits16; }
TV_HD int cfl_bits16(int au, int av) { return kCflModeBits16 + cfl_alpha_bits16(au) + cfl_alpha_bits16(av); }
TV_HD uint32_t with_cfl(uint32_t m, int au, int av) {
  return (m & 0x7FFFu) | ((uint32_t)(au + 16) << 15) | ((uint32_t)(av + 16) << 21);
}
TV_HD int mode_cfl_u(uint32_t m) { return (int)((m >> 15) & 63) - 16; }
TV_HD int mode_cfl_v(uint32_t m) { return (int)((m >> 21) & 63) - 16; }
// L of one chroma sample from its four luma samples; avg of the block from the sum of its 64 L
TV_HD int cfl_luma(int a, int b, int c, int d) { return (a + b + c + d) << 1; }
TV_HD int cfl_avg(int sum) { return (sum + 32) >> 6; }
TV_HD int cfl_pred_px(int dc, int alpha, int ac) {
  const int s = alpha * ac;  // Round2Signed(s, 6): the magnitude is rounded, the sign kept
  return clip_pixel(dc + (s < 0 ? -((-s + 32) >> 6) : (s + 32) >> 6));
}
// ac[64] (row-major) of the block whose luma origin is (x0, y0); get(x, y) reads reconstructed luma
template <class G>
TV_HD void cfl_ac_block(G get, int x0, int y0, int16_t* ac) {
  int sum = 0;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      const int x = x0 + 2 * j, y = y0 + 2 * i;
      const int l = cfl_luma(get(x, y), get(x + 1, y), get(x, y + 1), get(x + 1, y + 1));
      ac[i * 8 + j] = (int16_t)l;
      sum += l;
    }
  const int avg = cfl_avg(sum);
  for (int i = 0; i < 64; ++i) ac[i] = (int16_t)(ac[i] - avg);
}
// least-squares alpha of one plane in eighths: 64 * num / den rounded to nearest, halves away
// from zero, clamped to the coded range; 0 for a flat luma block
TV_HD int cfl_fit(int num, int den) {
  if (!den) return 0;
  const long long n = 64LL * num, d = den;
  const long long q = n >= 0 ? (2 * n + d) / (2 * d) : -((-2 * n + d) / (2 * d));
  return (int)clip3(-16LL, 16LL, q);
}
TV_HD int cfl_cand(int a0, int k) { return k == 0 ? a0 : (k == 1 ? a0 - 1 : a0 + 1); }
// alpha of one plane from the 8x8 SATDs sat3[k] of its candidates cfl_cand(a0, k); *sat = the
// chosen candidate's SATD
TV_HD int cfl_pick(int a0, const int* sat3, int lam, int* sat) {
  int best = 1 << 30, ba = 0;
  for (int k = 0; k < 3; ++k) {
    const int a = cfl_cand(a0, k);
    if (a < -16 || a > 16) continue;
    const int c = sat3[k] + ((lam * cfl_alpha_bits16(a)) >> 8);
    if (c < best) best = c, ba = a, *sat = sat3[k];
  }
  return ba;
}
// The block's chroma decision: true when CfL beats `best`, the cost of the best regular mode
TV_HD bool cfl_decide(int a0u, int a0v, const int* satu3, const int* satv3, int lam, int best, int* au, int* av) {
  int su = 0, sv = 0;
  *au = cfl_pick(a0u, satu3, lam, &su);
  *av = cfl_pick(a0v, satv3, lam, &sv);
  if (!*au && !*av) return false;
  return su + sv + ((lam * cfl_bits16(*au, *av)) >> 8) < best;
}
// the same with the mode term given (kToolDirIntra: uv[y mode][13] of the default CDFs)
TV_HD bool cfl_decide_bits(int a0u, int a0v, const int* satu3, const int* satv3, int lam, int best, int mode_bits16,
                           int* au, int* av) {
  int su = 0, sv = 0;
  *au = cfl_pick(a0u, satu3, lam, &su);
  *av = cfl_pick(a0v, satv3, lam, &sv);
  if (!*au && !*av) return false;
  return su + sv + ((lam * (mode_bits16 + cfl_alpha_bits16(*au) + cfl_alpha_bits16(*av))) >> 8) < best;
}

// ------------------------------------------------------------- directional intra -------
// Opt-in tool (kToolDirIntra, off by default): the luma and the chroma mode search of every
// intra block (key frames and the accepted intra blocks of inter frames) run over 34 (mode,
// angle delta) candidates with rates read from the default CDFs.  With the tool off every
// stream, mode word and kernel instruction is what it was.
//   angles      pAngle = base + 3 * delta, delta in -3..3, only 90 < pAngle < 180 (plus plain V
//               and H): V_PRED +1..+3 (93, 96, 99), H_PRED -1..-3 (177, 174, 171), D113 / D135 /
//               D157 -3..+3 (104..122, 126..144, 148..166).  D45 / D67 / D203, V with delta < 0
//               and H with delta > 0 are never produced; the writer and the oracle refuse them
//               (dir_delta_ok).  Such an angle reads above[-1 .. N-1] and left[-1 .. N-1] only
//               (intra_dir_px: base >= -1 and base + 1 <= N - 1 for every (i, j), N = 8 and 16,
//               tests/test_av1_dir_intra.py): nothing right of above[N-1] or below left[N-1],
//               so the key-frame anti-diagonal wavefront and the pass argument of "intra blocks
//               in inter frames" above hold unchanged.  The intra edge filter and upsampling
//               stay off in the sequence header, so intra_dir_px is the whole predictor:
//               dx = Dr_Intra_Derivative[180 - pAngle], dy = [pAngle - 90] (dr_deriv).
//   rates       1/16 bit, bits16(p) = round(16 * log2(32768 / p)) of the default CDFs
//               (tv/av1_tables.h k*Bits16, generated with the CDFs): luma cost = SATD16 + ((lam *
//               (ymode_bits + angle_bits)) >> 8), ymode_bits from kf_y[ctx(above)][ctx(left)] in
//               key frames (a missing neighbour counts as DC_PRED; intra_mode_ctx is the
//               writer's context map) and from y_mode[size group 2] in inter frames; angle_bits
//               = angle[mode][delta] of a directional mode, else 0.  Chroma cost = SATD8(U) +
//               SATD8(V) + ((lam * (uv[chosen y mode][uv mode] + angle_bits)) >> 8), the
//               CfL-allowed table.  With kToolCfl also on, CfL's mode term is uv[y mode][13]
//               instead of kCflModeBits16; its alpha terms and "strictly cheaper" rule stay.
//               All 34 candidates use these rates, the seven of intra_cand included.
//   search      exhaustive in the order of dir_cand: the seven intra_cand modes; V +1 +2 +3; H
//               -1 -2 -3; D135, D113, D157 each with deltas 0 -1 +1 -2 +2 -3 +3; the first strict
//               minimum wins.  Luma and chroma use the same list; chroma chooses independently.
//               The intra-in-inter analysis (ib_best_cost) keeps its seven modes and flat rates,
//               so the candidate and accepted maps do not depend on the tool.
//   mode word   luma delta as 3-bit two's complement in bits 27-29; chroma delta likewise in
//               bits 15-17 when the uv mode is directional (the field is the CfL alphas' only
//               when the uv mode is 13); delta 0 is stored as 0, so tool-off words are unchanged.
// The derivative table is written from memory; tests/test_av1_dir_intra.py compares it with
// the bundled decoder library's copy and dav1d decodes the streams sample for sample.
constexpr int kToolDirIntra = 4;  // bit of the encoders' tools word
constexpr int kNumDirCand = 34;
TV_HD bool mode_directional(int m) { return m >= V_PRED && m <= 8; }
// Dr_Intra_Derivative at the angles 3, 6, 9, 14, .. 87, indexed by angle / 3
TV_HD int dr_deriv(int a) {
  constexpr uint16_t t[30] = {0,  1023, 547, 372, 273, 215, 178, 151, 132, 116, 102, 0,  90, 80, 71,
                              64, 57,   51,  45,  40,  35,  31,  27,  23,  19,  15,  0,  11, 7,  3};
  return t[a / 3];
}
TV_HD int dir_base_angle(int m) {
  return m == V_PRED ? 90 : (m == H_PRED ? 180 : (m == D135_PRED ? 135 : (m == D113_PRED ? 113 : 157)));
}
// (mode, delta) pairs of the encoder subset: 90 <= pAngle <= 180, the ends only as plain V / H
TV_HD bool dir_delta_ok(int m, int delta) {
  if (delta < -3 || delta > 3) return false;
  if (!mode_directional(m)) return delta == 0;
  if (m == V_PRED) return delta >= 0;
  if (m == H_PRED) return delta <= 0;
  return m == D135_PRED || m == D113_PRED || m == D157_PRED;
}
// candidate k of the search: mode, angle delta
TV_HD int dir_cand_mode(int k) {
  constexpr int8_t m[3] = {D135_PRED, D113_PRED, D157_PRED};
  return k < kNumIntraCand ? intra_cand(k) : (k < 10 ? V_PRED : (k < 13 ? H_PRED : m[(k - 13) / 7]));
}
TV_HD int dir_cand_delta(int k) {
  if (k < kNumIntraCand) return 0;
  if (k < 10) return k - 6;
  if (k < 13) return 9 - k;
  const int r = (k - 13) % 7;  // 0 -1 +1 -2 +2 -3 +3
  return (r & 1) ? -((r + 1) >> 1) : (r >> 1);
}
TV_HD uint32_t with_angle_y(uint32_t m, int delta) { return (m & ~(7u << 27)) | ((uint32_t)(delta & 7) << 27); }
TV_HD uint32_t with_angle_uv(uint32_t m, int delta) { return (m & ~(7u << 15)) | ((uint32_t)(delta & 7) << 15); }
TV_HD int mode_angle_y(uint32_t m) { return (int)(((m >> 27) & 7) ^ 4) - 4; }
TV_HD int mode_angle_uv(uint32_t m) { return mode_directional(mode_uv(m)) ? (int)(((m >> 15) & 7) ^ 4) - 4 : 0; }
// predicted sample of (mode, delta); delta 0 is intra_pred_px
TV_HD int intra_pred_px_ang(int mode, int delta, const IntraEdge& e, int N, int i, int j, int dc) {
  if (!delta) return intra_pred_px(mode, e, N, i, j, dc);
  const int a = dir_base_angle(mode) + 3 * delta;
  return intra_dir_px(e, i, j, dr_deriv(180 - a), dr_deriv(a - 90));
}
// rate terms (1/16 bit).  Intra_Mode_Context of a neighbour's y mode (the writer's kIntraModeCtx)
TV_HD int intra_mode_ctx(int m) {
  constexpr int8_t c[13] = {0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0};
  return c[m];
}
TV_HD int dir_angle_bits16(int m, int delta) { return mode_directional(m) ? tab::kAngleDeltaBits16[m - V_PRED][delta + 3] : 0; }
// kf: key frame, above / left = the neighbours' y modes (DC_PRED where missing)
TV_HD int dir_y_bits16(bool kf, int above, int left, int m, int delta) {
  const int mb = kf ? tab::kKfYModeBits16[intra_mode_ctx(above)][intra_mode_ctx(left)][m] : tab::kYModeBits16[m];
  return mb + dir_angle_bits16(m, delta);
}
TV_HD int dir_uv_bits16(int ym, int uvm, int delta) { return tab::kUvMode1Bits16[ym][uvm] + dir_angle_bits16(uvm, delta); }
// y mode of a neighbour's mode word for the key-frame context
TV_HD int dir_ctx_mode(uint32_t m) { return mode_inter(m) ? DC_PRED : mode_y(m); }

// ------------------------------------------------------------- transform split ----------
// Opt-in tool (kToolTxSplit, off by default): a non-skip 16x16 inter block may code its luma as
// four 8x8 DCT_DCT transforms instead of one 16x16 (chroma keeps its two 8x8 transforms).  With
// the tool on, inter frames signal TX_MODE_SELECT; key frames keep TX_MODE_LARGEST, so the key
// frame of a tool-on stream is the tool-off key frame.  With the tool off every stream, mode
// word and kernel instruction is what it was.
//   candidates  after prediction the luma residual is coded both ways with the frame's inter
//               rounding: one 16x16 transform, and the four 8x8 quadrants (raster order, each
//               with its own DC step).
//   cost        J = (SSE(source, reconstruction) << 8) + tx_lambda(q) * bits16: bits16 (1/16
//               bit) is a closed-form proxy over the quantised levels (tx_tb_bits16 per
//               transform block: an all-zero flag, or a coded-block term, an eob-position term
//               per bit of the eob, a term per zero before the eob and, per nonzero level, a
//               base plus a term per floor(log2 |l|)), plus the txfm_split symbols from the
//               default CDFs (tv/av1_tables.h kTxfmSplitBits16): split = the 16x16 flag (context
//               12: neighbours with transforms of 16 or more) + four 8x8 "no further split" flags
//               (context 15); kept = the 16x16 flag alone.  tx_lambda(q) = 9 * ac_q^2 / 64, the
//               SSE-per-bit slope of lr_rate_cost in these units.
//   decision    split when J(split) < J(16x16) and at least one quadrant has a nonzero level;
//               ties keep 16x16.  A pure function of the block's source, prediction and q: inter
//               frames stay embarrassingly parallel.  A block whose chosen luma and chroma are
//               all zero is a skip block and never carries the split bit.
//   mode word   bit 30 = split, bits 15-18 = nonzero mask of the quadrants (raster order; those
//               bits hold intra-only fields otherwise and are zero for inter blocks).  Bit 10
//               (Y) of a split block is set, and its 256 luma level slots hold four 8x8 rasters.
//   syntax      read_block_tx_size: txfm_split at 16x16 and, if 1, one txfm_split = 0 per 8x8
//               (depth 1; 4x4 is never coded); intra blocks of such frames code tx_depth = 0.
//               Each 8x8 luma TB codes txb_skip with the general luma context.
//   deblocking  luma transform size 8 for the 4x4 units of a split block (lf_word).
// Constants: profiles/av1_tx_split/README.md.
constexpr int kToolTxSplit = 8;  // bit of the encoders' tools word
constexpr int kTxTbZeroBits16 = 8, kTxTbCodedBits16 = 24, kTxEobBits16 = 24, kTxZeroCoefBits16 = 10;
constexpr int kTxLevelBits16 = 40, kTxLevelLogBits16 = 32;
constexpr int kTxSplitCtx16 = 12, kTxSplitCtx8 = 15;  // txfm_split contexts the rate term reads
TV_HD int mode_tx(uint32_t m) { return (int)((m >> 30) & 1); }
TV_HD int mode_txq(uint32_t m) { return mode_tx(m) ? (int)((m >> 15) & 15) : 0; }
TV_HD uint32_t with_tx_split(uint32_t m, int qmask) {
  return (m & ~((15u << 15) | (1u << 30))) | (1u << 30) | ((uint32_t)(qmask & 15) << 15);
}
// scan index (zigzag_scan order) of raster position (r, c) of an N x N block
TV_HD int zigzag_index(int N, int r, int c) {
  const int s = r + c;
  const int before = s < N ? s * (s + 1) / 2 : N * N - (2 * N - 1 - s) * (2 * N - s) / 2;
  const int lo = s - N + 1 > 0 ? s - N + 1 : 0, hi = s < N - 1 ? s : N - 1;
  return before + ((s & 1) ? r - lo : hi - r);
}
TV_HD int tx_level_bits16(int l) {
  const int a = l < 0 ? -l : l;
  return a ? kTxLevelBits16 + kTxLevelLogBits16 * (tv_bitlen((unsigned)a) - 1) : 0;
}
// rate of one transform block from its eob (scan index of the last nonzero level + 1), its
// count of nonzero levels and the sum of their tx_level_bits16
TV_HD int tx_tb_bits16(int eob, int nnz, int level_bits) {
  if (!eob) return kTxTbZeroBits16;
  return kTxTbCodedBits16 + kTxEobBits16 * tv_bitlen((unsigned)eob) + kTxZeroCoefBits16 * (eob - nnz) + level_bits;
}
TV_HD int tx_split_flag_bits16(bool split) {
  return split ? tab::kTxfmSplitBits16[kTxSplitCtx16][1] + 4 * tab::kTxfmSplitBits16[kTxSplitCtx8][0]
               : tab::kTxfmSplitBits16[kTxSplitCtx16][0];
}
TV_HD int tx_lambda(int q) { return (ac_q(q) * ac_q(q) * 9) >> 6; }
TV_HD long long tx_cost(int sse, int bits16, int q) { return ((long long)sse << 8) + (long long)tx_lambda(q) * bits16; }
// sse / bits16 of the two codings (bits16 without the flag terms); qmask8 = nonzero quadrants
TV_HD bool tx_split_wins(int q, int sse16, int bits16_16, int sse8, int bits16_8, int qmask8) {
  return qmask8 != 0 && tx_cost(sse8, bits16_8 + tx_split_flag_bits16(true), q) <
                            tx_cost(sse16, bits16_16 + tx_split_flag_bits16(false), q);
}
// rate of the N x N raster levels of one transform block
TV_HD int tx_tb_rate(const int16_t* lev, int N) {
  int eob = 0, nnz = 0, lb = 0;
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      const int l = lev[r * N + c];
      if (!l) continue;
      const int k = zigzag_index(N, r, c) + 1;
      eob = k > eob ? k : eob;
      ++nnz;
      lb += tx_level_bits16(l);
    }
  return tx_tb_bits16(eob, nnz, lb);
}

// deblocking info word for a 4x4 unit (av1_defs.h layout): block = 16 << bsz luma, 8 << bsz
// chroma; tx = block, or 8 for the luma of a transform-split block
TV_HD uint32_t lf_word(bool chroma, int lvl_v, int lvl_h, bool skip_inter, int bsz = 0, bool split = false) {
  const uint32_t l = (chroma ? 1u : 2u) + (uint32_t)bsz, t = split && !chroma ? 1u : l;
  return t | (t << 3) | (l << 6) | (l << 9) | ((uint32_t)(lvl_v & 63) << 12) | ((uint32_t)(lvl_h & 63) << 18) |
         ((uint32_t)skip_inter << 24);
}

}  // namespace av1
}  // namespace tv
