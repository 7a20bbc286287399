// av1_codec.cpp — AV1 encode path of the C++ golden model (BASELINE
// config #4): OBU / sequence header / uncompressed frame header / tile syntax, the decoder
// oracle, shared reconstruction (intra / inter prediction, dequantisation, inverse
// transform, deblocking, CDEF) and the golden encoder the gfx950 engine reproduces.
//
// The partition / mode-info / motion-vector / coefficient syntax is written ONCE as a
// template over the symbol direction (SymW encodes the given values, SymR decodes them),
// so writer and oracle parse the same grammar; the oracle's reconstruction then has to
// match the encoder's (golden or GPU) bit for bit.  The symbol contexts follow the AV1
// specification's derivations (partition, skip, is_inter, y/uv modes, single_ref_p*,
// new/zero/ref mv + drl from the spatial MV stack of 7.10.2, mv joints/classes, all_zero,
// eob_pt / eob_extra, coeff_base(_eob) / coeff_br with the 2-D context offsets, dc_sign,
// Golomb remainders).  CDFs start from the specification's defaults (tv/av1_tables.h) and
// adapt with the AV1 counter-based rate.
//
// Reference parity: thinvids rejects AV1 sources (/root/reference/worker/tasks.py:929-939)
// and encodes H.264 (:1532-1586); this is the north-star AV1 encoder of BASELINE.json.
#include "tv/av1_codec.h"

#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>

#include "tv/av1.h"
#include "tv/av1_defs.h"
#include "tv/av1_itx.h"
#include "tv/av1_tables.h"
#include "tv/av1_txfm.h"
#include "tv/bitstream.h"

namespace tv {
namespace av1 {

void txfm2d_ref(const int16_t* in, int16_t* out, int nblk, int log2N, int tcol, int trow, bool inverse);

SeqGeo make_seq_geo(int dw, int dh) {
  if (dw < 16 || dh < 16 || dw > 8192 || dh > 8192 || (dw & 1) || (dh & 1))
    throw std::runtime_error("av1: unsupported frame size");
  SeqGeo g;
  g.dw = dw;
  g.dh = dh;
  g.W = (dw + 15) & ~15;
  g.H = (dh + 15) & ~15;
  g.bw = g.W / 16;
  g.bh = g.H / 16;
  g.sbw = (g.W + 63) / 64;
  g.sbh = (g.H + 63) / 64;
  return g;
}

FrameDecisions FrameData::view() const {
  FrameDecisions d;
  d.fp = fp;
  d.mode = mode.data();
  d.mv = mv.data();
  d.ly = ly.data();
  d.lu = lu.data();
  d.lv = lv.data();
  d.cdef_idx = cdef_idx.data();
  d.lr = lr.empty() ? nullptr : lr.data();
  d.packed = false;
  return d;
}

namespace {

// ------------------------------------------------------------------ scans / tables ------
struct Scans {
  int16_t s8[64], s16[256];
};
const Scans& scans() {
  static const Scans s = [] {
    Scans t;
    zigzag_scan(8, t.s8);
    zigzag_scan(16, t.s16);
    return t;
  }();
  return s;
}
// writer fast path: per scan index of an N x N TB the padded-raster index (stride N + 4) and
// the base-context offset of its position
struct ScanPad {
  int16_t pad8[64], pad16[256];
  uint8_t off8[64], off16[256];
};
const ScanPad& scan_pad();
constexpr int kCoeffBaseOffset[5][5] = {
    {0, 1, 6, 6, 21}, {1, 6, 6, 21, 21}, {6, 6, 21, 21, 21}, {6, 21, 21, 21, 21}, {21, 21, 21, 21, 21}};
constexpr int kIntraModeCtx[13] = {0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0};
const ScanPad& scan_pad() {
  static const ScanPad s = [] {
    ScanPad t;
    for (int lg = 3; lg <= 4; ++lg) {
      const int N = 1 << lg, S = N + 4;
      const int16_t* sc = lg == 4 ? scans().s16 : scans().s8;
      for (int c = 0; c < N * N; ++c) {
        const int r = sc[c] >> lg, k = sc[c] & (N - 1);
        (lg == 4 ? t.pad16 : t.pad8)[c] = (int16_t)(r * S + k);
        (lg == 4 ? t.off16 : t.off8)[c] = (uint8_t)kCoeffBaseOffset[std::min(r, 4)][std::min(k, 4)];
      }
    }
    return t;
  }();
  return s;
}
inline bool directional(int m) { return m >= V_PRED && m <= 8; }

// ------------------------------------------------------------------------ CDFs ----------
typedef uint16_t C17[17];  // up to 16 symbols + adaptation counter
struct Cdfs {
  C17 partition[4][4];          // [bsl - 1][ctx]: 8x8 (4 syms), 16 / 32 / 64 (10 syms)
  C17 kf_y[5][5], y_mode[4], uv[2][13], angle[8];
  C17 cfl_sign, cfl_alpha[6];
  C17 skip[3], is_inter[4], single_ref[3][6];
  C17 new_mv[6], zero_mv[2], ref_mv[6], drl[3];
  C17 mv_joint, mv_sign[2], mv_class[2], class0_bit[2], class0_fr[2][2], mv_fr[2], mv_bits[2][10];
  C17 intra_tx[4][13], inter_tx[4];
  C17 txfm_split[21], tx_size[3];  // tx_size: the 16x16 category (max depth 2) by context
  C17 txb_skip[5][13], eob_pt[7][2][2], eob_extra[5][2][9], base_eob[5][2][4], base[5][2][42], br[4][2][21];
  C17 dc_sign[2][3];
  C17 use_sgrproj;
};
template <class F> void each(C17& c, int n, F& f) { f(c, n); }
template <size_t K, class F> void each(C17 (&a)[K], int n, F& f) {
  for (auto& c : a) f(c, n);
}
template <size_t K, size_t L, class F> void each(C17 (&a)[K][L], int n, F& f) {
  for (auto& r : a) each(r, n, f);
}
template <size_t K, size_t L, size_t M, class F> void each(C17 (&a)[K][L][M], int n, F& f) {
  for (auto& r : a) each(r, n, f);
}
// f(cdf, number of symbols) for every CDF of the set
template <class F> void visit_cdfs(Cdfs& c, F f) {
  each(c.partition[0], 4, f);
  for (int b = 1; b < 4; ++b) each(c.partition[b], 10, f);
  each(c.kf_y, 13, f);
  each(c.y_mode, 13, f);
  each(c.uv[0], 13, f);
  each(c.uv[1], 14, f);
  each(c.angle, 7, f);
  each(c.cfl_sign, 8, f);
  each(c.cfl_alpha, 16, f);
  each(c.skip, 2, f);
  each(c.is_inter, 2, f);
  each(c.single_ref, 2, f);
  each(c.new_mv, 2, f);
  each(c.zero_mv, 2, f);
  each(c.ref_mv, 2, f);
  each(c.drl, 2, f);
  each(c.mv_joint, 4, f);
  each(c.mv_sign, 2, f);
  each(c.mv_class, 11, f);
  each(c.class0_bit, 2, f);
  each(c.class0_fr, 4, f);
  each(c.mv_fr, 4, f);
  each(c.mv_bits, 2, f);
  each(c.intra_tx, 5, f);
  each(c.inter_tx, 2, f);
  each(c.txfm_split, 2, f);
  each(c.tx_size, 3, f);
  each(c.txb_skip, 2, f);
  for (int s = 0; s < 7; ++s) each(c.eob_pt[s], s + 5, f);
  each(c.eob_extra, 2, f);
  each(c.base_eob, 3, f);
  each(c.base, 4, f);
  each(c.br, 4, f);
  each(c.dc_sign, 2, f);
  each(c.use_sgrproj, 2, f);
}
// The specification's default CDFs (tv/av1_tables.h holds them as cumulative values):
// init_non_coeff_cdfs + init_coeff_cdfs with the coefficient set of base_q_idx's context.
void set_cdf(uint16_t* c, const uint16_t* cum, int n) {
  for (int i = 0; i < n - 1; ++i) c[i] = (uint16_t)(32768 - cum[i]);
  c[n - 1] = 0;
  c[n] = 0;
}
template <size_t K> void set_cdfs(C17 (&c)[K], const uint16_t* cum, int stride, int n) {
  for (size_t k = 0; k < K; ++k) set_cdf(c[k], cum + k * stride, n);
}
int coeff_qctx(int qidx) { return qidx <= 20 ? 0 : (qidx <= 60 ? 1 : (qidx <= 120 ? 2 : 3)); }
void init_cdfs(Cdfs& c, int qidx) {
  using namespace tab;
  std::memset(&c, 0, sizeof(c));
  for (int b = 0; b < 4; ++b) set_cdfs(c.partition[b], kPartition[b * 4], 9, b ? 10 : 4);
  for (int a = 0; a < 5; ++a) set_cdfs(c.kf_y[a], kKfYMode[a][0], 12, 13);
  set_cdfs(c.y_mode, kYMode[0], 12, 13);
  set_cdfs(c.uv[0], kUvMode0[0], 12, 13);
  set_cdfs(c.uv[1], kUvMode1[0], 13, 14);
  set_cdfs(c.angle, kAngleDelta[0], 6, 7);
  set_cdf(c.cfl_sign, kCflSign, 8);
  set_cdfs(c.cfl_alpha, kCflAlpha[0], 15, 16);
  set_cdfs(c.skip, kSkip[0], 1, 2);
  set_cdfs(c.is_inter, kIntraInter[0], 1, 2);
  for (int r = 0; r < 3; ++r) set_cdfs(c.single_ref[r], kSingleRef[r][0], 1, 2);
  set_cdfs(c.new_mv, kNewmv[0], 1, 2);
  set_cdfs(c.zero_mv, kZeromv[0], 1, 2);
  set_cdfs(c.ref_mv, kRefmv[0], 1, 2);
  set_cdfs(c.drl, kDrl[0], 1, 2);
  set_cdf(c.mv_joint, kMvJoint, 4);
  for (int k = 0; k < 2; ++k) {
    const uint16_t half[1] = {16384};
    set_cdf(c.mv_sign[k], half, 2);
    set_cdf(c.mv_class[k], kMvClass, 11);
    set_cdf(c.class0_bit[k], kMvClass0Bit, 2);
    set_cdfs(c.class0_fr[k], kMvClass0Fr[0], 3, 4);
    set_cdf(c.mv_fr[k], kMvFr, 4);
    set_cdfs(c.mv_bits[k], kMvBits[0], 1, 2);
  }
  for (int t = 0; t < 4; ++t) set_cdfs(c.intra_tx[t], kIntraTxSet2[t][0], 4, 5);
  set_cdfs(c.inter_tx, kInterTxSet3[0], 1, 2);
  set_cdfs(c.txfm_split, kTxfmSplit[0], 1, 2);
  set_cdfs(c.tx_size, kTxSizeCat123[0][0], 2, 3);
  set_cdf(c.use_sgrproj, kUseSgrproj, 2);
  const int q = coeff_qctx(qidx);
  for (int t = 0; t < 5; ++t) {
    set_cdfs(c.txb_skip[t], kTxbSkip[q][t][0], 1, 2);
    for (int p = 0; p < 2; ++p) {
      set_cdfs(c.eob_extra[t][p], kEobExtra[q][t][p][0], 1, 2);
      set_cdfs(c.base_eob[t][p], kCoeffBaseEob[q][t][p][0], 2, 3);
      set_cdfs(c.base[t][p], kCoeffBase[q][t][p][0], 3, 4);
      if (t < 4) set_cdfs(c.br[t][p], kCoeffBr[q][t][p][0], 3, 4);
    }
  }
  for (int p = 0; p < 2; ++p) {
    set_cdfs(c.dc_sign[p], kDcSign[q][p][0], 1, 2);
    for (int k = 0; k < 2; ++k) {
      set_cdf(c.eob_pt[0][p][k], kEobPt16[q][p][k], 5);
      set_cdf(c.eob_pt[1][p][k], kEobPt32[q][p][k], 6);
      set_cdf(c.eob_pt[2][p][k], kEobPt64[q][p][k], 7);
      set_cdf(c.eob_pt[3][p][k], kEobPt128[q][p][k], 8);
      set_cdf(c.eob_pt[4][p][k], kEobPt256[q][p][k], 9);
      set_cdf(c.eob_pt[5][p][k], kEobPt512[q][p][k], 10);
      set_cdf(c.eob_pt[6][p][k], kEobPt1024[q][p][k], 11);
    }
  }
}
// CDFs saved at the end of a frame (disable_frame_end_update_cdf = 0) and loaded by the
// next frame through primary_ref_frame: probabilities kept, adaptation counters cleared
void load_saved_cdfs(Cdfs& c, const Cdfs& saved) {
  c = saved;
  visit_cdfs(c, [](uint16_t* p, int n) { p[n] = 0; });
}
// P(symbol s) of an inverse CDF (15-bit)
inline int sym_prob(const uint16_t* icdf, int s) { return (s ? icdf[s - 1] : 32768) - icdf[s]; }

// ------------------------------------------------------------------ symbol I/O ----------
struct SymW {
  static constexpr bool kW = true;
  RangeEncoder rc;
  void sym(int& v, uint16_t* c, int n) { rc.encode(v, c, n); }
  void boolp(int& v, int p0) { rc.encode_bool(v, p0); }
  void lit(int& v, int bits) { rc.encode_literal((uint32_t)v, bits); }
};
struct SymR {
  static constexpr bool kW = false;
  RangeDecoder rd;
  SymR(const uint8_t* p, size_t n) : rd(p, n) {}
  void sym(int& v, uint16_t* c, int n) { v = rd.decode(c, n); }
  void boolp(int& v, int p0) { v = rd.decode_bool(p0); }
  void lit(int& v, int bits) { v = (int)rd.decode_literal(bits); }
};

struct MvStack {
  int n = 0;
  int mv[8][2] = {};
  int w[8] = {};
  int newctx = 0, refctx = 0, zeroctx = 0;
};

// ------------------------------------------------------------------ tile syntax ---------
// Block-level state of one frame (one tile).  For the writer `mode`, `mv`, levels and
// cdef_idx are inputs; for the reader they are outputs.
template <class IO>
struct Tile {
  IO& io;
  const SeqGeo& g;
  FrameParams& fp;
  int MiRows, MiCols;
  Cdfs cdf;
  std::vector<uint32_t>& mode;
  std::vector<uint32_t>& mv;
  std::vector<int8_t>& cdef_idx;
  int32_t* lr = nullptr;                  // [3][nu][3]: writer input / reader output (null: no LR)
  int lr_type[3] = {0, 0, 0};
  int ref_xqd[3][2];
  std::vector<uint8_t> ymode, coded;      // inter mode (NEARESTMV..NEWMV) or intra y mode
  std::vector<int8_t> cdef_seen;
  std::vector<uint8_t> aLvl[3], aDc[3], lLvl[3], lDc[3];
  // transform-width contexts (above) / transform-height contexts (left) per 4x4 unit, in samples;
  // 64 where nothing was coded yet (TX_MODE_SELECT frames: av1_enc.h "transform split")
  std::vector<uint8_t> aTx, lTx;
  bool tx_select = false;
  // level access: writer reads, reader writes (full layout [nblk][N*N])
  std::function<const int16_t*(int, int)> lev_in;
  const int16_t* eob_in[3] = {nullptr, nullptr, nullptr};  // writer: eob per packed TB (scan_packed)
  const int32_t* eob_off[3] = {nullptr, nullptr, nullptr};   // block -> packed TB index (-1: none)
  const int16_t* scan_in[3] = {nullptr, nullptr, nullptr};   // writer: scan-packed stream per plane
  const int32_t* scan_off[3] = {nullptr, nullptr, nullptr};  // block -> offset of its [eob, ...] record
  int16_t* lev_out[3] = {nullptr, nullptr, nullptr};

  Tile(IO& io_, const SeqGeo& g_, FrameParams& fp_, std::vector<uint32_t>& mode_, std::vector<uint32_t>& mv_,
       std::vector<int8_t>& cdef_)
      : io(io_), g(g_), fp(fp_), MiRows(g_.H / 4), MiCols(g_.W / 4), mode(mode_), mv(mv_), cdef_idx(cdef_) {
    init_cdfs(cdf, fp_.qindex);
    ymode.assign(g.nblk(), 0);
    coded.assign(g.nblk(), 0);
    cdef_seen.assign(g.nsb(), -1);
    tx_select = fp_.tx_select && !fp_.key;
    aTx.assign(MiCols, 64);
    lTx.assign(MiRows, 64);
    for (int p = 0; p < 3; ++p) {
      const int ss = p ? 1 : 0;
      aLvl[p].assign(MiCols >> ss, 0);
      aDc[p].assign(MiCols >> ss, 0);
      lLvl[p].assign(MiRows >> ss, 0);
      lDc[p].assign(MiRows >> ss, 0);
    }
  }

  int blk(int mir, int mic) const { return (mir >> 2) * g.bw + (mic >> 2); }
  bool inside(int r, int c) const { return r >= 0 && c >= 0 && r < MiRows && c < MiCols; }

  // ---- coefficients (5.11.39) ----
  int base_ctx(const int* q, int pos, int lg) const {
    const int N = 1 << lg, row = pos >> lg, col = pos & (N - 1);
    if (!row && !col) return 0;
    constexpr int off[5][2] = {{0, 1}, {1, 0}, {1, 1}, {0, 2}, {2, 0}};
    int mag = 0;
    for (auto& o : off) {
      const int rr = row + o[0], cc = col + o[1];
      if (rr < N && cc < N) mag += std::min(q[(rr << lg) + cc], 3);
    }
    return std::min((mag + 1) >> 1, 4) + kCoeffBaseOffset[std::min(row, 4)][std::min(col, 4)];
  }
  int br_ctx(const int* q, int pos, int lg) const {
    const int N = 1 << lg, row = pos >> lg, col = pos & (N - 1);
    constexpr int off[3][2] = {{0, 1}, {1, 0}, {1, 1}};
    int mag = 0;
    for (auto& o : off) {
      const int rr = row + o[0], cc = col + o[1];
      if (rr < N && cc < N) mag += std::min(q[(rr << lg) + cc], 15);
    }
    mag = std::min((mag + 1) >> 1, 6);
    if (!pos) return mag;
    return (row < 2 && col < 2) ? mag + 7 : mag + 14;
  }

  // Writer fast path of coeffs(): the levels come in scan order (lv[0..eob-1], the engine's
  // scan-packed layout), the contexts read a zero-padded raster of the coded magnitudes
  // (stride N + 4: no bounds checks) that is cleared again at the eob positions only.
  uint8_t qpad_[20 * 20] = {};
  // txb_skip context of a luma TB smaller than its block (the general luma context): from the
  // largest level context above and left of the TB
  int luma_skip_ctx(int x4, int y4, int w4) const {
    int top = 0, left = 0;
    for (int i = 0; i < w4; ++i) {
      if (x4 + i < (int)aLvl[0].size()) top = std::max<int>(top, aLvl[0][x4 + i]);
      if (y4 + i < (int)lLvl[0].size()) left = std::max<int>(left, lLvl[0][y4 + i]);
    }
    if (!top && !left) return 1;
    if (!top || !left) return 2 + (std::max(top, left) > 3);
    if (std::max(top, left) <= 3) return 4;
    return std::min(top, left) <= 3 ? 5 : 6;
  }
  // sub: a luma TB smaller than its block (a quadrant of a transform-split block)
  void coeffs_w(int plane, int lg, int x4, int y4, const int16_t* lv, int eob, bool is_inter, int intra_dir,
                bool sub = false) {
    const int N = 1 << lg, area = N * N, w4 = N >> 2, ptype = plane > 0, txc = lg - 2, S = N + 4;
    auto& AL = aLvl[plane];
    auto& AD = aDc[plane];
    auto& LL = lLvl[plane];
    auto& LD = lDc[plane];
    const int na = std::max(0, std::min(w4, (int)AL.size() - x4)), nl = std::max(0, std::min(w4, (int)LL.size() - y4));
    int ctx = sub ? luma_skip_ctx(x4, y4, w4) : 0;
    if (plane) {
      int above = 0, left = 0;
      for (int i = 0; i < na; ++i) above |= AL[x4 + i] | AD[x4 + i];
      for (int i = 0; i < nl; ++i) left |= LL[y4 + i] | LD[y4 + i];
      ctx = 7 + (above != 0) + (left != 0);
    }
    auto set_ctx = [&](int lvl, int dc) {
      for (int i = 0; i < na; ++i) AL[x4 + i] = (uint8_t)lvl, AD[x4 + i] = (uint8_t)dc;
      for (int i = 0; i < nl; ++i) LL[y4 + i] = (uint8_t)lvl, LD[y4 + i] = (uint8_t)dc;
    };
    int all_zero = eob == 0;
    io.sym(all_zero, cdf.txb_skip[txc][ctx], 2);
    if (all_zero) {
      set_ctx(0, 0);
      return;
    }
    if (plane == 0) {
      int s = 1;
      if (is_inter) io.sym(s, cdf.inter_tx[txc], 2);
      else io.sym(s, cdf.intra_tx[txc][intra_dir], 5);
    }
    const int ems = 2 * lg - 4;
    const int eobPt = eob <= 2 ? eob : floor_log2((unsigned)(eob - 1)) + 2;
    int s = eobPt - 1;
    io.sym(s, cdf.eob_pt[ems][ptype][0], ems + 5);
    if (eobPt >= 3) {
      const int rem = eob - ((1 << (eobPt - 2)) + 1);
      int bit = (rem >> (eobPt - 3)) & 1;
      io.sym(bit, cdf.eob_extra[txc][ptype][eobPt - 3], 2);
      for (int i = 1; i < eobPt - 2; ++i) {
        bit = (rem >> (eobPt - 3 - i)) & 1;
        io.lit(bit, 1);
      }
    }
    const ScanPad& sp = scan_pad();
    const int16_t* pad = lg == 4 ? sp.pad16 : sp.pad8;
    const uint8_t* boff = lg == 4 ? sp.off16 : sp.off8;
    uint8_t* Q = qpad_;
    C17* cb = cdf.base[txc][ptype];
    C17* cbr = cdf.br[std::min(txc, 3)][ptype];
    for (int c = eob - 1; c >= 0; --c) {
      const int pi = pad[c], a = std::abs((int)lv[c]);
      int level;
      if (c == eob - 1) {
        const int bctx = c == 0 ? 0 : (c <= area / 8 ? 1 : (c <= area / 4 ? 2 : 3));
        int v = std::min(a, 3) - 1;
        io.sym(v, cdf.base_eob[txc][ptype][bctx], 3);
        level = v + 1;
      } else {
        int v = std::min(a, 3);
        int bc = 0;
        if (c) {
          const int mag = std::min<int>(Q[pi + 1], 3) + std::min<int>(Q[pi + S], 3) + std::min<int>(Q[pi + S + 1], 3) +
                          std::min<int>(Q[pi + 2], 3) + std::min<int>(Q[pi + 2 * S], 3);
          bc = std::min((mag + 1) >> 1, 4) + boff[c];
        }
        io.sym(v, cb[bc], 4);
        level = v;
      }
      if (level > 2) {
        const int mag = std::min((Q[pi + 1] + Q[pi + S] + Q[pi + S + 1] + 1) >> 1, 6);
        const int row = pi / S, col = pi - row * S;
        const int bctx = !c ? mag : ((row < 2 && col < 2) ? mag + 7 : mag + 14);
        for (int k = 0; k < 4; ++k) {
          int v = std::min(a - level, 3);
          io.sym(v, cbr[bctx], 4);
          level += v;
          if (v < 3) break;
        }
      }
      Q[pi] = (uint8_t)level;  // <= 15
    }
    int dcs = 0;
    for (int i = 0; i < na; ++i) dcs += AD[x4 + i] == 1 ? -1 : (AD[x4 + i] == 2 ? 1 : 0);
    for (int i = 0; i < nl; ++i) dcs += LD[y4 + i] == 1 ? -1 : (LD[y4 + i] == 2 ? 1 : 0);
    const int dctx = dcs < 0 ? 1 : (dcs > 0 ? 2 : 0);
    int cul = 0, dcCat = 0;
    for (int c = 0; c < eob; ++c) {
      const int l = lv[c];
      Q[pad[c]] = 0;
      if (!l) continue;
      int sign = l < 0;
      if (c == 0) io.sym(sign, cdf.dc_sign[ptype][dctx], 2);
      else io.lit(sign, 1);
      const int a = std::abs(l);
      if (a >= 15) {  // Golomb of a - 14
        const int x = a - 14, length = floor_log2((unsigned)x) + 1;
        for (int i = 0; i < length; ++i) {
          int b = i == length - 1;
          io.lit(b, 1);
        }
        for (int i = length - 2; i >= 0; --i) {
          int b = (x >> i) & 1;
          io.lit(b, 1);
        }
      }
      if (c == 0) dcCat = sign ? 1 : 2;  // scan index 0 is position 0
      cul += std::min(a, 15);  // as the raster path: only culLevel != 0 reaches a context
    }
    set_ctx(std::min(63, cul), dcCat);
  }

  // one transform block; L = raster levels (writer: input, reader: output)
  void coeffs(int plane, int lg, int x4, int y4, int16_t* L, bool is_inter, int intra_dir, int eob_hint = -1,
              bool sub = false) {
    const int N = 1 << lg, area = N * N, w4 = N >> 2, ptype = plane > 0, txc = lg - 2;
    const int16_t* scan = lg == 4 ? scans().s16 : scans().s8;
    auto& AL = aLvl[plane];
    auto& AD = aDc[plane];
    auto& LL = lLvl[plane];
    auto& LD = lDc[plane];
    int ctx = sub ? luma_skip_ctx(x4, y4, w4) : 0;
    if (plane) {
      int above = 0, left = 0;
      for (int i = 0; i < w4; ++i) {
        if (x4 + i < (int)AL.size()) above |= AL[x4 + i] | AD[x4 + i];
        if (y4 + i < (int)LL.size()) left |= LL[y4 + i] | LD[y4 + i];
      }
      ctx = 7 + (above != 0) + (left != 0);
    }
    int eob = IO::kW && eob_hint >= 0 ? eob_hint : 0;
    if (IO::kW && eob_hint < 0)
      for (int c = area - 1; c >= 0; --c)
        if (L[scan[c]]) {
          eob = c + 1;
          break;
        }
    int all_zero = eob == 0;
    io.sym(all_zero, cdf.txb_skip[txc][ctx], 2);
    auto set_ctx = [&](int lvl, int dc) {
      for (int i = 0; i < w4; ++i) {
        if (x4 + i < (int)AL.size()) AL[x4 + i] = (uint8_t)lvl, AD[x4 + i] = (uint8_t)dc;
        if (y4 + i < (int)LL.size()) LL[y4 + i] = (uint8_t)lvl, LD[y4 + i] = (uint8_t)dc;
      }
    };
    if (all_zero) {
      if (!IO::kW) std::memset(L, 0, sizeof(int16_t) * area);
      set_ctx(0, 0);
      return;
    }
    if (plane == 0) {  // transform_type: DCT_DCT is symbol 1 of both reduced sets
      int s = 1;
      if (is_inter) io.sym(s, cdf.inter_tx[txc], 2);
      else io.sym(s, cdf.intra_tx[txc][intra_dir], 5);
      if (s != 1) throw std::runtime_error("av1 oracle: transform type outside the encoder subset");
    }
    const int ems = 2 * lg - 4;  // eobMultisize: 8x8 -> 2 (eob_pt_64), 16x16 -> 4 (eob_pt_256)
    int eobPt = 0;
    if (IO::kW) eobPt = eob <= 2 ? eob : floor_log2((unsigned)(eob - 1)) + 2;
    int s = eobPt - 1;
    io.sym(s, cdf.eob_pt[ems][ptype][0], ems + 5);
    eobPt = s + 1;
    const int rem = IO::kW && eobPt >= 3 ? eob - ((1 << (eobPt - 2)) + 1) : 0;
    int e = eobPt < 2 ? eobPt : (1 << (eobPt - 2)) + 1;
    if (eobPt - 3 >= 0) {
      int bit = (rem >> (eobPt - 3)) & 1;
      io.sym(bit, cdf.eob_extra[txc][ptype][eobPt - 3], 2);
      if (bit) e += 1 << (eobPt - 3);
      for (int i = 1; i < std::max(1, eobPt - 2); ++i) {
        const int sh = std::max(1, eobPt - 2) - 1 - i;
        bit = (rem >> sh) & 1;
        io.lit(bit, 1);
        if (bit) e += 1 << sh;
      }
    }
    if (IO::kW && e != eob) throw std::runtime_error("av1 writer: eob coding mismatch");
    eob = e;
    if (eob > area) throw std::runtime_error("av1 oracle: eob out of range");
    int q[256];
    std::memset(q, 0, sizeof(int) * area);
    for (int c = eob - 1; c >= 0; --c) {
      const int pos = scan[c];
      const int a = IO::kW ? std::abs((int)L[pos]) : 0;
      int level;
      if (c == eob - 1) {
        const int bctx = c == 0 ? 0 : (c <= area / 8 ? 1 : (c <= area / 4 ? 2 : 3));
        int v = std::min(a, 3) - 1;
        io.sym(v, cdf.base_eob[txc][ptype][bctx], 3);
        level = v + 1;
      } else {
        int v = std::min(a, 3);
        io.sym(v, cdf.base[txc][ptype][base_ctx(q, pos, lg)], 4);
        level = v;
      }
      if (level > 2) {
        for (int k = 0; k < 4; ++k) {
          int v = IO::kW ? std::min(a - level, 3) : 0;
          io.sym(v, cdf.br[std::min(txc, 3)][ptype][br_ctx(q, pos, lg)], 4);
          level += v;
          if (v < 3) break;
        }
      }
      q[pos] = level;
    }
    // dc_sign context from the neighbours' dc categories
    int dcs = 0;
    for (int i = 0; i < w4; ++i) {
      if (x4 + i < (int)AD.size()) dcs += AD[x4 + i] == 1 ? -1 : (AD[x4 + i] == 2 ? 1 : 0);
      if (y4 + i < (int)LD.size()) dcs += LD[y4 + i] == 1 ? -1 : (LD[y4 + i] == 2 ? 1 : 0);
    }
    const int dctx = dcs < 0 ? 1 : (dcs > 0 ? 2 : 0);
    int cul = 0, dcCat = 0;
    for (int c = 0; c < eob; ++c) {
      const int pos = scan[c];
      int sign = 0;
      if (q[pos]) {
        sign = IO::kW ? (L[pos] < 0) : 0;
        if (c == 0) io.sym(sign, cdf.dc_sign[ptype][dctx], 2);
        else io.lit(sign, 1);
      }
      if (q[pos] > 14) {
        const int x = IO::kW ? std::abs((int)L[pos]) - 14 : 0;
        int length = 0;
        if (IO::kW) {
          length = floor_log2((unsigned)x) + 1;
          for (int i = 0; i < length; ++i) {
            int b = i == length - 1;
            io.lit(b, 1);
          }
          for (int i = length - 2; i >= 0; --i) {
            int b = (x >> i) & 1;
            io.lit(b, 1);
          }
        } else {
          int b = 0;
          do {
            ++length;
            io.lit(b, 1);
            if (length > 20) throw std::runtime_error("av1 oracle: bad golomb length");
          } while (!b);
          int xx = 1;
          for (int i = length - 2; i >= 0; --i) {
            io.lit(b, 1);
            xx = (xx << 1) | b;
          }
          q[pos] = xx + 14;
        }
      }
      if (pos == 0 && q[pos] > 0) dcCat = sign ? 1 : 2;
      q[pos] &= 0xFFFFF;
      cul += q[pos];
      if (!IO::kW) L[pos] = (int16_t)(sign ? -q[pos] : q[pos]);
    }
    if (!IO::kW)
      for (int i = 0; i < area; ++i)
        if (!q[i]) L[i] = 0;
    set_ctx(std::min(63, cul), dcCat);
  }

  // ---- MV stack (7.10.2, single reference, no temporal candidates) ----
  MvStack S;
  int found = 0, newcount = 0;
  void search_stack(int b, int weight) {
    int m[2] = {mv_row(mv[b]), mv_col(mv[b])};
    for (int& v : m)
      if (v & 1) v += v > 0 ? -1 : 1;  // lower_mv_precision (allow_high_precision_mv = 0)
    if (ymode[b] == NEWMV) ++newcount;
    found = 1;
    for (int i = 0; i < S.n; ++i)
      if (S.mv[i][0] == m[0] && S.mv[i][1] == m[1]) {
        S.w[i] += weight;
        return;
      }
    if (S.n < 8) {
      S.mv[S.n][0] = m[0];
      S.mv[S.n][1] = m[1];
      S.w[S.n] = weight;
      ++S.n;
    }
  }
  void add_cand(int r, int c, int weight) {
    const int b = blk(r, c);
    if (!mode_inter(mode[b])) return;
    search_stack(b, weight);
  }
  int cur4 = 4;  // width (= height) of the current block in 4x4 units
  int cand4(int r, int c) const { return 4 << mode_bsz(mode[blk(r, c)]); }
  void scan_row(int mir, int mic, int dr) {
    const int bw4 = cur4, end4 = std::min(std::min(bw4, MiCols - mic), 16);
    const bool step16 = bw4 >= 16;
    int dc = 0;
    if (std::abs(dr) > 1) {
      dr += mir & 1;
      dc = 1 - (mic & 1);
    }
    for (int i = 0; i < end4;) {
      const int r = mir + dr, c = mic + dc + i;
      if (!inside(r, c)) break;
      int len = std::min(bw4, cand4(r, c));
      if (std::abs(dr) > 1) len = std::max(2, len);
      if (step16) len = std::max(4, len);
      add_cand(r, c, 2 * len);
      i += len;
    }
  }
  void scan_col(int mir, int mic, int dc) {
    const int bh4 = cur4, end4 = std::min(std::min(bh4, MiRows - mir), 16);
    const bool step16 = bh4 >= 16;
    int dr = 0;
    if (std::abs(dc) > 1) {
      dr = 1 - (mir & 1);
      dc += mic & 1;
    }
    for (int i = 0; i < end4;) {
      const int r = mir + dr + i, c = mic + dc;
      if (!inside(r, c)) break;
      int len = std::min(bh4, cand4(r, c));
      if (std::abs(dc) > 1) len = std::max(2, len);
      if (step16) len = std::max(4, len);
      add_cand(r, c, 2 * len);
      i += len;
    }
  }
  void scan_point(int mir, int mic, int dr, int dc) {
    const int r = mir + dr, c = mic + dc;
    if (inside(r, c) && coded[blk(r, c)]) add_cand(r, c, 4);
  }
  void sort_stack(int start, int end) {
    while (end > start) {
      int ne = start;
      for (int i = start + 1; i < end; ++i)
        if (S.w[i - 1] < S.w[i]) {
          std::swap(S.w[i - 1], S.w[i]);
          std::swap(S.mv[i - 1][0], S.mv[i][0]);
          std::swap(S.mv[i - 1][1], S.mv[i][1]);
          ne = i;
        }
      end = ne;
    }
  }
  void find_mv_stack(int mir, int mic) {
    S = MvStack();
    newcount = 0;
    found = 0;
    scan_row(mir, mic, -1);
    int fa = found;
    found = 0;
    scan_col(mir, mic, -1);
    int fl = found;
    found = 0;
    scan_point(mir, mic, -1, cur4);
    if (found) fa = 1;
    const int close = fa + fl, nearest = S.n, nnew = newcount;
    for (int i = 0; i < nearest; ++i) S.w[i] += 640;
    found = 0;
    scan_point(mir, mic, -1, -1);
    if (found) fa = 1;
    found = 0;
    scan_row(mir, mic, -3);
    if (found) fa = 1;
    found = 0;
    scan_col(mir, mic, -3);
    if (found) fl = 1;
    found = 0;
    scan_row(mir, mic, -5);
    if (found) fa = 1;
    found = 0;
    scan_col(mir, mic, -5);
    if (found) fl = 1;
    const int total = fa + fl;
    sort_stack(0, nearest);
    sort_stack(nearest, S.n);
    if (S.n < 2) {  // extra_search
      const int num4 = std::min(std::min(std::min(16, cur4), MiCols - mic), std::min(std::min(16, cur4), MiRows - mir));
      for (int pass = 0; pass < 2 && S.n < 2; ++pass) {
        for (int idx = 0; idx < num4 && S.n < 2;) {
          const int r = pass ? mir + idx : mir - 1, c = pass ? mic - 1 : mic + idx;
          if (!inside(r, c)) break;
          idx += cand4(r, c);
          const int b = blk(r, c);
          if (!mode_inter(mode[b])) continue;
          const int m0 = mv_row(mv[b]), m1 = mv_col(mv[b]);
          int i = 0;
          for (; i < S.n; ++i)
            if (S.mv[i][0] == m0 && S.mv[i][1] == m1) break;
          if (i == S.n) {
            S.mv[i][0] = m0;
            S.mv[i][1] = m1;
            S.w[i] = 2;
            ++S.n;
          }
        }
      }
      for (int i = S.n; i < 2; ++i) S.mv[i][0] = S.mv[i][1] = 0;  // GlobalMvs (identity)
    }
    for (int i = 0; i < S.n; ++i) {
      const int top = -(mir * 4 * 8), bottom = (MiRows - cur4 - mir) * 4 * 8, border = 128 + cur4 * 4 * 8;
      const int left = -(mic * 4 * 8), right = (MiCols - cur4 - mic) * 4 * 8;
      S.mv[i][0] = clip3(top - border, bottom + border, S.mv[i][0]);
      S.mv[i][1] = clip3(left - border, right + border, S.mv[i][1]);
    }
    if (close == 0) {
      S.newctx = std::min(total, 1);
      S.refctx = total;
    } else if (close == 1) {
      S.newctx = 3 - std::min(nnew, 1);
      S.refctx = 2 + total;
    } else {
      S.newctx = 5 - std::min(nnew, 1);
      S.refctx = 5;
    }
    S.zeroctx = 0;
  }
  int drl_ctx(int idx) const {
    const int a = idx < 8 ? S.w[idx] : 0, b = idx + 1 < 8 ? S.w[idx + 1] : 0;
    if (a >= 640 && b >= 640) return 0;
    if (a >= 640) return 1;
    return 2;
  }

  void mv_component(int comp, int& v) {
    int sign = v < 0, z = std::abs(v) - 1;
    int cls = IO::kW ? (z < 16 ? 0 : floor_log2((unsigned)z) - 3) : 0;
    io.sym(sign, cdf.mv_sign[comp], 2);
    io.sym(cls, cdf.mv_class[comp], 11);
    int d, fr;
    if (cls == 0) {
      d = (z >> 3) & 1;
      fr = (z >> 1) & 3;
      io.sym(d, cdf.class0_bit[comp], 2);
      io.sym(fr, cdf.class0_fr[comp][d], 4);
      z = (d << 3) | (fr << 1) | 1;
    } else {
      const int off = IO::kW ? z - (1 << (cls + 3)) : 0;
      d = 0;
      for (int b = 0; b < cls; ++b) {
        int bit = (off >> (3 + b)) & 1;
        io.sym(bit, cdf.mv_bits[comp][b], 2);
        d |= bit << b;
      }
      fr = (off >> 1) & 3;
      io.sym(fr, cdf.mv_fr[comp], 4);
      z = (1 << (cls + 3)) + ((d << 3) | (fr << 1) | 1);
    }
    const int mag = z + 1;
    if (IO::kW && mag != std::abs(v)) throw std::runtime_error("av1 writer: mv not representable (odd?)");
    v = sign ? -mag : mag;
  }
  void mv_diff(int* diff) {
    int j = (diff[0] != 0) * 2 + (diff[1] != 0);
    io.sym(j, cdf.mv_joint, 4);
    if (!IO::kW) diff[0] = diff[1] = 0;
    if (j == 2 || j == 3) mv_component(0, diff[0]);
    if (j == 1 || j == 3) mv_component(1, diff[1]);
  }

  // ---- block (decode_block for a 16x16 block) ----
  void intra_modes(int b, bool kf, bool availU, bool availL) {
    int y = mode_y(mode[b]), uvm = mode_uv(mode[b]);
    if (kf) {
      const int am = availU ? ymode[b - g.bw] : DC_PRED, lm = availL ? ymode[b - 1] : DC_PRED;
      io.sym(y, cdf.kf_y[kIntraModeCtx[am]][kIntraModeCtx[lm]], 13);
    } else {
      io.sym(y, cdf.y_mode[2], 13);  // Size_Group[BLOCK_16X16] = 2
    }
    // angle deltas (av1_enc.h "directional intra"): only 90 <= pAngle <= 180 is in the subset
    auto angle_delta = [&](int m, int delta) {
      if (IO::kW && !dir_delta_ok(m, delta)) throw std::runtime_error("av1 writer: angle delta outside the encoder subset");
      int ad = 3 + delta;
      io.sym(ad, cdf.angle[m - V_PRED], 7);
      if (!dir_delta_ok(m, ad - 3)) throw std::runtime_error("av1 oracle: angle delta outside the encoder subset");
      return ad - 3;
    };
    int yd = 0, uvd = 0;
    if (directional(y)) yd = angle_delta(y, IO::kW ? mode_angle_y(mode[b]) : 0);
    else if (IO::kW && mode_angle_y(mode[b])) throw std::runtime_error("av1 writer: angle delta on a non-directional mode");
    io.sym(uvm, cdf.uv[1][y], 14);  // CfL allowed for 16x16
    int au = 0, av = 0;
    if (uvm == UV_CFL_PRED) {  // read_cfl_alphas: joint sign, then |alpha| - 1 of each nonzero plane
      if (IO::kW) {
        au = mode_cfl_u(mode[b]), av = mode_cfl_v(mode[b]);
        if ((!au && !av) || std::abs(au) > 16 || std::abs(av) > 16)
          throw std::runtime_error("av1 writer: CfL block without a codable alpha pair");
      }
      auto sgn = [](int a) { return a == 0 ? 0 : (a < 0 ? 1 : 2); };  // CFL_SIGN_ZERO / NEG / POS
      int joint = sgn(au) * 3 + sgn(av) - 1;
      io.sym(joint, cdf.cfl_sign, 8);
      const int su = (joint + 1) / 3, sv = (joint + 1) % 3;
      int magu = std::abs(au) - 1, magv = std::abs(av) - 1;
      if (su) {
        io.sym(magu, cdf.cfl_alpha[(su - 1) * 3 + sv], 16);
        au = su == 1 ? -(magu + 1) : magu + 1;
      }
      if (sv) {
        io.sym(magv, cdf.cfl_alpha[(sv - 1) * 3 + su], 16);
        av = sv == 1 ? -(magv + 1) : magv + 1;
      }
    } else if (directional(uvm)) {
      uvd = angle_delta(uvm, IO::kW ? mode_angle_uv(mode[b]) : 0);
    }
    ymode[b] = (uint8_t)y;
    if (!IO::kW) {
      mode[b] = pack_mode(0, y, uvm, mode_skip(mode[b]), mode_nz(mode[b]));
      if (uvm == UV_CFL_PRED) mode[b] = with_cfl(mode[b], au, av);
      else if (uvd) mode[b] = with_angle_uv(mode[b], uvd);
      if (yd) mode[b] = with_angle_y(mode[b], yd);
    }
  }

  void inter_modes(int b, int mir, int mic, bool availU, bool availL) {
    int cnt = 0;  // neighbours referencing LAST
    if (availU && mode_inter(mode[b - g.bw])) ++cnt;
    if (availL && mode_inter(mode[b - 1])) ++cnt;
    auto rc = [](int c0, int c1) { return c0 == c1 ? 1 : (c0 < c1 ? 0 : 2); };
    int v = 0;
    io.sym(v, cdf.single_ref[rc(cnt, 0)][0], 2);  // p1: LAST..GOLDEN vs BWD..ALT
    if (v) throw std::runtime_error("av1 oracle: reference outside the encoder subset");
    io.sym(v, cdf.single_ref[rc(cnt, 0)][2], 2);  // p3: LAST/LAST2 vs LAST3/GOLDEN
    if (v) throw std::runtime_error("av1 oracle: reference outside the encoder subset");
    io.sym(v, cdf.single_ref[rc(cnt, 0)][3], 2);  // p4: LAST vs LAST2
    if (v) throw std::runtime_error("av1 oracle: reference outside the encoder subset");
    find_mv_stack(mir, mic);
    int m[2] = {mv_row(mv[b]), mv_col(mv[b])};
    int ym = NEWMV, idx = 0;
    if (IO::kW) {
      auto eq = [&](int k) { return S.mv[k][0] == m[0] && S.mv[k][1] == m[1]; };
      if (eq(0)) ym = NEARESTMV;
      else if (!m[0] && !m[1]) ym = GLOBALMV;
      else {
        for (int k = 1; k <= 3; ++k)
          if ((k == 1 || S.n > k) && eq(k)) {
            ym = NEARMV;
            idx = k;
            break;
          }
        if (ym == NEWMV && S.n > 1) {  // predictor with the cheapest difference
          int best = 1 << 30;
          for (int k = 0; k < 3 && (k == 0 || S.n > k); ++k) {
            const int bits = mv_comp_bits(m[0] - S.mv[k][0]) + mv_comp_bits(m[1] - S.mv[k][1]);
            if (bits < best) best = bits, idx = k;
          }
        }
      }
    }
    int nm = ym != NEWMV;
    io.sym(nm, cdf.new_mv[S.newctx], 2);
    if (!nm) ym = NEWMV;
    else {
      int zm = ym != GLOBALMV;
      io.sym(zm, cdf.zero_mv[S.zeroctx], 2);
      if (!zm) ym = GLOBALMV;
      else {
        int rm = ym == NEARMV;
        io.sym(rm, cdf.ref_mv[S.refctx], 2);
        ym = rm ? NEARMV : NEARESTMV;
      }
    }
    if (ym == NEWMV) {
      int ri = 0;
      for (int k = 0; k < 2; ++k)
        if (S.n > k + 1) {
          int bit = idx != k;
          io.sym(bit, cdf.drl[drl_ctx(k)], 2);
          if (!bit) {
            ri = k;
            break;
          }
          ri = k + 1;
        }
      idx = ri;
    } else if (ym == NEARMV) {
      int ri = 1;
      for (int k = 1; k < 3; ++k)
        if (S.n > k + 1) {
          int bit = idx != k;
          io.sym(bit, cdf.drl[drl_ctx(k)], 2);
          if (!bit) {
            ri = k;
            break;
          }
          ri = k + 1;
        }
      idx = ri;
    }
    if (ym == GLOBALMV) m[0] = m[1] = 0;
    else if (ym == NEARESTMV) m[0] = S.mv[0][0], m[1] = S.mv[0][1];
    else if (ym == NEARMV) {
      if (idx > 7) throw std::runtime_error("av1 oracle: bad ref mv idx");
      m[0] = S.mv[idx][0], m[1] = S.mv[idx][1];
    } else {
      const int pos = S.n <= 1 ? 0 : idx;
      int diff[2] = {m[0] - S.mv[pos][0], m[1] - S.mv[pos][1]};
      mv_diff(diff);
      m[0] = S.mv[pos][0] + diff[0];
      m[1] = S.mv[pos][1] + diff[1];
    }
    if (IO::kW && (m[0] != mv_row(mv[b]) || m[1] != mv_col(mv[b])))
      throw std::runtime_error("av1 writer: mv mode reconstruction mismatch");
    ymode[b] = (uint8_t)ym;
    if (!IO::kW) {
      mv[b] = pack_mv(m[0], m[1]);
      mode[b] = pack_mode(1, 0, 0, mode_skip(mode[b]), mode_nz(mode[b]));
    }
  }

  void block(int mir, int mic, int bsl) {
    const int b = blk(mir, mic);
    const bool availU = mir > 0, availL = mic > 0, kf = fp.key != 0;
    cur4 = 1 << bsl;
    int skip = mode_skip(mode[b]);
    const int sctx = (availU ? mode_skip(mode[b - g.bw]) : 0) + (availL ? mode_skip(mode[b - 1]) : 0);
    io.sym(skip, cdf.skip[sctx], 2);
    if (!IO::kW) mode[b] = pack_mode(0, 0, 0, skip, 0);
    if (!skip) {  // read_cdef
      const int sb = (mir >> 4) * g.sbw + (mic >> 4);
      if (cdef_seen[sb] == -1) {
        int v = IO::kW ? cdef_idx[sb] : 0;
        if (IO::kW && (v < 0 || v >= (1 << fp.cdef_bits))) throw std::runtime_error("av1 writer: cdef_idx missing");
        io.lit(v, fp.cdef_bits);
        cdef_seen[sb] = (int8_t)v;
        if (!IO::kW) cdef_idx[sb] = (int8_t)v;
      }
    }
    int inter = 0;
    if (!kf) {
      inter = mode_inter(mode[b]);
      const int aI = availU ? !mode_inter(mode[b - g.bw]) : 0, lI = availL ? !mode_inter(mode[b - 1]) : 0;
      int ictx = 0;
      if (availU && availL) ictx = (lI && aI) ? 3 : (lI || aI);
      else if (availU || availL) ictx = 2 * (availU ? aI : lI);
      io.sym(inter, cdf.is_inter[ictx], 2);
    }
    if (bsl > 2 && !(skip && inter)) throw std::runtime_error("av1: merged blocks are skip inter blocks only");
    const int wsplit = IO::kW ? mode_tx(mode[b]) : 0, wqmask = IO::kW ? (int)((mode[b] >> 15) & 15) : 0;
    if (wsplit && (skip || !inter || bsl > 2 || !tx_select))
      throw std::runtime_error(
          "av1 writer: transform split on a skip, intra or merged block (or a frame without the tool)");
    if (inter) inter_modes(b, mir, mic, availU, availL);
    else intra_modes(b, kf, availU, availL);
    // transform size (read_block_tx_size; av1_enc.h "transform split")
    int split = 0;
    if (tx_select) {
      auto set_tx = [&](int r4, int c4, int n4, int px) {
        for (int i = 0; i < n4; ++i) aTx[c4 + i] = lTx[r4 + i] = (uint8_t)px;
      };
      if (inter && !skip) {  // read_var_tx_size: 16x16, then depth 1 (8x8); 4x4 is outside the subset
        split = wsplit;
        io.sym(split, cdf.txfm_split[12 + (aTx[mic] < 16) + (lTx[mir] < 16)], 2);
        if (split) {
          for (int k = 0; k < 4; ++k) {
            const int r = mir + (k >> 1) * 2, c = mic + (k & 1) * 2;
            int deeper = 0;
            io.sym(deeper, cdf.txfm_split[15 + (aTx[c] < 8) + (lTx[r] < 8)], 2);
            if (deeper) throw std::runtime_error("av1 oracle: 4x4 transforms are outside the encoder subset");
            set_tx(r, c, 2, 8);
          }
        } else {
          set_tx(mir, mic, 4, 16);
        }
      } else if (!inter) {  // read_tx_size: tx_depth 0 of the 16x16 category
        int above = aTx[mic] >= 16, left = lTx[mir] >= 16;
        if (availU && mode_inter(mode[b - g.bw])) above = (16 << mode_bsz(mode[b - g.bw])) >= 16;
        if (availL && mode_inter(mode[b - 1])) left = (16 << mode_bsz(mode[b - 1])) >= 16;
        int depth = 0;
        io.sym(depth, cdf.tx_size[(availU ? above : 0) + (availL ? left : 0)], 3);
        if (depth) throw std::runtime_error("av1 oracle: intra transform split is outside the encoder subset");
        set_tx(mir, mic, 4, 16);
      } else {  // skip inter blocks take their block size
        set_tx(mir, mic, cur4, std::min(64, cur4 * 4));
      }
    }
    // residual
    int nz = 0, qmask = 0;
    const int x4 = mic, y4 = mir;
    if (IO::kW && !skip) {
      for (int p = 0; p < 3; ++p) {
        const int lg = p ? 3 : 4, area = 1 << (2 * lg);
        const int16_t* lv = nullptr;
        int eob = 0;
        int16_t tmp[256];
        if (p == 0 && split) {  // four 8x8 TBs in quadrant raster order
          const int16_t* rec = scan_in[0] && scan_off[0][b] >= 0 ? scan_in[0] + scan_off[0][b] : nullptr;
          const int16_t* src = scan_in[0] ? nullptr : lev_in(0, b);
          for (int k = 0; k < 4; ++k) {
            eob = 0;
            lv = nullptr;
            if (scan_in[0]) {  // the records of the nonzero quadrants back to back
              if ((wqmask >> k & 1) && rec) {
                eob = rec[0];
                lv = rec + 1;
                rec += 1 + eob;
              }
            } else if (src) {
              for (int c = 0; c < 64; ++c) {
                tmp[c] = src[k * 64 + scans().s8[c]];
                if (tmp[c]) eob = c + 1;
              }
              lv = tmp;
            }
            if ((eob != 0) != ((wqmask >> k & 1) != 0))
              throw std::runtime_error("av1 writer: quadrant mask of a transform-split block disagrees with its levels");
            coeffs_w(0, 3, x4 + (k & 1) * 2, y4 + (k >> 1) * 2, lv, eob, true, ymode[b], true);
            if (eob) qmask |= 1 << k;
          }
          if (!qmask) throw std::runtime_error("av1 writer: transform-split block with all-zero quadrants");
          nz |= 1;
          continue;
        }
        if (scan_in[p]) {  // engine layout: [eob, levels in scan order] per nonzero TB
          const int32_t o = scan_off[p][b];
          if (o >= 0) {
            eob = scan_in[p][o];
            lv = scan_in[p] + o + 1;
          }
        } else if (const int16_t* src = lev_in(p, b)) {  // raster input: to scan order
          const int16_t* sc = lg == 4 ? scans().s16 : scans().s8;
          for (int c = 0; c < area; ++c) {
            tmp[c] = src[sc[c]];
            if (tmp[c]) eob = c + 1;
          }
          lv = tmp;
        }
        coeffs_w(p, lg, p ? x4 >> 1 : x4, p ? y4 >> 1 : y4, lv, eob, inter != 0, ymode[b]);
        if (eob) nz |= 1 << p;
      }
      if (nz != mode_nz(mode[b])) throw std::runtime_error("av1 writer: nonzero mask mismatch");
      if (nz == 0) throw std::runtime_error("av1: non-skip block without coefficients");
    } else if (!skip) {
      for (int p = 0; p < 3; ++p) {
        const int lg = p ? 3 : 4;
        int16_t tmp[256];
        int16_t* L = tmp;
        if (!IO::kW && p == 0 && split) {  // four 8x8 rasters in the block's 256 slots
          for (int k = 0; k < 4; ++k) {
            int16_t* Lq = lev_out[0] + ((size_t)b << 8) + k * 64;
            coeffs(0, 3, x4 + (k & 1) * 2, y4 + (k >> 1) * 2, Lq, true, ymode[b], -1, true);
            for (int i = 0; i < 64; ++i)
              if (Lq[i]) {
                qmask |= 1 << k;
                break;
              }
          }
          if (qmask) nz |= 1;
          continue;
        }
        if (IO::kW) {
          const int16_t* src = lev_in(p, b);
          if (src) std::memcpy(tmp, src, sizeof(int16_t) << (2 * lg));
          else std::memset(tmp, 0, sizeof(int16_t) << (2 * lg));
        } else {
          L = lev_out[p] + ((size_t)b << (2 * lg));
        }
        int hint = -1;
        if (IO::kW && eob_in[p]) hint = eob_off[p][b] < 0 ? 0 : eob_in[p][eob_off[p][b]];
        coeffs(p, lg, p ? x4 >> 1 : x4, p ? y4 >> 1 : y4, L, inter != 0, ymode[b], hint);
        for (int i = 0; i < (1 << (2 * lg)); ++i)
          if (L[i]) {
            nz |= 1 << p;
            break;
          }
      }
      if (IO::kW && nz != mode_nz(mode[b])) throw std::runtime_error("av1 writer: nonzero mask mismatch");
      if (nz == 0) throw std::runtime_error("av1: non-skip block without coefficients");
    } else {
      for (int p = 0; p < 3; ++p) {  // reset_block_context
        const int ss = p ? 1 : 0, w4 = cur4 >> ss;
        for (int i = 0; i < w4; ++i) {
          aLvl[p][(x4 >> ss) + i] = aDc[p][(x4 >> ss) + i] = 0;
          lLvl[p][(y4 >> ss) + i] = lDc[p][(y4 >> ss) + i] = 0;
        }
        if (!IO::kW) std::memset(lev_out[p] + ((size_t)b << (p ? 6 : 8)), 0, sizeof(int16_t) << (p ? 6 : 8));
      }
    }
    if (!IO::kW) {
      mode[b] = with_bsz((mode[b] & ~(7u << 10)) | ((uint32_t)nz << 10), bsl - 2);
      if (split) mode[b] = with_tx_split(mode[b], qmask);
    }
    const int n16 = 1 << (bsl - 2);  // 16x16 cells per side of this block
    for (int dy = 0; dy < n16; ++dy)
      for (int dx = 0; dx < n16; ++dx) {
        const int c = b + dy * g.bw + dx;
        if (!IO::kW) mode[c] = mode[b], mv[c] = mv[b];
        ymode[c] = ymode[b];
        coded[c] = 1;
      }
  }

  // ---- loop restoration unit syntax (5.11.58 read_lr_unit, SGRPROJ frame type) ----
  void ns(int& v, int n) {  // non-symmetric unsigned literal of n values
    const int w = floor_log2((unsigned)n) + 1, m = (1 << w) - n;
    if (IO::kW) {
      if (v < m) {
        io.lit(v, w - 1);
      } else {
        int hi = (v + m) >> 1, ex = (v + m) & 1;
        io.lit(hi, w - 1);
        io.lit(ex, 1);
      }
      return;
    }
    int x = 0;
    io.lit(x, w - 1);
    if (x < m) {
      v = x;
      return;
    }
    int ex = 0;
    io.lit(ex, 1);
    v = (x << 1) - m + ex;
  }
  void subexp(int& v, int nsyms, int k) {
    int i = 0, mk = 0;
    for (;;) {
      const int b2 = i ? k + i - 1 : k, a = 1 << b2;
      if (nsyms <= mk + 3 * a) {
        int x = v - mk;
        ns(x, nsyms - mk);
        v = x + mk;
        return;
      }
      int more = IO::kW ? v >= mk + a : 0;
      io.lit(more, 1);
      if (!more) {
        int x = v - mk;
        io.lit(x, b2);
        v = x + mk;
        return;
      }
      ++i;
      mk += a;
    }
  }
  static int recenter(int r, int v) { return v > 2 * r ? v : (v >= r ? (v - r) << 1 : ((r - v) << 1) - 1); }
  static int inv_recenter(int r, int v) { return v > 2 * r ? v : ((v & 1) ? r - ((v + 1) >> 1) : r + (v >> 1)); }
  void signed_subexp_ref(int& v, int low, int high, int k, int r) {
    const int mx = high - low, rr = r - low;
    int x = 0;
    if (IO::kW) {
      const int u = v - low;
      x = (rr << 1) <= mx ? recenter(rr, u) : recenter(mx - 1 - rr, mx - 1 - u);
    }
    subexp(x, mx, k);
    const int u = (rr << 1) <= mx ? inv_recenter(rr, x) : mx - 1 - inv_recenter(mx - 1 - rr, x);
    if (IO::kW && u + low != v) throw std::runtime_error("av1 writer: subexp mismatch");
    v = u + low;
  }
  void lr_unit(int p, int u) {
    int32_t* P = lr + ((size_t)p * g.lr_nu() + u) * 3;
    int on = P[0] >= 0;
    io.sym(on, cdf.use_sgrproj, 2);
    if (!on) {
      if (!IO::kW) P[0] = -1, P[1] = P[2] = 0;
      return;
    }
    int set = P[0];
    io.lit(set, 4);
    const int r0 = sgr_param(set, 0), r1 = sgr_param(set, 2);
    int x0 = P[1], x1 = P[2];
    if (r0) signed_subexp_ref(x0, kXqdMin0, kXqdMax0 + 1, 4, ref_xqd[p][0]);
    else x0 = 0;
    ref_xqd[p][0] = x0;
    if (r1) signed_subexp_ref(x1, kXqdMin1, kXqdMax1 + 1, 4, ref_xqd[p][1]);
    else x1 = clip3(kXqdMin1, kXqdMax1, 128 - ref_xqd[p][0]);
    if (IO::kW && (x0 != P[1] || x1 != P[2])) throw std::runtime_error("av1 writer: sgr weights not representable");
    ref_xqd[p][1] = x1;
    P[0] = set, P[1] = x0, P[2] = x1;
  }
  void read_lr(int sr, int sc) {
    for (int p = 0; p < 3; ++p) {
      if (!lr_type[p]) continue;
      const int sbs = p ? 32 : 64, x0 = sc * sbs, y0 = sr * sbs;
      for (int uy = 0; uy < g.lr_uy(p); ++uy)
        for (int ux = 0; ux < g.lr_ux(p); ++ux)
          if (ux * 64 >= x0 && ux * 64 < x0 + sbs && uy * 64 >= y0 && uy * 64 < y0 + sbs) lr_unit(p, uy * g.lr_ux(p) + ux);
    }
  }

  void partition(int mir, int mic, int bsl) {
    if (mir >= MiRows || mic >= MiCols) return;
    const bool availU = mir > 0, availL = mic > 0;
    const int half = (1 << bsl) >> 1;
    const bool hasRows = mir + half < MiRows, hasCols = mic + half < MiCols;
    // PARTITION_SPLIT down to 16x16, then PARTITION_NONE; NONE at 32 / 64 for merged blocks
    int part = bsl > 2 ? 3 : 0;
    if (IO::kW && bsl > 2 && hasRows && hasCols && mode_bsz(mode[blk(mir, mic)]) == bsl - 2) part = 0;
    const int above = availU && 2 + mode_bsz(mode[blk(mir - 1, mic)]) < bsl;
    const int left = availL && 2 + mode_bsz(mode[blk(mir, mic - 1)]) < bsl;
    uint16_t* c = cdf.partition[bsl - 1][left * 2 + above];
    if (hasRows && hasCols) {
      io.sym(part, c, 10);
    } else if (hasCols) {  // split_or_horz
      const int ps = sym_prob(c, 2) + sym_prob(c, 3) + sym_prob(c, 4) + sym_prob(c, 6) + sym_prob(c, 7) +
                     sym_prob(c, 9);
      int bit = part == 3;
      io.boolp(bit, 32768 - ps);
      part = bit ? 3 : 1;
    } else if (hasRows) {  // split_or_vert
      const int ps = sym_prob(c, 1) + sym_prob(c, 3) + sym_prob(c, 4) + sym_prob(c, 5) + sym_prob(c, 6) +
                     sym_prob(c, 8);
      int bit = part == 3;
      io.boolp(bit, 32768 - ps);
      part = bit ? 3 : 2;
    } else {
      part = 3;
    }
    if (part == 3 && bsl > 2) {
      partition(mir, mic, bsl - 1);
      partition(mir, mic + half, bsl - 1);
      partition(mir + half, mic, bsl - 1);
      partition(mir + half, mic + half, bsl - 1);
    } else if (part == 0) {
      block(mir, mic, bsl);
    } else {
      throw std::runtime_error("av1 oracle: partition outside the encoder subset");
    }
  }

  void tile() {
    for (int p = 0; p < 3; ++p) ref_xqd[p][0] = kXqdMid0, ref_xqd[p][1] = kXqdMid1;
    for (int sr = 0; sr < g.sbh; ++sr) {
      for (int p = 0; p < 3; ++p) {  // clear_left_context
        std::fill(lLvl[p].begin(), lLvl[p].end(), 0);
        std::fill(lDc[p].begin(), lDc[p].end(), 0);
      }
      std::fill(lTx.begin(), lTx.end(), 64);
      for (int sc = 0; sc < g.sbw; ++sc) {
        read_lr(sr, sc);
        partition(sr * 16, sc * 16, 4);
      }
    }
  }
};

// ------------------------------------------------------------------ headers -------------
constexpr int OBU_SEQUENCE_HEADER = 1, OBU_TEMPORAL_DELIMITER = 2, OBU_FRAME = 6;

int bits_for(int v) {  // bits to code values 0..v
  int n = 1;
  while ((1 << n) <= v) ++n;
  return n;
}
int tile_log2(int blk, int target) {
  int k = 0;
  while ((blk << k) < target) ++k;
  return k;
}

void write_seq_header(BitWriter& w, const SeqGeo& g) {
  w.put(0, 3);  // seq_profile (Main)
  w.put(0, 1);  // still_picture
  w.put(0, 1);  // reduced_still_picture_header
  w.put(0, 1);  // timing_info_present_flag
  w.put(0, 1);  // initial_display_delay_present_flag
  w.put(0, 5);  // operating_points_cnt_minus_1
  w.put(0, 12); // operating_point_idc[0]
  w.put(31, 5); // seq_level_idx[0] (31: unconstrained)
  w.put(0, 1);  // seq_tier[0]
  const int wb = bits_for(g.W - 1), hb = bits_for(g.H - 1);
  w.put(wb - 1, 4);
  w.put(hb - 1, 4);
  w.put(g.W - 1, wb);
  w.put(g.H - 1, hb);
  w.put(0, 1);  // frame_id_numbers_present_flag
  w.put(0, 1);  // use_128x128_superblock
  w.put(0, 1);  // enable_filter_intra
  w.put(0, 1);  // enable_intra_edge_filter
  w.put(0, 1);  // enable_interintra_compound
  w.put(0, 1);  // enable_masked_compound
  w.put(0, 1);  // enable_warped_motion
  w.put(0, 1);  // enable_dual_filter
  w.put(0, 1);  // enable_order_hint
  w.put(0, 1);  // seq_choose_screen_content_tools
  w.put(0, 1);  // seq_force_screen_content_tools
  w.put(0, 1);  // enable_superres
  w.put(1, 1);  // enable_cdef
  w.put(1, 1);  // enable_restoration
  // color_config: 8-bit, not monochrome, no colour description, studio range, 4:2:0
  w.put(0, 1);  // high_bitdepth
  w.put(0, 1);  // mono_chrome
  w.put(0, 1);  // color_description_present_flag
  w.put(0, 1);  // color_range
  w.put(0, 2);  // chroma_sample_position
  w.put(0, 1);  // separate_uv_delta_q
  w.put(0, 1);  // film_grain_params_present
  w.trailing_bits();
}

SeqGeo read_seq_header(BitReader& r) {
  auto expect = [&](int n, uint32_t v, const char* what) {
    if (r.u(n) != v) throw std::runtime_error(std::string("av1 oracle: unsupported sequence header ") + what);
  };
  expect(3, 0, "profile");
  expect(1, 0, "still_picture");
  expect(1, 0, "reduced_still_picture_header");
  expect(1, 0, "timing_info");
  expect(1, 0, "initial_display_delay");
  expect(5, 0, "operating points");
  r.u(12);
  const int lvl = (int)r.u(5);
  if (lvl > 7) r.u(1);
  const int wb = (int)r.u(4) + 1, hb = (int)r.u(4) + 1;
  const int W = (int)r.u(wb) + 1, H = (int)r.u(hb) + 1;
  const char* flags[] = {"frame ids",     "128x128 SB",      "filter intra",   "intra edge filter",
                         "interintra",    "masked compound", "warped motion",  "dual filter",
                         "order hint",    "choose screen content", "force screen content", "superres"};
  for (auto f : flags) expect(1, 0, f);
  expect(1, 1, "enable_cdef");
  expect(1, 1, "enable_restoration");
  expect(1, 0, "high_bitdepth");
  expect(1, 0, "mono_chrome");
  expect(1, 0, "color_description");
  r.u(1);
  r.u(2);
  expect(1, 0, "separate_uv_delta_q");
  expect(1, 0, "film grain");
  SeqGeo g = make_seq_geo(W, H);  // render size arrives in the frame header
  if (g.W != W || g.H != H) throw std::runtime_error("av1 oracle: coded size not a multiple of 16");
  return g;
}

void write_frame_header(BitWriter& w, const SeqGeo& g, const FrameParams& fp, const int* lr_type) {
  w.put(0, 1);  // show_existing_frame
  w.put(fp.key ? 0 : 1, 2);  // frame_type KEY_FRAME / INTER_FRAME
  w.put(1, 1);  // show_frame
  if (!fp.key) w.put(0, 1);  // error_resilient_mode (key + shown: implied 1)
  w.put(0, 1);  // disable_cdf_update
  w.put(0, 1);  // frame_size_override_flag
  if (!fp.key) w.put(0, 3);  // primary_ref_frame: CDFs saved by the frame in ref slot 0
  if (!fp.key) w.put(0x01, 8);  // refresh_frame_flags: slot 0 (key frames refresh all)
  const bool diff = g.dw != g.W || g.dh != g.H;
  if (fp.key) {
    w.put(diff, 1);  // render_and_frame_size_different
    if (diff) {
      w.put(g.dw - 1, 16);
      w.put(g.dh - 1, 16);
    }
  } else {
    for (int i = 0; i < 7; ++i) w.put(0, 3);  // ref_frame_idx: every reference is slot 0
    w.put(diff, 1);
    if (diff) {
      w.put(g.dw - 1, 16);
      w.put(g.dh - 1, 16);
    }
    w.put(0, 1);  // allow_high_precision_mv
    w.put(0, 1);  // is_filter_switchable
    w.put(0, 2);  // interpolation_filter EIGHTTAP
    w.put(0, 1);  // is_motion_mode_switchable
  }
  w.put(0, 1);  // disable_frame_end_update_cdf: the CDFs at the end of the tile are saved
  // tile_info: uniform spacing, one tile
  const int sbc = g.sbw, sbr = g.sbh;
  w.put(1, 1);
  const int minc = tile_log2(64, sbc), maxc = tile_log2(1, std::min(sbc, 64));
  if (minc > 0) throw std::runtime_error("av1: frame too wide for one tile");
  if (minc < maxc) w.put(0, 1);
  const int maxr = tile_log2(1, std::min(sbr, 64));
  const int mint = std::max(minc, tile_log2(2304, sbr * sbc));
  if (mint > 0) throw std::runtime_error("av1: frame too large for one tile");
  if (0 < maxr) w.put(0, 1);
  // quantization_params
  w.put(fp.qindex, 8);
  w.put(0, 1);  // DeltaQYDc
  w.put(0, 1);  // DeltaQUDc
  w.put(0, 1);  // DeltaQUAc
  w.put(0, 1);  // using_qmatrix
  w.put(0, 1);  // segmentation_enabled
  if (fp.qindex > 0) w.put(0, 1);  // delta_q_present
  // loop_filter_params
  w.put(fp.lf[0], 6);
  w.put(fp.lf[1], 6);
  if (fp.lf[0] || fp.lf[1]) {
    w.put(fp.lf[2], 6);
    w.put(fp.lf[3], 6);
  }
  w.put(fp.sharp, 3);
  w.put(0, 1);  // loop_filter_delta_enabled
  // cdef_params
  w.put(fp.cdef_damping - 3, 2);
  w.put(fp.cdef_bits, 2);
  for (int i = 0; i < (1 << fp.cdef_bits); ++i) {
    w.put(fp.cdef_y[i] >> 2, 4);
    w.put(fp.cdef_y[i] & 3, 2);
    w.put(fp.cdef_uv[i] >> 2, 4);
    w.put(fp.cdef_uv[i] & 3, 2);
  }
  // lr_params: lr_type 3 = SGRPROJ (Remap_Lr_Type), 64x64 units (lr_unit_shift 0), no uv shift
  for (int p = 0; p < 3; ++p) w.put(lr_type[p] ? 3 : 0, 2);
  if (lr_type[0] || lr_type[1] || lr_type[2]) {
    w.put(0, 1);  // lr_unit_shift
    if (lr_type[1] || lr_type[2]) w.put(0, 1);  // lr_uv_shift
  }
  // tx_mode_select: TX_MODE_LARGEST, or TX_MODE_SELECT in the inter frames of a transform-split stream
  w.put(fp.tx_select && !fp.key ? 1 : 0, 1);
  if (!fp.key) w.put(0, 1);  // reference_select
  w.put(1, 1);  // reduced_tx_set
  if (!fp.key)
    for (int i = 0; i < 7; ++i) w.put(0, 1);  // is_global
}

FrameParams read_frame_header(BitReader& r, SeqGeo& g, bool& have_ref, int* lr_type) {
  auto expect = [&](int n, uint32_t v, const char* what) {
    if (r.u(n) != v) throw std::runtime_error(std::string("av1 oracle: unsupported frame header ") + what);
  };
  FrameParams fp;
  expect(1, 0, "show_existing_frame");
  const int ft = (int)r.u(2);
  if (ft > 1) throw std::runtime_error("av1 oracle: frame type outside the encoder subset");
  fp.key = ft == 0;
  expect(1, 1, "show_frame");
  if (!fp.key) expect(1, 0, "error_resilient_mode");
  expect(1, 0, "disable_cdf_update");
  expect(1, 0, "frame_size_override_flag");
  if (!fp.key) {
    expect(3, 0, "primary_ref_frame");
    r.u(8);
    if (!have_ref) throw std::runtime_error("av1 oracle: inter frame without a reference");
    for (int i = 0; i < 7; ++i) expect(3, 0, "ref_frame_idx");
  }
  if (r.u(1)) {
    const int dw = (int)r.u(16) + 1, dh = (int)r.u(16) + 1;
    const int W = g.W, H = g.H;
    g = make_seq_geo(dw, dh);
    if (g.W != W || g.H != H) throw std::runtime_error("av1 oracle: render size does not match the coded size");
  } else {
    g.dw = g.W;
    g.dh = g.H;
  }
  if (!fp.key) {
    expect(1, 0, "allow_high_precision_mv");
    expect(1, 0, "is_filter_switchable");
    expect(2, 0, "interpolation_filter");
    expect(1, 0, "is_motion_mode_switchable");
  }
  expect(1, 0, "disable_frame_end_update_cdf");
  expect(1, 1, "uniform_tile_spacing_flag");
  const int maxc = tile_log2(1, std::min(g.sbw, 64)), maxr = tile_log2(1, std::min(g.sbh, 64));
  if (0 < maxc) expect(1, 0, "increment_tile_cols_log2");
  if (0 < maxr) expect(1, 0, "increment_tile_rows_log2");
  fp.qindex = (int)r.u(8);
  for (int i = 0; i < 4; ++i) expect(1, 0, "delta q / qmatrix");
  expect(1, 0, "segmentation_enabled");
  if (fp.qindex > 0) expect(1, 0, "delta_q_present");
  fp.lf[0] = (int)r.u(6);
  fp.lf[1] = (int)r.u(6);
  if (fp.lf[0] || fp.lf[1]) {
    fp.lf[2] = (int)r.u(6);
    fp.lf[3] = (int)r.u(6);
  }
  fp.sharp = (int)r.u(3);
  expect(1, 0, "loop_filter_delta_enabled");
  fp.cdef_damping = (int)r.u(2) + 3;
  fp.cdef_bits = (int)r.u(2);
  for (int i = 0; i < (1 << fp.cdef_bits); ++i) {
    const int yp = (int)r.u(4), ys = (int)r.u(2), up = (int)r.u(4), us = (int)r.u(2);
    fp.cdef_y[i] = (uint8_t)(yp * 4 + ys);
    fp.cdef_uv[i] = (uint8_t)(up * 4 + us);
  }
  for (int p = 0; p < 3; ++p) {
    const int t = (int)r.u(2);
    if (t != 0 && t != 3) throw std::runtime_error("av1 oracle: restoration type outside the encoder subset");
    lr_type[p] = t == 3;
  }
  if (lr_type[0] || lr_type[1] || lr_type[2]) {
    expect(1, 0, "lr_unit_shift");
    if (lr_type[1] || lr_type[2]) expect(1, 0, "lr_uv_shift");
  }
  fp.tx_select = (int)r.u(1);
  if (fp.key && fp.tx_select)
    throw std::runtime_error("av1 oracle: unsupported frame header tx_mode_select on a key frame");
  if (!fp.key) expect(1, 0, "reference_select");
  expect(1, 1, "reduced_tx_set");
  if (!fp.key)
    for (int i = 0; i < 7; ++i) expect(1, 0, "is_global");
  return fp;
}

void put_leb128(std::vector<uint8_t>& out, size_t v) {
  do {
    uint8_t b = v & 0x7f;
    v >>= 7;
    if (v) b |= 0x80;
    out.push_back(b);
  } while (v);
}
void put_obu(std::vector<uint8_t>& out, int type, const std::vector<uint8_t>& payload) {
  out.push_back((uint8_t)((type << 3) | 2));  // obu_has_size_field
  put_leb128(out, payload.size());
  out.insert(out.end(), payload.begin(), payload.end());
}

}  // namespace

// ================================================================== writer ==============
std::vector<uint8_t> write_temporal_unit(const SeqGeo& g, const FrameDecisions& d, bool seq_header, EntropyState* st) {
  const int nb = g.nblk();
  FrameParams fp = d.fp;
  thread_local std::vector<uint32_t> mode, mv;  // reused across calls (no per-frame page faults)
  mode.assign(d.mode, d.mode + nb);
  if (d.mv) mv.assign(d.mv, d.mv + nb);
  else mv.assign(nb, 0);
  std::vector<int8_t> cdef(d.cdef_idx, d.cdef_idx + g.nsb());
  SymW io;
  Tile<SymW> t(io, g, fp, mode, mv, cdef);
  if (!fp.key) {
    if (!st || st->saved.size() != sizeof(Cdfs)) throw std::runtime_error("av1 writer: inter frame without saved CDFs");
    Cdfs saved;
    std::memcpy(&saved, st->saved.data(), sizeof(Cdfs));
    load_saved_cdfs(t.cdf, saved);
  }
  std::vector<int32_t> lr;
  if (d.lr) {
    lr.assign(d.lr, d.lr + (size_t)3 * g.lr_nu() * 3);
    t.lr = lr.data();
    for (int p = 0; p < 3; ++p)
      for (int u = 0; u < g.lr_ux(p) * g.lr_uy(p); ++u) t.lr_type[p] |= lr[((size_t)p * g.lr_nu() + u) * 3] >= 0;
  }
  // level access (packed layout: prefix offsets over the nonzero masks)
  std::vector<int32_t> off[3];
  const int16_t* base[3] = {d.ly, d.lu, d.lv};
  thread_local std::vector<int32_t> soff[3];
  if (d.scan_packed)  // [eob, eob levels in scan order] per nonzero TB: coded straight from it
    for (int p = 0; p < 3; ++p) {
      const int sz = p ? 64 : 256;
      soff[p].assign(nb, -1);
      int32_t o = 0;
      for (int b = 0; b < nb; ++b) {
        if (!(mode_nz(mode[b]) >> p & 1)) continue;
        soff[p][b] = o;
        // a transform-split block: the records of its nonzero quadrants back to back
        const int nrec = p == 0 && mode_tx(mode[b]) ? __builtin_popcount(mode_txq(mode[b])) : 1;
        const int lim = p == 0 && mode_tx(mode[b]) ? 64 : sz;
        for (int k = 0; k < nrec; ++k) {
          const int eob = base[p][o];
          if (eob < 1 || eob > lim) throw std::runtime_error("scan-packed levels: bad eob");
          o += 1 + eob;
        }
      }
      t.scan_in[p] = base[p];
      t.scan_off[p] = soff[p].data();
    }
  if (d.packed && !d.scan_packed)
    for (int p = 0; p < 3; ++p) {
      off[p].assign(nb, -1);
      int k = 0;
      for (int b = 0; b < nb; ++b)
        if (mode_nz(mode[b]) >> p & 1) off[p][b] = k++;
    }
  t.lev_in = [&](int p, int b) -> const int16_t* {
    const size_t sz = p ? 64 : 256;
    if (!d.packed) return base[p] + (size_t)b * sz;
    return off[p][b] < 0 ? nullptr : base[p] + (size_t)off[p][b] * sz;
  };
  t.tile();
  if (st) {  // frame end CDF update
    st->saved.resize(sizeof(Cdfs));
    std::memcpy(st->saved.data(), &t.cdf, sizeof(Cdfs));
  }
  const std::vector<uint8_t> tile = io.rc.finish();
  std::vector<uint8_t> out;
  put_obu(out, OBU_TEMPORAL_DELIMITER, {});
  if (seq_header) {
    BitWriter sw;
    write_seq_header(sw, g);
    put_obu(out, OBU_SEQUENCE_HEADER, sw.bytes());
  }
  BitWriter fw;
  write_frame_header(fw, g, fp, t.lr_type);
  fw.align_zero();  // byte_alignment (frame_obu); tile_group: one tile, no start/end flags
  std::vector<uint8_t> payload = fw.bytes();
  payload.insert(payload.end(), tile.begin(), tile.end());
  put_obu(out, OBU_FRAME, payload);
  return out;
}

// ================================================================== reconstruction ======
namespace {
struct PlaneRef {
  const uint8_t* p;
  int w, h;
  int operator()(int x, int y) const { return p[(size_t)clip3(0, h - 1, y) * w + clip3(0, w - 1, x)]; }
};

// dequantise + inverse transform a TB of levels into a residual (int16 raster): 7.12.3
// dequantisation and the 7.13.3 2-D inverse transform process
void residual_of(const int16_t* lev, int lg, int qidx, int txt, int16_t* res) {
  const int N = 1 << lg, area = N * N;
  int32_t dq[256], r[256];
  bool any = false;
  for (int i = 0; i < area; ++i) {
    dq[i] = dequant(lev[i], i == 0 ? dc_q(qidx) : ac_q(qidx));
    any |= dq[i] != 0;
  }
  if (!any) {
    std::memset(res, 0, sizeof(int16_t) * area);
    return;
  }
  inv_txfm2d(dq, lg, txt & 1, (txt >> 1) & 1, r);
  for (int i = 0; i < area; ++i) res[i] = (int16_t)r[i];
}

// normative self-guided restoration of the CDEF output `io` with the per-unit (set, xqd0,
// xqd1); `db` = the deblocked (pre-CDEF) frame the stripe boundaries read
void apply_lr(const SeqGeo& g, const int32_t* lr, const Planes& db, Planes& io) {
  for (int p = 0; p < 3; ++p) {
    const int nu = g.lr_ux(p) * g.lr_uy(p);
    const int32_t* P = lr + (size_t)p * g.lr_nu() * 3;
    bool any = false;
    for (int u = 0; u < nu; ++u) any |= P[3 * u] >= 0;
    if (!any) continue;
    std::vector<uint8_t>& X = p == 0 ? io.y : (p == 1 ? io.u : io.v);
    const std::vector<uint8_t>& D = p == 0 ? db.y : (p == 1 ? db.u : db.v);
    std::vector<uint8_t> o(X.size());
    lr_apply(X.data(), D.data(), p ? g.W / 2 : g.W, p ? g.H / 2 : g.H, p ? 1 : 0, P, o.data());
    X.swap(o);
  }
}

// flag the 8x8 blocks of skip blocks in a CDEF direction array (kCdefSkipBlock)
void mark_cdef_skip(const SeqGeo& g, const uint32_t* mode, uint8_t* dir) {
  const int w8 = g.W / 8, h8 = g.H / 8;
  for (int y = 0; y < h8; ++y)
    for (int x = 0; x < w8; ++x)
      if (mode_skip(mode[(y / 2) * g.bw + x / 2])) dir[y * w8 + x] |= kCdefSkipBlock;
}

void loop_filters(const SeqGeo& g, const FrameParams& fp, const uint32_t* mode, const int8_t* cdef_idx, Planes& rec,
                  Planes& out, const int32_t* lr = nullptr, Planes* db_out = nullptr) {
  const int W = g.W, H = g.H;
  // deblocking: one info word per 4x4 unit of each plane
  Planes db;
  db.y.resize(rec.y.size());
  db.u.resize(rec.u.size());
  db.v.resize(rec.v.size());
  for (int p = 0; p < 3; ++p) {
    const int w = p ? W / 2 : W, h = p ? H / 2 : H, w4 = w / 4, h4 = h / 4, bs4 = p ? 2 : 4;
    const int lv = p == 0 ? fp.lf[0] : fp.lf[p + 1], lh = p == 0 ? fp.lf[1] : fp.lf[p + 1];
    std::vector<uint32_t> info((size_t)w4 * h4);
    for (int y = 0; y < h4; ++y)
      for (int x = 0; x < w4; ++x) {
        const uint32_t m = mode[(y / bs4) * g.bw + x / bs4];
        info[(size_t)y * w4 + x] = lf_word(p > 0, lv, lh, mode_skip(m) && mode_inter(m), mode_bsz(m), mode_tx(m) != 0);
      }
    const std::vector<uint8_t>& in = p == 0 ? rec.y : (p == 1 ? rec.u : rec.v);
    std::vector<uint8_t>& o = p == 0 ? db.y : (p == 1 ? db.u : db.v);
    if ((p == 0 && !(fp.lf[0] || fp.lf[1])) || (p > 0 && !(fp.lf[0] || fp.lf[1]))) o = in;
    else deblock(in.data(), w, h, p > 0, info.data(), fp.sharp, o.data());
  }
  // CDEF with the per-SB preset of cdef_idx (-1: off)
  const int n8 = (W / 8) * (H / 8);
  std::vector<uint8_t> dir(n8);
  std::vector<int> var(n8);
  cdef_find_dirs(db.y.data(), W, H, dir.data(), var.data());
  mark_cdef_skip(g, mode, dir.data());
  std::vector<int8_t> py(g.nsb()), puv(g.nsb());
  for (int s = 0; s < g.nsb(); ++s) {
    py[s] = cdef_idx[s] < 0 ? -1 : (int8_t)fp.cdef_y[cdef_idx[s]];
    puv[s] = cdef_idx[s] < 0 ? -1 : (int8_t)fp.cdef_uv[cdef_idx[s]];
  }
  out.y.resize(db.y.size());
  out.u.resize(db.u.size());
  out.v.resize(db.v.size());
  cdef_apply(db.y.data(), W, H, false, dir.data(), var.data(), W / 8, fp.cdef_damping, py.data(), out.y.data());
  cdef_apply(db.u.data(), W / 2, H / 2, true, dir.data(), var.data(), W / 8, fp.cdef_damping, puv.data(),
             out.u.data());
  cdef_apply(db.v.data(), W / 2, H / 2, true, dir.data(), var.data(), W / 8, fp.cdef_damping, puv.data(),
             out.v.data());
  if (lr) apply_lr(g, lr, db, out);
  if (db_out) *db_out = std::move(db);
}

// prediction of one block (luma 16x16 or chroma 8x8) into pred[]
void predict(const SeqGeo& g, int p, int bx, int by, uint32_t m, uint32_t mvw, const Planes& rec, const Planes* ref,
             int* pred) {
  const int N = p ? 8 : 16, w = p ? g.W / 2 : g.W, h = p ? g.H / 2 : g.H;
  const int x0 = bx * N, y0 = by * N;
  if (mode_inter(m)) {
    if (!ref) throw std::runtime_error("av1: inter block without a reference");
    const std::vector<uint8_t>& R = p == 0 ? ref->y : (p == 1 ? ref->u : ref->v);
    PlaneRef get{R.data(), w, h};
    const int r = mv_row(mvw), c = mv_col(mvw);
    const int ix = mv_int(c, p > 0), iy = mv_int(r, p > 0), fx = mv_frac(c, p > 0), fy = mv_frac(r, p > 0);
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) pred[i * N + j] = inter_pred_px(get, x0 + j + ix, y0 + i + iy, fx, fy);
    return;
  }
  const std::vector<uint8_t>& C = p == 0 ? rec.y : (p == 1 ? rec.u : rec.v);
  auto get = [&](int x, int y) { return (int)C[(size_t)y * w + x]; };
  IntraEdge e;
  intra_edges(get, x0, y0, N, e);
  const int mode = p ? mode_uv(m) : mode_y(m), dc = intra_dc(e, N);
  if (p && mode == UV_CFL_PRED) {  // chroma from luma: the block's own luma reconstruction in rec.y
    int16_t ac[64];
    cfl_ac_block([&](int x, int y) { return (int)rec.y[(size_t)y * g.W + x]; }, bx * 16, by * 16, ac);
    const int alpha = p == 1 ? mode_cfl_u(m) : mode_cfl_v(m);
    for (int i = 0; i < 64; ++i) pred[i] = cfl_pred_px(dc, alpha, ac[i]);
    return;
  }
  const int delta = p ? mode_angle_uv(m) : mode_angle_y(m);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) pred[i * N + j] = intra_pred_px_ang(mode, delta, e, N, i, j, dc);
}

}  // namespace

void reconstruct(const SeqGeo& g, const FrameDecisions& d, const Planes* ref, Planes& out) {
  Planes rec;
  rec.y.assign((size_t)g.W * g.H, 0);
  rec.u.assign((size_t)g.W * g.H / 4, 0);
  rec.v.assign((size_t)g.W * g.H / 4, 0);
  const int nb = g.nblk();
  std::vector<int32_t> off[3];
  const int16_t* base[3] = {d.ly, d.lu, d.lv};
  for (int p = 0; p < 3; ++p) {
    off[p].assign(nb, -1);
    int k = 0;
    for (int b = 0; b < nb; ++b)
      if (!d.packed || (mode_nz(d.mode[b]) >> p & 1)) off[p][b] = d.packed ? k++ : b;
  }
  for (int by = 0; by < g.bh; ++by)
    for (int bx = 0; bx < g.bw; ++bx) {
      const int b = by * g.bw + bx;
      const uint32_t m = d.mode[b], mvw = d.mv ? d.mv[b] : 0;
      for (int p = 0; p < 3; ++p) {
        const int N = p ? 8 : 16, lg = p ? 3 : 4, w = p ? g.W / 2 : g.W;
        int pred[256];
        int16_t res[256];
        predict(g, p, bx, by, m, mvw, rec, ref, pred);
        const bool nz = !mode_skip(m) && (mode_nz(m) >> p & 1) && off[p][b] >= 0;
        if (nz && p == 0 && mode_tx(m)) {  // four 8x8 rasters (av1_enc.h "transform split")
          for (int k = 0; k < 4; ++k) {
            int16_t r8[64];
            residual_of(base[0] + (size_t)off[0][b] * 256 + k * 64, 3, d.fp.qindex, 0, r8);
            for (int i = 0; i < 64; ++i) res[((k >> 1) * 8 + (i >> 3)) * 16 + (k & 1) * 8 + (i & 7)] = r8[i];
          }
        } else if (nz) {
          const int txt = p == 0 || mode_inter(m) ? 0 : uv_txtype(mode_uv(m));
          residual_of(base[p] + (size_t)off[p][b] * N * N, lg, d.fp.qindex, txt, res);
        } else {
          std::memset(res, 0, sizeof(res));
        }
        std::vector<uint8_t>& P = p == 0 ? rec.y : (p == 1 ? rec.u : rec.v);
        for (int i = 0; i < N; ++i)
          for (int j = 0; j < N; ++j)
            P[(size_t)(by * N + i) * w + bx * N + j] = (uint8_t)clip_pixel(pred[i * N + j] + res[i * N + j]);
      }
    }
  loop_filters(g, d.fp, d.mode, d.cdef_idx, rec, out, d.lr);
}

// ================================================================== decoder oracle ======
namespace {
size_t read_leb128(const uint8_t* p, size_t n, size_t& pos) {
  size_t v = 0;
  for (int i = 0; i < 8; ++i) {
    if (pos >= n) throw std::runtime_error("av1 oracle: truncated leb128");
    const uint8_t b = p[pos++];
    v |= (size_t)(b & 0x7f) << (7 * i);
    if (!(b & 0x80)) return v;
  }
  throw std::runtime_error("av1 oracle: bad leb128");
}
}  // namespace

Decoded decode_stream(const uint8_t* p, size_t n) {
  Decoded out;
  Cdfs saved_cdfs;
  init_cdfs(saved_cdfs, 0);
  bool have_seq = false;
  size_t pos = 0;
  while (pos < n) {
    const uint8_t h = p[pos++];
    if (h & 0x80) throw std::runtime_error("av1 oracle: forbidden bit set");
    const int type = (h >> 3) & 15;
    if (h & 4) throw std::runtime_error("av1 oracle: extension headers unsupported");
    if (!(h & 2)) throw std::runtime_error("av1 oracle: OBU without size field");
    const size_t sz = read_leb128(p, n, pos);
    if (pos + sz > n) throw std::runtime_error("av1 oracle: truncated OBU");
    const uint8_t* q = p + pos;
    pos += sz;
    if (type == OBU_TEMPORAL_DELIMITER) continue;
    if (type == OBU_SEQUENCE_HEADER) {
      BitReader r(q, sz);
      out.geo = read_seq_header(r);
      have_seq = true;
      continue;
    }
    if (type != OBU_FRAME) throw std::runtime_error("av1 oracle: OBU type outside the encoder subset");
    if (!have_seq) throw std::runtime_error("av1 oracle: frame before sequence header");
    BitReader r(q, sz);
    bool have_ref = !out.frames.empty();
    SeqGeo g = out.geo;
    FrameData fd;
    int lr_type[3] = {0, 0, 0};
    fd.fp = read_frame_header(r, g, have_ref, lr_type);
    out.geo = g;
    r.byte_align();
    const size_t hdr = r.byte_pos();
    const int nb = g.nblk();
    fd.mode.assign(nb, 0);
    fd.mv.assign(nb, 0);
    fd.ly.assign((size_t)nb * 256, 0);
    fd.lu.assign((size_t)nb * 64, 0);
    fd.lv.assign((size_t)nb * 64, 0);
    fd.cdef_idx.assign(g.nsb(), -1);
    SymR io(q + hdr, sz - hdr);
    Tile<SymR> t(io, g, fd.fp, fd.mode, fd.mv, fd.cdef_idx);
    if (!fd.fp.key) load_saved_cdfs(t.cdf, saved_cdfs);
    t.lev_out[0] = fd.ly.data();
    t.lev_out[1] = fd.lu.data();
    t.lev_out[2] = fd.lv.data();
    fd.lr.assign((size_t)3 * g.lr_nu() * 3, 0);
    for (size_t i = 0; i < fd.lr.size(); i += 3) fd.lr[i] = -1;
    t.lr = fd.lr.data();
    for (int p = 0; p < 3; ++p) t.lr_type[p] = lr_type[p];
    t.tile();
    saved_cdfs = t.cdf;
    Planes rec;
    reconstruct(g, fd.view(), fd.fp.key ? nullptr : &out.frames.back(), rec);
    out.frames.push_back(std::move(rec));
    out.data.push_back(std::move(fd));
  }
  return out;
}

// ================================================================== golden encoder ======
void cdef_choose(const uint64_t* sse_y, const uint64_t* sse_uv, const uint8_t* active, int nfb, uint8_t* ytab,
                 uint8_t* uvtab, int8_t* fb_idx) {
  std::vector<uint64_t> best(nfb, ~0ull);
  for (int k = 0; k < kMaxPresets; ++k) {
    int bp = 0;
    uint64_t bt = ~0ull;
    for (int p = 0; p < kCdefPresets; ++p) {
      uint64_t t = 0;
      for (int f = 0; f < nfb; ++f)
        if (active[f]) t += std::min(best[f], sse_y[(size_t)f * kCdefPresets + p]);
      if (t < bt) bt = t, bp = p;
    }
    ytab[k] = (uint8_t)bp;
    for (int f = 0; f < nfb; ++f) best[f] = std::min(best[f], sse_y[(size_t)f * kCdefPresets + bp]);
  }
  std::vector<int> a(nfb, 0);
  for (int f = 0; f < nfb; ++f) {
    uint64_t bv = ~0ull;
    for (int k = 0; k < kMaxPresets; ++k) {
      const uint64_t v = sse_y[(size_t)f * kCdefPresets + ytab[k]];
      if (v < bv) bv = v, a[f] = k;
    }
  }
  for (int k = 0; k < kMaxPresets; ++k) {
    int bp = 0;
    uint64_t bt = ~0ull;
    for (int p = 0; p < kCdefPresets; ++p) {
      uint64_t t = 0;
      for (int f = 0; f < nfb; ++f)
        if (active[f] && a[f] == k) t += sse_uv[(size_t)f * kCdefPresets + p];
      if (t < bt) bt = t, bp = p;
    }
    uvtab[k] = (uint8_t)bp;
  }
  for (int f = 0; f < nfb; ++f) {
    if (!active[f]) {
      fb_idx[f] = -1;
      continue;
    }
    uint64_t bv = ~0ull;
    int bk = 0;
    for (int k = 0; k < kMaxPresets; ++k) {
      const uint64_t v = sse_y[(size_t)f * kCdefPresets + ytab[k]] + sse_uv[(size_t)f * kCdefPresets + uvtab[k]];
      if (v < bv) bv = v, bk = k;
    }
    fb_idx[f] = (int8_t)bk;
  }
}

namespace {
// per-64x64-unit SSE of two planes (ceil unit layout)
void unit_sse(const uint8_t* a, const uint8_t* b, int w, int h, long long* out) {
  const int ux = (w + 63) / 64, uy = (h + 63) / 64;
  std::fill(out, out + ux * uy, 0LL);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int d = (int)a[(size_t)y * w + x] - (int)b[(size_t)y * w + x];
      out[(y / 64) * ux + x / 64] += d * d;
    }
}
// run f(row) for rows [0, n) on up to hardware_concurrency threads (disjoint outputs)
template <class F> void parallel_rows(int n, F f) {
  const int nt = std::max(1, std::min(n, (int)std::thread::hardware_concurrency()));
  std::atomic<int> next{0};
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&] {
      for (int r; (r = next.fetch_add(1)) < n;) f(r);
    });
  for (auto& x : th) x.join();
}
// transform + quantise + reconstruct one TB: src/pred raster N x N -> levels, recon
int code_tb(const int* src, const int* pred, int lg, int qidx, int txt, int rnd, int16_t* lev, int* rec) {
  const int N = 1 << lg, area = N * N;
  int16_t r[256], c[256], res[256];
  for (int i = 0; i < area; ++i) r[i] = (int16_t)(src[i] - pred[i]);
  txfm2d_ref(r, c, 1, lg, txt & 1, (txt >> 1) & 1, false);
  int nz = 0;
  for (int i = 0; i < area; ++i) {
    lev[i] = (int16_t)quant(c[i], i == 0 ? dc_q(qidx) : ac_q(qidx), rnd);
    nz |= lev[i] != 0;
  }
  if (nz) residual_of(lev, lg, qidx, txt, res);
  else std::memset(res, 0, sizeof(int16_t) * area);
  for (int i = 0; i < area; ++i) rec[i] = clip_pixel(pred[i] + res[i]);
  return nz;
}
int satd_block(const int* a, const int* b, int N) {
  int s = 0;
  for (int by = 0; by < N; by += 4)
    for (int bx = 0; bx < N; bx += 4) {
      int d[16];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) d[i * 4 + j] = a[(by + i) * N + bx + j] - b[(by + i) * N + bx + j];
      s += satd4(d);
    }
  return s;
}
// Transform split of one inter block's luma (av1_enc.h "transform split"): the 16x16 coding
// (levels lev16, reconstruction rec16) against the four 8x8 quadrants coded here.
struct TxSplitTrial {
  int16_t lev8[256];  // four 8x8 rasters, quadrant raster order
  int rec8[256];      // block raster
  int qmask, sse16, sse8, bits16, bits8, split;
};
void tx_split_trial(const int* src, const int* pred, int qidx, int rnd, const int16_t* lev16, const int* rec16,
                    TxSplitTrial& t) {
  t.qmask = t.sse16 = t.sse8 = 0;
  t.bits16 = tx_tb_rate(lev16, 16);
  t.bits8 = 0;
  for (int k = 0; k < 4; ++k) {
    int sq[64], pq[64], rq[64];
    for (int i = 0; i < 64; ++i) {
      const int o = ((k >> 1) * 8 + (i >> 3)) * 16 + (k & 1) * 8 + (i & 7);
      sq[i] = src[o], pq[i] = pred[o];
    }
    if (code_tb(sq, pq, 3, qidx, 0, rnd, t.lev8 + k * 64, rq)) t.qmask |= 1 << k;
    t.bits8 += tx_tb_rate(t.lev8 + k * 64, 8);
    for (int i = 0; i < 64; ++i) t.rec8[((k >> 1) * 8 + (i >> 3)) * 16 + (k & 1) * 8 + (i & 7)] = rq[i];
  }
  for (int i = 0; i < 256; ++i) {
    t.sse16 += (src[i] - rec16[i]) * (src[i] - rec16[i]);
    t.sse8 += (src[i] - t.rec8[i]) * (src[i] - t.rec8[i]);
  }
  t.split = tx_split_wins(qidx, t.sse16, t.bits16, t.sse8, t.bits8, t.qmask);
}
}  // namespace

GoldenOut golden_encode(const SeqGeo& g, const std::vector<Planes>& src, int qidx0, const int* qmap, int tools) {
  GoldenOut out;
  const int nb = g.nblk();
  // TV_AV1_DBG (conformance bring-up): 1 no deblocking, 2 no CDEF, 4 no loop restoration,
  // 8 DC_PRED only, 16 no residual, 128 (with kToolTxSplit) the pre-transform split rule
  const char* dbg_env = std::getenv("TV_AV1_DBG");
  const int dbg = dbg_env ? std::atoi(dbg_env) : 0;
  for (size_t f = 0; f < src.size(); ++f) {
    const int qidx = qmap ? clip3(1, 255, qmap[f]) : qidx0, lam = lambda16(qidx);
    const Planes& S = src[f];
    const Planes* ref = f ? &out.recon.back() : nullptr;
    FrameData fd;
    fd.fp.key = f == 0;
    fd.fp.qindex = qidx;
    const int lvl = (dbg & 1) ? 0 : lf_level_for_q(qidx);
    for (int i = 0; i < 4; ++i) fd.fp.lf[i] = lvl;
    fd.fp.cdef_damping = cdef_damping_for_q(qidx0);  // per stream (the engine's CDEF launches take one damping)
    fd.fp.tx_select = (tools & kToolTxSplit) && f != 0;
    fd.mode.assign(nb, 0);
    fd.mv.assign(nb, 0);
    fd.ly.assign((size_t)nb * 256, 0);
    fd.lu.assign((size_t)nb * 64, 0);
    fd.lv.assign((size_t)nb * 64, 0);
    Planes rec;
    rec.y.assign((size_t)g.W * g.H, 0);
    rec.u.assign((size_t)g.W * g.H / 4, 0);
    rec.v.assign((size_t)g.W * g.H / 4, 0);
    // edge-extended luma reference for the full-pel search
    constexpr int kPad = kMeRange + 8;
    const int pw = g.W + 2 * kPad;
    std::vector<uint8_t> padY;
    if (ref) {
      padY.resize((size_t)pw * (g.H + 2 * kPad));
      PlaneRef ry{ref->y.data(), g.W, g.H};
      for (int y = 0; y < g.H + 2 * kPad; ++y)
        for (int x = 0; x < pw; ++x) padY[(size_t)y * pw + x] = (uint8_t)ry(x - kPad, y - kPad);
    }
    // intra blocks (every block of a key frame; as_intra: an accepted intra block of an inter
    // frame, tv/av1_enc.h), inter blocks at a given MV (force_mv), or the motion search alone
    // (search_out: the block's MV, nothing coded)
    int frame_rnd = kRndInter;
    auto code_block = [&](int by, int bx, const uint32_t* force_mv, uint32_t* search_out, bool as_intra = false) {
        const int b = by * g.bw + bx;
        int s[3][256], pred[3][256], rc[256];
        for (int p = 0; p < 3; ++p) {
          const int N = p ? 8 : 16, w = p ? g.W / 2 : g.W;
          const std::vector<uint8_t>& P = p == 0 ? S.y : (p == 1 ? S.u : S.v);
          for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) s[p][i * N + j] = P[(size_t)(by * N + i) * w + bx * N + j];
        }
        int ym = 0, uvm = 0, inter = 0, cfl_u = 0, cfl_v = 0, split = 0, qmask = 0;
        uint32_t mvw = 0;
        // TV_AV1_DBG bit 32: the search also tries D113 / D135 / D157 (conformance tests of
        // the directional predictor; the shipped search leaves them out, av1_enc.h)
        // directional intra (kToolDirIntra, av1_enc.h): 34 (mode, delta) candidates in dir_cand
        // order with CDF-based rates.  TV_AV1_DBG bit 64: those rates over the seven old modes
        // only (measurement: the rate model without the new angles)
        const bool dir = (tools & kToolDirIntra) && !(dbg & (8 | 32));
        const int ncand = dir ? ((dbg & 64) ? kNumIntraCand : kNumDirCand)
                              : ((dbg & 8) ? 1 : kNumIntraCand + ((dbg & 32) ? 3 : 0));
        auto cand = [&](int k) {
          if (dir) return dir_cand_mode(k);
          return k < kNumIntraCand ? intra_cand(k) : D135_PRED + (k - kNumIntraCand);
        };
        auto cand_delta = [&](int k) { return dir ? dir_cand_delta(k) : 0; };
        const bool kf_ctx = fd.fp.key;
        // key frames code in raster order: the neighbours' mode words are final (inter frames
        // take the y_mode table, no neighbour is read)
        const int ctx_a = kf_ctx && by ? dir_ctx_mode(fd.mode[b - g.bw]) : DC_PRED;
        const int ctx_l = kf_ctx && bx ? dir_ctx_mode(fd.mode[b - 1]) : DC_PRED;
        int yd = 0, uvd = 0;
        // chroma decision of an intra block; runs once the block's luma is reconstructed in rec
        // (chroma from luma reads it; the regular modes read the chroma neighbours only)
        auto chroma_search = [&] {
          int best = 1 << 30;
          for (int k = 0; k < ncand; ++k) {
            const uint32_t m = with_angle_uv(pack_mode(0, 0, cand(k), 0, 0), cand_delta(k));
            int pu[64], pv[64];
            predict(g, 1, bx, by, m, 0, rec, nullptr, pu);
            predict(g, 2, bx, by, m, 0, rec, nullptr, pv);
            const int bits = dir ? dir_uv_bits16(ym, cand(k), cand_delta(k)) : intra_mode_bits16(cand(k));
            const int cost = satd_block(s[1], pu, 8) + satd_block(s[2], pv, 8) + ((lam * bits) >> 8);
            if (cost < best) {
              best = cost, uvm = cand(k), uvd = cand_delta(k);
              std::memcpy(pred[1], pu, sizeof(pu));
              std::memcpy(pred[2], pv, sizeof(pv));
            }
          }
          if (!(tools & kToolCfl)) return;
          int16_t ac[64];
          cfl_ac_block([&](int x, int y) { return (int)rec.y[(size_t)y * g.W + x]; }, bx * 16, by * 16, ac);
          int den = 0, a0[2], dcv[2], sat[2][3] = {{0, 0, 0}, {0, 0, 0}}, pc[64];
          for (int i = 0; i < 64; ++i) den += ac[i] * ac[i];
          for (int pl = 0; pl < 2; ++pl) {
            predict(g, 1 + pl, bx, by, pack_mode(0, 0, DC_PRED, 0, 0), 0, rec, nullptr, pc);
            const int dc = dcv[pl] = pc[0];
            int num = 0;
            for (int i = 0; i < 64; ++i) num += ac[i] * (s[1 + pl][i] - dc);
            a0[pl] = cfl_fit(num, den);
            for (int k = 0; k < 3; ++k) {
              const int a = cfl_cand(a0[pl], k);
              if (a < -16 || a > 16) continue;
              for (int i = 0; i < 64; ++i) pc[i] = cfl_pred_px(dc, a, ac[i]);
              sat[pl][k] = satd_block(s[1 + pl], pc, 8);
            }
          }
          if (!(dir ? cfl_decide_bits(a0[0], a0[1], sat[0], sat[1], lam, best, dir_uv_bits16(ym, UV_CFL_PRED, 0), &cfl_u,
                                      &cfl_v)
                    : cfl_decide(a0[0], a0[1], sat[0], sat[1], lam, best, &cfl_u, &cfl_v)))
            return;
          uvm = UV_CFL_PRED;
          uvd = 0;
          for (int pl = 0; pl < 2; ++pl) {
            const int a = pl ? cfl_v : cfl_u;
            for (int i = 0; i < 64; ++i) pred[1 + pl][i] = cfl_pred_px(dcv[pl], a, ac[i]);
          }
        };
        if (fd.fp.key || as_intra) {
          int best = 1 << 30;
          for (int k = 0; k < ncand; ++k) {
            const uint32_t m = with_angle_y(pack_mode(0, cand(k), 0, 0, 0), cand_delta(k));
            int pr[256];
            predict(g, 0, bx, by, m, 0, rec, nullptr, pr);
            const int bits = dir ? dir_y_bits16(kf_ctx, ctx_a, ctx_l, cand(k), cand_delta(k)) : intra_mode_bits16(cand(k));
            const int cost = satd_block(s[0], pr, 16) + ((lam * bits) >> 8);
            if (cost < best) best = cost, ym = cand(k), yd = cand_delta(k), std::memcpy(pred[0], pr, sizeof(pr));
          }
        } else if (force_mv) {
          inter = 1;
          mvw = *force_mv;
          for (int p = 0; p < 3; ++p) predict(g, p, bx, by, pack_mode(1, 0, 0, 0, 0), mvw, rec, ref, pred[p]);
        } else {
          inter = 1;
          // integer search on the edge-extended reference
          auto fp_cost = [&](int dx, int dy) {
            int sad = 0;
            const uint8_t* rp = padY.data() + (size_t)(by * 16 + dy + kPad) * pw + bx * 16 + dx + kPad;
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) sad += std::abs(s[0][i * 16 + j] - (int)rp[(size_t)i * pw + j]);
            return sad + ((lam * (mv_comp_bits(dy * 8) + mv_comp_bits(dx * 8))) >> 4);
          };
          int bc = 1 << 30, bk = 0;
          for (int k = 0; k < kMeGrid * kMeGrid; ++k) {
            const int cost = fp_cost(me_cand_dx(k), me_cand_dy(k));
            if (cost < bc) bc = cost, bk = k;
          }
          int fx = me_cand_dx(bk), fy = me_cand_dy(bk), bring = -1;
          for (int k = 0; k < 8; ++k) {  // full-pel neighbours of the best grid point
            const int dx = fx + me_ring_dx(k), dy = fy + me_ring_dy(k);
            if (dx < -kMeRange || dx > kMeRange || dy < -kMeRange || dy > kMeRange) continue;
            const int cost = fp_cost(dx, dy);
            if (cost < bc) bc = cost, bring = k;
          }
          if (bring >= 0) fx += me_ring_dx(bring), fy += me_ring_dy(bring);
          int mr = fy * 8, mc = fx * 8;
          auto sub_cost = [&](int r, int c) {
            int pr[256];
            predict(g, 0, bx, by, pack_mode(1, 0, 0, 0, 0), pack_mv(r, c), rec, ref, pr);
            return satd_block(s[0], pr, 16) + ((lam * (mv_comp_bits(r) + mv_comp_bits(c))) >> 4);
          };
          for (int step = 4; step >= 2; step >>= 1) {
            int best = sub_cost(mr, mc), br = mr, bcc = mc;
            for (int k = 0; k < 8; ++k) {
              const int r = mr + me_ring_dy(k) * step, c = mc + me_ring_dx(k) * step;
              const int cst = sub_cost(r, c);
              if (cst < best) best = cst, br = r, bcc = c;
            }
            mr = br;
            mc = bcc;
          }
          mvw = pack_mv(mr, mc);
          if (search_out) {
            *search_out = mvw;
            return;
          }
          for (int p = 0; p < 3; ++p) predict(g, p, bx, by, pack_mode(1, 0, 0, 0, 0), mvw, rec, ref, pred[p]);
        }
        int nz = 0;
        for (int p = 0; p < 3; ++p) {
          const int N = p ? 8 : 16, lg = p ? 3 : 4, w = p ? g.W / 2 : g.W;
          if (p == 1 && !inter) chroma_search();
          const int txt = p == 0 || inter ? 0 : uv_txtype(uvm);
          int16_t* lev = p == 0 ? &fd.ly[(size_t)b * 256] : (p == 1 ? &fd.lu[(size_t)b * 64] : &fd.lv[(size_t)b * 64]);
          if (dbg & 16) {
            for (int i = 0; i < N * N; ++i) s[p][i] = pred[p][i];
          }
          if (code_tb(s[p], pred[p], lg, qidx, txt, inter ? frame_rnd : kRndIntra, lev, rc)) nz |= 1 << p;
          if (p == 0 && inter && (tools & kToolTxSplit)) {  // transform split (av1_enc.h): the cheaper of the two
            TxSplitTrial t;
            tx_split_trial(s[0], pred[0], qidx, frame_rnd, lev, rc, t);
            if (dbg & 128) {  // measurement: the pre-transform rule (quadrant SATD spread, as hevc rqt_split)
              int sat4[4];
              for (int k = 0; k < 4; ++k) {
                int sq[64], pq[64];
                for (int i = 0; i < 64; ++i) {
                  const int o = ((k >> 1) * 8 + (i >> 3)) * 16 + (k & 1) * 8 + (i & 7);
                  sq[i] = s[0][o], pq[i] = pred[0][o];
                }
                sat4[k] = satd_block(sq, pq, 8);
              }
              t.split = t.qmask != 0 && rqt_split(sat4, 64);
            }
            if (t.split) {
              std::memcpy(lev, t.lev8, sizeof(t.lev8));
              std::memcpy(rc, t.rec8, sizeof(t.rec8));
              nz |= 1;
              split = 1, qmask = t.qmask;
            }
          }
          std::vector<uint8_t>& P = p == 0 ? rec.y : (p == 1 ? rec.u : rec.v);
          for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) P[(size_t)(by * N + i) * w + bx * N + j] = (uint8_t)rc[i * N + j];
        }
        fd.mode[b] = pack_mode(inter, ym, uvm, nz == 0, nz);
        if (uvm == UV_CFL_PRED) fd.mode[b] = with_cfl(fd.mode[b], cfl_u, cfl_v);
        else if (uvd) fd.mode[b] = with_angle_uv(fd.mode[b], uvd);
        if (yd) fd.mode[b] = with_angle_y(fd.mode[b], yd);
        if (split) fd.mode[b] = with_tx_split(fd.mode[b], qmask);
        fd.mv[b] = inter ? mvw : 0;
    };
    if (fd.fp.key) {  // intra: left / above dependencies (raster order)
      for (int by = 0; by < g.bh; ++by)
        for (int bx = 0; bx < g.bw; ++bx) code_block(by, bx, nullptr, nullptr);
    } else {  // inter blocks only read the reference: rows in parallel
      // per-block search (the MVs only), kMvRefineRounds rounds of the neighbour-MV
      // refinement (tv/av1_enc.h), then every block coded with its final MV
      std::vector<uint32_t> mvs(nb), nxt(nb);
      parallel_rows(g.bh, [&](int by) {
        for (int bx = 0; bx < g.bw; ++bx) code_block(by, bx, nullptr, &mvs[by * g.bw + bx]);
      });
      for (int round = 0; round < kMvRefineRounds; ++round) {
        parallel_rows(g.bh, [&](int by) {
          for (int bx = 0; bx < g.bw; ++bx) {
            const int b = by * g.bw + bx;
            uint32_t cand[kMvRefineMaxCand];
            const int nc = mv_refine_cands(mvs.data(), g.bw, g.bh, bx, by, cand);
            int s0[256];
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) s0[i * 16 + j] = S.y[(size_t)(by * 16 + i) * g.W + bx * 16 + j];
            int best = 1 << 30;
            for (int k = 0; k < nc; ++k) {
              int pr[256];
              predict(g, 0, bx, by, pack_mode(1, 0, 0, 0, 0), cand[k], rec, ref, pr);
              const int c = satd_block(s0, pr, 16);
              if (c < best) best = c, nxt[b] = cand[k];
            }
          }
        });
        mvs.swap(nxt);
      }
      // MV unification (tv/av1_enc.h): every complete 32x32 quad, then every complete 64x64
      // superblock, takes one of its members' MVs when that costs at most a few bits' worth
      // of luma SATD (skip blocks then merge into 32x32 / 64x64 blocks)
      auto blk_satd = [&](int bx, int by, uint32_t m) {
        int s0[256], pr[256];
        for (int i = 0; i < 16; ++i)
          for (int j = 0; j < 16; ++j) s0[i * 16 + j] = S.y[(size_t)(by * 16 + i) * g.W + bx * 16 + j];
        predict(g, 0, bx, by, pack_mode(1, 0, 0, 0, 0), m, rec, ref, pr);
        return satd_block(s0, pr, 16);
      };
      parallel_rows(g.bh / 2, [&](int qy) {
        for (int qx = 0; qx < g.bw / 2; ++qx) {
          int sat[4][4];
          uint32_t m[4];
          for (int k = 0; k < 4; ++k) m[k] = mvs[(2 * qy + (k >> 1)) * g.bw + 2 * qx + (k & 1)];
          for (int k = 0; k < 4; ++k)
            for (int c = 0; c < 4; ++c) sat[k][c] = blk_satd(2 * qx + (k & 1), 2 * qy + (k >> 1), m[c]);
          const int c = quad_unify(sat, lam);
          if (c >= 0)
            for (int k = 0; k < 4; ++k) mvs[(2 * qy + (k >> 1)) * g.bw + 2 * qx + (k & 1)] = m[c];
        }
      });
      parallel_rows(g.sbh, [&](int sy) {
        for (int sx = 0; sx < g.sbw; ++sx) {
          if (sx * 4 + 3 >= g.bw || sy * 4 + 3 >= g.bh) continue;
          uint32_t cand[4];
          int own = 0, tot[4] = {0, 0, 0, 0};
          for (int q = 0; q < 4; ++q) cand[q] = mvs[(sy * 4 + (q >> 1) * 2) * g.bw + sx * 4 + (q & 1) * 2];
          for (int k = 0; k < 16; ++k) {
            const int bx = sx * 4 + (k & 3), by = sy * 4 + (k >> 2);
            own += blk_satd(bx, by, mvs[by * g.bw + bx]);
            for (int c = 0; c < 4; ++c) tot[c] += blk_satd(bx, by, cand[c]);
          }
          const int c = sb_unify(own, tot, lam);
          if (c >= 0)
            for (int k = 0; k < 16; ++k) mvs[(sy * 4 + (k >> 2)) * g.bw + sx * 4 + (k & 3)] = cand[c];
        }
      });
      {  // the frame's inter rounding from its luma SATD at the final MVs (tv/av1_enc.h)
        std::vector<long long> row(g.bh, 0);
        parallel_rows(g.bh, [&](int by) {
          for (int bx = 0; bx < g.bw; ++bx) row[by] += blk_satd(bx, by, mvs[by * g.bw + bx]);
        });
        long long tot = 0;
        for (long long r : row) tot += r;
        frame_rnd = inter_rounding(tot, g.W, g.H);
      }
      parallel_rows(g.bh, [&](int by) {
        for (int bx = 0; bx < g.bw; ++bx) code_block(by, bx, &mvs[by * g.bw + bx], nullptr);
      });
      fd.ib.assign(nb, 0);
      if (tools & kToolIntraInInter) {
        // intra blocks in inter frames (tv/av1_enc.h): candidates from source neighbours in
        // parallel, acceptance from the candidate map, accepted blocks re-coded in raster order
        parallel_rows(g.bh, [&](int by) {
          for (int bx = 0; bx < g.bw; ++bx) {
            const int ic = blk_satd(bx, by, mvs[by * g.bw + bx]);
            if (!ib_gated(ic)) continue;
            int s0[256];
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) s0[i * 16 + j] = S.y[(size_t)(by * 16 + i) * g.W + bx * 16 + j];
            IntraEdge e;
            intra_edges([&](int x, int y) { return (int)S.y[(size_t)y * g.W + x]; }, bx * 16, by * 16, 16, e);
            const int dc = intra_dc(e, 16);
            const int best = ib_best_cost(
                [&](int m) {
                  int pr[256];
                  for (int i = 0; i < 16; ++i)
                    for (int j = 0; j < 16; ++j) pr[i * 16 + j] = intra_pred_px(m, e, 16, i, j, dc);
                  return satd_block(s0, pr, 16);
                },
                lam);
            if (ib_candidate(ic, best, lam)) fd.ib[by * g.bw + bx] = 1;
          }
        });
        std::vector<uint8_t> cm(fd.ib);
        for (int by = 0; by < g.bh; ++by)
          for (int bx = 0; bx < g.bw; ++bx)
            if (ib_accepted(cm.data(), g.bw, bx, by)) {
              fd.ib[by * g.bw + bx] |= 2;
              code_block(by, bx, nullptr, nullptr, true);
            }
      }
      for (int sy = 0; sy < g.sbh; ++sy)
        for (int sx = 0; sx < g.sbw; ++sx) merge_sb(fd.mode.data(), fd.mv.data(), g.bw, g.bh, sx, sy);
    }
    // loop filters with the CDEF search on the deblocked frame
    const int W = g.W, H = g.H;
    Planes db;
    {
      // deblock only (cdef off) to obtain the search input
      std::vector<int8_t> off(g.nsb(), -1);
      loop_filters(g, fd.fp, fd.mode.data(), off.data(), rec, db);
    }
    const int n8 = (W / 8) * (H / 8), nfb = g.nsb();
    std::vector<uint8_t> dir(n8);
    std::vector<int> var(n8);
    cdef_find_dirs(db.y.data(), W, H, dir.data(), var.data());
    mark_cdef_skip(g, fd.mode.data(), dir.data());
    std::vector<uint64_t> sy((size_t)nfb * kCdefPresets), su(sy.size()), sv(sy.size());
    cdef_search(S.y.data(), db.y.data(), W, H, false, dir.data(), var.data(), W / 8, fd.fp.cdef_damping, sy.data(),
                kCdefMaskY, true);
    cdef_search(S.u.data(), db.u.data(), W / 2, H / 2, true, dir.data(), var.data(), W / 8, fd.fp.cdef_damping,
                su.data(), kCdefMaskUV, true);
    cdef_search(S.v.data(), db.v.data(), W / 2, H / 2, true, dir.data(), var.data(), W / 8, fd.fp.cdef_damping,
                sv.data(), kCdefMaskUV, true);
    for (size_t i = 0; i < su.size(); ++i) su[i] += sv[i];
    std::vector<uint8_t> active(nfb, 0);
    for (int b = 0; b < nb; ++b)
      if (!mode_skip(fd.mode[b])) active[((b / g.bw) / 4) * g.sbw + (b % g.bw) / 4] = 1;
    fd.cdef_idx.assign(nfb, -1);
    cdef_choose(sy.data(), su.data(), active.data(), nfb, fd.fp.cdef_y, fd.fp.cdef_uv, fd.cdef_idx.data());
    if (dbg & 2) {
      fd.fp.cdef_bits = 0;
      std::memset(fd.fp.cdef_y, 0, sizeof(fd.fp.cdef_y));
      std::memset(fd.fp.cdef_uv, 0, sizeof(fd.fp.cdef_uv));
      for (int f = 0; f < nfb; ++f) fd.cdef_idx[f] = active[f] ? 0 : -1;
    }
    // final recon: CDEF applied to the deblocked frame, then the self-guided restoration
    // search per 64x64 unit on the CDEF output (off / candidate sets, SSE + rate)
    Planes fin, dbk;
    loop_filters(g, fd.fp, fd.mode.data(), fd.cdef_idx.data(), rec, fin, nullptr, &dbk);
    fd.lr.assign((size_t)3 * g.lr_nu() * 3, 0);
    const long long rate = lr_rate_cost(qidx);
    for (int p = 0; p < 3; ++p) {
      const int pw = p ? W / 2 : W, ph = p ? H / 2 : H, nu = g.lr_ux(p) * g.lr_uy(p), ux = g.lr_ux(p);
      const std::vector<uint8_t>& X = p == 0 ? fin.y : (p == 1 ? fin.u : fin.v);
      const std::vector<uint8_t>& D = p == 0 ? dbk.y : (p == 1 ? dbk.u : dbk.v);
      const std::vector<uint8_t>& Sp = p == 0 ? S.y : (p == 1 ? S.u : S.v);
      int32_t* P = fd.lr.data() + (size_t)p * g.lr_nu() * 3;
      // per-unit SSE in the normative unit grid
      auto unit_sse = [&](const std::vector<uint8_t>& O, std::vector<long long>& e) {
        e.assign(nu, 0);
        for (int y = 0; y < ph; ++y)
          for (int x = 0; x < pw; ++x) {
            const int d = (int)Sp[(size_t)y * pw + x] - (int)O[(size_t)y * pw + x];
            e[lr_unit_row(y, ph, p ? 1 : 0) * ux + lr_unit_col(x, pw)] += d * d;
          }
      };
      std::vector<long long> best;
      unit_sse(X, best);
      for (int u = 0; u < nu; ++u) P[3 * u] = -1, P[3 * u + 1] = P[3 * u + 2] = 0;
      for (int k = 0; k < ((dbg & 4) ? 0 : kNumLrSets); ++k) {
        const int set = lr_set(k);
        std::vector<int64_t> st((size_t)nu * 5);
        lr_stats(Sp.data(), X.data(), D.data(), pw, ph, p ? 1 : 0, set, st.data());
        std::vector<int32_t> prm((size_t)nu * 3);
        for (int u = 0; u < nu; ++u) {
          prm[3 * u] = set;
          sgr_solve((const long long*)&st[5 * u], sgr_param(set, 0), sgr_param(set, 2), &prm[3 * u + 1],
                    &prm[3 * u + 2]);
        }
        std::vector<uint8_t> o(X.size());
        lr_apply(X.data(), D.data(), pw, ph, p ? 1 : 0, prm.data(), o.data());
        std::vector<long long> e;
        unit_sse(o, e);
        for (int u = 0; u < nu; ++u)
          if (e[u] + rate < best[u]) {
            best[u] = e[u] + rate;
            P[3 * u] = set, P[3 * u + 1] = prm[3 * u + 1], P[3 * u + 2] = prm[3 * u + 2];
          }
      }
    }
    apply_lr(g, fd.lr.data(), dbk, fin);
    out.recon.push_back(std::move(fin));
    out.frames.push_back(std::move(fd));
  }
  return out;
}

}  // namespace av1
}  // namespace tv

// ================================================================== C API ===============
namespace {
thread_local std::string g_codec_err;
template <class F> int codec_guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_codec_err = e.what();
    return -1;
  }
}
void split_planes(const uint8_t* yuv, const tv::av1::SeqGeo& g, tv::av1::Planes& P) {
  const size_t ys = (size_t)g.W * g.H, cs = ys / 4;
  P.y.assign(yuv, yuv + ys);
  P.u.assign(yuv + ys, yuv + ys + cs);
  P.v.assign(yuv + ys + cs, yuv + ys + 2 * cs);
}
// frame parameter vector of the C API: key, qindex, lf[4], sharp, damping, cdef_bits,
// cdef_y[8], cdef_uv[8]
void pack_fparams(const tv::av1::FrameParams& fp, int32_t* p) {
  p[0] = fp.key | (fp.tx_select << 1);  // bit 1: tx_mode_select of an inter frame
  p[1] = fp.qindex;
  for (int i = 0; i < 4; ++i) p[2 + i] = fp.lf[i];
  p[6] = fp.sharp;
  p[7] = fp.cdef_damping;
  p[8] = fp.cdef_bits;
  for (int i = 0; i < 8; ++i) {
    p[9 + i] = fp.cdef_y[i];
    p[17 + i] = fp.cdef_uv[i];
  }
}
tv::av1::FrameParams unpack_fparams(const int32_t* p) {
  tv::av1::FrameParams fp;
  fp.key = p[0] & 1;
  fp.tx_select = (p[0] >> 1) & 1;
  fp.qindex = p[1];
  for (int i = 0; i < 4; ++i) fp.lf[i] = p[2 + i];
  fp.sharp = p[6];
  fp.cdef_damping = p[7];
  fp.cdef_bits = p[8];
  for (int i = 0; i < 8; ++i) {
    fp.cdef_y[i] = (uint8_t)p[9 + i];
    fp.cdef_uv[i] = (uint8_t)p[17 + i];
  }
  return fp;
}
void join_planes(const tv::av1::Planes& P, uint8_t* out) {
  std::memcpy(out, P.y.data(), P.y.size());
  std::memcpy(out + P.y.size(), P.u.data(), P.u.size());
  std::memcpy(out + P.y.size() + P.u.size(), P.v.data(), P.v.size());
}
}  // namespace

extern "C" {
using namespace tv::av1;
const char* tv_av1c_last_error() { return g_codec_err.c_str(); }

// Dc_Qlookup / Ac_Qlookup (8-bit) of q-index q (dc != 0: the DC table)
int tv_av1c_qlookup(int q, int dc) { return dc ? dc_q(q) : ac_q(q); }

// Encoder model constants (av1_enc.h) for the GPU engine's host side.  out [7 + kNumLrSets] =
// kCdefMaskY, kCdefMaskUV, kMvMemoRecordBytes, kIbPasses, kToolIntraInInter, kToolCfl, then
// the lr_set() values, then kToolDirIntra, then kToolTxSplit; returns kNumLrSets.
int tv_av1c_model_constants(int64_t* out) {
  const int64_t c[6] = {(int64_t)kCdefMaskY, (int64_t)kCdefMaskUV, kMvMemoRecordBytes, kIbPasses, kToolIntraInInter,
                        kToolCfl};
  for (int i = 0; i < 6; ++i) out[i] = c[i];
  for (int k = 0; k < kNumLrSets; ++k) out[6 + k] = lr_set(k);
  out[6 + kNumLrSets] = kToolDirIntra;
  out[7 + kNumLrSets] = kToolTxSplit;
  return kNumLrSets;
}
// Per-q-index model values: out [3] = lf_level_for_q, lr_rate_cost, cdef_damping_for_q.
void tv_av1c_model_q(int q, int64_t* out) {
  out[0] = lf_level_for_q(q);
  out[1] = lr_rate_cost(q);
  out[2] = cdef_damping_for_q(q);
}

// Golden encode of n coded-size I420 frames (concatenated Y U V per frame) at `qidx`:
// the temporal units go to `out` (one Bytes object) and their byte sizes to tu_sizes[n];
// the post-filter reconstructions to recon (same layout); per-frame decisions to mode /
// mv [n][nblk] and levels ly [n][nblk][256], lu / lv [n][nblk][64] (may be null).
// tools: the coding-tools word (av1_enc.h kToolIntraInInter, kToolCfl, kToolDirIntra, kToolTxSplit);
// ib [n][nblk] (may be
// null): per frame and block, bit 0 = intra candidate, bit 1 = accepted.
int tv_av1c_golden_encode(int dw, int dh, int n, const uint8_t* yuv, int qidx, const int* qmap, int tools, void* out,
                          int64_t* tu_sizes, uint8_t* recon, uint32_t* mode, uint32_t* mv, int16_t* ly, int16_t* lu,
                          int16_t* lv, int32_t* fparams, int8_t* cdef, int32_t* lr, uint8_t* ib) {
  return codec_guard([&] {
    const SeqGeo g = make_seq_geo(dw, dh);
    const size_t fsz = (size_t)g.W * g.H * 3 / 2;
    std::vector<Planes> src(n);
    for (int i = 0; i < n; ++i) split_planes(yuv + i * fsz, g, src[i]);
    GoldenOut go = golden_encode(g, src, qidx, qmap, tools);
    auto* bytes = static_cast<std::vector<uint8_t>*>(out);
    bytes->clear();
    const int nb = g.nblk();
    EntropyState est;
    for (int i = 0; i < n; ++i) {
      const auto tu = write_temporal_unit(g, go.frames[i].view(), i == 0, &est);
      bytes->insert(bytes->end(), tu.begin(), tu.end());
      tu_sizes[i] = (int64_t)tu.size();
      if (recon) join_planes(go.recon[i], recon + i * fsz);
      const FrameData& fd = go.frames[i];
      if (mode) std::memcpy(mode + (size_t)i * nb, fd.mode.data(), sizeof(uint32_t) * nb);
      if (mv) std::memcpy(mv + (size_t)i * nb, fd.mv.data(), sizeof(uint32_t) * nb);
      if (ly) std::memcpy(ly + (size_t)i * nb * 256, fd.ly.data(), sizeof(int16_t) * nb * 256);
      if (lu) std::memcpy(lu + (size_t)i * nb * 64, fd.lu.data(), sizeof(int16_t) * nb * 64);
      if (lv) std::memcpy(lv + (size_t)i * nb * 64, fd.lv.data(), sizeof(int16_t) * nb * 64);
      if (fparams) pack_fparams(fd.fp, fparams + (size_t)i * 25);
      if (cdef) std::memcpy(cdef + (size_t)i * g.nsb(), fd.cdef_idx.data(), g.nsb());
      if (lr) std::memcpy(lr + (size_t)i * fd.lr.size(), fd.lr.data(), sizeof(int32_t) * fd.lr.size());
      if (ib) {
        if (fd.ib.empty()) std::memset(ib + (size_t)i * nb, 0, nb);
        else std::memcpy(ib + (size_t)i * nb, fd.ib.data(), nb);
      }
    }
  });
}

// Acceptance of intra candidates (av1_enc.h ib_accepted): cand [bh][bw] bytes (bit 0 =
// candidate) -> acc [bh][bw] (1 = accepted).
int tv_av1c_ib_accept(const uint8_t* cand, int bw, int bh, uint8_t* acc) {
  return codec_guard([&] {
    if (bw < 1 || bh < 1) throw std::runtime_error("av1: bad block grid");
    for (int by = 0; by < bh; ++by)
      for (int bx = 0; bx < bw; ++bx) acc[by * bw + bx] = ib_accepted(cand, bw, bx, by) ? 1 : 0;
  });
}

// Chroma-from-luma fit and decision of one block (av1_enc.h "chroma from luma"): luma [256]
// the block's reconstructed luma, su / sv [64] the chroma sources, dc_u / dc_v the planes'
// DC_PRED values, best the cost of the best regular mode.  out [9] = den, num_u, num_v, a0_u,
// a0_v, alpha_u, alpha_v, CfL wins (0 / 1), cfl_bits16(alpha_u, alpha_v).
int tv_av1c_cfl_decide(const uint8_t* luma, const uint8_t* su, const uint8_t* sv, int dc_u, int dc_v, int lam, int best,
                       int32_t* out) {
  return codec_guard([&] {
    int16_t ac[64];
    cfl_ac_block([&](int x, int y) { return (int)luma[y * 16 + x]; }, 0, 0, ac);
    int den = 0, num[2] = {0, 0}, a0[2], sat[2][3] = {{0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < 64; ++i) den += ac[i] * ac[i];
    for (int pl = 0; pl < 2; ++pl) {
      const uint8_t* s = pl ? sv : su;
      const int dc = pl ? dc_v : dc_u;
      int src[64], pr[64];
      for (int i = 0; i < 64; ++i) src[i] = s[i], num[pl] += ac[i] * (s[i] - dc);
      a0[pl] = cfl_fit(num[pl], den);
      for (int k = 0; k < 3; ++k) {
        const int a = cfl_cand(a0[pl], k);
        if (a < -16 || a > 16) continue;
        for (int i = 0; i < 64; ++i) pr[i] = cfl_pred_px(dc, a, ac[i]);
        sat[pl][k] = satd_block(src, pr, 8);
      }
    }
    int au = 0, av = 0;
    const bool win = cfl_decide(a0[0], a0[1], sat[0], sat[1], lam, best, &au, &av);
    const int32_t r[9] = {den, num[0], num[1], a0[0], a0[1], au, av, win ? 1 : 0, cfl_bits16(au, av)};
    std::memcpy(out, r, sizeof(r));
  });
}

// ---- directional intra (av1_enc.h "directional intra"): the model without an encode ----
namespace {
// edges [2 * N + 1] = above[0..N-1], left[0..N-1], top-left, as intra_edges leaves them
void dir_edges(const uint8_t* edges, int N, int have_a, int have_l, IntraEdge& e) {
  for (int i = 0; i < N; ++i) e.above[i] = edges[i], e.left[i] = edges[N + i];
  e.tl = edges[2 * N];
  e.have_a = have_a != 0;
  e.have_l = have_l != 0;
}
}  // namespace

// N x N (8 or 16) prediction of (mode, delta) from the given edges into pred [N * N].
int tv_av1c_dir_predict(int N, const uint8_t* edges, int have_a, int have_l, int mode, int delta, uint8_t* pred) {
  return codec_guard([&] {
    if ((N != 8 && N != 16) || mode < 0 || mode > PAETH_PRED || mode == 3 || mode == 7 || mode == 8 ||
        !dir_delta_ok(mode, delta))
      throw std::runtime_error("av1: (mode, delta) outside the encoder subset");
    IntraEdge e;
    dir_edges(edges, N, have_a, have_l, e);
    const int dc = intra_dc(e, N);
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) pred[i * N + j] = (uint8_t)intra_pred_px_ang(mode, delta, e, N, i, j, dc);
  });
}

// The rate tables (1/16 bit) and the derivative table: kf_y [5][5][13], y_mode [13] (size group
// 2), uv [13][14], angle [8][7], deriv [88] (Dr_Intra_Derivative by angle, 0 where undefined).
void tv_av1c_dir_tables(int32_t* kf_y, int32_t* y_mode, int32_t* uv, int32_t* angle, int32_t* deriv) {
  for (int a = 0; a < 5; ++a)
    for (int l = 0; l < 5; ++l)
      for (int m = 0; m < 13; ++m) kf_y[(a * 5 + l) * 13 + m] = tab::kKfYModeBits16[a][l][m];
  for (int m = 0; m < 13; ++m) y_mode[m] = tab::kYModeBits16[m];
  for (int y = 0; y < 13; ++y)
    for (int m = 0; m < 14; ++m) uv[y * 14 + m] = tab::kUvMode1Bits16[y][m];
  for (int k = 0; k < 8; ++k)
    for (int d = 0; d < 7; ++d) angle[k * 7 + d] = tab::kAngleDeltaBits16[k][d];
  for (int a = 0; a < 88; ++a) deriv[a] = 0;
  for (int k = 0; k < kNumDirCand; ++k) {
    if (!dir_cand_delta(k) && !(dir_cand_mode(k) >= D135_PRED && dir_cand_mode(k) <= D157_PRED)) continue;
    const int a = dir_base_angle(dir_cand_mode(k)) + 3 * dir_cand_delta(k);
    deriv[180 - a] = dr_deriv(180 - a);
    deriv[a - 90] = dr_deriv(a - 90);
  }
}

// The search order: out [34][2] = mode, delta of every candidate.
void tv_av1c_dir_cands(int32_t* out) {
  for (int k = 0; k < kNumDirCand; ++k) out[2 * k] = dir_cand_mode(k), out[2 * k + 1] = dir_cand_delta(k);
}

// The 34-candidate decision (dir_cand order, first strict minimum) of one block.  N = 16: luma,
// src [256] and edges; rate context kf (key frame), above / left (the neighbours' y modes);
// src_v / edges_v / ym unused (may be null).  N = 8: chroma, src / edges the U plane's and src_v
// / edges_v the V plane's, ym the block's chosen y mode; kf / above / left unused.  edges as in
// tv_av1c_dir_predict.  cost [34]: every candidate's cost; *win: the winner's index.
int tv_av1c_dir_decide(int N, const uint8_t* src, const uint8_t* src_v, const uint8_t* edges, const uint8_t* edges_v,
                       int have_a, int have_l, int lam, int kf, int above, int left, int ym, int32_t* cost, int* win) {
  return codec_guard([&] {
    if (N != 8 && N != 16) throw std::runtime_error("av1: bad block size");
    if (N == 8 && (!src_v || !edges_v)) throw std::runtime_error("av1: chroma decision needs both planes");
    IntraEdge e[2];
    int s[2][256], dc[2];
    for (int pl = 0; pl < (N == 8 ? 2 : 1); ++pl) {
      dir_edges(pl ? edges_v : edges, N, have_a, have_l, e[pl]);
      dc[pl] = intra_dc(e[pl], N);
      for (int i = 0; i < N * N; ++i) s[pl][i] = (pl ? src_v : src)[i];
    }
    int best = 1 << 30;
    for (int k = 0; k < kNumDirCand; ++k) {
      const int m = dir_cand_mode(k), d = dir_cand_delta(k);
      int c = 0, pr[256];
      for (int pl = 0; pl < (N == 8 ? 2 : 1); ++pl) {
        for (int i = 0; i < N; ++i)
          for (int j = 0; j < N; ++j) pr[i * N + j] = intra_pred_px_ang(m, d, e[pl], N, i, j, dc[pl]);
        c += satd_block(s[pl], pr, N);
      }
      c += (lam * (N == 16 ? dir_y_bits16(kf != 0, above, left, m, d) : dir_uv_bits16(ym, m, d))) >> 8;
      cost[k] = c;
      if (c < best) best = c, *win = k;
    }
  });
}

// Transform-split decision of one inter block's luma (av1_enc.h "transform split"): src / pred
// [256] (raster), q-index, inter rounding.  lev16 [256] / rec16 [256]: the 16x16 coding; lev8 [256]
// (four 8x8 rasters, quadrant raster order) / rec8 [256] (block raster): the split coding.
// out [7] = split (0 / 1), quadrant mask, sse16, bits16 of the 16x16 levels, sse8, bits16 of the
// split levels (both without the flag terms), tx_lambda(q).
int tv_av1c_tx_split_decide(const uint8_t* src, const uint8_t* pred, int qidx, int rnd, int16_t* lev16, uint8_t* rec16,
                            int16_t* lev8, uint8_t* rec8, int64_t* out) {
  return codec_guard([&] {
    if (qidx < 1 || qidx > 255 || rnd < 0 || rnd > 64) throw std::runtime_error("av1: bad q-index / rounding");
    int s[256], p[256], rc[256];
    for (int i = 0; i < 256; ++i) s[i] = src[i], p[i] = pred[i];
    code_tb(s, p, 4, qidx, 0, rnd, lev16, rc);
    TxSplitTrial t;
    tx_split_trial(s, p, qidx, rnd, lev16, rc, t);
    std::memcpy(lev8, t.lev8, sizeof(t.lev8));
    for (int i = 0; i < 256; ++i) rec16[i] = (uint8_t)rc[i], rec8[i] = (uint8_t)t.rec8[i];
    const int64_t r[7] = {t.split, t.qmask, t.sse16, t.bits16, t.sse8, t.bits8, tx_lambda(qidx)};
    std::memcpy(out, r, sizeof(r));
  });
}

// Decode a stream (concatenated temporal units) -> up to max_frames coded-size frames.
// geo[0..3] = display w, h, coded W, H; returns the frame count in *nframes.
int tv_av1c_decode(const uint8_t* data, size_t n, int max_frames, uint8_t* frames, int* geo, int* nframes) {
  return codec_guard([&] {
    Decoded d = decode_stream(data, n);
    geo[0] = d.geo.dw;
    geo[1] = d.geo.dh;
    geo[2] = d.geo.W;
    geo[3] = d.geo.H;
    *nframes = (int)d.frames.size();
    if (frames) {
      const size_t fsz = (size_t)d.geo.W * d.geo.H * 3 / 2;
      for (int i = 0; i < std::min(max_frames, (int)d.frames.size()); ++i) join_planes(d.frames[i], frames + i * fsz);
    }
  });
}

// The decoder oracle's mode and MV words of up to max_frames frames: mode / mv [frames][nblk].
int tv_av1c_decode_modes(const uint8_t* data, size_t n, int max_frames, uint32_t* mode, uint32_t* mv) {
  return codec_guard([&] {
    Decoded d = decode_stream(data, n);
    const size_t nb = (size_t)d.geo.nblk();
    for (int i = 0; i < std::min(max_frames, (int)d.data.size()); ++i) {
      std::memcpy(mode + i * nb, d.data[i].mode.data(), sizeof(uint32_t) * nb);
      std::memcpy(mv + i * nb, d.data[i].mv.data(), sizeof(uint32_t) * nb);
    }
  });
}

// Probe a stream's geometry / frame count without reconstructing (header walk).
int tv_av1c_probe(const uint8_t* data, size_t n, int* geo, int* nframes) {
  return tv_av1c_decode(data, n, 0, nullptr, geo, nframes);
}

// Write one frame's temporal unit from engine decisions (packed levels layout; packed == 2:
// eob-truncated scan-order TBs, FrameDecisions::scan_packed).
void* tv_av1c_state_new() { return new EntropyState(); }
void tv_av1c_state_free(void* s) { delete static_cast<EntropyState*>(s); }

// `state` (tv_av1c_state_new): the stream's entropy state, frames written in order.
int tv_av1c_write_tu(void* state, int dw, int dh, const int* fparams, const uint32_t* mode, const uint32_t* mv,
                     const int16_t* ly,
                     const int16_t* lu, const int16_t* lv, const int8_t* cdef_idx, const int32_t* lr, int packed,
                     int seq_header, void* out) {
  return codec_guard([&] {
    const SeqGeo g = make_seq_geo(dw, dh);
    FrameDecisions d;
    d.fp = unpack_fparams(fparams);
    d.mode = mode;
    d.mv = mv;
    d.ly = ly;
    d.lu = lu;
    d.lv = lv;
    d.cdef_idx = cdef_idx;
    d.lr = lr;
    d.packed = packed != 0;
    d.scan_packed = packed == 2;
    auto tu = write_temporal_unit(g, d, seq_header != 0, static_cast<EntropyState*>(state));
    auto* bytes = static_cast<std::vector<uint8_t>*>(out);
    bytes->insert(bytes->end(), tu.begin(), tu.end());
  });
}
}  // extern "C"
