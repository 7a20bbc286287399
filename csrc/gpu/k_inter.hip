// k_inter.hip — P-frame kernels.
//
//  k_inter_me     pass A per CTB (256 threads = 4 waves):
//                   * the source CTB and one 38-row window per candidate centre (up to 7)
//                     are staged in LDS as 32-bit words;
//                   * integer search of an 8 x 7 window around every centre: each thread owns
//                     4 horizontally adjacent positions of one 16x16 quadrant, loads 3 window
//                     words per row and derives the 4 shifted rows with v_alignbyte,
//                     accumulating its 4 8x8 SADs with v_sad_u8 (4 pixels / instruction);
//                     16x16 and 32x32 costs are sums of 8x8 SADs (SAD reuse);
//                   * half- then quarter-pel refinement of all 21 blocks at once, reading
//                     the precomputed phase planes (no per-block barriers);
//                   * bottom-up CU split decision.
//  k_inter_recon  pass B per CTB: luma prediction = phase-plane loads, chroma 4-tap MC,
//                 residual, MFMA transform/quant, exact inverse, reconstruction; the MFMA
//                 operands are f16 fragments (constant tables of tv/tb_frag.h, intermediates
//                 stored split by their producer), the quantiser 32-bit with per-tile parameters.
#include <stdexcept>
#include <type_traits>

#include "gpu_common.h"
#include "k_encode.h"
#include "tb_coder.h"
#include "wave_tb.h"
#include "tv/me_model.h"
#include "tv/rc_model.h"
#include "tv/rdq.h"
#include "tv/sdh.h"

namespace tv {
namespace gpu {

// ---------------------------------------------------------------------------------------
// Hierarchical motion search (tv/me_model.h; the CPU golden model is tv::analyze_inter).
//
//  k_quarter     quarter-resolution luma of the source: (sum of a 4x4 block + 8) >> 4,
//                one v_sad_u8 against zero per source row word.
//  k_coarse_me   one wave per CTB: the 8x8 quarter-res block vs the previous quarter-res
//                SOURCE frame, full search over [-Rq, Rq]^2 (Rq = range/4) from an LDS
//                window, 4 horizontally adjacent candidates per lane via v_qsad_pk_u16_u8
//                (qsad_row).  No recon dependency: the coarse field is a lookahead.
//  k_inter_me    four waves per CTB: up to 7 candidate centres (zero, coarse, 4 coarse
//                neighbours, temporal), an [-4,+3] x [-3,+3] integer window each staged in
//                LDS pre-aligned to the window origin; every lane owns 4 adjacent positions
//                of one (candidate, row, 16x16 quadrant) and accumulates its 4 8x8 SADs with
//                v_alignbyte + v_sad_u8 (16x16 / 32x32 are sums: SAD reuse; the 32x32 sum
//                crosses the quad's lanes by DPP; v_qsad_pk_u16_u8 measured no faster here:
//                profiles/README.md); then half/quarter-pel refinement of the 21 blocks from
//                the phase planes and the bottom-up CU split decision.  Rate = MVD bits
//                against the CTB predictor.
// ---------------------------------------------------------------------------------------
#ifndef TV_ME_THREADS
#define TV_ME_THREADS 256
#endif
constexpr int kMeThreads = TV_ME_THREADS;  // a multiple of 64 (the DPP group sums assume it)
static_assert(kMeThreads % 64 == 0 && kMeThreads >= 256, "k_inter_me block size");
constexpr int kFRows = kCtb + kMeWinH - 1;  // 38 window rows per candidate
constexpr int kFWords = 12;                 // 48 bytes staged (40 used: 32 + 7 offsets + 1)
constexpr int kFChunks = kFWords / 4;       // 16-byte chunks per staged row
// Window layout: pitch 12 words, rows >= 16 kWinSkew words further (per candidate).  A
// half-wave of the integer search reads 8 (row, 4-position group) items x 4 quadrants,
// rows r and r + 16 together; brute force over pitch / skew (ds_read_b32 banks (a/4) % 32)
// gives 1344 extra LDS cycles over all item phases for 12 / +2 against 2016 for the former
// odd pitch 13, in less LDS.
constexpr int kFPitch = kFWords, kWinSkew = 2, kWinCand = kFRows * kFPitch + kWinSkew;
__device__ __forceinline__ int win_word(int k, int r, int w) { return k * kWinCand + r * kFPitch + (r >= 16 ? kWinSkew : 0) + w; }
// LDS pitch (words) of a source-CTB row (uniform s0/s1 reads stay one aligned 8-byte read).
// Every 8-row band sits kSrcSkew (8) words further, so rows 8 apart land 8 banks apart: the
// sub-pel SAD lanes of one candidate read rows by + j of blocks 8 / 16 rows apart at the same
// time (with a flat 8-word pitch 64 words apart -- one bank, 4-way conflicts: 18.6 % of the
// kernel's LDS cycles, r6_prof), and the four quadrant lanes of an integer-search item read
// rows r and r + 16 (16 banks apart) at word offsets 0 / 4: 32 distinct banks either way.
constexpr int kSrcP = 8, kSrcSkew = 8;
__device__ __forceinline__ int src_word(int row, int w) { return row * kSrcP + w + (row >> 3) * kSrcSkew; }

// tv::dequant_level in 32-bit arithmetic: with m = 16 * levelScale << (qp / 6) and the level
// clamped to +-thr, where thr * m is at least (32768 + 1) << bdShift, a clamped level still
// saturates to the same int16 bound and every unclamped product fits in 32 bits -- the same
// result as the 64-bit golden form, with a med3 + mad + shift + med3 per level.  Any such thr
// gives the same levels, so it comes without a division: with 2^p <= m < 2^(p+1), thr =
// (32769 << bdShift >> p) + 1 >= (32769 << bdShift) / m, and thr * m < 2 * (32769 << bdShift)
// + 2^(p+1) <= 2^25 + 2^19 (bdShift <= 8, m < 2^19).
struct DeqParams {
  int m, thr, sh, rnd;
};
__device__ __forceinline__ DeqParams deq_params(int qp, int log2N) {
  DeqParams d;
  d.sh = 8 + log2N - 5;
  d.rnd = 1 << (d.sh - 1);
  d.m = (16 * level_scale(qp)) << (qp / 6);
  d.thr = (((32768 + 1) << d.sh) >> (31 - __builtin_clz(d.m))) + 1;
  return d;
}
__device__ __forceinline__ int deq_fast(int level, const DeqParams& d) {
  const int t = clip3(-d.thr, d.thr, level);
  return clip3(-32768, 32767, (t * d.m + d.rnd) >> d.sh);
}

// the 4 byte differences a - b as two dwords of int16 pairs (residual = source - prediction)
__device__ __forceinline__ uint2 bytes_minus(uint32_t a, uint32_t b) {
  typedef short s2 __attribute__((ext_vector_type(2)));
  const s2 lo = __builtin_bit_cast(s2, __builtin_amdgcn_perm(0u, a, 0x0c010c00u)) -
                __builtin_bit_cast(s2, __builtin_amdgcn_perm(0u, b, 0x0c010c00u));
  const s2 hi = __builtin_bit_cast(s2, __builtin_amdgcn_perm(0u, a, 0x0c030c02u)) -
                __builtin_bit_cast(s2, __builtin_amdgcn_perm(0u, b, 0x0c030c02u));
  return make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}
__device__ __forceinline__ int phase_at(const uint8_t* P, const Geo& g, int x, int y) {
  x = clip3(-8, g.W + 7, x);
  y = clip3(-8, g.H + 7, y);
  return P[(long)(y + 8) * g.pw16 + x + 8];
}
// 4 bytes of row `row` starting at byte x (any alignment), clamped horizontally to [0, w-1]
__device__ __forceinline__ uint32_t load4_clamped(const uint8_t* row, int x, int w) {
  const int a = x & ~3, sh = x & 3;
  if (x >= 0 && a + 7 < w) {
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row + a);
    if (!sh) return w0;
    const uint32_t w1 = *reinterpret_cast<const uint32_t*>(row + a + 4);
    return __builtin_amdgcn_alignbyte(w1, w0, sh);
  }
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) v |= (uint32_t)row[clip3(0, w - 1, x + k)] << (8 * k);
  return v;
}

// The sliding SAD step of the coarse search: an 8-pixel source row (s0, s1) against the 4
// horizontally adjacent positions starting at byte 0 of the window words wp[0..2].
// v_qsad_pk_u16_u8 adds SAD(bytes i..i+3 of a 64-bit operand, the 4 bytes of a dword) to the
// 16-bit lane i = 0..3 of a packed accumulator, so {wp[1]:wp[0]} against s0 and {wp[2]:wp[1]}
// against s1 are the whole row (v_alignbyte + v_sad_u8 take 14 instructions).  The two
// overlapping 8-byte LDS reads (4-byte aligned: ds_read2_b32) deliver the register pairs.
// An 8x8 block is at most 64 pixels x 255 = 16320 per lane: exact in 16 bits.
__device__ __forceinline__ uint64_t lds_pair(const uint32_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ uint64_t qsad_row(const uint32_t* wp, uint32_t s0, uint32_t s1, uint64_t acc) {
  acc = __builtin_amdgcn_qsad_pk_u16_u8(lds_pair(wp), s0, acc);
  return __builtin_amdgcn_qsad_pk_u16_u8(lds_pair(wp + 1), s1, acc);
}
__device__ __forceinline__ unsigned qsad_lane(uint64_t acc, int i) { return (unsigned)(acc >> (16 * i)) & 0xffffu; }

__global__ void __launch_bounds__(256) k_quarter(FrameSet src, uint8_t* q, Geo g) {
  const int b = blockIdx.y, qw = g.W >> 2, qh = g.H >> 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= qw * qh) return;
  const int x = i % qw, y = i / qw;
  const uint8_t* S = src.plane(0, b, g) + (long)(4 * y) * g.W + 4 * x;
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t*>(S + (long)j * g.W), 0u, s);
  q[(long)b * qw * qh + i] = (uint8_t)((s + 8) >> 4);
}

constexpr int kCoarseMaxRq = 32;
constexpr int kCoarseRows = 8 + 2 * kCoarseMaxRq;
constexpr int kCoarseWords = kCoarseMaxRq / 2 + 3;

__global__ void __launch_bounds__(64) k_coarse_me(const uint8_t* qcur, const uint8_t* qprev, Geo g, const RcTables* rc,
                                                  int seq_qp, int rq, int16_t* cmv, int* ccost) {
  const int lane = threadIdx.x;
  int ctu, b;
  xcd_ctb(ctu, b);
  const Penalties& pen = rc->pen[seq_qp];  // lookahead: the frame QP may depend on its result
  const int qw = g.W >> 2, qh = g.H >> 2;
  const int x0 = 8 * (ctu % g.wc), y0 = 8 * (ctu / g.wc);
  const uint8_t* C = qcur + (long)b * qw * qh;
  const uint8_t* P = qprev + (long)b * qw * qh;
  __shared__ uint32_t s32[16];
  extern __shared__ uint32_t win[];  // (8 + 2 rq) rows x ((rq / 2 + 3) | 1) words: sized per launch
  // the coarse MV-rate table (me_coarse_pen's scaling applied once): read per candidate
  __shared__ int penL[64];
  const int side = 2 * rq + 1, rows = 8 + 2 * rq, wpr = rq / 2 + 3, pitch = wpr | 1;
  penL[lane] = (pen.mv[lane] + 8) >> 4;
  if (lane < 16) s32[lane] = *reinterpret_cast<const uint32_t*>(C + (long)(y0 + (lane >> 1)) * qw + x0 + 4 * (lane & 1));
  for (int w = lane; w < rows * wpr; w += 64) {
    const int r = w / wpr, c = w - r * wpr;
    const uint8_t* row = P + (long)clip3(0, qh - 1, y0 - rq + r) * qw;
    win[r * pitch + c] = load4_clamped(row, x0 - rq + 4 * c, qw);
  }
  __syncthreads();
  unsigned best = 0xffffffffu;
  const int groups = rq / 2 + 1;
  uint32_t sv[16];  // the source block in registers (loop-invariant)
#pragma unroll
  for (int k = 0; k < 16; ++k) sv[k] = s32[k];
  // item = gi * side + dyi, advanced by 64 per pass without a division
  const int step_g = 64 / side, step_d = 64 - step_g * side;
  int gi = lane / side, dyi = lane - gi * side;
  for (int item = lane; item < groups * side; item += 64) {
    const int dy = dyi - rq, dx0 = 4 * gi - rq;
    const int leny = mv_bits_len(16 * dy);  // one dy per item: the 4 positions add their dx length
    uint64_t acc = 0;  // 4 positions x u16
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = qsad_row(win + (dyi + j) * pitch + gi, sv[2 * j], sv[2 * j + 1], acc);
#pragma unroll
    for (int sft = 0; sft < 4; ++sft) {  // no branch: the 4 table reads are in flight together
      const int dx = dx0 + sft;
      const unsigned rate = (unsigned)penL[me_pen_index_len(mv_bits_len(16 * dx), leny)];  // == me_coarse_pen
      const unsigned v = ((qsad_lane(acc, sft) + rate) << 13) | (unsigned)(dyi * side + dx + rq);
      best = (dx <= rq && v < best) ? v : best;  // the last group's positions past +rq do not count
    }
    gi += step_g;
    dyi += step_d;
    if (dyi >= side) {
      dyi -= side;
      ++gi;
    }
  }
  best = wave_min_u32(best);
  if (lane == 0) {
    const int idx = (int)(best & 8191), o = b * g.wc * g.hc + ctu;
    cmv[2 * o] = (int16_t)(4 * (idx % side - rq));
    cmv[2 * o + 1] = (int16_t)(4 * (idx / side - rq));
    ccost[o] = (int)(best >> 13);
  }
}

// The MV-rate table (Penalties::mv, 64 ints) is staged in LDS: the integer search and the
// sub-pel argmin read it per candidate.  8 waves per SIMD (<= 64 VGPRs): the LDS fits 8 CTBs
// per CU as well.
//
// kSatd (SeqConfig::subpel_satd, "SATD sub-pel decision" of tv/me_model.h): the two sub-pel
// rounds score every (8x8 group, candidate) cell by Hadamard SATD as well as SAD, on the matrix
// cores.  A 16x16 tile X holds four independent 8x8 cells of source - prediction; with
// Hbd = diag(H8, H8), Z = Hbd * (X * Hbd) transforms all four at once in two
// v_mfma_f32_16x16x16f16.  Operand maps (lane l, e / r = 0..3): A[row l & 15][k = 4 (l >> 4) + e],
// B[k = 4 (l >> 4) + e][col l & 15], C[row 4 (l >> 4) + r][col l & 15].  A lane's A fragment of X
// is 4 adjacent pixels of one row: one source dword of s32 minus 4 phase-plane samples.
// Y = X * Hbd comes out in the C map, which is the B map, so it feeds Hbd * Y without any
// lane movement, and Hbd is symmetric, so one constant fragment serves as B of the first and A
// of the second product.  |X| <= 255, |Y| <= 2040 (exact in f16), |Z| <= 16320 (exact in
// f32).  A lane loads the cell (row half (l >> 3) & 1, column half l >> 5) and ends with Z of
// the cell (row half l >> 5, column half (l >> 3) & 1); both lane sets are 8 lanes of a DPP
// half-row in two adjacent 16-lane rows, so SAD and SATD reduce the same way.  The per-cell
// tables live in the candidate windows' LDS, dead after the integer search.
__device__ __forceinline__ uint32_t phase4(const uint8_t* P, const Geo& g, int x, int y);
template <bool kSatd>
__global__ void __launch_bounds__(kMeThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) k_inter_me(FrameSet src, FrameSet ref, const uint8_t* phase,
                                                         DecisionSet dec, const int16_t* prev_mv, const int16_t* cmv,
                                                         Geo g, const RcTables* rc, int range,
                                                         CtbMeOut* bout, PIntraBuffers pi) {
  const int tid = threadIdx.x;
  int ctu, b;
  xcd_ctb(ctu, b);
  // the picture's QP is one value per workgroup: kept scalar, so the table's address does not
  // hold a VGPR pair down to the split decision at the end
  const Penalties& pen = rc->pen[__builtin_amdgcn_readfirstlane((int)dec.qp[b])];
  __shared__ int penmv[64];  // visible after the first barrier below
  if (tid < 64) penmv[tid] = pen.mv[tid];
  const int cxi = ctu % g.wc, cyi = ctu / g.wc, cx = cxi * 32, cy = cyi * 32;
  const uint8_t* S = src.plane(0, b, g);
  const uint8_t* R = ref.plane(0, b, g);
  __shared__ uint32_t s32[32 * kSrcP + 3 * kSrcSkew];
  __shared__ uint32_t win[kMeMaxCand * kWinCand];
  __shared__ int cand[kMeMaxCand][2];
  __shared__ int pmv[2], ncand;
  __shared__ unsigned best[21];
  __shared__ int bcost[21], bmv[21][2];
  __shared__ int subsad[21][8];
  for (int t = tid; t < 256; t += kMeThreads)
    s32[src_word(t >> 3, t & 7)] = *reinterpret_cast<const uint32_t*>(S + (long)(cy + (t >> 3)) * g.W + cx + 4 * (t & 7));
  // candidate sources: the coarse vectors of the CTB's 3x3 neighbourhood (clipped to the
  // picture) and the co-located previous vector, gathered by 10 lanes at once into LDS; thread
  // 0 then runs me_candidates on that local window (same bounds, so the same candidates)
  // instead of a chain of dependent global loads ahead of the window staging
  __shared__ int16_t nbmv[18], tmv[2];
  const int lx0 = cxi > 0 ? cxi - 1 : 0, ly0 = cyi > 0 ? cyi - 1 : 0;
  const int lw = (cxi + 1 < g.wc ? cxi + 1 : g.wc - 1) - lx0 + 1, lh = (cyi + 1 < g.hc ? cyi + 1 : g.hc - 1) - ly0 + 1;
  if (tid < 9) {
    const int i = tid % 3, j = tid / 3;
    if (i < lw && j < lh) {
      const int16_t* c = cmv + (long)b * g.wc * g.hc * 2 + 2 * ((long)(ly0 + j) * g.wc + lx0 + i);
      nbmv[2 * (j * lw + i)] = c[0];
      nbmv[2 * (j * lw + i) + 1] = c[1];
    }
  } else if (tid == 9) {
    const long u0 = b * g.usz + (long)(cy >> 3) * g.w8 + (cx >> 3);
    tmv[0] = prev_mv[2 * u0];
    tmv[1] = prev_mv[2 * u0 + 1];
  }
  if (tid < 21) best[tid] = 0xffffffffu;
  __syncthreads();
  if (tid == 0) ncand = me_candidates(nbmv, lw, lh, cxi - lx0, cyi - ly0, tmv[0], tmv[1], range - 4, cand, pmv);
  __syncthreads();
  const int nc = ncand;
  // candidate windows, each pre-aligned so byte 0 of a row is x = cx + cand_x + kMeWinX0
  // one lane per 16-byte chunk: a dwordx4 + dword load from the dword-aligned address, then
  // v_alignbyte to the candidate's byte offset (the clamped per-byte path only at the edges)
  // All of a thread's chunks (<= 4) are loaded before any is stored, so their global
  // latencies overlap instead of one round trip per loop pass.
  constexpr int kWinPer = (kMeMaxCand * kFRows * kFChunks + kMeThreads - 1) / kMeThreads;
  {
    const int ntot = nc * kFRows * kFChunks;
    uint4 u[kWinPer];
    uint32_t u4[kWinPer];
#pragma unroll
    for (int n = 0; n < kWinPer; ++n) {
      const int e = tid + n * kMeThreads;
      u[n] = make_uint4(0, 0, 0, 0);
      u4[n] = 0;
      if (e < ntot) {
        const int k = e / (kFRows * kFChunks), rem = e - k * (kFRows * kFChunks);
        const int r = rem / kFChunks, ch = rem - r * kFChunks;
        const uint8_t* row = R + (long)clip3(0, g.H - 1, cy + cand[k][1] + kMeWinY0 + r) * g.W;
        const int x = cx + cand[k][0] + kMeWinX0 + 16 * ch, a = x & ~3;
        if (x >= 0 && a + 20 <= g.W) {
          u[n] = *reinterpret_cast<const uint4*>(row + a);
          u4[n] = *reinterpret_cast<const uint32_t*>(row + a + 16);
        }
      }
    }
#pragma unroll
    for (int n = 0; n < kWinPer; ++n) {
      const int e = tid + n * kMeThreads;
      if (e >= ntot) break;
      const int k = e / (kFRows * kFChunks), rem = e - k * (kFRows * kFChunks);
      const int r = rem / kFChunks, ch = rem - r * kFChunks;
      const int x = cx + cand[k][0] + kMeWinX0 + 16 * ch, a = x & ~3, sh = x & 3;
      uint32_t* dst = win + win_word(k, r, 4 * ch);
      if (x >= 0 && a + 20 <= g.W) {
        dst[0] = __builtin_amdgcn_alignbyte(u[n].y, u[n].x, sh);
        dst[1] = __builtin_amdgcn_alignbyte(u[n].z, u[n].y, sh);
        dst[2] = __builtin_amdgcn_alignbyte(u[n].w, u[n].z, sh);
        dst[3] = __builtin_amdgcn_alignbyte(u4[n], u[n].w, sh);
      } else {  // the clamped per-byte path at the picture edges
        const uint8_t* row = R + (long)clip3(0, g.H - 1, cy + cand[k][1] + kMeWinY0 + r) * g.W;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = load4_clamped(row, x + 4 * j, g.W);
      }
    }
  }
  __syncthreads();

  // ------------------------------- integer refinement -----------------------------------
  // item = (candidate, window row, 4-position group, 16x16 quadrant): a lane accumulates
  // the 4 8x8 SADs of its quadrant for 4 adjacent positions (their sum is the quadrant's
  // 16x16 SAD); the 32x32 SADs are the sums of the 4 quadrants, which are the 4 lanes of a
  // quad (items 4j..4j+3): a DPP quad sum, no LDS round trip (a [position][quadrant] LDS
  // table cost 7.8 KB -- a CTB per CU of occupancy -- and a barrier).
  // Splitting by quadrant keeps every lane busy when few distinct candidates remain.
  unsigned lb[5];  // 4 8x8 blocks of my quadrant, then its 16x16
#pragma unroll
  for (int k = 0; k < 5; ++k) lb[k] = 0xffffffffu;
  unsigned lb32 = 0xffffffffu;  // the 32x32 minimum (quadrant-0 lanes)
  int qd = 0;
  for (int item = tid; item < nc * kMeWinH * 2 * 4; item += kMeThreads) {
    qd = item & 3;
    const int it = item >> 2;
    const int k = it / (kMeWinH * 2), rr = it - k * (kMeWinH * 2);
    const int dyi = rr >> 1, gs = rr & 1;
    const int pos0 = k * kMePosPerCand + dyi * kMeWinW + 4 * gs;
    const int my = cand[k][1] + kMeWinY0 + dyi;
    unsigned mvc[4];
    const int leny = mv_bits_len(4 * my - pmv[1]);  // one my per item, four mx
#pragma unroll
    for (int sft = 0; sft < 4; ++sft) {
      const int mx = cand[k][0] + kMeWinX0 + 4 * gs + sft;
      mvc[sft] = (unsigned)penmv[me_pen_index_len(mv_bits_len(4 * mx - pmv[0]), leny)];
    }
    const int qx = (qd & 1) * 16, qy = (qd >> 1) * 16;

    unsigned q16[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j8 = 0; j8 < 4; ++j8) {
      const int bx = qx + (j8 & 1) * 8, by = qy + (j8 >> 1) * 8;
      unsigned acc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int srow = src_word(by + j, bx >> 2);
        const uint32_t s0 = s32[srow], s1 = s32[srow + 1];
        const uint32_t* wp = win + win_word(k, dyi + by + j, gs + (bx >> 2));
        const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
        acc[0] = __builtin_amdgcn_sad_u8(w1, s1, __builtin_amdgcn_sad_u8(w0, s0, acc[0]));
#pragma unroll
        for (int sft = 1; sft < 4; ++sft) {
          const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sft);
          const uint32_t hi = __builtin_amdgcn_alignbyte(w2, w1, sft);
          acc[sft] = __builtin_amdgcn_sad_u8(hi, s1, __builtin_amdgcn_sad_u8(lo, s0, acc[sft]));
        }
      }
#pragma unroll
      for (int sft = 0; sft < 4; ++sft) {
        const unsigned v = ((acc[sft] + mvc[sft]) << 11) | (unsigned)(pos0 + sft);
        lb[j8] = v < lb[j8] ? v : lb[j8];
        q16[sft] += acc[sft];
      }
      __builtin_amdgcn_sched_barrier(0);  // bound live ranges: no hoisting across 8x8 blocks
    }
#pragma unroll
    for (int sft = 0; sft < 4; ++sft) {
      const unsigned v = ((q16[sft] + mvc[sft]) << 11) | (unsigned)(pos0 + sft);
      lb[4] = v < lb[4] ? v : lb[4];
      // the quad's lanes are one position's 4 quadrants (a quad is always wholly in range)
      int t = (int)q16[sft];
      t += dpp::mov<dpp::kQuadXor1>(t);
      t += dpp::mov<dpp::kQuadXor2>(t);
      const unsigned v32 = ((unsigned)(t + (int)mvc[sft]) << 11) | (unsigned)(pos0 + sft);
      lb32 = (qd == 0 && v32 < lb32) ? v32 : lb32;
    }
  }
  // a lane's quadrant is fixed (item stride is a multiple of 4: quadrant = lane & 3), so lb[]
  // maps to static slots.  Each slot is reduced over the 16 lanes of its quadrant class:
  // rotations by 4 and 8 inside a DPP row, then the row pairs and halves exchanged with
  // v_permlane16_swap / v_permlane32_swap (gfx950) -- lanes 0..3 end with quadrant 0..3's
  // minima and post them (5 x ~6 VALU instead of 20 full wave reductions)
  {
    auto umin = [](unsigned x, unsigned y) { return x < y ? x : y; };
    const int lane = tid & 63;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      unsigned v = lb[j];
      v = umin(v, (unsigned)dpp::mov<dpp::kRowRor4>((int)v));
      v = umin(v, (unsigned)dpp::mov<dpp::kRowRor8>((int)v));
      const auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
      v = umin(r16[0], r16[1]);
      const auto r32 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
      v = umin(r32[0], r32[1]);
      if (lane < 4) {  // quadrant q = lane: 8x8 block (q, j) in raster order, or its 16x16
        const int k = j < 4 ? ((lane >> 1) << 3) | ((j >> 1) << 2) | ((lane & 1) << 1) | (j & 1) : 16 + lane;
        atomicMin(&best[k], v);
      }
    }
  }
  {
    const unsigned m = wave_min_u32(lb32);
    if ((tid & 63) == 0) atomicMin(&best[20], m);
  }
  __syncthreads();
  if (tid < 21) {
    int mx = 0, my = 0;
    me_pos_to_mv((int)(best[tid] & 2047), cand, mx, my);
    bcost[tid] = (int)(best[tid] >> 11);
    bmv[tid][0] = 4 * mx;
    bmv[tid][1] = 4 * my;
  }

  // ------------------------ half- then quarter-pel refinement ---------------------------
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(s32);
  const uint8_t* ph = phase + (long)b * 16 * g.psz;
  // A group is 8 rows x 8 pixels of one block: 16 (8x8) + 16 (16x16) + 16 (32x32) groups.
  constexpr int ROWS = 8, N8 = 16, NC = 3 * N8;  // rows per group, groups per class / candidate
  auto grp_geom = [](int r, int& bi, int& row0, int& col0) {
    if (r < N8) {
      bi = r;
      row0 = 0;
      col0 = 0;
    } else if (r < 2 * N8) {
      const int q = (r - N8) % 4;
      bi = 16 + (r - N8) / 4;
      row0 = ROWS * (q >> 1);
      col0 = 8 * (q & 1);
    } else {
      const int q = r - 2 * N8;
      bi = 20;
      row0 = ROWS * (q >> 2);
      col0 = 8 * (q & 3);
    }
  };
  // the sub-pel argmin of the 21 blocks over the 8 neighbours at distance `step` (quarter pels)
  auto subpel_argmin = [&](int step) {
    if (tid < 21) {
      unsigned bestv = (unsigned)bcost[tid] << 4;
      for (int k = 0; k < 8; ++k) {
        int ox, oy;
        me_cand_offset(k, ox, oy);
        const int mx = bmv[tid][0] + ox * step, my = bmv[tid][1] + oy * step;
        const unsigned v =
            ((unsigned)(subsad[tid][k] + penmv[me_pen_index(mx - pmv[0], my - pmv[1])]) << 4) | (unsigned)(k + 1);
        bestv = v < bestv ? v : bestv;
      }
      const int kk = (int)(bestv & 15);
      bcost[tid] = (int)(bestv >> 4);
      if (kk) {
        int ox, oy;
        me_cand_offset(kk - 1, ox, oy);
        bmv[tid][0] += ox * step;
        bmv[tid][1] += oy * step;
      }
    }
  };
  // kSatd: per-cell tables [group r][position p] of one round (np positions: the centre and
  // the 8 neighbours in the half-pel round, the 8 neighbours in the quarter-pel round), the
  // blocks' running J between the rounds, and the round's cell descriptors
  int* const cellsatd = reinterpret_cast<int*>(win);
  int* const cellsad = cellsatd + NC * 9;
  int* const jbest = cellsad + NC * 9;
  int* const celld = jbest + 21;  // 2 ints per cell
  static_assert(4 * NC * 9 + 21 <= kMeMaxCand * kWinCand, "cell tables fit the window LDS");
  static_assert((NC * 9) % 4 == 0 && (NC * 8) % 4 == 0, "whole tiles");
  auto satd_tiles = [&](int step, auto NP) {
    constexpr int np = decltype(NP)::value;
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // One thread per cell decodes it once (every lane of a tile doing so was most of the
    // instructions of the round): d0 = x of the cell's left sample + 1024 | plane << 16 |
    // source word << 20 | source row << 23, d1 = y of its top row.
    for (int c = tid; c < NC * np; c += kMeThreads) {
      const int r = c / np, p = c - r * np;
      int bi, row0, col0;
      grp_geom(r, bi, row0, col0);
      int bx, by, l2b;
      me_blk_geom(bi, bx, by, l2b);
      const int k = p + 8 - np;  // neighbour index, -1 the centre (half-pel round only)
      int ox = 0, oy = 0;
      if (k >= 0) me_cand_offset(k, ox, oy);
      const int mx = bmv[bi][0] + ox * step, my = bmv[bi][1] + oy * step;
      const int gx0 = cx + bx + col0 + (mx >> 2);  // >= -range - 8 > -1024, < 2^16 - 1024 for any picture
      celld[2 * c] = (gx0 + 1024) | ((mx & 3) + 4 * (my & 3)) << 16 | ((bx + col0) >> 2) << 20 | (by + row0) << 23;
      celld[2 * c + 1] = cy + by + row0 + (my >> 2);
    }
    __syncthreads();
    const int i = lane & 15, kq = lane >> 4;
    h4 hb;  // Hbd[l & 15][4 (l >> 4) + e]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * kq + e;
      hb[e] = (i >> 3) == (k >> 3) ? (_Float16)me_h8(i & 7, k & 7) : (_Float16)0;
    }
    const int cin = ((lane >> 3) & 1) + 2 * (lane >> 5), cout = (lane >> 5) + 2 * ((lane >> 3) & 1);
    const int j = lane & 7, w = kq & 1;  // my row and dword of the cell I load
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    // bytes (b0, b1) or (b2, b3) of v as the f16 pair (1024 + b, 1024 + b'): 0x6400 | b
    auto f16_lo = [](uint32_t v) { return __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, v, 0x04010400u)); };
    auto f16_hi = [](uint32_t v) { return __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, v, 0x04030402u)); };
    auto pk = [](float a, float b) { return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b)); };
    // A wave takes its tiles T at a time (27 or 24 per wave): the T phase-plane dword pairs
    // are loaded first, then T independent MFMA chains.  The address clamps like the planes'
    // own border rule, which is exact for the rows; samples left or right of the padded plane
    // need the per-byte clamp: patched in between, which a wave away from the picture's sides
    // skips.
    constexpr int T = 3, nw = kMeThreads / 64, ntiles = NC * np / 4;
    static_assert(ntiles % (T * nw) == 0, "whole chunks");
    for (int t0 = wv; t0 < ntiles; t0 += T * nw) {  // wave-uniform
      uint32_t pv[T], sv[T];
      unsigned clampx = 0;  // tiles whose samples need the per-byte path
#pragma unroll
      for (int n = 0; n < T; ++n) {
        const int c = 4 * (t0 + n * nw) + cin, d0 = celld[2 * c], gy = celld[2 * c + 1] + j;
        const int gx = (d0 & 0xffff) - 1024 + 4 * w, a = gx & ~3;
        clampx |= (gx >= -8 && a <= g.W ? 0u : 1u) << n;
        const uint8_t* P = ph + (long)((d0 >> 16) & 15) * g.psz;
        const uint32_t* q =
            reinterpret_cast<const uint32_t*>(P + (long)(clip3(-8, g.H + 7, gy) + 8) * g.pw16 + clip3(-8, g.W, a) + 8);
        pv[n] = __builtin_amdgcn_alignbyte(q[1], q[0], (unsigned)(gx & 3));
        sv[n] = s32[src_word(((d0 >> 23) & 31) + j, ((d0 >> 20) & 7) + w)];
      }
      if (__builtin_amdgcn_ballot_w64(clampx != 0)) {
#pragma unroll
        for (int n = 0; n < T; ++n) {
          if (!((clampx >> n) & 1u)) continue;
          const int c = 4 * (t0 + n * nw) + cin, d0 = celld[2 * c], gy = celld[2 * c + 1] + j;
          const int gx = (d0 & 0xffff) - 1024 + 4 * w;
          const uint8_t* P = ph + (long)((d0 >> 16) & 15) * g.psz;
          uint32_t v = 0;
          for (int e = 0; e < 4; ++e) v |= (uint32_t)phase_at(P, g, gx + e, gy) << (8 * e);
          pv[n] = v;
        }
      }
#pragma unroll
      for (int n = 0; n < T; ++n) {
        // source - prediction in f16: (1024 + s) - (1024 + p), exact
        const h2 xl = f16_lo(sv[n]) - f16_lo(pv[n]), xh = f16_hi(sv[n]) - f16_hi(pv[n]);
        const h4 x = {xl[0], xl[1], xh[0], xh[1]};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 y = __builtin_amdgcn_mfma_f32_16x16x16f16(x, hb, zero, 0, 0, 0);
        const h4 yh = __builtin_bit_cast(h4, make_uint2(pk(y[0], y[1]), pk(y[2], y[3])));  // |y| <= 2040: exact
        const f32x4 z = __builtin_amdgcn_mfma_f32_16x16x16f16(hb, yh, zero, 0, 0, 0);
        // One reduction for both: a cell's sum of |Z| is at most sqrt(64 * sum Z^2) = sqrt(64 *
        // 64 * sum d^2) <= 512 * 255 < 2^17, its SAD at most 64 * 255 < 2^14.
        int v = (int)(__builtin_fabsf(z[0]) + __builtin_fabsf(z[1]) + __builtin_fabsf(z[2]) + __builtin_fabsf(z[3])) |
                (int)__builtin_amdgcn_sad_u8(sv[n], pv[n], 0u) << 17;
        v += dpp::mov<dpp::kQuadXor1>(v);  // the cell's 8 lanes x 2 rows; needs the full wave
        v += dpp::mov<dpp::kQuadXor2>(v);
        v += dpp::mov<dpp::kRowHalfMirror>(v);
        const auto r16 = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        const unsigned sum = r16[0] + r16[1];
        // my lane set loaded cell cin (the SAD bits) and holds the transform of cell cout
        if ((lane & 0x17) == 0) {
          const int t = t0 + n * nw;
          cellsad[4 * t + cin] = (int)(sum >> 17);
          cellsatd[4 * t + cout] = (int)(((sum & 0x1ffffu) + 2) >> 2);
        }
      }
    }
  };
  auto subpel_argmin_satd = [&](int step, int np) {
    if (tid < 21) {
      const int r0 = tid < 16 ? tid : (tid < 20 ? N8 + 4 * (tid - 16) : 2 * N8), ng = tid < 16 ? 1 : (tid < 20 ? 4 : 16);
      auto blk = [&](const int* tab, int p) {
        int s = 0;
        for (int q = 0; q < ng; ++q) s += tab[(r0 + q) * np + p];
        return s;
      };
      if (np == 9) jbest[tid] = me_subpel_j(blk(cellsatd, 0), penmv, bmv[tid][0], bmv[tid][1], pmv);
      unsigned key = me_subpel_key(jbest[tid], 0);
      for (int k = 0; k < 8; ++k) {
        int ox, oy;
        me_cand_offset(k, ox, oy);
        const int mx = bmv[tid][0] + ox * step, my = bmv[tid][1] + oy * step;
        const unsigned v = me_subpel_key(me_subpel_j(blk(cellsatd, k + np - 8), penmv, mx, my, pmv), k + 1);
        key = v < key ? v : key;
      }
      const int kk = (int)(key & 15);
      jbest[tid] = (int)(key >> 4);
      if (kk) {  // the reported cost stays in the SAD domain: SAD + MV rate at the new vector
        int ox, oy;
        me_cand_offset(kk - 1, ox, oy);
        bmv[tid][0] += ox * step;
        bmv[tid][1] += oy * step;
        bcost[tid] = blk(cellsad, kk - 1 + np - 8) + penmv[me_pen_index(bmv[tid][0] - pmv[0], bmv[tid][1] - pmv[1])];
      }
    }
  };
  __syncthreads();  // bmv of the integer search
  if constexpr (kSatd) {
    satd_tiles(2, std::integral_constant<int, 9>{});
  } else {
    // Half-pel round.  bmv is at integer pels, so the 8 neighbours lie on three phase planes
    // only: (+-2, 0) on plane fx = 2 at integer x - 1 and x, (0, +-2) on fy = 2 at rows y - 1
    // and y, the four diagonals on (2, 2) at both.  A wave takes one plane set, a lane one
    // group of it: it loads the set's patch once (8 or 9 rows of 3 aligned dwords, which
    // hold the 9 bytes from x - 1 at any alignment) and takes its 2 / 2 / 4 SADs from it --
    // 26 row loads per group instead of 64, in one pass.  sad[2 * lower + right].
    const int set = __builtin_amdgcn_readfirstlane(tid >> 6), r = tid & 63;  // H, V, HV
    if (set < 3 && r < NC) {
      const bool two_x = set != 1, two_y = set != 0;
      int bi, row0, col0;
      grp_geom(r, bi, row0, col0);
      int bx, by, l2b;
      me_blk_geom(bi, bx, by, l2b);
      const uint8_t* P = ph + (long)((two_x ? 2 : 0) + 4 * (two_y ? 2 : 0)) * g.psz;
      // patch origin = the position of the upper left candidate
      const int gx0 = cx + bx + col0 + (bmv[bi][0] >> 2) - (two_x ? 1 : 0);
      const int gy0 = cy + by + row0 + (bmv[bi][1] >> 2) - (two_y ? 1 : 0);
      const int sr0 = by + row0, sw0 = (bx + col0) >> 2;  // source row / word of row 0
      unsigned sad[4] = {0, 0, 0, 0};
      // straight-line per plane set (the flags are compile-time), so a lane's row loads are
      // all in flight together
      auto patch_sads = [&](auto TX, auto TY) {
        constexpr bool kTwoX = decltype(TX)::value, kTwoY = decltype(TY)::value;
        const int a = gx0 & ~3, sh = gx0 & 3;
        const uint8_t* rowp = P + (long)(gy0 + 8) * g.pw16 + a + 8;
        uint32_t p0 = 0, p1 = 0;  // the source row above
#pragma unroll
        for (int j = 0; j < ROWS + (kTwoY ? 1 : 0); ++j) {
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(rowp + (long)j * g.pw16);
          const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
          const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
          const uint32_t hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
          uint32_t lo1 = 0, hi1 = 0;  // one pixel to the right
          if (kTwoX) {
            lo1 = __builtin_amdgcn_alignbyte(hi, lo, 1);
            hi1 = __builtin_amdgcn_alignbyte(w2 >> (8 * sh), hi, 1);
          }
          uint32_t c0 = 0, c1 = 0;
          if (j < ROWS) {
            const int sw = src_word(sr0 + j, sw0);
            c0 = s32[sw];
            c1 = s32[sw + 1];
            sad[0] = __builtin_amdgcn_sad_u8(hi, c1, __builtin_amdgcn_sad_u8(lo, c0, sad[0]));
            if (kTwoX) sad[1] = __builtin_amdgcn_sad_u8(hi1, c1, __builtin_amdgcn_sad_u8(lo1, c0, sad[1]));
          }
          if (kTwoY && j > 0) {
            sad[2] = __builtin_amdgcn_sad_u8(hi, p1, __builtin_amdgcn_sad_u8(lo, p0, sad[2]));
            if (kTwoX) sad[3] = __builtin_amdgcn_sad_u8(hi1, p1, __builtin_amdgcn_sad_u8(lo1, p0, sad[3]));
          }
          p0 = c0;
          p1 = c1;
        }
      };
      if (gx0 >= -8 && gx0 + 11 <= g.W + 7 && gy0 >= -8 && gy0 + ROWS - 1 + (two_y ? 1 : 0) <= g.H + 7) {
        if (set == 0) {
          patch_sads(std::true_type{}, std::false_type{});
        } else if (set == 1) {
          patch_sads(std::false_type{}, std::true_type{});
        } else {
          patch_sads(std::true_type{}, std::true_type{});
        }
      } else {  // the patch touches the clamped border: per candidate, per pixel
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
          if (((c & 1) && !two_x) || ((c >> 1) && !two_y)) continue;
          unsigned t = 0;
          for (int j = 0; j < ROWS; ++j) {
            const int gy = clip3(-8, g.H + 7, gy0 + (c >> 1) + j);
            for (int i = 0; i < 8; ++i) {
              const int gx = clip3(-8, g.W + 7, gx0 + (c & 1) + i);
              t += tv_abs((int)sb[4 * src_word(sr0 + j, 0) + bx + col0 + i] - (int)P[(long)(gy + 8) * g.pw16 + gx + 8]);
            }
          }
          sad[c] = t;
        }
      }
      // group sums as in the quarter-pel round below; neighbour k of offset (ox, oy) is its
      // raster index in the 3 x 3 neighbourhood without the centre (me_cand_offset)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (((c & 1) && !two_x) || ((c >> 1) && !two_y)) continue;
        const int ox = two_x ? 2 * (c & 1) - 1 : 0, oy = two_y ? 2 * (c >> 1) - 1 : 0;
        const int idx = 3 * (oy + 1) + ox + 1, k = idx < 4 ? idx : idx - 1;
        const int s1 = (int)sad[c];
        int s4 = s1 + dpp::mov<dpp::kQuadXor1>(s1);
        s4 += dpp::mov<dpp::kQuadXor2>(s4);
        int s16 = s4 + dpp::mov<dpp::kRowHalfMirror>(s4);
        s16 += dpp::mov<dpp::kRowMirror>(s16);
        if (r < N8) {
          subsad[bi][k] = s1;
        } else if (r < 2 * N8) {
          if ((r - N8) % 4 == 0) subsad[bi][k] = s4;
        } else if (r == 2 * N8) {
          subsad[bi][k] = s16;
        }
      }
    }
  }
  __syncthreads();
  if constexpr (kSatd) subpel_argmin_satd(2, 9); else subpel_argmin(2);
  __syncthreads();  // bmv of the half-pel round
  // Quarter-pel round: the 8 neighbours lie on 8 different planes.  One wave per block class
  // (8x8, 16x16, 32x32 groups; the fourth wave goes straight to the barrier), a lane = one
  // group and one candidate pair (k = 2p, 2p + 1): it decodes its geometry and reads its 8
  // source rows once, then takes both candidates' SADs (per row 3 aligned dwords of the phase
  // plane, v_alignbyte, v_sad_u8) -- all 384 (group, candidate) cells in one pass.  A DPP row
  // is one pair's 16 groups, so the quad / row sums below are one block's.
  if constexpr (kSatd) {
    satd_tiles(1, std::integral_constant<int, 8>{});
  } else {
    constexpr int step = 1;
    const int cls = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
    if (cls < 3) {
      const int r = cls * N8 + (ln & 15), k0 = 2 * (ln >> 4);
      int bi, row0, col0;
      grp_geom(r, bi, row0, col0);
      int bx, by, l2b;
      me_blk_geom(bi, bx, by, l2b);
      const int sr0 = by + row0, sw0 = (bx + col0) >> 2;  // source row / word of row 0
      int oxa, oya, oxb, oyb;
      me_cand_offset(k0, oxa, oya);
      me_cand_offset(k0 + 1, oxb, oyb);
      const int mxa = bmv[bi][0] + oxa * step, mya = bmv[bi][1] + oya * step;
      const int mxb = bmv[bi][0] + oxb * step, myb = bmv[bi][1] + oyb * step;
      const uint8_t* Pa = ph + (long)((mxa & 3) + 4 * (mya & 3)) * g.psz;
      const uint8_t* Pb = ph + (long)((mxb & 3) + 4 * (myb & 3)) * g.psz;
      const int gxa = cx + bx + col0 + (mxa >> 2), gya = cy + by + row0 + (mya >> 2);
      const int gxb = cx + bx + col0 + (mxb >> 2), gyb = cy + by + row0 + (myb >> 2);
      auto inside = [&](int gx0, int gy0) { return gx0 >= -8 && gx0 + 11 <= g.W + 7 && gy0 >= -8 && gy0 + ROWS - 1 <= g.H + 7; };
      unsigned sada = 0, sadb = 0;
      if (inside(gxa, gya) && inside(gxb, gyb)) {
        const uint8_t* rpa = Pa + (long)(gya + 8) * g.pw16 + (gxa & ~3) + 8;
        const uint8_t* rpb = Pb + (long)(gyb + 8) * g.pw16 + (gxb & ~3) + 8;
        const int sha = gxa & 3, shb = gxb & 3;
        // 4 rows of both candidates (24 dwords) in flight at a time: all 48 do not fit 64 VGPRs
#pragma unroll 1
        for (int h = 0; h < ROWS; h += ROWS / 2) {
#pragma unroll
          for (int jj = 0; jj < ROWS / 2; ++jj) {
            const int j = h + jj;
            const uint32_t* wa = reinterpret_cast<const uint32_t*>(rpa + (long)j * g.pw16);
            const uint32_t* wb = reinterpret_cast<const uint32_t*>(rpb + (long)j * g.pw16);
            const uint32_t a0 = wa[0], a1 = wa[1], a2 = wa[2], b0 = wb[0], b1 = wb[1], b2 = wb[2];
            const int sw = src_word(sr0 + j, sw0);
            const uint32_t c0 = s32[sw], c1 = s32[sw + 1];
            sada = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a2, a1, sha), c1,
                                           __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a1, a0, sha), c0, sada));
            sadb = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(b2, b1, shb), c1,
                                           __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(b1, b0, shb), c0, sadb));
          }
        }
      } else {  // a candidate touches the clamped border: one at a time, per pixel where it does
#pragma unroll 1
        for (int c = 0; c < 2; ++c) {
          const uint8_t* P = c ? Pb : Pa;
          const int gx0 = c ? gxb : gxa, gy0 = c ? gyb : gya;
          unsigned sad = 0;
          if (inside(gx0, gy0)) {
            const int a = gx0 & ~3, sh = gx0 & 3;
            const uint8_t* rowp = P + (long)(gy0 + 8) * g.pw16 + a + 8;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
              const uint32_t* wp = reinterpret_cast<const uint32_t*>(rowp + (long)j * g.pw16);
              const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
              const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
              const uint32_t hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
              const int sw = src_word(sr0 + j, sw0);
              sad = __builtin_amdgcn_sad_u8(hi, s32[sw + 1], __builtin_amdgcn_sad_u8(lo, s32[sw], sad));
            }
          } else {
            for (int j = 0; j < ROWS; ++j) {
              const int gy = clip3(-8, g.H + 7, gy0 + j);
              for (int i = 0; i < 8; ++i) {
                const int gx = clip3(-8, g.W + 7, gx0 + i);
                sad += tv_abs((int)sb[4 * src_word(sr0 + j, 0) + bx + col0 + i] - (int)P[(long)(gy + 8) * g.pw16 + gx + 8]);
              }
            }
          }
          if (c) sadb = sad; else sada = sad;
        }
      }
      // group sums on the VALU (all 64 lanes of the wave are here): a lane = an 8x8 block, an
      // aligned group of 4 lanes = a 16x16 block, of 16 = the 32x32 block -- every (block,
      // candidate) cell is written exactly once, by a plain store
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int s1 = (int)(c ? sadb : sada), k = k0 + c;
        int s4 = s1 + dpp::mov<dpp::kQuadXor1>(s1);
        s4 += dpp::mov<dpp::kQuadXor2>(s4);
        int s16 = s4 + dpp::mov<dpp::kRowHalfMirror>(s4);
        s16 += dpp::mov<dpp::kRowMirror>(s16);
        if (cls == 0) {
          subsad[bi][k] = s1;
        } else if (cls == 1) {
          if ((ln & 3) == 0) subsad[bi][k] = s4;
        } else if ((ln & 15) == 0) {
          subsad[bi][k] = s16;
        }
      }
    }
  }
  __syncthreads();
  if constexpr (kSatd) subpel_argmin_satd(1, 8); else subpel_argmin(1);
  __syncthreads();

  // B picture: hand this list's 21 block results to k_bi_decide
  if (bout) {
    if (tid < 21) {
      CtbMeOut& o = bout[(long)b * g.wc * g.hc + ctu];
      o.cost[tid] = bcost[tid];
      o.mv[tid][0] = bmv[tid][0];
      o.mv[tid][1] = bmv[tid][1];
      o.pen[tid] = penmv[me_pen_index(bmv[tid][0] - pmv[0], bmv[tid][1] - pmv[1])];
    }
    return;
  }
  // ------------------------------- CU split decision ------------------------------------
  // the rule of tv::split_ctb (tv/me_model.h), lane-parallel:
  // one lane per 8x8 unit k (raster): every lane forms the same quadrant / CTB sums from the
  // 21 block costs (the same order of additions as the serial form), then writes its unit
  if (tid < 16) {
    const int ps = pen.split_inter, k = tid, ux = k & 3, uy = k >> 2;
    int sum16 = 0, qsplit = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int sum8 = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) sum8 += bcost[me_blk8_of(q, r)] + ps;
      const bool split = sum8 < bcost[16 + q] + ps;
      sum16 += split ? sum8 : bcost[16 + q] + ps;
      qsplit |= split ? 1 << q : 0;
    }
    const bool whole = bcost[20] + ps <= sum16;
    const int q = (uy >> 1) * 2 + (ux >> 1), r = (uy & 1) * 2 + (ux & 1);
    const bool split = (qsplit >> q) & 1;
    const int sbi = whole ? 20 : (split ? me_blk8_of(q, r) : 16 + q);
    const long u = b * g.usz + (long)((cy >> 3) + uy) * g.w8 + (cx >> 3) + ux;
    dec.cu_log2[u] = whole ? 5 : (split ? 3 : 4);
    dec.mv[2 * u] = (int16_t)bmv[sbi][0];
    dec.mv[2 * u + 1] = (int16_t)bmv[sbi][1];
    dec.intra[u] = 0;
    dec.ipm[u] = 1;
    if (pi.qcost && k < 4) {  // intra-in-P: quadrants past the gate go on k_pintra_analysis' list
      const long qi = ((long)b * g.wc * g.hc + ctu) * 4 + k;
      pi.qcost[qi] = bcost[16 + k];
      pi.cand[qi] = 0;
      if (bcost[16 + k] > kPIntraGate * 256) pi.gate[atomicAdd(&pi.count[0], 1)] = (int)qi;
    }
  }
}

// ---------------------------------------------------------------------------------------
// B picture pass A, second half (golden: tv::analyze_inter_b): the SAD of the 8-bit average
// of both lists' predictions for all 21 ME blocks (one wave covers one 8x8 block or a 64-
// sample quarter of a larger one: a wave sum, one LDS atomic), then per block the cheapest of
// list 0, list 1 and bi (ties keep the earlier), then the bottom-up CU split.
// ---------------------------------------------------------------------------------------
// 4 phase-plane samples at (x .. x+3, y), any alignment: two dword loads + v_alignbyte
// inside the padded plane, per-byte clamped loads at the border
__device__ __forceinline__ uint32_t phase4(const uint8_t* P, const Geo& g, int x, int y) {
  const int a = x & ~3;
  if (x >= -8 && a + 7 <= g.W + 7 && y >= -8 && y <= g.H + 7) {
    const uint8_t* row = P + (long)(y + 8) * g.pw16 + a + 8;
    const uint32_t w0 = *reinterpret_cast<const uint32_t*>(row), w1 = *reinterpret_cast<const uint32_t*>(row + 4);
    return __builtin_amdgcn_alignbyte(w1, w0, x & 3);
  }
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) v |= (uint32_t)phase_at(P, g, x + k, y) << (8 * k);
  return v;
}

__global__ void __launch_bounds__(256) k_bi_decide(FrameSet src, const uint8_t* phase0, const uint8_t* phase1,
                                                    const CtbMeOut* me0, const CtbMeOut* me1, DecisionSet dec, Geo g,
                                                    const RcTables* rc) {
  const int tid = threadIdx.x;
  int ctu, b;
  xcd_ctb(ctu, b);
  const long o = (long)b * g.wc * g.hc + ctu;
  const CtbMeOut& A = me0[o];
  const CtbMeOut& Bm = me1[o];
  const int cx = (ctu % g.wc) * 32, cy = (ctu / g.wc) * 32;
  __shared__ uint32_t s32[256];  // the source CTB, 8 words per row
  __shared__ int sad[21];
  __shared__ int mvs[2][21][2];
  const uint8_t* S = src.plane(0, b, g);
  s32[tid] = *reinterpret_cast<const uint32_t*>(S + (long)(cy + (tid >> 3)) * g.W + cx + 4 * (tid & 7));
  if (tid < 21) sad[tid] = 0;
  if (tid < 84) {
    const int l = tid / 42, r = tid - l * 42;
    mvs[l][r >> 1][r & 1] = (l ? Bm : A).mv[r >> 1][r & 1];
  }
  __syncthreads();
  const uint8_t* p0b = phase0 + (long)b * 16 * g.psz;
  const uint8_t* p1b = phase1 + (long)b * 16 * g.psz;
  // item = 4 horizontally adjacent samples of one block: 256 for the 16 8x8 blocks, 256 for
  // the 4 16x16, 256 for the 32x32; the 8-bit average of both predictions is one
  // (a | c) - ((a ^ c) >> 1) per dword and its SAD one v_sad_u8
  for (int item = tid; item < 768; item += 256) {
    int bi, x, y;
    if (item < 256) {
      bi = item >> 4;
      const int r = item & 15;
      x = (bi & 3) * 8 + (r & 1) * 4;
      y = (bi >> 2) * 8 + (r >> 1);
    } else if (item < 512) {
      const int j = item - 256;
      bi = 16 + (j >> 6);
      const int r = j & 63;
      x = ((bi - 16) & 1) * 16 + (r & 3) * 4;
      y = ((bi - 16) >> 1) * 16 + (r >> 2);
    } else {
      const int j = item - 512;
      bi = 20;
      x = (j & 7) * 4;
      y = j >> 3;
    }
    const int m0x = mvs[0][bi][0], m0y = mvs[0][bi][1], m1x = mvs[1][bi][0], m1y = mvs[1][bi][1];
    const uint32_t a = phase4(p0b + (long)((m0x & 3) + 4 * (m0y & 3)) * g.psz, g, cx + x + (m0x >> 2), cy + y + (m0y >> 2));
    const uint32_t c = phase4(p1b + (long)((m1x & 3) + 4 * (m1y & 3)) * g.psz, g, cx + x + (m1x >> 2), cy + y + (m1y >> 2));
    const uint32_t avg = (a | c) - (((a ^ c) >> 1) & 0x7f7f7f7fu);
    atomicAdd(&sad[bi], (int)__builtin_amdgcn_sad_u8(avg, s32[y * 8 + (x >> 2)], 0u));
  }
  __syncthreads();
  // per block: the cheapest of list 0, list 1 and bi (ties keep the earlier); then the
  // quadrant splits, the whole-CTB choice and each unit's motion, one lane each
  __shared__ int cost[21], dirb[21], qsum[4], qsplit[4], whole;
  const Penalties& pen = rc->pen[dec.qp[b]];
  const int ps = pen.split_inter;
  if (tid < 21) {
    const int cb = sad[tid] + A.pen[tid] + Bm.pen[tid];
    int c = A.cost[tid], d = 1;
    if (Bm.cost[tid] < c) {
      c = Bm.cost[tid];
      d = 2;
    }
    if (cb < c) {
      c = cb;
      d = 3;
    }
    cost[tid] = c;
    dirb[tid] = d;
  }
  __syncthreads();
  if (tid < 4) {  // the rule of tv::split_ctb (tv/me_model.h), a lane per quadrant, then per unit
    int sum8 = 0;
    for (int r = 0; r < 4; ++r) sum8 += cost[me_blk8_of(tid, r)] + ps;
    const bool split = sum8 < cost[16 + tid] + ps;
    qsplit[tid] = split;
    qsum[tid] = split ? sum8 : cost[16 + tid] + ps;
  }
  __syncthreads();
  if (tid == 0) whole = cost[20] + ps <= qsum[0] + qsum[1] + qsum[2] + qsum[3];
  __syncthreads();
  if (tid < 16) {
    const int k = tid, q = ((k >> 3) << 1) | ((k >> 1) & 1), r = ((k >> 2) & 1) * 2 + (k & 1);
    const int s = whole ? 20 : (qsplit[q] ? me_blk8_of(q, r) : 16 + q), d = dirb[s];
    const long u = b * g.usz + (long)((cy >> 3) + (k >> 2)) * g.w8 + (cx >> 3) + (k & 3);
    dec.cu_log2[u] = (uint8_t)(whole ? 5 : (qsplit[q] ? 3 : 4));
    dec.dir[u] = (uint8_t)d;
    dec.mv[2 * u] = (int16_t)(d & 1 ? mvs[0][s][0] : 0);
    dec.mv[2 * u + 1] = (int16_t)(d & 1 ? mvs[0][s][1] : 0);
    dec.mv1[2 * u] = (int16_t)(d & 2 ? mvs[1][s][0] : 0);
    dec.mv1[2 * u + 1] = (int16_t)(d & 2 ? mvs[1][s][1] : 0);
    dec.intra[u] = 0;
    dec.ipm[u] = 1;
  }
}

// ---------------------------------------------------------------------------------------
// P-frame pass B on matrix cores: every TB of the CTB is coded by 16x16 MFMA tiles.
//
// A P frame has only inter CUs, so all predictions and residuals of the CTB exist up front
// and every transform stage is a batch of small GEMMs.  TBs smaller than 16 are packed
// block-diagonally into one v_mfma 16x16x16 tile: a 16x16 luma quadrant of four 8x8 TBs is
// diag(T8, T8) * R (stage 1) / A * diag(T8, T8)^T (stage 2) — the shared DCT matrix makes the
// four products one MFMA; the Cb and Cr 8x8 regions of a quadrant (one 8x8 TB each, or four
// 4x4 TBs each) form the two diagonal blocks of one tile, diag(Rcb, Rcr).  So a CTB is 8
// tiles per stage (4 luma quadrants + 4 chroma pairs; a single 32x32 CU: 4 K=32 luma tiles +
// 2 chroma tiles) with no VALU dot products at all.  Every operand is an integer of <= 9
// bits (8-bit split halves where needed) so every product and partial sum is exact in f32:
// bit-identical to tv::forward_transform / tv::inverse_transform (see tb_coder.h).
//
// Operands are MFMA fragments (tb_coder.h frag_tile*), not per-element gathers.  The DCT side
// of every product -- T32, its transpose and the block-diagonal composites -- is a constant:
// tv/tb_frag.h builds it at compile time as f16 in lane order and the workgroup copies the
// 7 KB into LDS, one 16- / 8-byte read per lane and tile.  The intermediate of each
// direction (stage 1 -> 2, stage 3 -> 4) is written by its producer already split into f16
// hi / lo images, row-major, which is the K order of the consuming A operand.  Only the B
// operands of stages 1 and 3 (residual, dequantised levels: K runs down a column of the
// row-major int16 planes the entropy path reads) are still converted per element.  A lane's
// four outputs of a tile are consecutive columns of one row (tb_coder.h frag_tile): one
// 8-byte store into the f16 images or the level plane, one dword of reconstruction.  TB size,
// TB id and the quantiser parameters are uniform per tile and computed once per tile; a
// lane's four levels belong to one TB and update its statistics with one pair of atomics.
// ---------------------------------------------------------------------------------------
constexpr int kTmpYP = 40, kTmpCP = 16;  // f16 row pitches (luma padded by 16 bytes: rows stay 16-byte aligned)
__constant__ TbFragTables kTbFragDev = make_tb_frag();

struct PReconLds {
  alignas(16) TbFragTables F;  // the constant operands as f16 fragments (tv/tb_frag.h)
  // (between stage 2 and stage 3 both are dead: the rd_quant pass keeps its per-coefficient level drops
  // in tmpYh and its per-group costs in tmpYl)
  alignas(16) _Float16 tmpYh[32 * kTmpYP], tmpYl[32 * kTmpYP];        // stage 1 / stage 3 outputs (luma), v = 256 hi + lo
  alignas(16) _Float16 tmpCh[2][16 * kTmpCP], tmpCl[2][16 * kTmpCP];  // the same for Cb, Cr
  int16_t resY[32 * 32];      // residual, later levels (luma)
  int16_t resC[2][16 * 16];   // residual, later levels (chroma)
  uint8_t predY[32 * 32];
  uint8_t predC[2][16 * 16];
  int mv[16][2];              // per 8x8 unit (raster within the CTB)
  int mv1[16][2];             // B pictures: list-1 vectors and directions
  int dir[16];
  union {
    struct {
      uint8_t bwin[4][15 * 16];   // per wave: 15x15 luma reference window of a bi unit
      int16_t bh[4][15 * 8];      // per wave: horizontal filter pass (15 rows x 8)
    };
    // k_inter_recon<true, ..> (sign data hiding) and <.., true> (rd_quant), written by stage 2 when the prediction buffers
    // above are dead: per coefficient sdh_delta + 64 as a byte (inter rounding: -64 <= d < 192;
    // luma 32x32, Cb 16x16, Cr 16x16), and per lane's four coefficients of a row the bits
    // "coefficient r < 0" (a zero level takes its sign from there)
    struct {
      alignas(4) uint8_t sdh_d[32 * 32 + 2 * 16 * 16];
      uint8_t sdh_neg[(32 * 32 + 2 * 16 * 16) / 4];
    };
  };
  int nz[48], sa[48], dc[48];  // per-TB statistics: luma 0..15, Cb 16..31, Cr 32..47
  int qtype[4];               // luma quadrant: 0 part of a 32x32 CU, 1 16x16 CU, 2 four 8x8 CUs
  int tzero[8];               // stage-3/4 tile t has no surviving level: reconstruction = prediction
  int qsad[4], split;         // RQT: luma residual SAD per quadrant of a 32x32 CU, the decision
  int qsplit[4];              // RQT of the 16x16 CU in quadrant q (four 8x8 TBs)
  int qintra[4];              // quadrant q is an intra CU of a P picture (k_pintra_recon codes it)
  uint32_t ctap[8];           // chroma filter of fraction f as 4 signed bytes
  int cgmax[48];              // RDOQ-lite: highest scan key of a TB's groups that are kept
  int multi;                  // some TB has >= 2 non-zero levels (else RDOQ-lite changes nothing)
};

// block size (log2) of the TB owning luma sample (x, y) / chroma sample (x, y) of the CTB
__device__ __forceinline__ int pr_l2_luma(const PReconLds& L, int x, int y) {
  const int t = L.qtype[(y >> 4) * 2 + (x >> 4)];
  return t == 0 ? 5 : (t == 1 ? 4 : 3);
}
__device__ __forceinline__ int pr_tb_luma(const PReconLds& L, int x, int y) {
  const int q = (y >> 4) * 2 + (x >> 4), t = L.qtype[q];
  return t == 0 ? 0 : (t == 1 ? 4 * q : 4 * q + ((y >> 3) & 1) * 2 + ((x >> 3) & 1));
}
__device__ __forceinline__ int pr_tb_chroma(const PReconLds& L, int p, int x, int y) {
  const int q = (y >> 3) * 2 + (x >> 3), t = L.qtype[q];
  const int base = 16 + 16 * p;
  return t == 0 ? base : (t == 1 ? base + 4 * q : base + 4 * q + ((y >> 2) & 1) * 2 + ((x >> 2) & 1));
}
static_assert(sizeof(PReconLds) == 22096, "k_inter_recon: 7 workgroups of PReconLds per CU");
// a TB whose only non-zero level is a lone +-1 outside DC is dropped (tv code_tb, inter)
__device__ __forceinline__ bool pr_zeroed(const PReconLds& L, int id) {
  return L.nz[id] == 0 || (L.nz[id] == 1 && L.sa[id] == 1 && L.dc[id] == 0);
}

// 7 waves per SIMD: 72 VGPRs and no scratch (8 would need 64 and spills), and 7 workgroups
// of PReconLds (22096 B) are what fits the CU's 160 KiB of LDS.
// kSdh (SeqConfig::sign_hiding, tv/sdh.h): stage 2 also keeps every coefficient's distance
// from its level, and a pass after RDOQ-lite adjusts one level of each coefficient group whose
// parity does not carry its hidden sign.  <false> compiles none of it.
// kRdq (SeqConfig::rd_quant, tv/rdq.h): stage 2 keeps the distances as for kSdh, and a pass in
// the place of RDOQ-lite chooses the levels by rate-distortion cost, one thread per coefficient
// group.  <.., false> compiles none of it.
template <bool kSdh, bool kRdq>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) k_inter_recon(FrameSet src, FrameSet ref, const uint8_t* phase,
                                                     FrameSet rec, DecisionSet dec, Geo g,
                                                     FrameSet ref1, const uint8_t* phase1) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rdoq = g.rdoq;  // RDOQ-lite mode (tv code_tb), 0 off
  int ctu, b;
  xcd_ctb(ctu, b);
  const int qp = dec.qp[b];
  const int cx = (ctu % g.wc) * 32, cy = (ctu / g.wc) * 32;
  const long ub = b * g.usz;
  const int qpc = chroma_qp(qp, 0), Wc = g.W >> 1, Hc = g.H >> 1;
  const long W = g.W;  // the luma pitch, widened once up here (stays scalar: no spill at 72 VGPRs)
  __shared__ PReconLds L;
  for (int i = tid; i < (int)(sizeof(TbFragTables) / 16); i += 256)
    reinterpret_cast<uint4*>(&L.F)[i] = reinterpret_cast<const uint4*>(&kTbFragDev)[i];
  if (tid < 16) {
    const long u = ub + (long)((cy >> 3) + (tid >> 2)) * g.w8 + (cx >> 3) + (tid & 3);
    L.mv[tid][0] = dec.mv[2 * u];
    L.mv[tid][1] = dec.mv[2 * u + 1];
    L.dir[tid] = dec.dir ? dec.dir[u] : 1;
    L.mv1[tid][0] = dec.mv1 ? dec.mv1[2 * u] : 0;
    L.mv1[tid][1] = dec.mv1 ? dec.mv1[2 * u + 1] : 0;
  }
  if (tid < 48) {
    L.nz[tid] = L.sa[tid] = L.dc[tid] = 0;
    L.cgmax[tid] = -1;
  }
  if (tid < 8)
    L.ctap[tid] = (uint32_t)(uint8_t)kChromaFilter[tid][0] | (uint32_t)(uint8_t)kChromaFilter[tid][1] << 8 |
                  (uint32_t)(uint8_t)kChromaFilter[tid][2] << 16 | (uint32_t)(uint8_t)kChromaFilter[tid][3] << 24;
  if (tid == 0) L.split = 0, L.multi = 0;
  if (tid < 4) {
    L.qsplit[tid] = 0;
    L.qintra[tid] = dec.intra[ub + (long)((cy >> 3) + (tid >> 1) * 2) * g.w8 + (cx >> 3) + (tid & 1) * 2];
  }
  if (tid < 4) {
    const int l2 = dec.cu_log2[ub + (long)((cy >> 3) + (tid >> 1) * 2) * g.w8 + (cx >> 3) + (tid & 1) * 2];
    L.qtype[tid] = l2 == 5 ? 0 : (l2 == 4 ? 1 : 2);
  }
  __syncthreads();
  // ---- prediction + residual of all three planes
  {
    const uint8_t* S = src.plane(0, b, g);
    const uint8_t* ph = phase + (long)b * 16 * g.psz;
    const uint8_t* ph1 = phase1 ? phase1 + (long)b * 16 * g.psz : nullptr;
    {  // uni-prediction: the reference's phase plane holds the final samples; one item = 4
       // samples of a row of one 8x8 unit (a dword of prediction, two int16 residual pairs)
      const int x = (tid & 7) * 4, y = tid >> 3, un = (y >> 3) * 4 + (x >> 3);
      const int d = L.dir[un];
      if (d != 3) {  // bi units: below, one wave per unit
        const int mvx = d == 1 ? L.mv[un][0] : L.mv1[un][0], mvy = d == 1 ? L.mv[un][1] : L.mv1[un][1];
        const uint8_t* P = (d == 1 ? ph : ph1) + (long)((mvx & 3) + 4 * (mvy & 3)) * g.psz;
        const int px = cx + x + (mvx >> 2), py = clip3(-8, g.H + 7, cy + y + (mvy >> 2));
        const uint8_t* row = P + (long)(py + 8) * g.pw16;
        const int bx = px + 8, a4 = bx & ~3;
        uint32_t pw;
        if (bx >= 0 && a4 + 7 < g.pw16) {  // in the padded row: two aligned dwords
          const uint32_t d0 = *reinterpret_cast<const uint32_t*>(row + a4);
          const uint32_t d1 = *reinterpret_cast<const uint32_t*>(row + a4 + 4);
          pw = __builtin_amdgcn_alignbyte(d1, d0, bx & 3);
        } else {
          pw = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) pw |= (uint32_t)phase_at(P, g, px + k, cy + y + (mvy >> 2)) << (8 * k);
        }
        const uint32_t sw = *reinterpret_cast<const uint32_t*>(S + (cy + y) * W + cx + x);
        *reinterpret_cast<uint32_t*>(&L.predY[y * 32 + x]) = pw;
        *reinterpret_cast<uint2*>(&L.resY[y * 32 + x]) = bytes_minus(sw, pw);
      }
    }
    // bi-predicted 8x8 units (8.5.3.3.4.2): per list the 15x15 reference window is staged
    // in this wave's LDS, the 8-tap horizontal pass gives 15 x 8 intermediates, the vertical
    // pass one 14-bit sample per lane; then (p0 + p1 + 64) >> 7.  Wave-local: no barrier.
    for (int un = wave; un < 16; un += 4) {
      if (L.dir[un] != 3) continue;  // wave-uniform
      const int x0 = cx + (un & 3) * 8, y0 = cy + (un >> 2) * 8;
      int pl[2];
      for (int l = 0; l < 2; ++l) {
        const int mvx = l ? L.mv1[un][0] : L.mv[un][0], mvy = l ? L.mv1[un][1] : L.mv[un][1];
        const int fx = mvx & 3, fy = mvy & 3, bx = x0 + (mvx >> 2) - 3, by = y0 + (mvy >> 2) - 3;
        const uint8_t* R = (l ? ref1 : ref).plane(0, b, g);
        uint8_t* win = L.bwin[wave];
        for (int k = lane; k < 225; k += 64) {
          const int r = k / 15, c = k - r * 15;
          win[r * 16 + c] = R[(long)clip3(0, g.H - 1, by + r) * g.W + clip3(0, g.W - 1, bx + c)];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int16_t* hb = L.bh[wave];
        for (int k = lane; k < 120; k += 64) {
          const int r = k >> 3, c = k & 7;
          int h;
          if (fx) {
            h = 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) h += kLumaFilter[fx][t] * win[r * 16 + c + t];
          } else {
            h = win[r * 16 + c + 3] << 6;
          }
          hb[k] = (int16_t)h;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int xo = lane & 7, yo = lane >> 3;
        if (fy) {
          int v = 0;
#pragma unroll
          for (int t = 0; t < 8; ++t) v += kLumaFilter[fy][t] * hb[(yo + t) * 8 + xo];
          pl[l] = v >> 6;
        } else {
          pl[l] = hb[(yo + 3) * 8 + xo];
        }
        __builtin_amdgcn_wave_barrier();  // the window / pass buffers are reused by list 1
      }
      const int x = (un & 3) * 8 + (lane & 7), y = (un >> 2) * 8 + (lane >> 3);
      const int p = bipred_sample(pl[0], pl[1]);
      L.predY[y * 32 + x] = (uint8_t)p;
      L.resY[y * 32 + x] = (int16_t)((int)S[(cy + y) * W + cx + x] - p);
    }
    // chroma: one item = 4 samples of a row of one 4x4 unit (128 items), the separable 4-tap
    // filter on packed bytes: per reference row the 7 samples are two dwords, each output a
    // v_dot4 of a v_alignbyte window against the biased taps (samples ^ 0x80 as int8: the
    // bias is 128 * 64 = 8192), then the vertical taps.  The 0-fraction filter {0, 64, 0, 0}
    // makes the one 2-D formula exact for every fraction (8.5.3.3.3.2, as mc_chroma_inter).
    if (tid < 128) {
      const int pl = tid >> 6, y = (tid >> 2) & 15, x = (tid & 3) * 4, un = (y >> 2) * 4 + (x >> 2);
      const int d = L.dir[un];
      const int gx = (cx >> 1) + x, gy = (cy >> 1) + y;
      int prev[4] = {0, 0, 0, 0};  // bi: the list-0 intermediates
      uint32_t pw = 0;
#pragma unroll 1
      for (int l = 0; l < 2; ++l) {
        if (!(d & (1 << l))) continue;
        const int mvx = l ? L.mv1[un][0] : L.mv[un][0], mvy = l ? L.mv1[un][1] : L.mv[un][1];
        const uint8_t* Rf = (l ? ref1 : ref).plane(1 + pl, b, g);
        const uint32_t tx = L.ctap[mvx & 7], ty = L.ctap[mvy & 7];
        const int x0 = gx + (mvx >> 3) - 1, y0 = gy + (mvy >> 3) - 1;
        int acc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* row = Rf + (long)clip3(0, Hc - 1, y0 + j) * Wc;
          const int a4 = x0 & ~3;
          uint32_t w0, w1;
          if (x0 >= 0 && a4 + 11 < Wc) {
            const uint32_t d0 = *reinterpret_cast<const uint32_t*>(row + a4);
            const uint32_t d1 = *reinterpret_cast<const uint32_t*>(row + a4 + 4);
            const uint32_t d2 = *reinterpret_cast<const uint32_t*>(row + a4 + 8);
            w0 = __builtin_amdgcn_alignbyte(d1, d0, x0 & 3);
            w1 = __builtin_amdgcn_alignbyte(d2, d1, x0 & 3);
          } else {
            w0 = w1 = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              w0 |= (uint32_t)row[clip3(0, Wc - 1, x0 + k)] << (8 * k);
              w1 |= (uint32_t)row[clip3(0, Wc - 1, x0 + 4 + k)] << (8 * k);
            }
          }
          w0 ^= 0x80808080u;
          w1 ^= 0x80808080u;
          const int fyj = (int)(int8_t)(ty >> (8 * j));
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t win = k == 0 ? w0 : __builtin_amdgcn_alignbyte(w1, w0, k);
            acc[k] += fyj * __builtin_amdgcn_sdot4((int)win, (int)tx, 8192, false);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int v = acc[k] >> 6;  // the 14-bit intermediate
          if (d == 3 && l == 0) {
            prev[k] = v;
          } else {
            const int p = d == 3 ? bipred_sample(prev[k], v) : clip_pixel((v + 32) >> 6);
            pw |= (uint32_t)p << (8 * k);
          }
        }
      }
      const uint32_t sw = *reinterpret_cast<const uint32_t*>(src.plane(1 + pl, b, g) + (long)gy * Wc + gx);
      *reinterpret_cast<uint32_t*>(&L.predC[pl][y * 16 + x]) = pw;
      *reinterpret_cast<uint2*>(&L.resC[pl][y * 16 + x]) = bytes_minus(sw, pw);
    }
  }
  __syncthreads();
  if (dec.tu) {  // RQT (P pictures): a 32x32 CU may code four 16x16 TBs (hevc_defs.h rqt_split)
    if (L.qtype[0] == 0) {  // workgroup-uniform
      const int qx = (wave & 1) * 16, qy = (wave >> 1) * 16;
      int d = 0;
      for (int k = lane; k < 256; k += 64) d += tv_abs((int)L.resY[(qy + (k >> 4)) * 32 + qx + (k & 15)]);
      d = wave_sum(d);
      if (lane == 0) L.qsad[wave] = d;
      __syncthreads();
      if (tid == 0 && rqt_split(L.qsad)) {
        L.split = 1;
        L.qtype[0] = L.qtype[1] = L.qtype[2] = L.qtype[3] = 1;  // the 16x16-CU tile layout
      }
      __syncthreads();
    } else if (kRqtMinLog2 <= 4) {  // 16x16 CUs: quadrant `wave`'s four 8x8 SADs, four 8x8 TBs on a split
      if (L.qtype[wave] == 1 && !L.qintra[wave]) {  // wave-uniform
        const int qx = (wave & 1) * 16, qy = (wave >> 1) * 16;
        int s4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          s4[k] = wave_sum(tv_abs((int)L.resY[(qy + (k >> 1) * 8 + (lane >> 3)) * 32 + qx + (k & 1) * 8 + (lane & 7)]));
        if (lane == 0 && rqt_split(s4, 64)) L.qsplit[wave] = 1;
      }
      __syncthreads();
      if (tid < 4 && L.qsplit[tid]) L.qtype[tid] = 2;  // the 8x8-CU tile layout
      __syncthreads();
    }
    if (tid < 16)
      dec.tu[ub + (long)((cy >> 3) + (tid >> 2)) * g.w8 + (cx >> 3) + (tid & 3)] =
          (uint8_t)(L.split | L.qsplit[((tid >> 3) << 1) | ((tid >> 1) & 1)]);
  }
  const bool whole = L.qtype[0] == 0;
  const int ntiles = whole ? 6 : 8;
  // tile t: luma (whole: 32x32 tile ti,tj = t>>1, t&1; else quadrant t) for t < 4, chroma
  // (whole: plane t-4 as one 16x16 TB; else the Cb|Cr pair of quadrant t-4) for t >= 4.
  // ---------------------------------------------------------------- stage 1: T * R
  // A lane's place in a fragment: operand row / column fi, K-run kq (tv/tb_frag.h); its four
  // outputs are columns 4 * kq + r of row fi (tb_coder.h frag_tile).  The Cb|Cr pair tile is
  // block-diagonal in the data too: lane (fi, kq) of its data operand is inside a block iff
  // pin, plane pp as a B operand, fi >> 3 as an A operand -- and its outputs are inside one
  // iff pin, plane fi >> 3, row fi & 7, columns 4 * (kq & 1) + r.
  const int fi = lane & 15, kq = lane >> 4;
  const bool pin = (fi >> 3) == (kq >> 1);
  const int pp = kq >> 1;
  auto T32 = [&](int o, int tile) { return frag8(reinterpret_cast<const _Float16*>(&L.F.t32[o][16 * tile + fi][8 * kq])); };
  auto C16 = [&](int l2, int o) { return frag4(reinterpret_cast<const _Float16*>(&L.F.c16[4 - l2][o][fi][4 * kq])); };
  const h4 zero4 = {0, 0, 0, 0};
  // a lane's four outputs (row y, columns x .. x + 3) into the split f16 images of a stage output
  auto put_y = [&](int y, int x, const int* v) { frag_store_split(&L.tmpYh[y * kTmpYP + x], &L.tmpYl[y * kTmpYP + x], v); };
  auto put_c = [&](int pl, int y, int x, const int* v) {
    frag_store_split(&L.tmpCh[pl][y * kTmpCP + x], &L.tmpCl[pl][y * kTmpCP + x], v);
  };
  for (int t = wave; t < ntiles; t += 4) {
    int o[4];
    if (t < 4) {
      int sh1;
      if (whole) {
        h8 b;
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = (_Float16)L.resY[(8 * kq + e) * 32 + 16 * (t & 1) + fi];
        frag_tile(T32(0, t >> 1), b, o);
        sh1 = 4;
      } else {
        const int ox = (t & 1) * 16, oy = (t >> 1) * 16, l2 = L.qtype[t] == 1 ? 4 : 3;
        h4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (_Float16)L.resY[(oy + 4 * kq + e) * 32 + ox + fi];
        frag_tile(C16(l2, 0), b, o);
        sh1 = l2 - 1;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (o[r] + (1 << (sh1 - 1))) >> sh1;
      put_y((t >> 1) * 16 + fi, (t & 1) * 16 + kq * 4, o);
    } else if (whole) {
      const int pl = t - 4;
      h4 b;
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = (_Float16)L.resC[pl][(4 * kq + e) * 16 + fi];
      frag_tile(C16(4, 0), b, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (o[r] + 4) >> 3;  // 16-point: sh1 = 3
      put_c(pl, fi, kq * 4, o);
    } else {
      const int q = t - 4, ox = (q & 1) * 8, oy = (q >> 1) * 8, l2 = L.qtype[q] == 1 ? 3 : 2;
      h4 b;
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = (_Float16)L.resC[pp][(oy + 4 * (kq & 1) + e) * 16 + ox + (fi & 7)];
      frag_tile(C16(l2, 0), pin ? b : zero4, o);
      const int sh1 = l2 - 1;
      if (pin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (o[r] + (1 << (sh1 - 1))) >> sh1;
        put_c(fi >> 3, oy + (fi & 7), ox + 4 * (kq & 1), o);
      }
    }
  }
  __syncthreads();
  // ------------------------------------------------- stage 2: A * T^T + quantisation
  // One tile = TBs of one size: shift and quantiser parameters are computed once per tile
  // (wave-uniform), the level by the 32-bit quant_fast (tv/tb_frag.h has the range proof).
  // A lane's four outputs are columns x .. x + 3 (x a multiple of 4) of one row: one TB, as
  // TBs are 4-aligned, so the levels are one 8-byte store, the TB statistics one pair of LDS
  // atomics per lane, and only the first column can be the TB's origin.  multi: some TB has
  // >= 2 levels -- this lane adds two, or finds the count already non-zero.
  // kSdh / kRdq: di = the lane's first coefficient in sdh_d (luma y * 32 + x, chroma 1024 + 256 pl + y * 16 + x)
  auto emit_levels = [&](int16_t* dst, int id, int sh2, const QuantParams& q, const int* v, bool origin, int di) {
    int cnt = 0, sum = 0, lev[4];
    uint32_t dd = 0, neg = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cf = (v[r] + (1 << (sh2 - 1))) >> sh2;
      lev[r] = quant_fast(cf, q);
      cnt += lev[r] != 0;
      sum += tv_abs(lev[r]);
      if constexpr (kSdh || kRdq) {
        dd |= (uint32_t)(sdh_delta_fast(cf, lev[r], q) + 64) << (8 * r);
        neg |= (cf < 0 ? 1u : 0u) << r;
      }
    }
    if constexpr (kSdh || kRdq) {
      *reinterpret_cast<uint32_t*>(&L.sdh_d[di]) = dd;
      L.sdh_neg[di >> 2] = (uint8_t)neg;
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)(lev[0] & 0xffff) | (uint32_t)lev[1] << 16,
                                                (uint32_t)(lev[2] & 0xffff) | (uint32_t)lev[3] << 16);
    if (origin) L.dc[id] = lev[0];
    if (cnt) {
      if (atomicAdd(&L.nz[id], cnt) | (cnt > 1)) L.multi = 1;
      atomicAdd(&L.sa[id], sum);
    }
  };
  for (int t = wave; t < ntiles; t += 4) {
    int o[4];
    if (t < 4) {
      int l2;
      if (whole) {
        const int ia = (16 * (t >> 1) + fi) * kTmpYP + 8 * kq;
        frag_tile_split_a(frag8(&L.tmpYh[ia]), frag8(&L.tmpYl[ia]), T32(0, t & 1), o);
        l2 = 5;
      } else {
        const int ox = (t & 1) * 16, oy = (t >> 1) * 16;
        l2 = L.qtype[t] == 1 ? 4 : 3;
        const int ia = (oy + fi) * kTmpYP + ox + 4 * kq;
        frag_tile_split_a(frag4(&L.tmpYh[ia]), frag4(&L.tmpYl[ia]), C16(l2, 0), o);
      }
      const QuantParams qy = quant_params(qp, l2);
      const int m = (1 << l2) - 1, y = (t >> 1) * 16 + fi, x = (t & 1) * 16 + kq * 4;
      const int id = whole ? 0 : 4 * t + (l2 == 3 ? (fi >> 3) * 2 + (kq >> 1) : 0);
      emit_levels(&L.resY[y * 32 + x], id, l2 + 6, qy, o, (x & m) == 0 && (y & m) == 0, kSdh || kRdq ? y * 32 + x : 0);
    } else if (whole) {
      const int pl = t - 4;
      const int ia = fi * kTmpCP + 4 * kq;
      frag_tile_split_a(frag4(&L.tmpCh[pl][ia]), frag4(&L.tmpCl[pl][ia]), C16(4, 0), o);
      emit_levels(&L.resC[pl][fi * 16 + kq * 4], 16 + 16 * pl, 10, quant_params(qpc, 4), o, lane == 0,
                  kSdh || kRdq ? 1024 + 256 * pl + fi * 16 + kq * 4 : 0);
    } else {
      const int q = t - 4, ox = (q & 1) * 8, oy = (q >> 1) * 8, l2 = L.qtype[q] == 1 ? 3 : 2;
      // A(r = fi, k = 4 kq ..): inside plane fi >> 3's block iff pin; the read is in bounds either way
      const int ia = (oy + (fi & 7)) * kTmpCP + ox + 4 * (kq & 1);
      const h4 ahi = frag4(&L.tmpCh[fi >> 3][ia]), alo = frag4(&L.tmpCl[fi >> 3][ia]);
      frag_tile_split_a(pin ? ahi : zero4, pin ? alo : zero4, C16(l2, 0), o);
      const QuantParams qc = quant_params(qpc, l2);
      if (pin) {
        const int m = (1 << l2) - 1, pl = fi >> 3, y = oy + (fi & 7), x = ox + 4 * (kq & 1);
        const int id = 16 + 16 * pl + 4 * q + (l2 == 2 ? ((fi >> 2) & 1) * 2 + (kq & 1) : 0);
        emit_levels(&L.resC[pl][y * 16 + x], id, l2 + 6, qc, o, (x & m) == 0 && (y & m) == 0,
                    kSdh || kRdq ? 1024 + 256 * pl + y * 16 + x : 0);
      }
    }
  }
  __syncthreads();
  // ---- RDOQ-lite (tv code_tb, inter TBs of 8x8 and up): trailing coefficient groups whose
  // only level is a lone +-1 are dropped -- tv walks the TB's groups in reverse up-right
  // diagonal scan to the first group holding anything else, down to diagonal rdoq_dmin.  In
  // parallel that is: a lone group is dropped iff its scan key (diagonal major, then rows
  // from the bottom) is above every other non-empty-non-lone group's of its TB (one LDS max
  // per TB) and its diagonal is >= rdoq_dmin.  One thread per 4x4 group (luma 64, Cb / Cr 16).
  // A CTB whose TBs hold at most one level each skips it (workgroup-uniform): a lone level
  // the pass could drop is dropped by the whole-TB rule (pr_zeroed) anyway.
  if (!kRdq && rdoq && L.multi) {
    int code = 0, key = 0, id = 0, dmin = 1 << 20;
    int16_t* p = nullptr;
    int st = 32;
    if (tid < 96) {
      int x, y, l2, pl = -1;
      if (tid < 64) {
        x = (tid & 7) * 4, y = (tid >> 3) * 4;
        l2 = pr_l2_luma(L, x, y);
        id = pr_tb_luma(L, x, y);
        p = &L.resY[y * 32 + x];
      } else {
        const int c = tid - 64;
        pl = c >> 4, x = (c & 3) * 4, y = ((c & 15) >> 2) * 4;
        l2 = pr_l2_luma(L, 2 * x, 2 * y) - 1;
        id = pr_tb_chroma(L, pl, x, y);
        p = &L.resC[pl][y * 16 + x];
        st = 16;
      }
      int t = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 w = *reinterpret_cast<const uint2*>(p + j * st);
        t += tv_abs((int)(int16_t)(w.x & 0xffff)) + tv_abs((int)(int16_t)(w.x >> 16)) + tv_abs((int)(int16_t)(w.y & 0xffff)) +
             tv_abs((int)(int16_t)(w.y >> 16));
      }
      const int m = (1 << l2) - 1, gx = (x & m) >> 2, gy = (y & m) >> 2;
      code = tv_min(t, 2);
      key = (gx + gy) * 16 + 15 - gy;
      const int q = pl < 0 ? (y >> 4) * 2 + (x >> 4) : (y >> 3) * 2 + (x >> 3);
      if (l2 >= 3 && !L.qintra[L.qtype[0] == 0 ? 0 : q]) dmin = rdoq_dmin(rdoq, 1 << (l2 - 2));
      if (code == 2) atomicMax(&L.cgmax[id], key);
      if (gx + gy < dmin) code = 0;  // groups this TB keeps whatever they hold
    }
    // all groups of a TB are in one wave (luma wave 0, chroma wave 1) and one wave's LDS
    // operations execute in order: the max needs no workgroup barrier before it is read
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (code == 1 && key > L.cgmax[id]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<uint2*>(p + j * st) = make_uint2(0u, 0u);
      atomicSub(&L.nz[id], 1);
      atomicSub(&L.sa[id], 1);
    }
    __syncthreads();
  }
  // ---- rate-distortion quantisation (tv/rdq.h) in the place of RDOQ-lite: one thread per 4x4
  // group runs stages 1 and 2 on its sixteen coefficients (rdq_group: the levels it changes go
  // straight back into the level plane), stage 3 is a sum and a minimum over the TB's groups
  // in coding order.  All groups of a TB are in one wave (luma wave 0, chroma wave 1), so the
  // per-group values cross lanes through LDS with wave fences only; they live in the f16
  // images, dead between stage 2 and stage 3.  The TB statistics follow the levels.
  // kSdh: the sign-hiding pass needs the distance from the final level, d + 256 (|l0| - |l|);
  // |l0| - |l| + 1 (0..4) per coefficient is kept as a byte beside d, in tmpYh.
  if constexpr (kRdq) {
    int* gf = reinterpret_cast<int*>(L.tmpYl);  // [96] stage-2 J of the group at TB slot + rank
    int* je = gf + 96;                          // [96] J of ending the TB in that group
    uint8_t* drop = reinterpret_cast<uint8_t*>(L.tmpYh);
    static_assert(sizeof(L.tmpYl) >= 2 * 96 * sizeof(int) && sizeof(L.tmpYh) >= sizeof(L.sdh_d), "rdq scratch fits the f16 images");
    if (wave < 2) {
      int x, y, l2, pl = -1, id, st, di, base, q;
      int16_t* p;
      if (tid < 64) {
        x = (tid & 7) * 4, y = (tid >> 3) * 4;
        l2 = pr_l2_luma(L, x, y);
        id = pr_tb_luma(L, x, y);
        p = &L.resY[y * 32 + x], st = 32, di = y * 32 + x, base = 4 * id;
        q = (y >> 4) * 2 + (x >> 4);
      } else {
        const int c = (tid - 64) & 31;
        pl = c >> 4, x = (c & 3) * 4, y = ((c & 15) >> 2) * 4;
        l2 = pr_l2_luma(L, 2 * x, 2 * y) - 1;
        id = pr_tb_chroma(L, pl, x, y);
        p = &L.resC[pl][y * 16 + x], st = 16, di = 1024 + 256 * pl + y * 16 + x, base = 64 + id - 16;
        q = (y >> 3) * 2 + (x >> 3);
      }
      // a quadrant that is an intra CU keeps its levels: k_pintra_recon codes it again, whole
      const bool act = tid < 96 && !L.qintra[L.qtype[0] == 0 ? 0 : q];
      const int s = 1 << (l2 - 2), m = (1 << l2) - 1, gx = (x & m) >> 2, gy = (y & m) >> 2, rank = rdq_rank(gx, gy, s);
      auto at = [&](int n) {
        const int sp = sdh_scan_pos(0, n);
        return (sp >> 2) * st + (sp & 3);
      };
      auto stats = [&](int& cnt, int& sum) {
        cnt = sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint2 w = *reinterpret_cast<const uint2*>(p + j * st);
          const int a = (int)(int16_t)(w.x & 0xffff), b = (int)(int16_t)(w.x >> 16), c = (int)(int16_t)(w.y & 0xffff), d = (int)(int16_t)(w.y >> 16);
          cnt += (a != 0) + (b != 0) + (c != 0) + (d != 0);
          sum += tv_abs(a) + tv_abs(b) + tv_abs(c) + tv_abs(d);
        }
      };
      int cnt0, sum0;
      stats(cnt0, sum0);
      const unsigned long long any = __ballot(act && cnt0 != 0);  // the wave's non-empty groups
      const int nb = tid < 64 ? 8 : 4;                           // lanes to the group below
      const int right = gx + 1 < s ? (int)((any >> ((lane + 1) & 63)) & 1) : 0;
      const int below = gy + 1 < s ? (int)((any >> ((lane + nb) & 63)) & 1) : 0;
      if constexpr (kSdh) {  // |l0| - |l| + 1 per coefficient: 1 until a level moves
        if (tid < 96) {
#pragma unroll
          for (int j = 0; j < 4; ++j) *reinterpret_cast<uint32_t*>(&drop[di + j * st]) = 0x01010101u;
        }
      }
      RdqGroup g{};
      if (act) {
        g = rdq_group([&](int n) { return tv_abs((int)p[at(n)]); }, [&](int n) { return (int)L.sdh_d[di + at(n)] - 64; },
                      [&](int n, int a) {
                        const int o = at(n), l = p[o];  // l != 0: a zero stays zero
                        if constexpr (kSdh) drop[di + o] = (uint8_t)(1 + tv_abs(l) - a);
                        p[o] = (int16_t)(l < 0 ? -a : a);
                      },
                      pl >= 0 ? 1 : 0, rank == 0, right, below, kRdqLambda);
        if (g.maxmag > 2) atomicMax(&L.cgmax[id], rank);  // the TB cannot end before this group
        gf[base + rank] = g.gfull;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (act) {
        int before = 0;
        for (int j = 0; j < rank; ++j) before += gf[base + j];
        const bool valid = (g.nlast >= 0 || rank == 0) && rank >= L.cgmax[id];
        je[base + rank] = valid ? rdq_end_cost(g, before, pl >= 0 ? 1 : 0, gx + gy, kRdqLambda) : 0x7fffffff;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (act) {
        int best = 0x7fffffff, k = 0;
        for (int j = 0; j < s * s; ++j) {
          const int e = je[base + j];
          if (e <= best) best = e, k = j;
        }
        const int keep = rank > k ? -1 : (rank == k ? g.nlast : (g.emptied ? -1 : 15));  // last scan position kept
        for (int n = keep + 1; n < 16; ++n) {
          const int o = at(n), a = tv_abs((int)p[o]);
          if (a) {
            if constexpr (kSdh) drop[di + o] = (uint8_t)(drop[di + o] + a);
            p[o] = 0;
          }
        }
        int cnt1, sum1;
        stats(cnt1, sum1);
        if (cnt1 != cnt0) atomicAdd(&L.nz[id], cnt1 - cnt0);
        if (sum1 != sum0) atomicAdd(&L.sa[id], sum1 - sum0);
        if (rank == 0) L.dc[id] = p[0];
      }
    }
    __syncthreads();
  }
  // ---- sign data hiding (tv/sdh.h) on the final levels: after RDOQ-lite, only in TBs the
  // lone-level rule keeps, and without touching nz / sa / dc -- a TB that now looks like a lone
  // +-1 stays.  One thread per 4x4 group as above; inter TBs scan diagonally.  (A quadrant that
  // is an intra CU is coded again, whole, by k_pintra_recon.)
  if constexpr (kSdh) {
    if (tid < 96) {
      int16_t* p;
      int st, di, id;
      if (tid < 64) {
        const int x = (tid & 7) * 4, y = (tid >> 3) * 4;
        id = pr_tb_luma(L, x, y);
        p = &L.resY[y * 32 + x], st = 32, di = y * 32 + x;
      } else {
        const int c = tid - 64, pl = c >> 4, x = (c & 3) * 4, y = ((c & 15) >> 2) * 4;
        id = pr_tb_chroma(L, pl, x, y);
        p = &L.resC[pl][y * 16 + x], st = 16, di = 1024 + 256 * pl + y * 16 + x;
      }
      if (!pr_zeroed(L, id)) {
        auto at = [&](int n) {
          const int s = sdh_scan_pos(0, n);
          return (s >> 2) * st + (s & 3);
        };
        int pos, value;
        // kRdq: the distance from the final level (the pass above left |l0| - |l| + 1 in tmpYh)
        if (sdh_adjust([&](int n) { return (int)p[at(n)]; },
                       [&](int n) {
                         int d = (int)L.sdh_d[di + at(n)] - 64;
                         if constexpr (kRdq) d += 256 * ((int)reinterpret_cast<const uint8_t*>(L.tmpYh)[di + at(n)] - 1);
                         return d;
                       },
                       [&](int n) { const int a = di + at(n); return ((L.sdh_neg[a >> 2] >> (a & 3)) & 1) != 0; }, pos, value))
          p[at(pos)] = (int16_t)value;
      }
    }
    __syncthreads();
  }
  // ---- final levels (dropped TBs zeroed) -> the level planes; cbf per CU
  {
    // 4 levels (one TB: TBs are >= 4 wide and 4-aligned) per item, one 8-byte store
    int16_t* LY = dec.coef_y + b * g.ysz + cy * W + cx;
    {
      const int x = (tid & 7) * 4, y = tid >> 3;
      uint2* r = reinterpret_cast<uint2*>(&L.resY[y * 32 + x]);
      if (pr_zeroed(L, pr_tb_luma(L, x, y))) *r = make_uint2(0u, 0u);
      *reinterpret_cast<uint2*>(LY + y * W + x) = *r;
    }
    if (tid < 128) {
      const int pl = tid >> 6, y = (tid >> 2) & 15, x = (tid & 3) * 4;
      uint2* r = reinterpret_cast<uint2*>(&L.resC[pl][y * 16 + x]);
      if (pr_zeroed(L, pr_tb_chroma(L, pl, x, y))) *r = make_uint2(0u, 0u);
      *reinterpret_cast<uint2*>((pl ? dec.coef_v : dec.coef_u) + b * g.csz + (long)((cy >> 1) + y) * Wc + (cx >> 1) + x) = *r;
    }
    if (tid < 8) {  // tiles whose TBs all dropped out skip the inverse transform
      bool z = true;
      if (tid < 4) {
        if (L.qtype[0] == 0) z = pr_zeroed(L, 0);
        else for (int k = 0; k < 4; ++k) z = z && pr_zeroed(L, pr_tb_luma(L, (tid & 1) * 16 + (k & 1) * 8, (tid >> 1) * 16 + (k >> 1) * 8));
      } else if (L.qtype[0] == 0) {
        z = pr_zeroed(L, 16 + 16 * (tid - 4));
      } else {
        const int q = tid - 4;  // Cb | Cr pair of quadrant q (Cb and Cr 8x8 regions)
        for (int pl = 0; pl < 2; ++pl)
          for (int k = 0; k < 4; ++k) z = z && pr_zeroed(L, pr_tb_chroma(L, pl, (q & 1) * 8 + (k & 1) * 4, (q >> 1) * 8 + (k >> 1) * 4));
      }
      L.tzero[tid] = z;
    }
    if (tid < 16) {
      const int x = (tid & 3) * 8, y = (tid >> 2) * 8;  // this unit's CU = its TBs
      const int cb = (pr_zeroed(L, pr_tb_luma(L, x, y)) ? 0 : 1) | (pr_zeroed(L, pr_tb_chroma(L, 0, x >> 1, y >> 1)) ? 0 : 2) |
                     (pr_zeroed(L, pr_tb_chroma(L, 1, x >> 1, y >> 1)) ? 0 : 4);
      dec.cbf[ub + (long)((cy >> 3) + (tid >> 2)) * g.w8 + (cx >> 3) + (tid & 3)] = (uint8_t)cb;
    }
  }
  __syncthreads();
  // --------------------------------------- stage 3: T^T * dequant(levels)  (split d)
  const DeqParams dq5 = deq_params(qp, 5), dqc4 = deq_params(qpc, 4);
  for (int t = wave; t < ntiles; t += 4) {
    if (L.tzero[t]) continue;  // wave-uniform: an all-zero tile reconstructs to the prediction
    int o[4];
    if (t < 4) {
      if (whole) {
        h8 bhi, blo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int d = deq_fast(L.resY[(8 * kq + e) * 32 + 16 * (t & 1) + fi], dq5);
          bhi[e] = f16_hi(d), blo[e] = f16_lo(d);
        }
        frag_tile_split_b(T32(1, t >> 1), bhi, blo, o);
      } else {
        const int ox = (t & 1) * 16, oy = (t >> 1) * 16, l2 = L.qtype[t] == 1 ? 4 : 3;
        const DeqParams dql = deq_params(qp, l2);
        h4 bhi, blo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int d = deq_fast(L.resY[(oy + 4 * kq + e) * 32 + ox + fi], dql);
          bhi[e] = f16_hi(d), blo[e] = f16_lo(d);
        }
        frag_tile_split_b(C16(l2, 1), bhi, blo, o);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = clip3(-32768, 32767, (o[r] + 64) >> 7);
      put_y((t >> 1) * 16 + fi, (t & 1) * 16 + kq * 4, o);
    } else if (whole) {
      const int pl = t - 4;
      h4 bhi, blo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = deq_fast(L.resC[pl][(4 * kq + e) * 16 + fi], dqc4);
        bhi[e] = f16_hi(d), blo[e] = f16_lo(d);
      }
      frag_tile_split_b(C16(4, 1), bhi, blo, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = clip3(-32768, 32767, (o[r] + 64) >> 7);
      put_c(pl, fi, kq * 4, o);
    } else {
      const int q = t - 4, ox = (q & 1) * 8, oy = (q >> 1) * 8, l2 = L.qtype[q] == 1 ? 3 : 2;
      const DeqParams dqcl = deq_params(qpc, l2);
      h4 bhi, blo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = deq_fast(L.resC[pp][(oy + 4 * (kq & 1) + e) * 16 + ox + (fi & 7)], dqcl);
        bhi[e] = f16_hi(d), blo[e] = f16_lo(d);
      }
      frag_tile_split_b(C16(l2, 1), pin ? bhi : zero4, pin ? blo : zero4, o);
      if (pin) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = clip3(-32768, 32767, (o[r] + 64) >> 7);
        put_c(fi >> 3, oy + (fi & 7), ox + 4 * (kq & 1), o);
      }
    }
  }
  __syncthreads();
  // ------------------------------------- stage 4: G * T + prediction -> reconstruction
  // a lane's four pixels (one row, 4-aligned) are one prediction dword and one dword store
  auto recon4 = [&](uint32_t pw, const int* v) {
    uint32_t w = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) w |= (uint32_t)clip_pixel((int)((pw >> (8 * r)) & 255u) + ((v[r] + 2048) >> 12)) << (8 * r);
    return w;
  };
  for (int t = wave; t < ntiles; t += 4) {
    int o[4];
    const bool tz = L.tzero[t];
    if (tz) {  // copy the prediction (what clip(pred + 0) gives)
      o[0] = o[1] = o[2] = o[3] = 0;
    }
    if (t < 4) {
      if (tz) {  // o = 0
      } else if (whole) {
        const int ia = (16 * (t >> 1) + fi) * kTmpYP + 8 * kq;
        frag_tile_split_a(frag8(&L.tmpYh[ia]), frag8(&L.tmpYl[ia]), T32(1, t & 1), o);
      } else {
        const int ox = (t & 1) * 16, oy = (t >> 1) * 16, l2 = L.qtype[t] == 1 ? 4 : 3;
        const int ia = (oy + fi) * kTmpYP + ox + 4 * kq;
        frag_tile_split_a(frag4(&L.tmpYh[ia]), frag4(&L.tmpYl[ia]), C16(l2, 1), o);
      }
      const int y = (t >> 1) * 16 + fi, x = (t & 1) * 16 + kq * 4;
      *reinterpret_cast<uint32_t*>(rec.plane(0, b, g) + (cy + y) * W + cx + x) =
          recon4(*reinterpret_cast<const uint32_t*>(&L.predY[y * 32 + x]), o);
    } else if (whole) {
      const int pl = t - 4;
      if (!tz) {
        const int ia = fi * kTmpCP + 4 * kq;
        frag_tile_split_a(frag4(&L.tmpCh[pl][ia]), frag4(&L.tmpCl[pl][ia]), C16(4, 1), o);
      }
      *reinterpret_cast<uint32_t*>(rec.plane(1 + pl, b, g) + (long)((cy >> 1) + fi) * Wc + (cx >> 1) + kq * 4) =
          recon4(*reinterpret_cast<const uint32_t*>(&L.predC[pl][fi * 16 + kq * 4]), o);
    } else {
      const int q = t - 4, ox = (q & 1) * 8, oy = (q >> 1) * 8, l2 = L.qtype[q] == 1 ? 3 : 2;
      if (!tz) {
        const int ia = (oy + (fi & 7)) * kTmpCP + ox + 4 * (kq & 1);
        const h4 ahi = frag4(&L.tmpCh[fi >> 3][ia]), alo = frag4(&L.tmpCl[fi >> 3][ia]);
        frag_tile_split_a(pin ? ahi : zero4, pin ? alo : zero4, C16(l2, 1), o);
      }
      if (pin) {
        const int pl = fi >> 3, y = oy + (fi & 7), x = ox + 4 * (kq & 1);
        *reinterpret_cast<uint32_t*>(rec.plane(1 + pl, b, g) + (long)((cy >> 1) + y) * Wc + (cx >> 1) + x) =
            recon4(*reinterpret_cast<const uint32_t*>(&L.predC[pl][y * 16 + x]), o);
      }
    }
  }
}

void launch_quarter(FrameSet src, uint8_t* q, const Geo& g, int B, hipStream_t s) {
  const int n = (g.W >> 2) * (g.H >> 2);
  k_quarter<<<dim3((n + 255) / 256, B), 256, 0, s>>>(src, q, g);
}

void launch_coarse_me(const MeBuffers& me, const Geo& g, const RcTables* rc, int seq_qp, int range, int B,
                      hipStream_t s) {
  const int rq = range / 4;
  if (rq > kCoarseMaxRq) throw std::runtime_error("coarse search range too large");
  const size_t lds = sizeof(uint32_t) * (size_t)(8 + 2 * rq) * (size_t)((rq / 2 + 3) | 1);  // the window only
  k_coarse_me<<<dim3(g.wc * g.hc, B), 64, lds, s>>>(me.qcur, me.qprev, g, rc, seq_qp, rq, me.cmv, me.ccost);
}

// CRF (tv/rc_model.h): the frame QP of every segment from its lookahead complexity — the
// summed coarse-search cost (P) or the quarter-res activity (IDR) — written into dec.qp
__global__ void __launch_bounds__(256) k_rc_crf(const uint8_t* q, const int* ccost, int8_t* qp, Geo g, int crf,
                                                int intra) {
  const int b = blockIdx.x, nctu = g.wc * g.hc, qw = g.W >> 2;
  __shared__ unsigned long long sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  unsigned long long acc = 0;
  for (int c = threadIdx.x; c < nctu; c += 256) {
    if (intra) {
      const uint8_t* Q = q + (long)b * qw * (g.H >> 2) + (long)(8 * (c / g.wc)) * qw + 8 * (c % g.wc);
      acc += rc_block_activity(Q, qw);
    } else {
      acc += (unsigned long long)ccost[(long)b * nctu + c];
    }
  }
  atomicAdd(&sum, acc);
  __syncthreads();
  if (threadIdx.x == 0) qp[b] = (int8_t)rc_crf_qp(crf, intra != 0, sum, nctu);
}

void launch_rc_crf(const uint8_t* q, const int* ccost, int8_t* qp, const Geo& g, int crf, bool intra, int B,
                   hipStream_t s) {
  k_rc_crf<<<B, 256, 0, s>>>(q, ccost, qp, g, crf, intra ? 1 : 0);
}

// the instantiation SeqConfig::sign_hiding / rd_quant select
static auto inter_recon_kernel(const Geo& g) {
  if (g.rd_quant) return g.sign_hiding ? k_inter_recon<true, true> : k_inter_recon<false, true>;
  return g.sign_hiding ? k_inter_recon<true, false> : k_inter_recon<false, false>;
}

void launch_inter_frame(FrameSet src, FrameSet ref, const uint8_t* phase, FrameSet rec, DecisionSet dec,
                        const Geo& g, const RcTables* rc, int range, const MeBuffers& me, int B, hipStream_t s,
                        const PIntraBuffers* pi) {
  const PIntraBuffers none{};
  if (pi && hipMemsetAsync(pi->count, 0, 6 * sizeof(int), s) != hipSuccess) return;
  const dim3 grid(g.wc * g.hc, B);
  (g.subpel_satd ? k_inter_me<true> : k_inter_me<false>)<<<grid, kMeThreads, 0, s>>>(src, ref, phase, dec, me.prev_mv, me.cmv, g, rc, range, nullptr, pi ? *pi : none);
  if (pi) launch_pintra_decide(src, dec, g, rc, *pi, B, s);
  inter_recon_kernel(g)<<<grid, 256, 0, s>>>(src, ref, phase, rec, dec, g, FrameSet{}, nullptr);
  if (pi) launch_pintra_recon(src, rec, dec, g, *pi, B, s);
}

void launch_inter_frame_b(FrameSet src, FrameSet ref0, const uint8_t* phase0, FrameSet ref1, const uint8_t* phase1,
                          FrameSet rec, DecisionSet dec, const Geo& g, const RcTables* rc, const int* range,
                          const MeBuffers& me0, const MeBuffers& me1, CtbMeOut* meout, int B, hipStream_t s) {
  const dim3 grid(g.wc * g.hc, B);
  CtbMeOut* o1 = meout + (long)B * g.wc * g.hc;
  const PIntraBuffers none{};
  const auto k_me = g.subpel_satd ? k_inter_me<true> : k_inter_me<false>;
  k_me<<<grid, kMeThreads, 0, s>>>(src, ref0, phase0, dec, me0.prev_mv, me0.cmv, g, rc, range[0], meout, none);
  k_me<<<grid, kMeThreads, 0, s>>>(src, ref1, phase1, dec, me1.prev_mv, me1.cmv, g, rc, range[1], o1, none);
  k_bi_decide<<<grid, 256, 0, s>>>(src, phase0, phase1, meout, o1, dec, g, rc);
  inter_recon_kernel(g)<<<grid, 256, 0, s>>>(src, ref0, phase0, rec, dec, g, ref1, phase1);
}

}  // namespace gpu
}  // namespace tv
