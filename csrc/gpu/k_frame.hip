// k_frame.hip — frame-level kernels: synthetic source, PSNR SSE, quarter-pel phase planes,
// in-loop deblocking.  Batched: blockIdx.z (or .y) selects the segment.
#include <cstring>

#include "gpu_common.h"
#include "k_encode.h"
#include "tv/synth.h"
#include "tv/synth_tile.h"

namespace tv {
namespace gpu {

// ---------------------------------- synthetic source ------------------------------------
// One workgroup per 256 x 32 tile of one plane of one segment, in the separable form of
// tv/synth_tile.h (bit-identical to synth_sample_ctx of tv/synth.h, which the CPU golden
// encoder uses; tests/test_synth_tiles.py walks the same routines on the host):
//   1. the lattice hashes of every octave's window over the tile go into LDS, one point per
//      lane, a lattice row per wave;
//   2. thread x builds column x of every octave's `top` rows (16-bit) from them: the cell
//      index and the horizontal smoothstep are taken once per column and octave;
//   3. a lane takes 4 adjacent samples of 8 rows: per row and octave two 8-byte LDS reads and
//      the vertical blend, whose cell row and smoothstep are wave-uniform.  A wave writes
//      256 contiguous bytes of a row with one dword store per lane.
// An object whose bounding box meets the tile (workgroup-uniform; most tiles meet none) has
// its two octaves' tables built the same way in object-relative coordinates, reusing the LDS,
// and is applied in ascending k so later objects stay on top; the ellipse test is a 64-bit
// compare of a per-column with a per-row term (synth_cover_col / _row).  The frame contexts (object
// trajectories) are computed by the launcher and travel as kernel arguments: no workgroup
// evaluates synth_frame_ctx.
constexpr int kSynTW = kSynthTileW, kSynTH = kSynthTileH, kSynRows = kSynTH / 4;  // rows per wave
static_assert(kSynTW == 256 && kSynTH % 4 == 0, "a wave of 4-sample items spans the tile; 4 waves share its rows");

struct SynthArgs {
  SynthObject obj[kSynthObjects];  // depend on (seed, W, H) only
  int32_t t[kMaxBatch];
  int32_t ox[kMaxBatch][kSynthObjects], oy[kMaxBatch][kSynthObjects];  // per segment, after the bounce
};
static_assert(sizeof(SynthArgs) + sizeof(Geo) + sizeof(FrameSet) + 16 <= 4096, "kernel arguments are limited to 4 KB");

// Table sizes: the coordinate span of a tile is (n - 1) * 16 on the luma grid, twice that for
// the chroma planes.
constexpr int kSynSpanX = (kSynTW - 1) * 16, kSynSpanY = (kSynTH - 1) * 16;
constexpr int syn_max(int a, int b) { return a > b ? a : b; }
constexpr int syn_pts(int lp, int s) { return synth_win_max(kSynSpanX << s, lp) * synth_win_max(kSynSpanY << s, lp); }
constexpr int syn_rows(int lp, int s) { return synth_win_max(kSynSpanY << s, lp); }
// background luma (lp 7, 5, 3 and the textured 1), object luma (4, 2), chroma (8; object 5)
constexpr int syn_lat_size(bool tex) {
  return syn_max(syn_max(syn_pts(7, 0) + syn_pts(5, 0) + syn_pts(3, 0) + (tex ? syn_pts(1, 0) : 0), syn_pts(4, 0) + syn_pts(2, 0)),
                 syn_max(syn_pts(8, 1), syn_pts(5, 1)));
}
constexpr int syn_top_rows(bool tex) {
  return syn_max(syn_max(syn_rows(7, 0) + syn_rows(5, 0) + syn_rows(3, 0) + (tex ? syn_rows(1, 0) : 0), syn_rows(4, 0) + syn_rows(2, 0)),
                 syn_max(syn_rows(8, 1), syn_rows(5, 1)));
}

// Lattice of window w: wave r takes lattice rows r, r + 4, ..; a lane one point of the row.
__device__ __forceinline__ void syn_lattice(const SynthWin& w, uint8_t* lat, int wave, int lane) {
  for (int r = wave; r < w.npy; r += 4)
    for (int i = lane; i < w.npx; i += 64) lat[r * w.npx + i] = (uint8_t)synth_win_lattice(w, i, r);
}
// Column `col` (coordinate p16, inside the window) of the window's top rows.
__device__ __forceinline__ void syn_top(const SynthWin& w, const uint8_t* lat, uint16_t* top, int col, int32_t p16) {
  int ci, sx;
  synth_axis(p16, w.sh, w.cx0, ci, sx);
  for (int r = 0; r < w.npy; ++r)
    top[r * kSynTW + col] = (uint16_t)synth_top(lat[r * w.npx + ci], lat[r * w.npx + ci + 1], sx);
}
// The octave at the 4 samples from column x (a multiple of 4) of the row at coordinate p16.
__device__ __forceinline__ void syn_eval(const SynthWin& w, const uint16_t* top, int x, int32_t p16, int n[4]) {
  int cy, sy;
  synth_axis(p16, w.sh, w.cy0, cy, sy);
  const uint2 a = *reinterpret_cast<const uint2*>(top + cy * kSynTW + x);
  const uint2 b = *reinterpret_cast<const uint2*>(top + (cy + 1) * kSynTW + x);
  n[0] = synth_rows((int)(a.x & 0xffff), (int)(b.x & 0xffff), sy);
  n[1] = synth_rows((int)(a.x >> 16), (int)(b.x >> 16), sy);
  n[2] = synth_rows((int)(a.y & 0xffff), (int)(b.y & 0xffff), sy);
  n[3] = synth_rows((int)(a.y >> 16), (int)(b.y >> 16), sy);
}

// One tile.  kTex: the textured variant (seed bit 31) adds the 2-pixel octave (more top rows of
// LDS) and the per-sample grain hash.  kChroma: the chroma planes have one octave of their
// own; a body per plane kind keeps the sample loops free of branches on the plane.
template <bool kTex, bool kChroma>
__device__ __forceinline__ void syn_tile(uint16_t* top, uint8_t* lat, FrameSet src, const Geo& g, uint32_t seed,
                                         const SynthArgs& a, int c, int x0, int y0) {
  constexpr int kBg = kChroma ? 1 : (kTex ? 4 : 3), kOb = kChroma ? 1 : 2, s = kChroma ? 1 : 0;
  __builtin_assume(kChroma ? c != 0 : c == 0);
  const int b = blockIdx.y;
  const int pw = g.W >> s, ph = g.H >> s, dw = g.dw >> s, dh = g.dh >> s;
  const int t = a.t[b];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // coordinate range of the tile, of this thread's table column and of its 4 sample columns
  const int32_t tx0 = synth_tile_pos(x0, dw, s), tx1 = synth_tile_pos(x0 + kSynTW - 1, dw, s);
  const int32_t ty0 = synth_tile_pos(y0, dh, s), ty1 = synth_tile_pos(y0 + kSynTH - 1, dh, s);
  const int32_t colp = synth_tile_pos(x0 + tid, dw, s);
  const int x = 4 * lane, yw = y0 + wave * kSynRows;
  int32_t sp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sp[j] = synth_tile_pos(x0 + x + j, dw, s);

  SynthWin w[kBg];
  int lat0[kBg], row0[kBg];
  const int panx = t * synth_pan_x(kTex), pany = t * synth_pan_y(kTex);
  {
    int lo = 0, ro = 0;
#pragma unroll
    for (int i = 0; i < kBg; ++i) {
      w[i] = synth_win(synth_bg_lp(c, i), synth_bg_seed(seed, c, i), tx0 + panx, tx1 + panx, ty0 + pany, ty1 + pany);
      lat0[i] = lo;
      row0[i] = ro;
      syn_lattice(w[i], lat + lo, wave, lane);
      lo += w[i].npx * w[i].npy;
      ro += w[i].npy;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kBg; ++i) syn_top(w[i], lat + lat0[i], top + row0[i] * kSynTW, tid, colp + panx);
  __syncthreads();
  uint32_t word[kSynRows];  // every value before the grain is 0..255 (tv/synth.h)
#pragma unroll
  for (int j = 0; j < kSynRows; ++j) {
    const int32_t py = synth_tile_pos(yw + j, dh, s) + pany;
    int n[4][4] = {};
#pragma unroll
    for (int i = 0; i < kBg; ++i) syn_eval(w[i], top + row0[i] * kSynTW, x, py, n[i]);
    word[j] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m[4] = {n[0][q], n[1][q], n[2][q], n[3][q]};
      word[j] |= (uint32_t)synth_bg_mix(c, kTex, m) << (8 * q);
    }
  }

  for (int k = 0; k < kSynthObjects; ++k) {  // later objects on top
    const SynthObject& o = a.obj[k];
    const int32_t ox = a.ox[b][k], oy = a.oy[b][k];
    int32_t xlo, xhi, ylo, yhi;
    synth_obj_range(tx0, tx1, ox, o.w, xlo, xhi);
    synth_obj_range(ty0, ty1, oy, o.h, ylo, yhi);
    if (xlo > xhi || ylo > yhi) continue;  // workgroup-uniform: the tile misses the bounding box
    const int base = synth_obj_base(seed, k, c);
    SynthWin wo[kOb];
    int olat[kOb], orow[kOb];
    __syncthreads();  // the tables are reused
    {
      int lo = 0, ro = 0;
#pragma unroll
      for (int i = 0; i < kOb; ++i) {
        wo[i] = synth_win(synth_obj_lp(c, i), synth_obj_seed(o, c, i), xlo, xhi, ylo, yhi);
        olat[i] = lo;
        orow[i] = ro;
        syn_lattice(wo[i], lat + lo, wave, lane);
        lo += wo[i].npx * wo[i].npy;
        ro += wo[i].npy;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kOb; ++i) syn_top(wo[i], lat + olat[i], top + orow[i] * kSynTW, tid, clip3(xlo, xhi, colp - ox));
    __syncthreads();
    int64_t cover[4];  // the shape test's column term; never passes outside the box
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int32_t rx16 = sp[q] - ox;
      cover[q] = rx16 < xlo || rx16 > xhi ? INT64_MAX : synth_cover_col(o, rx16);
    }
#pragma unroll
    for (int j = 0; j < kSynRows; ++j) {
      const int32_t ry16 = synth_tile_pos(yw + j, dh, s) - oy;
      if (ry16 < ylo || ry16 > yhi) continue;  // wave-uniform
      const int64_t cover_row = synth_cover_row(o, ry16);
      int n[2][4] = {};
#pragma unroll
      for (int i = 0; i < kOb; ++i) syn_eval(wo[i], top + orow[i] * kSynTW, x, ry16, n[i]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (cover[q] > cover_row) continue;
        const int m[2] = {n[0][q], n[1][q]};
        word[j] = (word[j] & ~(0xffu << (8 * q))) | (uint32_t)synth_obj_mix(c, base, m) << (8 * q);
      }
    }
  }

  if (x0 + x >= pw) return;
  uint8_t* P = src.plane(c, b, g);
#pragma unroll
  for (int j = 0; j < kSynRows; ++j) {
    const int y = yw + j;
    if (y >= ph) break;
    uint32_t out = word[j];
    if (kTex) {  // per-frame grain at the clamped position, as synth_sample_ctx
      const int yc = tv_min(y, dh - 1);
      out = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int v = (int)((word[j] >> (8 * q)) & 255) + synth_grain(seed, t, c, tv_min(x0 + x + q, dw - 1), yc);
        out |= (uint32_t)clip_pixel(v) << (8 * q);
      }
    }
    *reinterpret_cast<uint32_t*>(P + (long)y * pw + x0 + x) = out;
  }
}

template <bool kTex>
__global__ void __launch_bounds__(256) k_synth(FrameSet src, Geo g, uint32_t seed, SynthArgs a) {
  __shared__ __attribute__((aligned(8))) uint16_t top[syn_top_rows(kTex) * kSynTW];
  __shared__ uint8_t lat[syn_lat_size(kTex)];
  // blockIdx.x: the luma tiles, then the U and the V tiles, row-major
  const int nlx = (g.W + kSynTW - 1) / kSynTW, ncx = (g.W / 2 + kSynTW - 1) / kSynTW;
  const int nl = nlx * ((g.H + kSynTH - 1) / kSynTH), nc = ncx * ((g.H / 2 + kSynTH - 1) / kSynTH);
  int id = blockIdx.x, c = 0;
  if (id >= nl) {
    c = id >= nl + nc ? 2 : 1;
    id -= nl + (c - 1) * nc;
  }
  const int ntx = c ? ncx : nlx, ty = id / ntx, x0 = (id - ty * ntx) * kSynTW, y0 = ty * kSynTH;
  if (c)
    syn_tile<kTex, true>(top, lat, src, g, seed, a, c, x0, y0);
  else
    syn_tile<kTex, false>(top, lat, src, g, seed, a, 0, x0, y0);
}

// ------------------------------------------ SSE -----------------------------------------
// One workgroup per (row block, plane, segment); 4-byte vector loads along rows.
__global__ void __launch_bounds__(256) k_sse(FrameSet a, FrameSet r, Geo g, unsigned long long* sse) {
  const int c = blockIdx.y, b = blockIdx.z;
  const int pw = c ? g.W / 2 : g.W;
  const int dw = c ? g.dw / 2 : g.dw, dh = c ? g.dh / 2 : g.dh;
  const uint8_t* A = a.plane(c, b, g);
  const uint8_t* R = r.plane(c, b, g);
  const int wq = (dw + 3) >> 2;  // 4-pixel groups per row (pw is a multiple of 16)
  unsigned s = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < wq * dh; i += gridDim.x * blockDim.x) {
    const int y = i / wq, x = (i - y * wq) * 4;
    const uint32_t va = *reinterpret_cast<const uint32_t*>(A + (long)y * pw + x);
    const uint32_t vr = *reinterpret_cast<const uint32_t*>(R + (long)y * pw + x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = (int)((va >> (8 * k)) & 255) - (int)((vr >> (8 * k)) & 255);
      s += (x + k < dw) ? (unsigned)(d * d) : 0u;
    }
  }
  unsigned long long t = s;
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __shared__ unsigned long long part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sse + b * 3 + c, part[0] + part[1] + part[2] + part[3]);
}

// --------------------------------- quarter-pel phase planes -----------------------------
// Plane p = fx + 4*fy holds the exact HEVC 8-tap interpolated luma sample at every integer
// position of the padded domain [-8, W+8) x [-8, H+8) (beyond 4 samples outside the
// picture the clamped interpolation is constant, so clamping the query to the pad is
// exact).  Motion search and luma motion compensation then become plain byte loads.
//
// One 32x32 output tile per workgroup, all 16 planes.  The 8-tap filters run on the packed
// integer dot-product units instead of scalar multiply-adds:
//  * horizontal (int8 samples): a sample window of 8 bytes is two dwords (v_alignbyte from
//    the tile row held as dwords in LDS); samples are biased to signed bytes (x ^ 0x80) so
//    each half is one v_dot4_i32_i8 against the packed taps, the bias is 128 * sum(taps) =
//    8192 added back — 2 dot4 per output instead of 8 MACs;
//  * vertical over integer rows: the 4x4 byte blocks of 8 rows are transposed with 16
//    v_perm_b32, then 2 dot4 per output;
//  * vertical over the 16-bit horizontal intermediates: row pairs are packed with v_perm and
//    reduced with v_dot2_i32_i16 (4 per output).
// Every product and sum is exact (|intermediate| < 2^15, |2-D sum| < 2^21): bit-identical
// to tv::mc_luma_sample.
typedef short tv_short2 __attribute__((ext_vector_type(2)));

__device__ constexpr uint32_t pack_taps4(int f, int k0) {
  return (uint32_t)(uint8_t)kLumaFilter[f][k0] | (uint32_t)(uint8_t)kLumaFilter[f][k0 + 1] << 8 |
         (uint32_t)(uint8_t)kLumaFilter[f][k0 + 2] << 16 | (uint32_t)(uint8_t)kLumaFilter[f][k0 + 3] << 24;
}
__device__ constexpr uint32_t pack_taps2(int f, int k0) {
  return (uint32_t)(uint16_t)kLumaFilter[f][k0] | (uint32_t)(uint16_t)kLumaFilter[f][k0 + 1] << 16;
}
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(tv_short2, a), __builtin_bit_cast(tv_short2, b), c, false);
}
__device__ __forceinline__ uint32_t pack4_pixels(int v0, int v1, int v2, int v3) {
  return (uint32_t)clip_pixel(v0) | (uint32_t)clip_pixel(v1) << 8 | (uint32_t)clip_pixel(v2) << 16 |
         (uint32_t)clip_pixel(v3) << 24;
}

constexpr int kPhW = 10;  // dwords per staged source row: 40 bytes = tile 32 + 8 tap reach
__global__ void __launch_bounds__(256) k_phase_planes(FrameSet ref, uint8_t* phase, Geo g) {
  const int tid = threadIdx.x;
  const int L = xcd_remap(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                          gridDim.x * gridDim.y * gridDim.z);
  const int tpf = gridDim.x * gridDim.y, b = L / tpf, tyi = (L - b * tpf) / gridDim.x;
  const int tx0 = (L - b * tpf - tyi * gridDim.x) * 32 - 8, ty0 = tyi * 32 - 8;
  const uint8_t* R = ref.plane(0, b, g);
  // raw[rr] dword w = samples (tx0 - 4 + 4w .. +3, ty0 - 3 + rr), clamped, biased to int8
  __shared__ uint32_t raw[39][kPhW];
  // hf[fx-1][rr][c]: horizontal filter fx at (tx0 + c, ty0 - 3 + rr)
  __shared__ __align__(16) int16_t hf[3][39][32];
  for (int i = tid; i < 39 * kPhW; i += 256) {
    const int rr = i / kPhW, w = i - rr * kPhW;
    const uint8_t* row = R + (long)clip3(0, g.H - 1, ty0 - 3 + rr) * g.W;
    const int x = tx0 - 4 + 4 * w;
    uint32_t v;
    if (x >= 0 && x + 3 < g.W) {
      v = *reinterpret_cast<const uint32_t*>(row + x);  // x is 4-aligned (tx0 = 32k - 8)
    } else {
      v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= (uint32_t)row[clip3(0, g.W - 1, x + k)] << (8 * k);
    }
    raw[rr][w] = v ^ 0x80808080u;
  }
  __syncthreads();
  // horizontal pass: item = (row, 4 output columns), the 3 fractional filters at once
  for (int i = tid; i < 39 * 8; i += 256) {
    const int rr = i >> 3, c4 = i & 7;
    // column c = 4*c4 + j takes bytes c+1 .. c+8 of the row (taps at x-3 .. x+4)
    const uint32_t w0 = raw[rr][c4], w1 = raw[rr][c4 + 1], w2 = raw[rr][c4 + 2];
    int out[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = j == 3 ? w1 : __builtin_amdgcn_alignbyte(w1, w0, j + 1);
      const uint32_t hi = j == 3 ? w2 : __builtin_amdgcn_alignbyte(w2, w1, j + 1);
#pragma unroll
      for (int f = 1; f < 4; ++f) out[f - 1][j] = dot4(lo, pack_taps4(f, 0), dot4(hi, pack_taps4(f, 4), 8192));
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      uint2 v;
      v.x = (uint32_t)(uint16_t)out[f][0] | (uint32_t)out[f][1] << 16;
      v.y = (uint32_t)(uint16_t)out[f][2] | (uint32_t)out[f][3] << 16;
      *reinterpret_cast<uint2*>(&hf[f][rr][4 * c4]) = v;
    }
  }
  __syncthreads();
  const int r = tid >> 3, c0 = (tid & 7) * 4;
  const int X = tx0 + c0, Y = ty0 + r;
  if (X + 8 >= g.pw16 || Y >= g.H + 8) return;
  uint8_t* base = phase + (long)b * 16 * g.psz + (long)(Y + 8) * g.pw16 + (X + 8);
  auto store = [&](int plane, uint32_t w) { *reinterpret_cast<uint32_t*>(base + (long)plane * g.psz) = w; };
  // ---- fx = 0: integer column, rows Y-3 .. Y+4 = raw rows r .. r+7, word c0/4 + 1
  {
    uint32_t R8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) R8[k] = raw[r + k][(c0 >> 2) + 1];
    store(0, R8[3] ^ 0x80808080u);
    uint32_t C[2][4];  // C[h][j]: column j, rows 4h .. 4h+3 (one byte each)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t* q = R8 + 4 * h;
      const uint32_t t01l = __builtin_amdgcn_perm(q[1], q[0], 0x05010400u);
      const uint32_t t01h = __builtin_amdgcn_perm(q[1], q[0], 0x07030602u);
      const uint32_t t23l = __builtin_amdgcn_perm(q[3], q[2], 0x05010400u);
      const uint32_t t23h = __builtin_amdgcn_perm(q[3], q[2], 0x07030602u);
      C[h][0] = __builtin_amdgcn_perm(t23l, t01l, 0x05040100u);
      C[h][1] = __builtin_amdgcn_perm(t23l, t01l, 0x07060302u);
      C[h][2] = __builtin_amdgcn_perm(t23h, t01h, 0x05040100u);
      C[h][3] = __builtin_amdgcn_perm(t23h, t01h, 0x07060302u);
    }
#pragma unroll
    for (int fy = 1; fy < 4; ++fy) {
      int v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[j] = dot4(C[0][j], pack_taps4(fy, 0), dot4(C[1][j], pack_taps4(fy, 4), 8192 + 32)) >> 6;  // rounding folded in
      store(4 * fy, pack4_pixels(v[0], v[1], v[2], v[3]));
    }
  }
  // ---- fx = 1..3: vertical over the int16 intermediates, row pairs packed for v_dot2
#pragma unroll
  for (int fx = 1; fx < 4; ++fx) {
    uint2 H8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) H8[k] = *reinterpret_cast<const uint2*>(&hf[fx - 1][r + k][c0]);
    {
      const int h0 = (int16_t)(H8[3].x & 0xffff), h1 = (int16_t)(H8[3].x >> 16);
      const int h2 = (int16_t)(H8[3].y & 0xffff), h3 = (int16_t)(H8[3].y >> 16);
      store(fx, pack4_pixels((h0 + 32) >> 6, (h1 + 32) >> 6, (h2 + 32) >> 6, (h3 + 32) >> 6));
    }
    uint32_t P[4][4];  // P[m][j]: column j, rows 2m (low half) and 2m + 1 (high half)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      P[m][0] = __builtin_amdgcn_perm(H8[2 * m + 1].x, H8[2 * m].x, 0x05040100u);
      P[m][1] = __builtin_amdgcn_perm(H8[2 * m + 1].x, H8[2 * m].x, 0x07060302u);
      P[m][2] = __builtin_amdgcn_perm(H8[2 * m + 1].y, H8[2 * m].y, 0x05040100u);
      P[m][3] = __builtin_amdgcn_perm(H8[2 * m + 1].y, H8[2 * m].y, 0x07060302u);
    }
#pragma unroll
    for (int fy = 1; fy < 4; ++fy) {
      int v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int a = dot2(P[0][j], pack_taps2(fy, 0), 0);
        a = dot2(P[1][j], pack_taps2(fy, 2), a);
        a = dot2(P[2][j], pack_taps2(fy, 4), a);
        a = dot2(P[3][j], pack_taps2(fy, 6), a);
        v[j] = ((a >> 6) + 32) >> 6;
      }
      store(fx + 4 * fy, pack4_pixels(v[0], v[1], v[2], v[3]));
    }
  }
}

// ------------------------------------ deblocking ----------------------------------------
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) k_deblock(FrameSet rec, DecisionSet dec, Geo g, int horizontal) {
  const int b = blockIdx.y;
  const int qp = dec.qp[b];
  const long ub = b * g.usz;
  const uint8_t* cl = dec.cu_log2 + ub;
  const uint8_t* in = dec.intra + ub;
  const uint8_t* cb = dec.cbf + ub;
  const int16_t* mv = dec.mv + 2 * ub;
  const uint8_t* dir = dec.dir ? dec.dir + ub : nullptr;  // B pictures
  const int16_t* mv1 = dec.mv1 ? dec.mv1 + 2 * ub : nullptr;
  const uint8_t* tu = dec.tu ? dec.tu + ub : nullptr;  // RQT-split 32x32 CUs (P pictures)
  uint8_t* Y = rec.plane(0, b, g);
  uint8_t* U = rec.plane(1, b, g);
  uint8_t* V = rec.plane(2, b, g);
  const int W = g.W, H = g.H, Wc = W / 2;
  const int qpc = chroma_qp(qp, 0);
  const int nl = horizontal ? (H / 8 - 1) * (W / 4) : (W / 8 - 1) * (H / 4);
  const int nc = horizontal ? (H / 16 - 1) * (Wc / 4) : (W / 16 - 1) * (H / 8);
  // Each item's samples are moved as aligned dwords into registers (a vertical edge: the
  // 8 bytes x-4..x+3 of each of its 4 lines; a horizontal edge: 8 rows x the segment's 4
  // columns), filtered there by the shared tv::deblock_* functions and written back the same
  // way: 8 dword loads per luma segment instead of 32 byte loads.  Items of a pass never
  // share a dword (edges are 8 samples apart), so the write-back of unchanged bytes is safe.
  auto ld = [](const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); };
  auto st = [](uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; };
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nl + nc; i += gridDim.x * blockDim.x) {
    if (i < nl) {
      if (!horizontal) {
        const int x = 8 * (1 + i % (W / 8 - 1)), y = 4 * (i / (W / 8 - 1));
        const int bs = deblock_edge_bs(cl, in, cb, mv, g.w8, x - 1, y, x, y, dir, mv1, tu);
        if (bs) {
          uint32_t v[4][2];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            v[k][0] = ld(Y + (long)(y + k) * W + x - 4);
            v[k][1] = ld(Y + (long)(y + k) * W + x);
          }
          deblock_luma_edge4(reinterpret_cast<uint8_t*>(&v[0][1]), 1, 8, bs, qp);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            st(Y + (long)(y + k) * W + x - 4, v[k][0]);
            st(Y + (long)(y + k) * W + x, v[k][1]);
          }
        }
      } else {
        const int y = 8 * (1 + i % (H / 8 - 1)), x = 4 * (i / (H / 8 - 1));
        const int bs = deblock_edge_bs(cl, in, cb, mv, g.w8, x, y - 1, x, y, dir, mv1, tu);
        if (bs) {
          uint32_t v[8];  // rows y-4 .. y+3, columns x .. x+3
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = ld(Y + (long)(y - 4 + r) * W + x);
          deblock_luma_edge4(reinterpret_cast<uint8_t*>(&v[4]), 4, 1, bs, qp);
#pragma unroll
          for (int r = 1; r < 7; ++r) st(Y + (long)(y - 4 + r) * W + x, v[r]);  // rows p2..q2
        }
      }
    } else {
      const int j = i - nl;
      if (!horizontal) {
        const int xc = 8 * (1 + j % (W / 16 - 1)), yc = 4 * (j / (W / 16 - 1));
        const int bs = deblock_edge_bs(cl, in, cb, mv, g.w8, 2 * xc - 1, 2 * yc, 2 * xc, 2 * yc, dir, mv1, tu);
        if (bs == 2) {
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) {
            uint8_t* P = pl ? V : U;
            uint32_t v[4][2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              v[k][0] = ld(P + (long)(yc + k) * Wc + xc - 4);
              v[k][1] = ld(P + (long)(yc + k) * Wc + xc);
            }
            deblock_chroma_edge(reinterpret_cast<uint8_t*>(&v[0][1]), 1, 8, 4, qpc);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              st(P + (long)(yc + k) * Wc + xc - 4, v[k][0]);
              st(P + (long)(yc + k) * Wc + xc, v[k][1]);
            }
          }
        }
      } else {
        const int yc = 8 * (1 + j % (H / 16 - 1)), xc = 4 * (j / (H / 16 - 1));
        const int bs = deblock_edge_bs(cl, in, cb, mv, g.w8, 2 * xc, 2 * yc - 1, 2 * xc, 2 * yc, dir, mv1, tu);
        if (bs == 2) {
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) {
            uint8_t* P = pl ? V : U;
            uint32_t v[4];  // rows yc-2 .. yc+1
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = ld(P + (long)(yc - 2 + r) * Wc + xc);
            deblock_chroma_edge(reinterpret_cast<uint8_t*>(&v[2]), 4, 1, 4, qpc);
            st(P + (long)(yc - 1) * Wc + xc, v[1]);
            st(P + (long)yc * Wc + xc, v[2]);
          }
        }
      }
    }
  }
}

// ------------------------------------ launchers -----------------------------------------
// The frame contexts travel as kernel arguments (the QpArgs precedent below): the objects
// depend on (seed, W, H) only, a segment adds its frame time and the objects' positions.
void launch_synth(FrameSet src, const Geo& g, uint32_t seed, const FrameIdx& fi, int B, hipStream_t s) {
  SynthArgs a;
  std::memset(&a, 0, sizeof a);
  SynthFrameCtx f;
  for (int b = 0; b < B; ++b) {
    synth_frame_ctx(seed, fi.t[b], g.dw, g.dh, f);
    a.t[b] = f.t;
    std::memcpy(a.ox[b], f.ox, sizeof f.ox);
    std::memcpy(a.oy[b], f.oy, sizeof f.oy);
  }
  if (B > 0) std::memcpy(a.obj, f.obj, sizeof f.obj);
  auto tiles = [](int w, int h) { return ((w + kSynTW - 1) / kSynTW) * ((h + kSynTH - 1) / kSynTH); };
  dim3 grid((unsigned)(tiles(g.W, g.H) + 2 * tiles(g.W / 2, g.H / 2)), (unsigned)B);
  if (synth_textured(seed))
    k_synth<true><<<grid, 256, 0, s>>>(src, g, seed, a);
  else
    k_synth<false><<<grid, 256, 0, s>>>(src, g, seed, a);
}
// One picture of B device-resident segments ([segment][frame][Y | U | V] at the coded size,
// segment stride seg_stride bytes) into the B source planes: one launch instead of 3 B
// copyBuffer blits in front of every picture's analysis (the node job's file sources).
__global__ void __launch_bounds__(256) k_gather_frames(const uint8_t* frames, long seg_stride, FrameSet src, Geo g,
                                                       int B) {
  const long f16 = (g.ysz + 2 * g.csz) / 16, y16 = g.ysz / 16, c16 = g.csz / 16;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < B * f16; i += (long)gridDim.x * 256) {
    const int b = (int)(i / f16);
    const long r = i - b * f16;
    const uint4 v = reinterpret_cast<const uint4*>(frames + b * seg_stride)[r];
    uint4* d = r < y16 ? reinterpret_cast<uint4*>(src.y + b * g.ysz) + r
               : r < y16 + c16 ? reinterpret_cast<uint4*>(src.u + b * g.csz) + (r - y16)
                               : reinterpret_cast<uint4*>(src.v + b * g.csz) + (r - y16 - c16);
    *d = v;
  }
}
void launch_gather_frames(const uint8_t* frames, long seg_stride, FrameSet src, const Geo& g, int B, hipStream_t s) {
  const long n = B * (g.ysz + 2 * g.csz) / 16;
  k_gather_frames<<<(unsigned)tv_min(4096L, (n + 255) / 256), 256, 0, s>>>(frames, seg_stride, src, g, B);
}
// Per-frame slice QPs into the device slot: the values travel as kernel arguments (64 per
// launch) instead of a pinned-host -> device hipMemcpyAsync, which this runtime runs as a
// blit kernel that reads host memory over PCIe (~77 us per picture in the kernel trace).
struct QpArgs {
  int8_t q[64];
};
__global__ void __launch_bounds__(64) k_set_qp(int8_t* dst, QpArgs a, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = a.q[threadIdx.x];
}
void launch_set_qp(int8_t* dst, const int8_t* host, int n, hipStream_t s) {
  for (int o = 0; o < n; o += 64) {
    QpArgs a;
    const int m = n - o < 64 ? n - o : 64;
    std::memcpy(a.q, host + o, (size_t)m);
    k_set_qp<<<1, 64, 0, s>>>(dst + o, a, m);
  }
}

void launch_sse(FrameSet a, FrameSet r, const Geo& g, unsigned long long* sse, int B, hipStream_t s) {
  dim3 grid((unsigned)tv_min(256, (int)((g.ysz / 4 + 4095) / 4096)), 3, B);
  k_sse<<<grid, 256, 0, s>>>(a, r, g, sse);
}
void launch_phase_planes(FrameSet ref, uint8_t* phase, const Geo& g, int B, hipStream_t s) {
  dim3 grid((g.W + 16 + 31) / 32, (g.H + 16 + 31) / 32, B);
  k_phase_planes<<<grid, 256, 0, s>>>(ref, phase, g);
}
// ---------------------------------------- SAO ------------------------------------------
// One workgroup per strip of kSaoStrip horizontally adjacent CTBs, one wave per CTB:
// statistics -> integer RD decision -> the SAO'd CTB, in one launch.  The deblocked strip of
// every component plus a one-sample ring is staged once in LDS as int16 pairs (-1 marks
// samples outside the picture; every global load of a wave's rows is issued before its first
// store), so the EO neighbour reads of both the statistics and the filter never touch global
// memory, and the filtered CTB is written straight from the tile.  After the staging barrier
// a wave works alone on its CTB, all three components:
//   * statistics: a lane keeps one pair column and walks down consecutive rows (luma 16 pair
//     columns x 4 groups of 8 rows; chroma Cb | Cr on the 32-lane halves, 8 pair columns x 4
//     groups of 4 rows), each tile row read once, the vertical sign of a row reused negated
//     by the next; 4 classes x 4 packed 16-bit accumulators per component;
//   * one transpose-reduce per component leaves every counter on the lanes that run
//     tv::sao_best_offset for it; class sums, the luma argmin and the joint Cb + Cr argmin
//     (the order of tv::sao_finish_pos) with DPP row sums and scalar compares;
//   * the filter takes the parameters from SGPRs, a straight-line body per EO class.
// Waves of a partial strip whose CTB lies beyond the picture only stage and meet the barriers.
// The display-area squared error is summed per wave, combined in LDS, one global atomic per
// component and strip.
constexpr int kSaoStrip = 4;                    // CTBs (= waves) per workgroup
constexpr int kSaoRows = 34, kSaoRowsC = 18;    // tile rows with the ring
// Tile rows in dwords (one int16 pair each): sample x of the strip sits at int16 index x + 2,
// so a pair (even x, x + 1) is one aligned dword and the ring columns -1 / 32 S are the odd /
// even half of the first / last dword.  Pitch % 32 = 2: the row groups of a 32-lane half land
// on disjoint banks (luma 16 rg + p, chroma 8 rg + p).
constexpr int kSaoPd = 16 * kSaoStrip + 2, kSaoPdC = 8 * kSaoStrip + 2;
constexpr int kSaoLumaDw = kSaoRows * kSaoPd, kSaoChromaDw = kSaoRowsC * kSaoPdC;
constexpr int kSaoTileDw = kSaoLumaDw + 2 * kSaoChromaDw;
constexpr int kSaoSrcDw = 8 * kSaoStrip + 2, kSaoSrcDwC = 4 * kSaoStrip + 2;  // plane dwords per tile row
static_assert(kSaoSrcDw <= 64 && kSaoSrcDwC <= 32, "a tile row is staged by one wave (chroma: one half per plane)");
static_assert(8 * (kSaoTileDw * 4 + 64) <= 160 * 1024, "8 workgroups per CU");
typedef short sao_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sao_s2 sao_pair(uint32_t w) { return __builtin_bit_cast(sao_s2, w); }
typedef unsigned short sao_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sao_u2 sao_upair(sao_s2 w) { return __builtin_bit_cast(sao_u2, w); }
// per half: -1, 0, 1 for |d| < 2^15 -- shifts and an OR (v_pk_ashrrev / v_pk_lshrrev), no
// compares: (d >> 15) is -1 for d < 0, ((-d) >>> 15) is 1 for d > 0
__device__ __forceinline__ sao_s2 sao_sign2(sao_s2 d) {
  const sao_s2 z = {0, 0};
  const sao_u2 f = {15, 15};
  return (d >> 15) | __builtin_bit_cast(sao_s2, __builtin_bit_cast(sao_u2, z - d) >> f);
}
__device__ __forceinline__ sao_s2 sao_relu2(sao_s2 e) { return e & ~(e >> 15); }  // max(e, 0)
// v_pk_max_i16 / v_pk_min_i16 (clang lowers a packed clamp to -1..1 as a sign idiom of
// per-half compares and selects, so these are spelled out)
__device__ __forceinline__ sao_s2 sao_pkmax(sao_s2 a, sao_s2 b) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, a)), "v"(__builtin_bit_cast(uint32_t, b)));
  return sao_pair(r);
}
__device__ __forceinline__ sao_s2 sao_pkmin(sao_s2 a, sao_s2 b) {
  uint32_t r;
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, a)), "v"(__builtin_bit_cast(uint32_t, b)));
  return sao_pair(r);
}
__device__ __forceinline__ sao_s2 sao_clamp1(sao_s2 d) {  // per half: sign of d
  return sao_pkmin(sao_pkmax(d, sao_s2{-1, -1}), sao_s2{1, 1});
}

// EO statistics of ROWS consecutive rows of one pair column.  t: the pair's dword in the tile
// row above the first (tile pitch PD dwords); sp[r]: the two source bytes of row r.  Row r's
// pair and its neighbours one sample to the left / right come from three dwords; the rows
// move down a register window, so every tile row is read once.  Classes (sao_eo_dir): 0
// horizontal, 1 vertical, 2 135 degrees, 3 45 degrees; e = sign(v - a) + sign(v - b) per half.
// The vertical sign against the row below is the next row's sign against the row above,
// negated.  MASK (CTBs on the picture border): e = 0 where a class neighbour is outside (-1).
// Per class four accumulators of w = 16 (orig - v) + 1 per half, in wrapping 16-bit
// arithmetic: w [e = -2], w |e| over e < 0, w e over e > 0, w [e = 2]; sao_counters takes
// the categories e = -1 / e = 1 out of the middle two.
template <bool MASK, int ROWS, int PD>
__device__ __forceinline__ void sao_walk(const uint32_t* t, const uint32_t (&sp)[ROWS], sao_u2 (&acc)[4][4]) {
  sao_s2 L0, C0, R0, L1, C1, R1, L2, C2, R2;
  auto row = [&](int r, sao_s2& L, sao_s2& C, sao_s2& R) {
    const uint32_t Pv = t[r * PD - 1], Cv = t[r * PD], Nv = t[r * PD + 1];
    L = sao_pair(__builtin_amdgcn_alignbyte(Cv, Pv, 2));  // samples (x - 1, x)
    R = sao_pair(__builtin_amdgcn_alignbyte(Nv, Cv, 2));  // samples (x + 1, x + 2)
    C = sao_pair(Cv);
  };
  row(0, L0, C0, R0);
  row(1, L1, C1, R1);
  const sao_s2 zero = {0, 0}, one = {1, 1}, sixteen = {16, 16};
  const sao_u2 uone = {1, 1};
  sao_s2 pdn = sao_clamp1(C0 - C1);  // sign(row above - row): what the row above saw downwards
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    row(r + 2, L2, C2, R2);
    const sao_s2 v = C1;
    const sao_s2 orig = sao_pair(__builtin_amdgcn_perm(0u, sp[r], 0x0c010c00u));
    const sao_u2 w = sao_upair((orig - v) * sixteen + one);
    const sao_s2 dn = sao_clamp1(v - C2);
    sao_s2 e[4] = {sao_clamp1(v - L1) + sao_clamp1(v - R1), dn - pdn, sao_clamp1(v - L0) + sao_clamp1(v - R2),
                   sao_clamp1(v - R0) + sao_clamp1(v - L2)};
    pdn = dn;
    if (MASK) {  // samples are >= -1: min(a, b, 0) + 1 is 0 where a neighbour is outside, else 1
      e[0] *= sao_pkmin(sao_pkmin(L1, R1), zero) + one;
      e[1] *= sao_pkmin(sao_pkmin(C0, C2), zero) + one;
      e[2] *= sao_pkmin(sao_pkmin(L0, R2), zero) + one;
      e[3] *= sao_pkmin(sao_pkmin(R0, L2), zero) + one;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const sao_s2 pos = sao_pkmax(e[d], zero), neg = pos - e[d];
      const sao_u2 up = sao_upair(pos), un = sao_upair(neg);
      acc[d][0] += w * (un >> uone);
      acc[d][1] += w * un;
      acc[d][2] += w * up;
      acc[d][3] += w * (up >> uone);
    }
    L0 = L1, C0 = C1, R0 = R1;
    L1 = L2, C1 = C2, R1 = R2;
  }
}
// The lane's 16 counters (class d, category q + 1 at 4 d + q) as sum * 2048 + count, the
// format of the wave reduction.  Per half an accumulator is 16 sum + count with count <= 8
// (its low 4 bits, |16 sum + count| < 2^15): sum * 2048 + count = 128 (16 sum + count) - 127 count.
__device__ __forceinline__ void sao_counters(const sao_u2 (&acc)[4][4], int (&t)[16]) {
  const sao_u2 two = {2, 2};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const sao_u2 x[4] = {acc[d][0], acc[d][1] - two * acc[d][0], acc[d][2] - two * acc[d][3], acc[d][3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t xv = __builtin_bit_cast(uint32_t, x[q]);
      const int cn = __builtin_amdgcn_sdot2(sao_pair(xv & 0x000F000Fu), sao_s2{-127, -127}, 0, false);
      t[4 * d + q] = __builtin_amdgcn_sdot2(sao_pair(xv), sao_s2{128, 128}, cn, false);
    }
  }
}
// The 16 counters of the wave in one transpose-reduce: each exchange step (lanes 32, 16, 8,
// 4 apart) halves the values a lane holds -- it keeps one half and adds the partner's copy
// of it -- and DPP quad adds finish the sum.  Lanes 32 / 16 apart swap with
// v_permlane32_swap / v_permlane16_swap (gfx950), lanes 8 apart with a DPP row rotate; the
// halves are chosen with xor masks, not selects (a select of two array elements became a
// dynamically indexed array).  Whole wave: lane L ends with counter L >> 2.  HALF: the two
// 32-lane halves are reduced apart (Cb | Cr, one more step 2 lanes apart): lane L ends with
// counter (L & 31) >> 1 of its half.  Full wave only (no DPP in a divergent branch).
template <bool HALF>
__device__ __forceinline__ int sao_reduce16(int (&t)[16], int lane) {
  if (!HALF) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // lanes 0-31 keep t[j], lanes 32-63 t[j + 8]
      const auto r = __builtin_amdgcn_permlane32_swap((unsigned)t[j], (unsigned)t[j + 8], false, false);
      t[j] = (int)(r[0] + r[1]);
    }
  }
  constexpr int n16 = HALF ? 8 : 4, n8 = n16 / 2, n4 = n8 / 2;
#pragma unroll
  for (int j = 0; j < n16; ++j) {  // even 16-lane rows keep t[j], odd rows t[j + n16]
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)t[j], (unsigned)t[j + n16], false, false);
    t[j] = (int)(r[0] + r[1]);
  }
  const int m8 = -((lane >> 3) & 1), m4 = -((lane >> 2) & 1), m2 = -((lane >> 1) & 1);
#pragma unroll
  for (int j = 0; j < n8; ++j) {
    const int x = (t[j] ^ t[j + n8]) & m8;
    t[j] = (t[j] ^ x) + dpp::mov<dpp::kRowRor8>(t[j + n8] ^ x);
  }
#pragma unroll
  for (int j = 0; j < n4; ++j) {
    const int x = (t[j] ^ t[j + n4]) & m4;
    t[j] = (t[j] ^ x) + __shfl_xor(t[j + n4] ^ x, 4, 64);
  }
  int tot;
  if (HALF) {
    const int x = (t[0] ^ t[1]) & m2;
    tot = (t[0] ^ x) + dpp::mov<dpp::kQuadXor2>(t[1] ^ x);
  } else {
    tot = t[0];
    tot += dpp::mov<dpp::kQuadXor2>(tot);
  }
  tot += dpp::mov<dpp::kQuadXor1>(tot);
  return tot;
}
template <int CTRL>
__device__ __forceinline__ long long sao_dpp_add64(long long v) {
  const unsigned lo = (unsigned)dpp::mov<CTRL>((int)v), hi = (unsigned)dpp::mov<CTRL>((int)(v >> 32));
  return v + (long long)((unsigned long long)hi << 32 | lo);
}
__device__ __forceinline__ long long sao_readlane64(long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
  return (long long)((unsigned long long)hi << 32 | lo);
}

// One dword (4 samples) of an EO-filtered component: the tile pairs at dwords i0, i0 + 1 and
// the class neighbours (a +-1 column shift is a v_alignbyte of two pairs); the category index
// e + 2 of both halves selects the biased offsets with one v_perm.  Neighbours outside the
// picture (-1) leave the sample as is.
template <int S>
__device__ __forceinline__ uint32_t sao_shifted(const uint32_t (&W)[4], int k) {  // pair k shifted by S columns
  if constexpr (S == 0) return W[k + 1];
  if constexpr (S < 0) return __builtin_amdgcn_alignbyte(W[k + 1], W[k], 2);
  if constexpr (S > 0) return __builtin_amdgcn_alignbyte(W[k + 2], W[k + 1], 2);
}
template <int CLS, int PD>
__device__ __forceinline__ uint32_t sao_eo_dword(const uint32_t* t, int i0, uint32_t p) {
  constexpr int dx = CLS == 1 ? 0 : (CLS == 3 ? 1 : -1), dy = CLS == 0 ? 0 : -1;  // sao_eo_dir
  const int ra = i0 + dy * PD, rb = i0 - dy * PD;
  const uint32_t Wa[4] = {t[ra - 1], t[ra], t[ra + 1], t[ra + 2]};
  const uint32_t Wb[4] = {t[rb - 1], t[rb], t[rb + 1], t[rb + 2]};
  const uint32_t Cv[2] = {t[i0], t[i0 + 1]};
  // biased offsets (o + 8) by category index e + 2: bytes {o0, o1, 8 (none), o2 | o3}
  const uint32_t t0 = ((p >> 7) & 15) | ((p >> 11) & 15) << 8 | 8u << 16 | ((p >> 15) & 15) << 24;
  const uint32_t t1 = (p >> 19) & 15;
  const sao_s2 two = {2, 2}, eight = {8, 8};
  const sao_u2 u8s = {8, 8};
  uint32_t r2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const sao_s2 v = sao_pair(Cv[k]);
    const sao_s2 A = sao_pair(sao_shifted<dx>(Wa, k)), B = sao_pair(sao_shifted<-dx>(Wb, k));
    const sao_s2 inv = (A | B) >> 15;  // -1 where a neighbour is outside the picture
    const sao_s2 e = (sao_sign2(v - A) + sao_sign2(v - B)) & ~inv;
    const uint32_t sel = __builtin_bit_cast(uint32_t, e + two) | 0x0c000c00u;
    const sao_s2 off = sao_pair(__builtin_amdgcn_perm(t1, t0, sel));
    const sao_s2 r = sao_relu2(v + off - eight);  // -7 .. 262 -> 0 .. 262
    // >= 256 -> low byte 0xFF (only the low byte of each half is kept)
    r2[k] = __builtin_bit_cast(uint32_t, r | (sao_s2{0, 0} - __builtin_bit_cast(sao_s2, __builtin_bit_cast(sao_u2, r) >> u8s)));
  }
  return __builtin_amdgcn_perm(r2[1], r2[0], 0x06040200u);
}
// p is wave-uniform: the type and class tests are scalar branches
template <int PD>
__device__ __forceinline__ uint32_t sao_filter_dword(const uint32_t* t, int i0, uint32_t p) {
  static_assert(!kSaoBandOffsets, "the SAO filter has no band-offset path");
  if (sao_type(p) == 2) {
    switch (sao_class(p)) {
      case 0: return sao_eo_dword<0, PD>(t, i0, p);
      case 1: return sao_eo_dword<1, PD>(t, i0, p);
      case 2: return sao_eo_dword<2, PD>(t, i0, p);
      default: return sao_eo_dword<3, PD>(t, i0, p);
    }
  }
  return __builtin_amdgcn_perm(t[i0 + 1], t[i0], 0x06040200u);
}
// squared error of a dword against the source over the display columns (x0 .. x0 + 3 < dwc)
__device__ __forceinline__ unsigned sao_sse_dword(uint32_t sw, uint32_t word, int x0, int dwc) {
  unsigned e2 = 0;
  if (x0 + 4 <= dwc) {  // the whole dword is in the display area
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t sel = h ? 0x0c030c02u : 0x0c010c00u;
      const sao_s2 d = sao_pair(__builtin_amdgcn_perm(0u, sw, sel)) - sao_pair(__builtin_amdgcn_perm(0u, word, sel));
      const sao_u2 dd = __builtin_bit_cast(sao_u2, d * d);  // <= 65025 per half
      e2 = __builtin_amdgcn_udot2(dd, sao_u2{1, 1}, e2, false);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = (int)((sw >> (8 * q)) & 255) - (int)((word >> (8 * q)) & 255);
      e2 += x0 + q < dwc ? (unsigned)(d * d) : 0u;
    }
  }
  return e2;
}

// 8 workgroups per CU (8 waves per SIMD): 64 VGPRs, no scratch; the tile is 13.9 KB of LDS.
__global__ void __launch_bounds__(64 * kSaoStrip, 8) k_sao_decide(FrameSet src, FrameSet deb, FrameSet out, uint32_t* sao,
                                                               Geo g, const int8_t* qp, const RcTables* rc,
                                                               unsigned long long* sse) {
  static_assert(!kSaoBandOffsets, "the statistics carry no band histogram, the decision no band window or argmin");
  constexpr int S = kSaoStrip;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar CTB logic
  int strip, b;
  xcd_ctb(strip, b);
  const int spr = (g.wc + S - 1) / S;  // strips per CTB row
  const int sx = strip % spr, cy = strip / spr, cx = sx * S + wave;
  const bool active = cx < g.wc;
  const long long lam16 = rc->sao_lam16[qp[b]];
  __shared__ __align__(16) uint32_t tile[kSaoTileDw];  // luma 34 rows, then Cb, Cr 18 rows each
  __shared__ unsigned long long esum[3];
  if (tid < 3) esum[tid] = 0;
  const int cw = g.W / 2;
  // statistics lanes: luma pair column p of row group rg (8 rows); chroma plane cp, 4 rows
  const int rgY = lane >> 4, pY = lane & 15;
  const int cp = lane >> 5, rgC = (lane >> 3) & 3, pC = lane & 7;
  uint32_t spY[8];
  {  // the deblocked strip + ring: wave w stages tile rows w, w + S, ...; a lane takes one plane
     // dword of the row (luma: lane, chroma: Cb | Cr on the 32-lane halves), so the row base
     // is a scalar.  A CTB edge is a multiple of 4: a dword is wholly inside or wholly
     // outside the plane.  Plane dword d of a row covers strip samples 4d - 4 .. 4d - 1 and
     // lands as two int16 pairs (v_perm) in tile dwords 2d - 1 and 2d; the first plane dword
     // has only its second pair in the tile, the last only its first.
    constexpr int nY = (kSaoRows + S - 1) / S, nC = (kSaoRowsC + S - 1) / S;
    uint32_t vy[nY], vc[nC];
    bool iy[nY], ic[nC];
    const int dY = lane, xY = sx * (32 * S) - 4 + 4 * dY;
    const bool colY = dY < kSaoSrcDw && xY >= 0 && xY < g.W;
    const uint8_t* PY = deb.plane(0, b, g);
#pragma unroll
    for (int i = 0; i < nY; ++i) {
      const int row = wave + S * i, y = cy * 32 - 1 + row;
      iy[i] = colY && row < kSaoRows && y >= 0 && y < g.H;
      vy[i] = iy[i] ? *reinterpret_cast<const uint32_t*>(PY + (long)y * g.W + xY) : 0u;
    }
    const int dC = lane & 31, xC = sx * (16 * S) - 4 + 4 * dC;
    const bool colC = dC < kSaoSrcDwC && xC >= 0 && xC < cw;
    const uint8_t* PC = deb.plane(1 + cp, b, g);
#pragma unroll
    for (int i = 0; i < nC; ++i) {
      const int row = wave + S * i, y = cy * 16 - 1 + row;
      ic[i] = colC && row < kSaoRowsC && y >= 0 && y < g.H / 2;
      vc[i] = ic[i] ? *reinterpret_cast<const uint32_t*>(PC + (long)y * cw + xC) : 0u;
    }
    // source pairs of this lane's luma statistics rows, in flight over the staging
    const uint8_t* SY = src.plane(0, b, g) + (long)(cy * 32 + 8 * rgY) * g.W + cx * 32 + 2 * pY;
#pragma unroll
    for (int r = 0; r < 8; ++r) spY[r] = active ? *reinterpret_cast<const uint16_t*>(SY + r * g.W) : 0u;
#pragma unroll
    for (int i = 0; i < nY; ++i) {
      const int row = wave + S * i;
      if (row >= kSaoRows || dY >= kSaoSrcDw) continue;
      const uint32_t lo = iy[i] ? __builtin_amdgcn_perm(0u, vy[i], 0x0c010c00u) : 0xFFFFFFFFu;  // outside: -1 pairs
      const uint32_t hi = iy[i] ? __builtin_amdgcn_perm(0u, vy[i], 0x0c030c02u) : 0xFFFFFFFFu;
      uint32_t* T = tile + row * kSaoPd + 2 * dY;
      if (dY >= 1) T[-1] = lo;
      if (dY < kSaoSrcDw - 1) T[0] = hi;
    }
#pragma unroll
    for (int i = 0; i < nC; ++i) {
      const int row = wave + S * i;
      if (row >= kSaoRowsC || dC >= kSaoSrcDwC) continue;
      const uint32_t lo = ic[i] ? __builtin_amdgcn_perm(0u, vc[i], 0x0c010c00u) : 0xFFFFFFFFu;
      const uint32_t hi = ic[i] ? __builtin_amdgcn_perm(0u, vc[i], 0x0c030c02u) : 0xFFFFFFFFu;
      uint32_t* T = tile + kSaoLumaDw + cp * kSaoChromaDw + row * kSaoPdC + 2 * dC;
      if (dC >= 1) T[-1] = lo;
      if (dC < kSaoSrcDwC - 1) T[0] = hi;
    }
  }
  __syncthreads();
  unsigned e2[3] = {0, 0, 0};
  if (active) {  // wave-uniform: the whole wave is in, the DPP and permlane steps below are safe
    // A CTB away from the picture edge has no outside (-1) neighbours and skips the masks.
    const bool interior = cx > 0 && cy > 0 && cx < g.wc - 1 && cy < g.hc - 1;
    const uint32_t* tY = tile + wave * 16 + 1;                  // dword of the CTB's sample 0 in tile row 0
    const uint32_t* tC0 = tile + kSaoLumaDw + wave * 8 + 1;     // the same of Cb; Cr + kSaoChromaDw
    int totY, totC;
    {
      sao_u2 acc[4][4];
      int t[16];
      uint32_t spC[4];
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[d][q] = sao_u2{0, 0};
      const uint32_t* tp = tY + 8 * rgY * kSaoPd + pY;
      if (interior)
        sao_walk<false, 8, kSaoPd>(tp, spY, acc);
      else
        sao_walk<true, 8, kSaoPd>(tp, spY, acc);
      sao_counters(acc, t);
      totY = sao_reduce16<false>(t, lane);
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[d][q] = sao_u2{0, 0};
      tp = tC0 + cp * kSaoChromaDw + 4 * rgC * kSaoPdC + pC;
      const uint8_t* SC = src.plane(1 + cp, b, g) + (long)(cy * 16 + 4 * rgC) * cw + cx * 16 + 2 * pC;
#pragma unroll
      for (int r = 0; r < 4; ++r) spC[r] = *reinterpret_cast<const uint16_t*>(SC + r * cw);
      if (interior)
        sao_walk<false, 4, kSaoPdC>(tp, spC, acc);
      else
        sao_walk<true, 4, kSaoPdC>(tp, spC, acc);
      sao_counters(acc, t);
      totC = sao_reduce16<true>(t, lane);
    }
    // The 48 items of the CTB at once: even lanes the luma counter lane >> 2, odd lanes the
    // counter (lane & 31) >> 1 of Cb (lanes < 32) / Cr; class k >> 2, category (k & 3) + 1.
    uint32_t prm[3];
    {
      const bool chroma = lane & 1;
      const int tot = chroma ? totC : totY, k = chroma ? (lane & 31) >> 1 : lane >> 2;
      const int n = tot & 2047, s = (tot - n) >> 11;
      const bool pos = (k & 3) < 2;  // categories 1, 2 >= 0; 3, 4 <= 0 (tv::sao_item)
      int o;
      const long long j = sao_best_offset(n, s, pos ? 0 : -kSaoMaxOff, pos ? kSaoMaxOff : 0, lam16, false, o);
      const uint32_t ob = (uint32_t)(o + 8) << (7 + 4 * (k & 3));  // the item's field of sao_pack
      // class sums (tv::sao_eo_j) and offset fields: luma class = 16-lane row (one item on
      // every fourth lane), chroma (plane, class) = 8-lane group (the odd lanes)
      const bool ly = (lane & 3) == 0;
      long long jy = ly ? j : 0, jc = chroma ? j : 0;
      int py = ly ? (int)ob : 0, pc = chroma ? (int)ob : 0;
      jy = sao_dpp_add64<dpp::kQuadXor1>(jy);
      jy = sao_dpp_add64<dpp::kQuadXor2>(jy);
      jc = sao_dpp_add64<dpp::kQuadXor1>(jc);
      jc = sao_dpp_add64<dpp::kQuadXor2>(jc);
      jy = sao_dpp_add64<dpp::kRowHalfMirror>(jy);
      jc = sao_dpp_add64<dpp::kRowHalfMirror>(jc);
      jy = sao_dpp_add64<dpp::kRowMirror>(jy);
      py += dpp::mov<dpp::kQuadXor1>(py);
      py += dpp::mov<dpp::kQuadXor2>(py);
      pc += dpp::mov<dpp::kQuadXor1>(pc);
      pc += dpp::mov<dpp::kQuadXor2>(pc);
      py += dpp::mov<dpp::kRowHalfMirror>(py);
      pc += dpp::mov<dpp::kRowHalfMirror>(pc);
      py += dpp::mov<dpp::kRowMirror>(py);
      // the choices of tv::sao_finish_pos on scalars.  Rate in bits: type 1 (off) / 2 (edge), class 2.
      long long best = lam16 * 1;
      int cls = -1;
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2) {
        const long long jj = sao_readlane64(jy, 16 * c2) + lam16 * 4;
        if (jj < best) {
          best = jj;
          cls = c2;
        }
      }
      prm[0] = cls < 0 ? sao_off_param() : 2u | (uint32_t)cls << 2 | (uint32_t)__builtin_amdgcn_readlane(py, 16 * cls);
      best = lam16 * 1;
      cls = -1;
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2) {  // one type (and EO class) for Cb and Cr
        const long long jj = sao_readlane64(jc, 8 * c2) + sao_readlane64(jc, 32 + 8 * c2) + lam16 * 4;
        if (jj < best) {
          best = jj;
          cls = c2;
        }
      }
      prm[1] = cls < 0 ? sao_off_param() : 2u | (uint32_t)cls << 2 | (uint32_t)__builtin_amdgcn_readlane(pc, 8 * cls);
      prm[2] = cls < 0 ? sao_off_param() : 2u | (uint32_t)cls << 2 | (uint32_t)__builtin_amdgcn_readlane(pc, 32 + 8 * cls);
      if (lane < 3) sao[3 * ((long)b * g.wc * g.hc + cy * g.wc + cx) + lane] = lane == 0 ? prm[0] : (lane == 1 ? prm[1] : prm[2]);
    }
    // the SAO'd CTB from the tile, 4 samples per dword store: luma 32 rows x 8 dwords (4 per
    // lane), chroma 16 x 4 (one per lane and plane); the squared error against the source
    // (display area) is summed on the way (no k_sse).  The 8 / 4 lanes of a row segment are
    // adjacent; the rows of a 32-lane half are 8 (luma) / 4 (chroma) apart, which spreads
    // their tile reads over the banks.
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ly = 8 * ((lane >> 3) & 3) + 4 * (lane >> 5) + k, lx0 = 4 * (lane & 7);
      const long at = (long)(cy * 32 + ly) * g.W + cx * 32 + lx0;
      const bool want_sse = sse && cy * 32 + ly < g.dh;
      const uint32_t sw = want_sse ? *reinterpret_cast<const uint32_t*>(src.plane(0, b, g) + at) : 0u;
      const uint32_t word = sao_filter_dword<kSaoPd>(tY, (ly + 1) * kSaoPd + (lx0 >> 1), prm[0]);
      *reinterpret_cast<uint32_t*>(out.plane(0, b, g) + at) = word;
      if (want_sse) e2[0] += sao_sse_dword(sw, word, cx * 32 + lx0, g.dw);
    }
#pragma unroll
    for (int cc = 1; cc < 3; ++cc) {
      const int ly = 4 * ((lane >> 2) & 3) + (lane >> 4), lx0 = 4 * (lane & 3);
      const long at = (long)(cy * 16 + ly) * cw + cx * 16 + lx0;
      const bool want_sse = sse && cy * 16 + ly < g.dh / 2;
      const uint32_t sw = want_sse ? *reinterpret_cast<const uint32_t*>(src.plane(cc, b, g) + at) : 0u;
      const uint32_t word =
          sao_filter_dword<kSaoPdC>(tC0 + (cc - 1) * kSaoChromaDw, (ly + 1) * kSaoPdC + (lx0 >> 1), prm[cc]);
      *reinterpret_cast<uint32_t*>(out.plane(cc, b, g) + at) = word;
      if (want_sse) e2[cc] += sao_sse_dword(sw, word, cx * 16 + lx0, g.dw / 2);
    }
  }
  if (sse) {
    if (active) {
#pragma unroll
      for (int c2 = 0; c2 < 3; ++c2) {
        const int t = wave_sum((int)e2[c2]);  // <= 4 dwords x 4 x 65025 per lane: fits
        if (lane == 0 && t) atomicAdd(&esum[c2], (unsigned long long)(unsigned)t);
      }
    }
    __syncthreads();
    if (tid < 3 && esum[tid]) atomicAdd(sse + b * 3 + tid, esum[tid]);
  }
}

void launch_sao(FrameSet src, FrameSet deb, FrameSet out, uint32_t* sao, const int8_t* qp, const RcTables* rc,
                const Geo& g, int B, hipStream_t s, unsigned long long* sse) {
  const int strips = (g.wc + kSaoStrip - 1) / kSaoStrip * g.hc;
  k_sao_decide<<<dim3(strips, B), 64 * kSaoStrip, 0, s>>>(src, deb, out, sao, g, qp, rc, sse);
}

void launch_deblock(FrameSet rec, DecisionSet dec, const Geo& g, int B, hipStream_t s) {
  dim3 grid((unsigned)tv_min(1024, (int)(g.ysz / 32 / 256 + 1)), B);
  k_deblock<<<grid, 256, 0, s>>>(rec, dec, g, 0);
  k_deblock<<<grid, 256, 0, s>>>(rec, dec, g, 1);
}

}  // namespace gpu
}  // namespace tv
