// synth_tile.h — the synthetic source of tv/synth.h, evaluated one tile of one plane at a time.
//
// synth_sample_ctx (tv/synth.h) is the definition of the source.  This header holds the
// separable form of its value-noise octaves, shared by the generator kernel (k_synth,
// csrc/gpu/k_frame.hip) and its host mirror (tv_synth_frame_tiled), so the tiled arithmetic
// can be compared with the definition byte for byte without a GPU.
//
// synth_vnoise(px16, py16, lp, seed) is
//     top = a * 256 + (b - a) * sx;   bot = c * 256 + (d - c) * sx;
//     (top * 256 + (bot - top) * sy) >> 16
// where the cell column cx and sx depend only on px16, the cell row cy and sy only on py16,
// and (a, b) / (c, d) are the lattice hashes of rows cy / cy + 1 at columns cx, cx + 1.  So
// for one octave over a tile:
//   * the lattice hashes are taken once per lattice point of the tile's window (SynthWin);
//   * top[r][x] = a * 256 + (b - a) * sx is taken once per (lattice row r, column x);
//   * a sample is (top[cy][x] * 256 + (top[cy + 1][x] - top[cy][x]) * sy) >> 16.
// These are the same integer expressions in the same order as synth_vnoise, only evaluated
// once where their inputs repeat: `bot` of lattice row cy is `top` of lattice row cy + 1.
//
// Range: fx <= 255, so sx = fx * fx * (768 - 2 * fx) >> 16 <= 255 (fx = 255 gives 255), and
// top = a * (256 - sx) + b * sx with a, b <= 255 lies in 0 .. 255 * 256: a table of `top`
// holds it in 16 bits.
//
// Columns and rows are clamped to the display size before anything else (synth_tile_pos), so
// the replicated padding of the coded planes falls out of the tables.
#pragma once
#include <cstdint>

#include "synth.h"

namespace tv {

// The kernel's tile: 256 samples wide (a wavefront of 4-sample items writes 256 contiguous
// bytes of a row), 32 rows (8, 16 and 64 were measured: profiles/README.md, synth_tiles/).
constexpr int kSynthTileW = 256, kSynthTileH = 32;

// Luma-grid position in 1/16 pel of column (or row) i of a plane with display extent d;
// s = 1 for the chroma planes.
TV_HD int32_t synth_tile_pos(int i, int d, int s) { return (int32_t)((tv_min(i, d - 1) << s) * 16); }

// Lattice window of one octave over a tile: the cells that the 1/16-pel coordinate ranges
// [px_lo, px_hi] x [py_lo, py_hi] touch, plus the far corner of the last cell.
struct SynthWin {
  int sh;            // lp + 4: cell size in 1/16 pel is 1 << sh
  uint32_t seed;
  int32_t cx0, cy0;  // first cell
  int npx, npy;      // lattice points per row / rows
};
TV_HD SynthWin synth_win(int lp, uint32_t seed, int32_t px_lo, int32_t px_hi, int32_t py_lo, int32_t py_hi) {
  SynthWin w;
  w.sh = lp + 4;
  w.seed = seed;
  w.cx0 = px_lo >> w.sh;
  w.cy0 = py_lo >> w.sh;
  w.npx = (px_hi >> w.sh) - w.cx0 + 2;
  w.npy = (py_hi >> w.sh) - w.cy0 + 2;
  return w;
}
// Upper bound of npx / npy for a coordinate range of `span16` (hi - lo): sizes the tables.
constexpr int synth_win_max(int span16, int lp) { return (span16 >> (lp + 4)) + 3; }

// Lattice value of point (i, r) of the window.
TV_HD int synth_win_lattice(const SynthWin& w, int i, int r) {
  return (int)(synth_hash(w.cx0 + i, w.cy0 + r, w.seed) & 255);
}
// One axis of synth_vnoise: cell index relative to the window's first cell c0 and smoothstep
// weight (0..255) of coordinate p16.
TV_HD void synth_axis(int32_t p16, int sh, int32_t c0, int& ci, int& sw) {
  const int32_t cc = p16 >> sh;
  const int f = (int)((p16 - (cc << sh)) << 8 >> sh);  // 0..255
  sw = (f * f * (768 - 2 * f)) >> 16;
  ci = (int)(cc - c0);
}
// top[r][x] from the lattice values a (cell column) and b (next column) of lattice row r.
TV_HD int synth_top(int a, int b, int sx) { return a * 256 + (b - a) * sx; }
// The octave's value from the column's entries of lattice rows cy and cy + 1.
TV_HD int synth_rows(int top, int bot, int sy) { return (top * 256 + (bot - top) * sy) >> 16; }

// ---- what synth_sample_ctx does with the octaves ----------------------------------------
TV_HD int synth_pan_x(bool tex) { return tex ? 88 : 36; }
TV_HD int synth_pan_y(bool tex) { return tex ? 36 : 12; }
// Background octaves of plane c: lattice period and seed of octave i, and their number.
TV_HD int synth_bg_octaves(int c, bool tex) { return c ? 1 : (tex ? 4 : 3); }
TV_HD int synth_bg_lp(int c, int i) { return c ? 8 : 7 - 2 * i; }
TV_HD uint32_t synth_bg_seed(uint32_t seed, int c, int i) { return c ? seed + 10 * c : seed + i; }
TV_HD int synth_bg_mix(int c, bool tex, const int n[4]) {
  if (c) return 96 + (n[0] >> 1);
  return tex ? (n[0] * 3 + n[1] * 2 + n[2] * 2 + n[3]) >> 3 : (n[0] * 5 + n[1] * 2 + n[2]) >> 3;
}
// Object octaves (object-relative coordinates rx16 = xl * 16 - ox, ry16 = yl * 16 - oy).
TV_HD int synth_obj_octaves(int c) { return c ? 1 : 2; }
TV_HD int synth_obj_lp(int c, int i) { return c ? 5 : 4 - 2 * i; }
TV_HD uint32_t synth_obj_seed(const SynthObject& o, int c, int i) { return c ? o.seed + c : o.seed + 5 * i; }
// base: synth_obj_base of the object (chroma only)
TV_HD int synth_obj_mix(int c, int base, const int n[2]) {
  return c ? 64 + base + (n[0] >> 3) : 40 + ((n[0] * 3 + n[1]) >> 2) * 3 / 4;
}
TV_HD int synth_obj_base(uint32_t seed, int k, int c) { return (int)(synth_hash(k, c, seed) & 127); }
// Shape test of a sample inside the object's bounding box, split by axis: the sample is
// covered iff synth_cover_col(o, rx16) <= synth_cover_row(o, ry16).  For the ellipse this is
// synth_sample_ctx's dx^2 hh^2 + dy^2 ww^2 <= ww^2 hh^2 with the row term moved to the right
// (exact in integers; no term exceeds ww^2 hh^2, which synth_sample_ctx forms too); a
// rectangle compares 0 <= 0.  The column term is taken once per column, the row term once per
// row.
TV_HD int64_t synth_cover_col(const SynthObject& o, int32_t rx16) {
  if (o.shape != 1) return 0;
  const int64_t dx = 2 * (int64_t)rx16 - o.w * 16, hh = (int64_t)o.h * 16;
  return dx * dx * hh * hh;
}
TV_HD int64_t synth_cover_row(const SynthObject& o, int32_t ry16) {
  if (o.shape != 1) return 0;
  const int64_t dy = 2 * (int64_t)ry16 - o.h * 16, ww = (int64_t)o.w * 16, hh = (int64_t)o.h * 16;
  return ww * ww * hh * hh - dy * dy * ww * ww;
}
// Per-frame grain of the textured variant at the clamped plane position (xc, yc).
TV_HD int synth_grain(uint32_t seed, int t, int c, int xc, int yc) {
  const uint32_t g = synth_hash(xc + t * 7919, yc + c * 104729, seed ^ 0x5bd1e995u);
  return c ? (int)(g & 3) - 2 : (int)(g & 7) - 4;
}

// Overlap of object k's bounding box with the coordinate range [p_lo, p_hi] of a tile along
// one axis, in object-relative 1/16 pel: [lo, hi], empty when lo > hi.  extent = w or h.
TV_HD void synth_obj_range(int32_t p_lo, int32_t p_hi, int32_t o16, int extent, int32_t& lo, int32_t& hi) {
  lo = tv_max(p_lo - o16, 0);
  hi = tv_min(p_hi - o16, extent * 16 - 1);
}

}  // namespace tv
