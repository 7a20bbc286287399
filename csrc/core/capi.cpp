// capi.cpp — extern "C" surface of libtvcore.so (loaded from Python with ctypes).
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "tv/av1_enc.h"
#include "tv/container.h"
#include "tv/cpu_encoder.h"
#include "tv/hevc_codec.h"
#include "tv/me_model.h"
#include "tv/rdq.h"
#include "tv/sdh.h"
#include "tv/synth.h"
#include "tv/synth_tile.h"
#include "tv/tb_frag.h"

using namespace tv;

namespace {
thread_local std::string g_err;
template <class F> int guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
struct Bytes {
  std::vector<uint8_t> v;
};

// Host image of one octave's tables over a tile (tv/synth_tile.h): what the generator kernel
// keeps in LDS.  px / py: the octave's 1/16-pel coordinate of every column / row of the tile.
struct TileOctave {
  int nx = 0;
  std::vector<uint8_t> lat;
  std::vector<uint16_t> top;
  std::vector<int> cy, sy;
  void build(int lp, uint32_t seed, const std::vector<int32_t>& px, const std::vector<int32_t>& py) {
    const SynthWin w = synth_win(lp, seed, px.front(), px.back(), py.front(), py.back());
    nx = (int)px.size();
    lat.resize((size_t)w.npx * w.npy);
    for (int r = 0; r < w.npy; ++r)
      for (int i = 0; i < w.npx; ++i) lat[(size_t)r * w.npx + i] = (uint8_t)synth_win_lattice(w, i, r);
    top.resize((size_t)w.npy * nx);
    for (int x = 0; x < nx; ++x) {
      int ci, sx;
      synth_axis(px[x], w.sh, w.cx0, ci, sx);
      for (int r = 0; r < w.npy; ++r)
        top[(size_t)r * nx + x] = (uint16_t)synth_top(lat[(size_t)r * w.npx + ci], lat[(size_t)r * w.npx + ci + 1], sx);
    }
    cy.resize(py.size());
    sy.resize(py.size());
    for (size_t y = 0; y < py.size(); ++y) synth_axis(py[y], w.sh, w.cy0, cy[y], sy[y]);
  }
  int at(int x, int y) const {
    const uint16_t* t = &top[(size_t)cy[y] * nx + x];
    return synth_rows(t[0], t[nx], sy[y]);
  }
};

// One tile of plane c of the coded picture (pitch pw), as the kernel's workgroup does it.
void synth_tile_fill(const SynthFrameCtx& f, int c, int x0, int y0, int nx, int ny, int pw, uint8_t* P) {
  const int s = c ? 1 : 0, dw = c ? f.W / 2 : f.W, dh = c ? f.H / 2 : f.H;
  const bool tex = synth_textured(f.seed);
  std::vector<int32_t> px(nx), py(ny), qx(nx), qy(ny);
  for (int x = 0; x < nx; ++x) px[x] = synth_tile_pos(x0 + x, dw, s);
  for (int y = 0; y < ny; ++y) py[y] = synth_tile_pos(y0 + y, dh, s);
  std::vector<int> v((size_t)nx * ny);
  TileOctave oct[4];
  for (int x = 0; x < nx; ++x) qx[x] = px[x] + f.t * synth_pan_x(tex);
  for (int y = 0; y < ny; ++y) qy[y] = py[y] + f.t * synth_pan_y(tex);
  const int nb = synth_bg_octaves(c, tex);
  for (int i = 0; i < nb; ++i) oct[i].build(synth_bg_lp(c, i), synth_bg_seed(f.seed, c, i), qx, qy);
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) {
      int n[4] = {0, 0, 0, 0};
      for (int i = 0; i < nb; ++i) n[i] = oct[i].at(x, y);
      v[(size_t)y * nx + x] = synth_bg_mix(c, tex, n);
    }
  for (int k = 0; k < kSynthObjects; ++k) {  // ascending: later objects on top
    const SynthObject& o = f.obj[k];
    int32_t xlo, xhi, ylo, yhi;
    synth_obj_range(px.front(), px.back(), f.ox[k], o.w, xlo, xhi);
    synth_obj_range(py.front(), py.back(), f.oy[k], o.h, ylo, yhi);
    if (xlo > xhi || ylo > yhi) continue;  // the tile misses the bounding box
    for (int x = 0; x < nx; ++x) qx[x] = clip3(xlo, xhi, px[x] - f.ox[k]);
    for (int y = 0; y < ny; ++y) qy[y] = clip3(ylo, yhi, py[y] - f.oy[k]);
    const int no = synth_obj_octaves(c), base = synth_obj_base(f.seed, k, c);
    for (int i = 0; i < no; ++i) oct[i].build(synth_obj_lp(c, i), synth_obj_seed(o, c, i), qx, qy);
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const int32_t rx16 = px[x] - f.ox[k], ry16 = py[y] - f.oy[k];
        if (rx16 != qx[x] || ry16 != qy[y] || synth_cover_col(o, rx16) > synth_cover_row(o, ry16)) continue;
        int n[2] = {0, 0};
        for (int i = 0; i < no; ++i) n[i] = oct[i].at(x, y);
        v[(size_t)y * nx + x] = synth_obj_mix(c, base, n);
      }
  }
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) {
      int r = v[(size_t)y * nx + x];
      if (tex) r += synth_grain(f.seed, f.t, c, tv_min(x0 + x, dw - 1), tv_min(y0 + y, dh - 1));
      P[(size_t)(y0 + y) * pw + x0 + x] = (uint8_t)clip_pixel(r);
    }
}
}  // namespace

extern "C" {

const char* tv_last_error() { return g_err.c_str(); }
int tv_core_version() { return 1; }

// ------------------------------------ byte buffers --------------------------------------
void* tv_bytes_new() { return new Bytes(); }
void tv_bytes_free(void* b) { delete static_cast<Bytes*>(b); }
size_t tv_bytes_size(void* b) { return static_cast<Bytes*>(b)->v.size(); }
const uint8_t* tv_bytes_data(void* b) { return static_cast<Bytes*>(b)->v.data(); }
void tv_bytes_clear(void* b) { static_cast<Bytes*>(b)->v.clear(); }

// ------------------------------------ synthetic source ----------------------------------
void tv_synth_frame(uint32_t seed, int t, int W, int H, uint8_t* y, uint8_t* u, uint8_t* v) {
  SynthFrameCtx ctx;
  synth_frame_ctx(seed, t, W, H, ctx);
  for (int c = 0; c < 3; ++c) {
    uint8_t* P = c == 0 ? y : (c == 1 ? u : v);
    const int w = c ? W / 2 : W, h = c ? H / 2 : H;
    for (int j = 0; j < h; ++j)
      for (int i = 0; i < w; ++i) P[(size_t)j * w + i] = (uint8_t)synth_sample_ctx(ctx, c, i, j);
  }
}

// The frame at the coded size (width and height rounded up to kCtb, edge replicated), built
// tile by tile with the tables of tv/synth_tile.h: the host mirror of the generator kernel.
void tv_synth_frame_tiled(uint32_t seed, int t, int W, int H, int tile_w, int tile_h, uint8_t* y, uint8_t* u,
                          uint8_t* v) {
  SynthFrameCtx ctx;
  synth_frame_ctx(seed, t, W, H, ctx);
  const int cw = (W + kCtb - 1) / kCtb * kCtb, ch = (H + kCtb - 1) / kCtb * kCtb;
  for (int c = 0; c < 3; ++c) {
    uint8_t* P = c == 0 ? y : (c == 1 ? u : v);
    const int pw = c ? cw / 2 : cw, ph = c ? ch / 2 : ch;
    for (int y0 = 0; y0 < ph; y0 += tile_h)
      for (int x0 = 0; x0 < pw; x0 += tile_w)
        synth_tile_fill(ctx, c, x0, y0, tv_min(tile_w, pw - x0), tv_min(tile_h, ph - y0), pw, P);
  }
}

// tv::satd8x8 (tv/me_model.h) of one 8x8 block of differences, for the tests
int tv_satd8x8(const int* d, int stride) { return satd8x8(d, stride); }

// The golden SAO of one W x H picture (multiples of kCtb): tv::sao_decide_picture of the
// deblocked planes dy, du, dv against the source at slice QP qp -> 3 packed words per CTB in
// params, then tv::sao_picture -> oy, ou, ov.
int tv_sao_picture_cpu(int W, int H, int qp, const uint8_t* sy, const uint8_t* su, const uint8_t* sv,
                       const uint8_t* dy, const uint8_t* du, const uint8_t* dv, uint32_t* params, uint8_t* oy,
                       uint8_t* ou, uint8_t* ov) {
  if (W <= 0 || H <= 0 || W % kCtb || H % kCtb || qp < 0 || qp > 51) {
    g_err = "tv_sao_picture_cpu: bad geometry or QP";
    return -1;
  }
  return guard([&] {
    Picture src, deb;
    src.alloc(W, H);
    deb.alloc(W, H);
    const uint8_t* s[3] = {sy, su, sv};
    const uint8_t* d[3] = {dy, du, dv};
    uint8_t* o[3] = {oy, ou, ov};
    for (int c = 0; c < 3; ++c) {
      const size_t n = (size_t)src.pw(c) * src.ph(c);
      std::memcpy(src.plane(c), s[c], n);
      std::memcpy(deb.plane(c), d[c], n);
    }
    sao_decide_picture(src, deb, qp, params);
    sao_picture(deb, params);
    for (int c = 0; c < 3; ++c) std::memcpy(o[c], deb.plane(c), (size_t)deb.pw(c) * deb.ph(c));
  });
}

// ------------------------------------ CPU encoder ---------------------------------------
void* tv_cpu_encoder_new(int width, int height, int qp, int deblock, int range, int max_merge) {
  SeqConfig cfg;
  cfg.width = width;
  cfg.height = height;
  cfg.qp = qp;
  cfg.set_flags(deblock);  // the kFlag* bits (tv/hevc_codec.h)
  cfg.max_merge_cand = max_merge;
  cfg.finalize();
  CpuEncoder* e = nullptr;  // a bad config becomes tv_last_error, not an abort across the FFI
  guard([&] { e = new CpuEncoder(cfg, range); });
  return e;
}
// hierarchical-B golden encoder (mgop > 1): frames go in the plan's coding order
void* tv_cpu_encoder_new_b(int width, int height, int qp, int deblock, int range, int max_merge, int mgop) {
  SeqConfig cfg;
  cfg.width = width;
  cfg.height = height;
  cfg.qp = qp;
  cfg.set_flags(deblock);
  cfg.max_merge_cand = max_merge;
  cfg.mgop = mgop;
  cfg.finalize();
  CpuEncoder* e = nullptr;
  guard([&] { e = new CpuEncoder(cfg, range); });
  return e;
}
// plan the next segment; disp (capacity nframes) receives the coding order's display indices
int tv_cpu_encoder_begin_gop(void* e, int nframes, int* disp) {
  return guard([&] {
    auto* enc = static_cast<CpuEncoder*>(e);
    enc->begin_gop(nframes);
    for (size_t k = 0; k < enc->plan().pics.size(); ++k) disp[k] = enc->plan().pics[k].disp;
  });
}
// GOP plan of nframes with mini-GOP mgop: per coded picture (coding order) display index,
// slice type, list-0 / list-1 reference, temporal layer; info = {dpb_size, num_reorder}
int tv_gop_plan(int nframes, int mgop, int* disp, int* type, int* ref0, int* ref1, int* layer, int* info) {
  const GopPlan g = plan_gop(nframes, mgop);
  for (size_t k = 0; k < g.pics.size(); ++k) {
    disp[k] = g.pics[k].disp;
    type[k] = g.pics[k].type;
    ref0[k] = g.pics[k].ref[0];
    ref1[k] = g.pics[k].ref[1];
    layer[k] = g.pics[k].layer;
  }
  info[0] = g.dpb_size;
  info[1] = g.num_reorder;
  return (int)g.pics.size();
}
void* tv_cpu_encoder_new_crf(int width, int height, int qp, int deblock, int range, int max_merge, int crf) {
  SeqConfig cfg;
  cfg.width = width;
  cfg.height = height;
  cfg.qp = qp;
  cfg.set_flags(deblock);
  cfg.max_merge_cand = max_merge;
  cfg.crf = crf;
  cfg.finalize();
  CpuEncoder* e = nullptr;  // a bad config becomes tv_last_error, not an abort across the FFI
  guard([&] { e = new CpuEncoder(cfg, range); });
  return e;
}
void tv_cpu_encoder_free(void* e) { delete static_cast<CpuEncoder*>(e); }
int tv_cpu_encoder_encode(void* e, const uint8_t* y, const uint8_t* u, const uint8_t* v, int sy,
                          int sc, int idr, int poc, void* out) {
  return guard([&] {
    const uint8_t* planes[3] = {y, u, v};
    const int strides[3] = {sy, sc, sc};
    static_cast<CpuEncoder*>(e)->encode_frame(planes, strides, idr != 0, poc, static_cast<Bytes*>(out)->v);
  });
}
// same with an explicit slice QP for this frame (rate control)
int tv_cpu_encoder_encode_qp(void* e, const uint8_t* y, const uint8_t* u, const uint8_t* v, int sy, int sc, int idr,
                             int poc, int qp, void* out) {
  return guard([&] {
    const uint8_t* planes[3] = {y, u, v};
    const int strides[3] = {sy, sc, sc};
    static_cast<CpuEncoder*>(e)->encode_frame(planes, strides, idr != 0, poc, static_cast<Bytes*>(out)->v, qp);
  });
}
// copy the coded-size reconstruction
void tv_cpu_encoder_recon(void* e, uint8_t* y, uint8_t* u, uint8_t* v) {
  const Picture& p = static_cast<CpuEncoder*>(e)->recon();
  std::memcpy(y, p.y.data(), p.y.size());
  std::memcpy(u, p.u.data(), p.u.size());
  std::memcpy(v, p.v.data(), p.v.size());
}
void tv_cpu_encoder_decisions(void* e, uint8_t* cu_log2, uint8_t* intra, uint8_t* ipm, int16_t* mv,
                              uint8_t* cbf) {
  const FrameDecisions& d = static_cast<CpuEncoder*>(e)->dec;
  std::memcpy(cu_log2, d.cu_log2.data(), d.cu_log2.size());
  std::memcpy(intra, d.intra.data(), d.intra.size());
  std::memcpy(ipm, d.ipm.data(), d.ipm.size());
  std::memcpy(mv, d.mv.data(), d.mv.size() * 2);
  std::memcpy(cbf, d.cbf.data(), d.cbf.size());
}
// the level planes (coded size, int16) of the last encoded frame
void tv_cpu_encoder_levels(void* e, int16_t* cy, int16_t* cu, int16_t* cv) {
  const FrameDecisions& d = static_cast<CpuEncoder*>(e)->dec;
  std::memcpy(cy, d.coef_y.data(), d.coef_y.size() * 2);
  std::memcpy(cu, d.coef_u.data(), d.coef_u.size() * 2);
  std::memcpy(cv, d.coef_v.data(), d.coef_v.size() * 2);
}

// ---------------------------- decisions -> reconstruction / bitstream ---------------------
// Reconstruct a frame from externally supplied decisions (golden model for the GPU).
// src/ref/rec planes are coded size. coef planes are outputs.  ref may be null for intra.
// `deblock`: non-zero = deblocking; kFlagSignHiding: sign data hiding.
int tv_reconstruct_frame(int width, int height, int qp, int deblock, const uint8_t* src_y,
                         const uint8_t* src_u, const uint8_t* src_v, const uint8_t* ref_y,
                         const uint8_t* ref_u, const uint8_t* ref_v, const uint8_t* cu_log2,
                         const uint8_t* intra, const uint8_t* ipm, const int16_t* mv,
                         uint8_t* cbf_out, int16_t* cy, int16_t* cu, int16_t* cv, uint8_t* rec_y,
                         uint8_t* rec_u, uint8_t* rec_v) {
  return guard([&] {
    SeqConfig cfg;
    cfg.width = width;
    cfg.height = height;
    cfg.qp = qp;
    cfg.deblock = (deblock & ~kFlagSignHiding) != 0;
    cfg.sign_hiding = (deblock & kFlagSignHiding) != 0;
    cfg.rqt = false;  // no transform splits (tv_write_frame codes every split flag as 0)
    cfg.finalize();
    const int W = cfg.coded_w, H = cfg.coded_h;
    Picture src, ref, rec;
    src.alloc(W, H);
    rec.alloc(W, H);
    std::memcpy(src.y.data(), src_y, src.y.size());
    std::memcpy(src.u.data(), src_u, src.u.size());
    std::memcpy(src.v.data(), src_v, src.v.size());
    if (ref_y) {
      ref.alloc(W, H);
      std::memcpy(ref.y.data(), ref_y, ref.y.size());
      std::memcpy(ref.u.data(), ref_u, ref.u.size());
      std::memcpy(ref.v.data(), ref_v, ref.v.size());
    }
    FrameDecisions fd;
    fd.alloc(W, H);
    std::memcpy(fd.cu_log2.data(), cu_log2, fd.cu_log2.size());
    std::memcpy(fd.intra.data(), intra, fd.intra.size());
    std::memcpy(fd.ipm.data(), ipm, fd.ipm.size());
    std::memcpy(fd.mv.data(), mv, fd.mv.size() * 2);
    reconstruct_frame(cfg, src, ref_y ? &ref : nullptr, fd, rec);
    std::memcpy(cbf_out, fd.cbf.data(), fd.cbf.size());
    std::memcpy(cy, fd.coef_y.data(), fd.coef_y.size() * 2);
    std::memcpy(cu, fd.coef_u.data(), fd.coef_u.size() * 2);
    std::memcpy(cv, fd.coef_v.data(), fd.coef_v.size() * 2);
    std::memcpy(rec_y, rec.y.data(), rec.y.size());
    std::memcpy(rec_u, rec.u.data(), rec.u.size());
    std::memcpy(rec_v, rec.v.data(), rec.v.size());
  });
}

// Write parameter sets (if idr) + a slice NAL from decision arrays (`deblock` as above: with
// kFlagSignHiding the level planes must satisfy the hidden signs' parity, else this fails).
int tv_write_frame(int width, int height, int qp, int deblock, int max_merge, int idr, int poc,
                   const uint8_t* cu_log2, const uint8_t* intra, const uint8_t* ipm,
                   const int16_t* mv, const uint8_t* cbf, const int16_t* cy, const int16_t* cu,
                   const int16_t* cv, void* out) {
  return guard([&] {
    SeqConfig cfg;
    cfg.width = width;
    cfg.height = height;
    cfg.qp = qp;
    cfg.deblock = (deblock & ~kFlagSignHiding) != 0;
    cfg.sign_hiding = (deblock & kFlagSignHiding) != 0;
    cfg.max_merge_cand = max_merge;
    cfg.finalize();  // no tu plane: inter CUs code split_transform_flag 0
    FrameData f;
    f.w8 = cfg.w8();
    f.h8 = cfg.h8();
    f.cu_log2 = cu_log2;
    f.intra = intra;
    f.ipm = ipm;
    f.mv = mv;
    f.cbf = cbf;
    f.coef[0] = cy;
    f.coef[1] = cu;
    f.coef[2] = cv;
    auto& o = static_cast<Bytes*>(out)->v;
    if (idr) write_parameter_sets(cfg, o);
    write_slice(cfg, f, poc, idr != 0, o);
  });
}

// ------------------------------------ decoder -------------------------------------------
void* tv_decoder_new() { return new HevcDecoder(); }
void tv_decoder_free(void* d) { delete static_cast<HevcDecoder*>(d); }
int tv_decoder_decode(void* d, const uint8_t* data, size_t n) {
  return guard([&] { static_cast<HevcDecoder*>(d)->decode(data, n); });
}
int tv_decoder_decode_range(void* d, const uint8_t* data, size_t n, int first, int count) {
  return guard([&] { static_cast<HevcDecoder*>(d)->decode_range(data, n, first, count); });
}
// header-only probe: geometry + picture count, no slice decoding
// spatial MV scaling of the B-slice AMVP (8.5.3.2.7), exported for the formula test
void tv_hevc_scale_mv(int mvx, int mvy, int td, int tb, int* out) {
  const Mv m = scale_mv(Mv{mvx, mvy}, td, tb);
  out[0] = m.x;
  out[1] = m.y;
}
// display index - decoding index of every picture (hierarchical-B reordering); returns the
// picture count (out receives at most cap values)
int tv_hevc_display_offsets(const uint8_t* data, size_t n, int* out, int cap) {
  int r = -1;
  guard([&] {
    const std::vector<int> off = display_offsets(data, n);
    for (int i = 0; i < (int)off.size() && i < cap; ++i) out[i] = off[i];
    r = (int)off.size();
  });
  return r;
}
int tv_hevc_probe(const uint8_t* data, size_t n, int* w, int* h, int* pictures, int* idrs) {
  return guard([&] {
    const StreamInfo s = probe_annexb(data, n);
    *w = s.width;
    *h = s.height;
    *pictures = s.pictures;
    *idrs = s.idrs;
  });
}
void tv_decoder_info(void* d, int* w, int* h, int* cw, int* ch, int* nframes) {
  auto* D = static_cast<HevcDecoder*>(d);
  *w = D->width;
  *h = D->height;
  *cw = D->coded_w;
  *ch = D->coded_h;
  *nframes = (int)D->pictures.size();
}
// copy frame idx; cropped=1 -> display size, else coded size
int tv_decoder_frame(void* d, int idx, int cropped, uint8_t* y, uint8_t* u, uint8_t* v) {
  return guard([&] {
    auto* D = static_cast<HevcDecoder*>(d);
    const Picture& p = D->pictures.at(idx).pic;
    const int w = cropped ? D->width : p.w, h = cropped ? D->height : p.h;
    for (int c = 0; c < 3; ++c) {
      uint8_t* dst = c == 0 ? y : (c == 1 ? u : v);
      const int cw = c ? w / 2 : w, chh = c ? h / 2 : h, sw = p.pw(c);
      for (int j = 0; j < chh; ++j) std::memcpy(dst + (size_t)j * cw, p.plane(c) + (size_t)j * sw, cw);
    }
  });
}

// ------------------------------------ containers ----------------------------------------
int tv_mux_mp4(const uint8_t* annexb, size_t n, int w, int h, int fps_num, int fps_den, void* out) {
  return guard([&] { static_cast<Bytes*>(out)->v = mux_mp4(annexb, n, w, h, fps_num, fps_den); });
}
int tv_mux_mp4_file(const uint8_t* const* segs, const size_t* sizes, int nseg, int w, int h, int fps_num, int fps_den,
                    const char* path, unsigned long long* out_size) {
  return guard([&] { *out_size = mux_mp4_file(segs, sizes, nseg, w, h, fps_num, fps_den, path); });
}
int tv_mux_file(const uint8_t* const* segs, const size_t* sizes, int nseg, int w, int h, int fps_num, int fps_den,
                const SideTrack* tracks, int ntracks, int container, const char* path, unsigned long long* out_size) {
  return guard([&] {
    *out_size = mux_file(segs, sizes, nseg, w, h, fps_num, fps_den, tracks, ntracks, container, path);
  });
}
size_t tv_side_track_size() { return sizeof(SideTrack); }

// ------------------------------------ cost model (tests) --------------------------------
// the MV-rate model evaluated over arrays: est[i] = mv_bits_est, idx[i] = me_pen_index of
// (dx[i], dy[i]); bits[i] = av1::mv_comp_bits(d[i])
void tv_mv_rate(const int* dx, const int* dy, int n, int* est, int* idx) {
  for (int i = 0; i < n; ++i) {
    est[i] = mv_bits_est(dx[i], dy[i]);
    idx[i] = me_pen_index(dx[i], dy[i]);
  }
}
void tv_av1_mv_comp_bits(const int* d, int n, int* bits) {
  for (int i = 0; i < n; ++i) bits[i] = av1::mv_comp_bits(d[i]);
}
// the f16 fragment tables of the GPU TB path (tv/tb_frag.h) expanded to integer matrices
// [n][k]: which = 0 / 1 the 32x32 pair into out[1024]; 2 + 2 * s + o the 16x16 composite of
// TB size 16 >> s, orientation o, into out[256].  Returns the matrix side, 0 for a bad index.
int tv_tb_frag_expand(int which, int* out) {
  static constexpr TbFragTables t = make_tb_frag();
  if (which < 0 || which >= 8) return 0;
  const int side = which < 2 ? 32 : 16;
  for (int n = 0; n < side; ++n)
    for (int k = 0; k < side; ++k)
      out[n * side + k] = int_of_f16_bits(which < 2 ? t.t32[which][n][k] : t.c16[(which - 2) >> 1][which & 1][n][k]);
  return side;
}
// ref[i] = quant_level(coef[i], qp, log2N, inter), fast[i] = the 32-bit quant_fast of the GPU path
void tv_quant_levels(const int* coef, int n, int qp, int log2N, int* ref, int* fast) {
  const QuantParams q = quant_params(qp, log2N);
  for (int i = 0; i < n; ++i) {
    ref[i] = quant_level(coef[i], qp, log2N, false);
    fast[i] = quant_fast(coef[i], q);
  }
}
// sign data hiding: ref[i] = sdh_delta of coef[i] and its quant_level (tv/sdh.h), fast[i] = the
// 32-bit sdh_delta_fast of the GPU paths
void tv_sdh_deltas(const int* coef, int n, int qp, int log2N, int intra, int* ref, int* fast) {
  const QuantParams q = quant_params(qp, log2N);
  for (int i = 0; i < n; ++i) {
    const int l = quant_level(coef[i], qp, log2N, intra != 0);
    ref[i] = sdh_delta(coef[i], l, qp, log2N);
    fast[i] = sdh_delta_fast(coef[i], l, q);
  }
}
// rate-distortion quantisation (tv/rdq.h) of one inter TB: coef N x N row-major, c 0 luma / 1
// chroma, lambda <= 0: kRdqLambda.  lev (N x N) receives the levels, J[3] the model's J after
// each of the three stages.  Returns kRdqLambda.
int tv_rdq_tb(const int* coef, int qp, int log2N, int c, int lambda, int16_t* lev, long long* J) {
  rdq_tb(coef, qp, log2N, c, lev, 1 << log2N, J, lambda > 0 ? lambda : kRdqLambda);
  return kRdqLambda;
}
int tv_demux_mp4(const uint8_t* mp4, size_t n, int* w, int* h, int* nframes, int* timescale,
                 int* delta, void* out) {
  return guard([&] { static_cast<Bytes*>(out)->v = demux_mp4(mp4, n, w, h, nframes, timescale, delta); });
}

}  // extern "C"
