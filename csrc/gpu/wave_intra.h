// wave_intra.h — the intra reference-sample logic of the HEVC kernels, stated once.
//
//  wave_intra_predict  the normative prediction of one TB by one wave (k_intra_recon,
//                      k_pintra_recon): reference samples from the RECONSTRUCTION, substitution
//                      (H.265 8.4.4.2.2), [1 2 1] smoothing, prediction and residual.
//  src_ref_entry, intra_smooth_entry, intra_cost_key
//                      the per-entry pieces of the mode search from SOURCE neighbours
//                      (k_intra_analysis, k_pintra_analysis).
#pragma once
#include "gpu_common.h"
#include "k_encode.h"
#include "wave_tb.h"

namespace tv {
namespace gpu {

// the angular-mode tables in LDS (indexed constexpr tables become global loads on the GPU)
struct AngleLds {
  int8_t angle[35];
  int16_t inv[35];
  __device__ void load(int tid, int nthreads) {
    for (int m = tid; m < 35; m += nthreads) {
      angle[m] = m >= 2 ? (int8_t)intra_angle(m) : 0;
      inv[m] = m >= 2 ? (int16_t)intra_inv_angle(m) : 0;
    }
  }
};

// entry i of the [1 2 1] smoothed references FL / FT of L / T (2N+1 entries each, N2 = 2N)
template <class R>
__device__ __forceinline__ void intra_smooth_entry(const R* L, const R* T, R* FL, R* FT, int i, int N2) {
  if (i == 0) {
    FL[0] = FT[0] = (R)((L[1] + 2 * L[0] + T[1] + 2) >> 2);
  } else if (i == N2) {
    FL[i] = L[i];
    FT[i] = T[i];
  } else {
    FL[i] = (R)((L[i + 1] + 2 * L[i] + L[i - 1] + 2) >> 2);
    FT[i] = (R)((T[i + 1] + 2 * T[i] + T[i - 1] + 2) >> 2);
  }
}

// entry i of the SOURCE references of the block at (x, y) of luma plane S: left sample i and top
// sample i (i = 0: both are the corner); unavailable entries are 0 until tv::intra_substitute
__device__ __forceinline__ void src_ref_entry(const uint8_t* S, int W, int H, int x, int y, int i, int16_t* L,
                                              int16_t* T, bool* avl, bool* avt) {
  const bool al = zscan_available(x, y, x - 1, y + i - 1, W, H);
  avl[i] = al;
  L[i] = al ? S[(long)(y + i - 1) * W + x - 1] : 0;
  const bool at = zscan_available(x, y, x + i - 1, y - 1, W, H);
  avt[i] = at;
  T[i] = at ? S[(long)(y - 1) * W + x + i - 1] : 0;
}

// mode-search key: the smallest wins, cost first, then the lower mode
__device__ __forceinline__ unsigned intra_cost_key(int satd, int mode, const Penalties& pen) {
  return ((unsigned)(satd + (mode <= 1 ? pen.mode_dcpl : pen.mode_ang)) << 6) | (unsigned)mode;
}

// reference state of one wave for TBs up to S x S
template <int S>
struct IntraRefsT {
  int V[4 * S + 4];  // canonical order: bottom-left .. corner .. top-right
  int L[2 * S + 1], T[2 * S + 1], FL[2 * S + 1], FT[2 * S + 1];
};

// One wave predicts the 2^l2-sided TB of component c whose CU sits at luma (x0, y0): on return
// pred and resid (N*N, row-major) are filled for wave_code_tb.  nb(xn, yn) is the reconstructed
// sample at component position (xn, yn), asked only where z-scan order makes it available;
// src(px, py) the source sample at (px, py) within the TB.
template <int S, class NB, class SRC>
__device__ __forceinline__ void wave_intra_predict(IntraRefsT<S>& R, const AngleLds& ang, int c, int x0, int y0,
                                                   int l2, int mode, int W, int H, NB nb, SRC src, uint8_t* pred,
                                                   int16_t* resid) {
  // one round = 64 reference positions; the common 8x8 / 4x4 TBs (4N+1 <= 64) need one
  constexpr int kRounds = (4 * S + 1 + 63) / 64;
  const int lane = threadIdx.x & 63, sh = c ? 1 : 0, N = 1 << l2, total = 4 * N + 1;
  const int x = x0 >> sh, y = y0 >> sh;  // TB position (component samples)
  unsigned long long m[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    m[r] = 0;
    if (r && total <= 64 * r) continue;  // wave-uniform
    const int i = lane + 64 * r;
    bool av = false;
    if (i < total) {
      const int xn = i < 2 * N ? x - 1 : x - 1 + (i - 2 * N), yn = i < 2 * N ? y + 2 * N - 1 - i : y - 1;
      av = zscan_available(x0, y0, xn << sh, yn << sh, W, H);
      R.V[i] = av ? (int)nb(xn, yn) : 0;
    }
    m[r] = __ballot(av);
  }
  wave_sync();
  // --- substitution (H.265 8.4.4.2.2) as a parallel nearest-available search
  for (int i = lane; i < total; i += 64) {
    int j = -1;
    for (int w = i >> 6; w >= 0 && j < 0; --w) {
      const unsigned long long mm =
          (w == (i >> 6)) ? (m[w] & (((i & 63) == 63) ? ~0ull : ((2ull << (i & 63)) - 1))) : m[w];
      if (mm) j = w * 64 + 63 - __clzll(mm);
    }
    if (j < 0)
      for (int w = 0; w < kRounds && j < 0; ++w)
        if (m[w]) j = w * 64 + __ffsll(m[w]) - 1;
    const int v = j < 0 ? 128 : R.V[j];
    if (i < 2 * N) R.L[2 * N - i] = v;
    else if (i == 2 * N) R.L[0] = R.T[0] = v;
    else R.T[i - 2 * N] = v;
  }
  wave_sync();
  const bool filt = c == 0 && intra_filter_refs(l2, mode);
  if (filt) {
    for (int i = lane; i <= 2 * N; i += 64) intra_smooth_entry(R.L, R.T, R.FL, R.FT, i, 2 * N);
    wave_sync();
  }
  const int* RL = filt ? R.FL : R.L;
  const int* RT = filt ? R.FT : R.T;
  const int dc = mode == 1 ? intra_dc_value(RL, RT, l2) : 0;
  const int ang_a = ang.angle[mode], ang_i = ang.inv[mode];
  const bool edge = c == 0 && N < 32;  // DC / horizontal / vertical edge filters: luma below 32x32
  for (int i = lane; i < N * N; i += 64) {
    const int px = i & (N - 1), py = i >> l2;
    const int p = intra_pred_pixel_ai(RL, RT, l2, mode, ang_a, ang_i, edge, dc, px, py);
    pred[i] = (uint8_t)p;
    resid[i] = (int16_t)((int)src(px, py) - p);
  }
  wave_sync();
}

}  // namespace gpu
}  // namespace tv
