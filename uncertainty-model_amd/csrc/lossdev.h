// Device helpers shared by the kernels that evaluate the reference's loss
// arithmetic -- loss.hip (the fused training loss), lossterms.hip (the
// standalone terms) and eval.hip (the evaluation engine's maps):
//   * the linspace grid and bilinear warp of train/utils.py:65-97;
//   * the 3x3 SSIM window of train/loss.py:43-74;
//   * the tile geometry and the grid-to-pixel upsample of the DSSIM map
//     (F.interpolate align_corners, train/loss.py:120; up_index itself is in
//     common.h).
#pragma once

#include "common.h"

namespace {

__device__ __forceinline__ float lin01(int i, int n) {
  // torch.linspace(0, 1, n) (CPU kernel: symmetric halves)
  if (n <= 1) return 0.f;
  const float step = 1.f / (float)(n - 1);
  return (i < n / 2) ? step * (float)i : 1.f - step * (float)(n - 1 - i);
}

struct Samp {
  int x0, y0;
  float w, e, n, s;  // torch naming: w = x - x0, e = 1 - w, n = y - y0, s = 1 - n
};

__device__ __forceinline__ Samp warp_at(int x, int y, float shift, int W, int H) {
  const float gx = 2.f * (lin01(x, W) + shift) - 1.f;
  const float gy = 2.f * lin01(y, H) - 1.f;
  const float ix = (gx + 1.f) * ((float)W * 0.5f) - 0.5f;
  const float iy = (gy + 1.f) * ((float)H * 0.5f) - 0.5f;
  Samp t;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  t.w = ix - fx;
  t.e = 1.f - t.w;
  t.n = iy - fy;
  t.s = 1.f - t.n;
  return t;
}

// value of plane at (y, x) with zero padding; plane element (y,x) at p[(y*W + x) * st]
__device__ __forceinline__ float pv(const float* p, int y, int x, int H, int W, long st) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? p[((long)y * W + x) * st] : 0.f;
}

// sample value and d(value)/d(ix)
__device__ __forceinline__ float sample(const float* p, const Samp& t, int H, int W, long st,
                                        float* dix) {
  const float nw = pv(p, t.y0, t.x0, H, W, st), ne = pv(p, t.y0, t.x0 + 1, H, W, st);
  const float sw = pv(p, t.y0 + 1, t.x0, H, W, st), se = pv(p, t.y0 + 1, t.x0 + 1, H, W, st);
  if (dix) *dix = t.s * (ne - nw) + t.n * (se - sw);
  return nw * (t.s * t.e) + ne * (t.s * t.w) + sw * (t.n * t.e) + se * (t.n * t.w);
}

__device__ __forceinline__ float sgnf(float x) { return (x > 0.f) - (x < 0.f); }

// The same warp with the per-image constants hoisted: lin01 with a
// precomputed step, the row part (which does not depend on the shift) from a
// per-row table.  Bit-identical to warp_at.
struct RowW {
  int y0;
  float n;  // iy - y0
};
__device__ __forceinline__ float lin01s(int i, int n, int half, float step) {
  return n <= 1 ? 0.f : (i < half) ? step * (float)i : 1.f - step * (float)(n - 1 - i);
}
__device__ __forceinline__ RowW row_w(int y, int H) {
  const float gy = 2.f * lin01(y, H) - 1.f;
  const float iy = (gy + 1.f) * ((float)H * 0.5f) - 0.5f;
  const float fy = floorf(iy);
  RowW r;
  r.y0 = (int)fy;
  r.n = iy - fy;
  return r;
}
__device__ __forceinline__ Samp warp_tab(float linx, const RowW& rw, float shift, float Wh) {
  const float gx = 2.f * (linx + shift) - 1.f;
  const float ix = (gx + 1.f) * Wh - 0.5f;
  Samp t;
  const float fx = floorf(ix);
  t.x0 = (int)fx;
  t.y0 = rw.y0;
  t.w = ix - fx;
  t.e = 1.f - t.w;
  t.n = rw.n;
  t.s = 1.f - rw.n;
  return t;
}

// --------------------------------------------------------- 3x3 SSIM window --
// Moments of one channel over the 3x3 window whose top-left is (r, q) of the
// staged tiles (reference train/loss.py:43-74: valid 3x3 average pools)
struct Stats {
  float mx, my, vx, vy, vxy;
};
template <int RX>
__device__ __forceinline__ Stats win_stats(const float (*I)[RX], const float (*R)[RX], int r,
                                           int q) {
  float sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const float xv = I[r + u][q + w], yv = R[r + u][q + w];
      sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv; sxy += xv * yv;
    }
  // the 3x3 mean as a multiply by 1/9 (within an ulp of the reference's
  // avg_pool division; an IEEE division here is ~10 instructions)
  constexpr float k9 = 1.f / 9.f;
  Stats st;
  st.mx = sx * k9;
  st.my = sy * k9;
  st.vx = sxx * k9 - st.mx * st.mx;
  st.vy = syy * k9 - st.my * st.my;
  st.vxy = sxy * k9 - st.mx * st.my;
  return st;
}
__device__ __forceinline__ float ssim_of(const Stats& t, float c1, float c2) {
  return ((2 * t.mx * t.my + c1) * (2 * t.vxy + c2)) /
         ((t.mx * t.mx + t.my * t.my + c1) * (t.vx + t.vy + c2));
}

// ------------------------------------------------------------------ tiles --
// A tile of TY x TX pixels: the staged region is rows [ty0-2, ty0+TY+3),
// cols [tx0-2, tx0+TX+3) (the pixels, the SSIM windows of the DSSIM grid
// points the tile's upsample reads and the smoothness neighbours), the grid
// points are rows [ty0-2, ty0+TY+1), cols [tx0-2, tx0+TX+1)
template <int TY, int TX>
struct Tile {
  static constexpr int RY = TY + 5, RX = TX + 5;  // staged region
  static constexpr int GY = TY + 3, GX = TX + 3;  // grid points
  static constexpr int NP = RY * RX;
};

// the two DSSIM grid taps of a pixel row or column, as indices into the
// tile's grid (grid point g0 = tile origin - 2 is index 0)
struct UpTap {
  int i0, i1;
  float l1;
};
// taps of pixel i of the upsample n - 2 -> n.  The clamp at 0 never changes a
// value (int(sc * i) >= i - 2 for every i < n, 3 <= n <= 8192, in f32); it
// keeps the LDS index non-negative whatever the rounding of the scale.
__device__ __forceinline__ UpTap up_tap(int i, int n, int g0) {
  UpTap u;
  up_index(i, n - 2, n, u.i0, u.i1, u.l1);
  u.i0 = max(u.i0 - g0, 0);
  u.i1 = max(u.i1 - g0, 0);
  return u;
}
// DSSIM upsampled to a pixel of the tile from the grid tile
template <int GX>
__device__ __forceinline__ float dssim_up(const float (*sD)[GX], const UpTap& uy,
                                          const UpTap& ux) {
  return (1.f - uy.l1) * ((1.f - ux.l1) * sD[uy.i0][ux.i0] + ux.l1 * sD[uy.i0][ux.i1]) +
         uy.l1 * ((1.f - ux.l1) * sD[uy.i1][ux.i0] + ux.l1 * sD[uy.i1][ux.i1]);
}

}  // namespace
