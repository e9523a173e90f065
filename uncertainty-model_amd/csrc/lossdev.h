// Device helpers shared by the loss kernels (loss.hip, lossterms.hip): the
// reference's linspace grid and bilinear warp (train/utils.py:65-97) and the
// align_corners resize index (F.interpolate, train/loss.py:120).
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

__device__ __forceinline__ void up_index(int i, int in, int out, int& i0, int& i1, float& l1) {
  const float sc = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float src = sc * (float)i;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = src - (float)i0;
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

}  // namespace
