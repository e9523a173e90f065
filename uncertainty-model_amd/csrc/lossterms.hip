// The loss terms of reference train/loss.py as standalone, differentiable
// entries (the fused stack of loss.hip evaluates the same terms for the
// reference's own composition; these serve every other composition):
//   um_image_error_k / _bwd   WeightedSSIMLoss.image_error (:96-131) with
//                             alpha, c1, c2 at run time, and its adjoint
//                             w.r.t. either operand for any upstream gradient
//   um_warp_bwd_img           adjoint of um_warp w.r.t. the sampled image
//   um_consistency_fwd/_bwd   ConsistencyLoss.forward (:167-188)
//   um_smoothness_fwd/_bwd    SmoothnessLoss.forward (:248-264)
//   um_nll_fwd/_bwd           ReprojectionErrorLoss.loss_function (:389-403)
//
// Strided [N][C][h][w] operands: element (n, c, y, x) at
// p[n*sn + c*sc + (y*w + x)*sp] (NCHW planes and channel slices of an NHWC
// tensor both qualify).
//
// Scalars: every term kernel writes one f64 partial per workgroup into the
// caller's workspace (um_lossterm_ws bytes); lt_finish_kernel sums them in a
// fixed order and stores the f32 device scalar.  No entry allocates or
// synchronises.  An upstream scalar gradient is a device pointer.
#include "common.h"
#include "lossdev.h"

namespace {

constexpr int LNT = 256;        // threads of the elementwise term kernels
constexpr int LMAXB = 1024;     // their workgroup cap (grid-stride loops)
constexpr int LTY = 16, LTX = 64;  // image-error tiles

// strided [N][C][h][w] operand
struct SView {
  const float* p;
  long sn, sc, sp;
  __device__ __forceinline__ const float* plane(int n, int c) const {
    return p + n * sn + c * sc;
  }
};

// block sum of v as an f64 partial: parts[blockIdx.x] (every thread calls)
template <int NT>
__device__ __forceinline__ void block_partial(float v, double* parts, int slot) {
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x;
  const float ws = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = (double)ws;
  __syncthreads();
  if (tid == 0) {
    double r = 0.0;
    for (int w = 0; w < NT / 64; ++w) r += red[w];
    parts[slot] = r;
  }
}

// out[0] = scale * sum(parts[0 .. n)) in a fixed order
__global__ void __launch_bounds__(LNT) lt_finish_kernel(const double* __restrict__ parts, int n,
                                                        double scale, float* __restrict__ out) {
  __shared__ double red[LNT];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n; i += LNT) s += parts[i];
  red[tid] = s;
  __syncthreads();
  for (int o = LNT / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)(red[0] * scale);
}

// --------------------------------------------------------- image error ------
using ET = Tile<LTY, LTX>;

// WeightedSSIMLoss.image_error of an explicit recon: out[n][v][y][x] =
// alpha * up(mean_c dssim_c) + (1 - alpha) * mean_c |I - R|;
// parts (optional): the workgroup's sum of both views
__global__ void __launch_bounds__(LNT) lt_image_error_kernel(
    const float* __restrict__ img, const float* __restrict__ rec, int N, int H, int W, float alpha,
    float c1, float c2, float* __restrict__ out, double* __restrict__ parts, int tiles_x,
    int tiles_y) {
  __shared__ float sI[3][ET::RY][ET::RX], sR[3][ET::RY][ET::RX];
  __shared__ float sD[ET::GY][ET::GX];
  const int tid = threadIdx.x;
  const long HW = (long)H * W;
  const int per = tiles_x * tiles_y;
  const int n = blockIdx.x / per, t = blockIdx.x - n * per;
  const int ty0 = (t / tiles_x) * LTY, tx0 = (t % tiles_x) * LTX;
  const int gh = H - 2, gw = W - 2;
  float acc = 0.f;
  for (int v = 0; v < 2; ++v) {
    const float* Iv = img + ((long)n * 6 + v * 3) * HW;
    const float* Rv = rec + ((long)n * 6 + v * 3) * HW;
    for (int i = tid; i < ET::RY * ET::RX; i += LNT) {
      const int r = i / ET::RX, q = i - r * ET::RX;
      const int y = ty0 - 2 + r, x = tx0 - 2 + q;
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sI[c][r][q] = in ? Iv[c * HW + (long)y * W + x] : 0.f;
        sR[c][r][q] = in ? Rv[c * HW + (long)y * W + x] : 0.f;
      }
    }
    __syncthreads();
    for (int i = tid; i < ET::GY * ET::GX; i += LNT) {
      const int r = i / ET::GX, q = i - r * ET::GX;
      const int gy = ty0 - 2 + r, gx = tx0 - 2 + q;
      float dv = 0.f;
      if (gy >= 0 && gy < gh && gx >= 0 && gx < gw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float ss = ssim_of(win_stats<ET::RX>(sI[c], sR[c], r, q), c1, c2);
          dv += fminf(fmaxf((1.f - ss) * 0.5f, 0.f), 1.f);
        }
        dv /= 3.f;
      }
      sD[r][q] = dv;
    }
    __syncthreads();
    for (int i = tid; i < LTY * LTX; i += LNT) {
      const int ly = i / LTX, lx = i - ly * LTX;
      const int y = ty0 + ly, x = tx0 + lx;
      if (y >= H || x >= W) continue;
      const float up = dssim_up<ET::GX>(sD, up_tap(y, H, ty0 - 2), up_tap(x, W, tx0 - 2));
      float l1 = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) l1 += fabsf(sI[c][ly + 2][lx + 2] - sR[c][ly + 2][lx + 2]);
      const float e = alpha * up + (1.f - alpha) * (l1 / 3.f);
      out[((long)n * 2 + v) * HW + (long)y * W + x] = e;
      acc += e;
    }
    __syncthreads();
  }
  if (parts != nullptr) block_partial<LNT>(acc, parts, blockIdx.x);
}

// weight with which output index o of the 1D align_corners upsample in -> out
// reads cell j
__device__ __forceinline__ float up_weight(int o, int j, int in, int out) {
  int i0, i1;
  float l1;
  up_index(o, in, out, i0, i1, l1);
  return (i0 == j ? 1.f - l1 : 0.f) + (i1 == j ? l1 : 0.f);
}

constexpr int BRY = LTY + 4, BRX = LTX + 4;  // staged pixels: rows [ty0-2, ty0+TY+2)
constexpr int BGY = LTY + 2, BGX = LTX + 2;  // cells whose window covers a tile pixel

// Gradient of the error map w.r.t. one operand X (Y = the other; SSIM is
// symmetric, |X - Y| differentiates to sign(X - Y)): one workgroup per tile,
// view and channel (blockIdx.y = v*3 + c).  Upstream gradient of the map:
// g[n][v][y][x] (or null) + *gs * gs_scale (or null): the mean's scalar path.
//   1. stage X, Y (zeros outside);
//   2. per grid cell: G = the resize adjoint of the upstream gradient (a gather
//      over the <= 3x3 of the 5x5 output pixels around the cell that read it),
//      then the cell's adjoints (a0, a1, a2): d(map)/dX(p) += a0 + a1 X(p) +
//      a2 Y(p) for the 9 pixels p of its window.  The clamp passes where
//      0 <= (1 - ssim)/2 <= 1;
//   3. per pixel: the sum over the <= 9 covering cells, plus the L1 part.
__global__ void __launch_bounds__(LNT) lt_image_error_bwd_kernel(
    const float* __restrict__ X6, const float* __restrict__ Y6, int N, int H, int W, float alpha,
    float c1, float c2, const float* __restrict__ g, const float* __restrict__ gs, float gs_scale,
    float* __restrict__ gX, int tiles_x, int tiles_y) {
  __shared__ float sX[BRY][BRX], sY[BRY][BRX];
  __shared__ float sA[3][BGY][BGX];
  const int tid = threadIdx.x;
  const long HW = (long)H * W;
  const int per = tiles_x * tiles_y;
  const int n = blockIdx.x / per, t = blockIdx.x - n * per;
  const int ty0 = (t / tiles_x) * LTY, tx0 = (t % tiles_x) * LTX;
  const int vc = blockIdx.y, v = vc / 3;
  const int gh = H - 2, gw = W - 2;
  const float* Xp = X6 + ((long)n * 6 + vc) * HW;
  const float* Yp = Y6 + ((long)n * 6 + vc) * HW;
  const float* gp = g != nullptr ? g + ((long)n * 2 + v) * HW : nullptr;
  const float gconst = gs != nullptr ? gs[0] * gs_scale : 0.f;
  for (int i = tid; i < BRY * BRX; i += LNT) {
    const int r = i / BRX, q = i - r * BRX;
    const int y = ty0 - 2 + r, x = tx0 - 2 + q;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    sX[r][q] = in ? Xp[(long)y * W + x] : 0.f;
    sY[r][q] = in ? Yp[(long)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < BGY * BGX; i += LNT) {
    const int r = i / BGX, q = i - r * BGX;
    const int gy = ty0 - 2 + r, gx = tx0 - 2 + q;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (gy >= 0 && gy < gh && gx >= 0 && gx < gw) {
      // output rows gy-1 .. gy+3 are the only ones that can read cell gy:
      // src = o * (gh-1)/(H-1) lies in [o - 2, o]
      float wy[5], wx[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int oy = gy - 1 + k, ox = gx - 1 + k;
        wy[k] = (oy >= 0 && oy < H) ? up_weight(oy, gy, gh, H) : 0.f;
        wx[k] = (ox >= 0 && ox < W) ? up_weight(ox, gx, gw, W) : 0.f;
      }
      float G = 0.f;
#pragma unroll
      for (int a = 0; a < 5; ++a) {
        if (wy[a] == 0.f) continue;
        const int oy = gy - 1 + a;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          if (wx[b] == 0.f) continue;
          const int ox = gx - 1 + b;
          const float gv = (gp != nullptr ? gp[(long)oy * W + ox] : 0.f) + gconst;
          G += wy[a] * wx[b] * gv;
        }
      }
      const Stats s = win_stats<BRX>(sX, sY, r, q);
      const float A = 2 * s.mx * s.my + c1, B = 2 * s.vxy + c2;
      const float C = s.mx * s.mx + s.my * s.my + c1, D = s.vx + s.vy + c2;
      const float ss = (A * B) / (C * D);
      const float dd = (1.f - ss) * 0.5f;
      if (dd >= 0.f && dd <= 1.f) {
        // d(map)/d(ssim) of this cell and channel, with the 1/9 of the means
        const float k = G * (alpha / 3.f) * -0.5f * (1.f / 9.f);
        const float dA = B / (C * D), dB = A / (C * D), dC = -ss / C, dD = -ss / D;
        a0 = k * (dA * 2.f * s.my + dC * 2.f * s.mx - dD * 2.f * s.mx - 2.f * dB * s.my);
        a1 = k * 2.f * dD;
        a2 = k * 2.f * dB;
      }
    }
    sA[0][r][q] = a0;
    sA[1][r][q] = a1;
    sA[2][r][q] = a2;
  }
  __syncthreads();
  for (int i = tid; i < LTY * LTX; i += LNT) {
    const int ly = i / LTX, lx = i - ly * LTX;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    // cells (y-2 .. y, x-2 .. x) = sA rows ly .. ly+2 (out-of-grid cells hold zeros)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        s0 += sA[0][ly + u][lx + w];
        s1 += sA[1][ly + u][lx + w];
        s2 += sA[2][ly + u][lx + w];
      }
    const float xv = sX[ly + 2][lx + 2], yv = sY[ly + 2][lx + 2];
    const float gv = (gp != nullptr ? gp[(long)y * W + x] : 0.f) + gconst;
    gX[((long)n * 6 + vc) * HW + (long)y * W + x] =
        s0 + s1 * xv + s2 * yv + ((1.f - alpha) / 3.f) * sgnf(xv - yv) * gv;
  }
}

// ------------------------------------------------- warp adjoint (image) -----
// One target row t of one image: the source rows t-1, t, t+1 (the only ones
// whose bilinear row taps reach t; the row taps do not depend on the shift)
// scatter along x into acc[c][W] (LDS, f32 atomics), in that order.  src:
// gradient planes, element (c, y, x) at src[c*ssc + y*W + x] * scale; shift of
// source pixel (y, x) = sign * dsp_[(y*W + x) * dsp].
__device__ __forceinline__ void scatter_target_row(float* acc, int C, int H, int W, int t,
                                                   const float* src, long ssc, float scale,
                                                   const float* disp, long dsp, float sign) {
  const int half = W / 2;
  const float step = W > 1 ? 1.f / (float)(W - 1) : 0.f;
  const float Wh = (float)W * 0.5f;
  for (int i = threadIdx.x; i < C * W; i += blockDim.x) acc[i] = 0.f;
  __syncthreads();
  for (int y = t - 1; y <= t + 1; ++y) {
    if (y < 0 || y >= H) continue;
    const RowW rw = row_w(y, H);
    const float wr = (rw.y0 == t ? 1.f - rw.n : 0.f) + (rw.y0 + 1 == t ? rw.n : 0.f);
    if (wr == 0.f) continue;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
      const float d = disp[((long)y * W + x) * dsp];
      const Samp s = warp_tab(lin01s(x, W, half, step), rw, sign * d, Wh);
      const bool in0 = s.x0 >= 0 && s.x0 < W, in1 = s.x0 >= -1 && s.x0 < W - 1;
      if (!in0 && !in1) continue;
      for (int c = 0; c < C; ++c) {
        const float gv = src[c * ssc + (long)y * W + x] * scale * wr;
        if (in0) atomicAdd(&acc[c * W + s.x0], gv * s.e);
        if (in1) atomicAdd(&acc[c * W + s.x0 + 1], gv * s.w);
      }
    }
    __syncthreads();
  }
}

// gimg[n][c][t][:] of um_warp: grid (H, N)
__global__ void __launch_bounds__(LNT) lt_warp_bwd_img_kernel(
    const float* __restrict__ gout, int C, int H, int W, const float* __restrict__ disp, long dsn,
    long dsp, float sign, float* __restrict__ gimg) {
  extern __shared__ float acc[];
  const int t = blockIdx.x, n = blockIdx.y;
  const long HW = (long)H * W;
  scatter_target_row(acc, C, H, W, t, gout + (long)n * C * HW, HW, 1.f, disp + n * dsn, dsp, sign);
  for (int i = threadIdx.x; i < C * W; i += blockDim.x) {
    const int c = i / W, x = i - c * W;
    gimg[((long)n * C + c) * HW + (long)t * W + x] = acc[i];
  }
}

// ------------------------------------------------------- consistency --------
// view v: |d_v - warp(i_(1-v), s_v d_v)|, s_0 = -1, s_1 = +1
__global__ void __launch_bounds__(LNT) lt_consistency_fwd_kernel(SView disp, SView img, int N,
                                                                 int H, int W,
                                                                 double* __restrict__ parts) {
  const long HW = (long)H * W, total = 2 * N * HW;
  float acc = 0.f;
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const int x = i % W, y = (i / W) % H;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const float d = disp.plane(n, v)[((long)y * W + x) * disp.sp];
    const Samp s = warp_at(x, y, v == 0 ? -d : d, W, H);
    acc += fabsf(d - sample(img.plane(n, 1 - v), s, H, W, img.sp, nullptr));
  }
  block_partial<LNT>(acc, parts, blockIdx.x);
}

// adjoint: gd[n][v][y][x] = k (1 - d(warp)/d(d_v)) (the compared map and the
// shift), gsamp[n][v][y][x] = -k: the gradient of view v's sample, which the
// scatter takes to channel 1-v of the sampled tensor.  k = sign(r) g / (N h w)
__global__ void __launch_bounds__(LNT) lt_consistency_adj_kernel(SView disp, SView img, int N,
                                                                 int H, int W,
                                                                 const float* __restrict__ gs,
                                                                 float* __restrict__ gd,
                                                                 float* __restrict__ gsamp) {
  const long HW = (long)H * W, total = 2 * N * HW;
  const float gk = gs[0] / (float)((double)N * HW);
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const int x = i % W, y = (i / W) % H;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const float d = disp.plane(n, v)[((long)y * W + x) * disp.sp];
    const float sign = v == 0 ? -1.f : 1.f;
    const Samp s = warp_at(x, y, sign * d, W, H);
    float dix;
    const float r = d - sample(img.plane(n, 1 - v), s, H, W, img.sp, &dix);
    const float k = sgnf(r) * gk;
    if (gd != nullptr) gd[i] = k * (1.f - dix * sign * (float)W);
    if (gsamp != nullptr) gsamp[i] = -k;
  }
}

// gimg[n][1-v][t][:] = scatter of gsamp[n][v] (+ add[n][1-v][t][:], the direct
// gradient when the sampled tensor is the disparity itself): grid (H, 2, N)
__global__ void __launch_bounds__(LNT) lt_consistency_scatter_kernel(
    const float* __restrict__ gsamp, SView disp, int H, int W, const float* __restrict__ add,
    float* __restrict__ gimg) {
  extern __shared__ float acc[];
  const int t = blockIdx.x, v = blockIdx.y, n = blockIdx.z;
  const long HW = (long)H * W;
  scatter_target_row(acc, 1, H, W, t, gsamp + ((long)n * 2 + v) * HW, HW, 1.f, disp.plane(n, v),
                     disp.sp, v == 0 ? -1.f : 1.f);
  const long o = ((long)n * 2 + (1 - v)) * HW + (long)t * W;
  for (int x = threadIdx.x; x < W; x += blockDim.x)
    gimg[o + x] = acc[x] + (add != nullptr ? add[o + x] : 0.f);
}

// -------------------------------------------------------- smoothness --------
// replicate-padded forward differences: 0 at the last column / row
struct Smooth {
  float gx, gy, wx, wy;
};
__device__ __forceinline__ Smooth smooth_at(const float* dp, long dsp, const float* im, int H,
                                            int W, int y, int x) {
  const long HW = (long)H * W, o = (long)y * W + x;
  Smooth s{0.f, 0.f, 1.f, 1.f};
  const float d = dp[o * dsp];
  float ax = 0.f, ay = 0.f;
  if (x + 1 < W) {
    s.gx = d - dp[(o + 1) * dsp];
#pragma unroll
    for (int c = 0; c < 3; ++c) ax += fabsf(im[c * HW + o] - im[c * HW + o + 1]);
  }
  if (y + 1 < H) {
    s.gy = d - dp[(o + W) * dsp];
#pragma unroll
    for (int c = 0; c < 3; ++c) ay += fabsf(im[c * HW + o] - im[c * HW + o + W]);
  }
  s.wx = expf(-ax / 3.f);
  s.wy = expf(-ay / 3.f);
  return s;
}

__global__ void __launch_bounds__(LNT) lt_smoothness_fwd_kernel(SView disp,
                                                                const float* __restrict__ img,
                                                                int N, int H, int W,
                                                                double* __restrict__ parts) {
  const long HW = (long)H * W, total = 2 * N * HW;
  float acc = 0.f;
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const int x = i % W, y = (i / W) % H;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const Smooth s =
        smooth_at(disp.plane(n, v), disp.sp, img + ((long)n * 6 + v * 3) * HW, H, W, y, x);
    acc += fabsf(s.gx * s.wx) + fabsf(s.gy * s.wy);
  }
  block_partial<LNT>(acc, parts, blockIdx.x);
}

// gd(y, x) gathers from its own differences and those of its left / upper neighbour
__global__ void __launch_bounds__(LNT) lt_smoothness_bwd_kernel(SView disp,
                                                                const float* __restrict__ img,
                                                                int N, int H, int W,
                                                                const float* __restrict__ gs,
                                                                float* __restrict__ gd) {
  const long HW = (long)H * W, total = 2 * N * HW;
  const float gk = gs[0] / (float)((double)N * HW);
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const int x = i % W, y = (i / W) % H;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const float* dp = disp.plane(n, v);
    const float* im = img + ((long)n * 6 + v * 3) * HW;
    const Smooth s = smooth_at(dp, disp.sp, im, H, W, y, x);
    float r = sgnf(s.gx) * s.wx + sgnf(s.gy) * s.wy;
    if (x > 0) {
      const Smooth l = smooth_at(dp, disp.sp, im, H, W, y, x - 1);
      r -= sgnf(l.gx) * l.wx;
    }
    if (y > 0) {
      const Smooth u = smooth_at(dp, disp.sp, im, H, W, y - 1, x);
      r -= sgnf(u.gy) * u.wy;
    }
    gd[i] = r * gk;
  }
}

// --------------------------------------------------------------- NLL --------
// loss_type 0: |u - e|; 1: e/u + log u; 2: (e / exp(-u) + u) / 2; mean over
// all N*2*h*w elements
__global__ void __launch_bounds__(LNT) lt_nll_fwd_kernel(SView unc, SView err, int N, int H, int W,
                                                         int loss_type,
                                                         double* __restrict__ parts) {
  const long HW = (long)H * W, total = 2 * N * HW;
  float acc = 0.f;
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const long p = i % HW;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const float u = unc.plane(n, v)[p * unc.sp], e = err.plane(n, v)[p * err.sp];
    acc += loss_type == 0 ? fabsf(u - e)
                          : loss_type == 1 ? e / u + logf(u) : 0.5f * (e / expf(-u) + u);
  }
  block_partial<LNT>(acc, parts, blockIdx.x);
}

__global__ void __launch_bounds__(LNT) lt_nll_bwd_kernel(SView unc, SView err, int N, int H, int W,
                                                         int loss_type,
                                                         const float* __restrict__ gs,
                                                         float* __restrict__ gu) {
  const long HW = (long)H * W, total = 2 * N * HW;
  const float gk = gs[0] / (float)(2.0 * N * HW);
  for (long i = blockIdx.x * (long)LNT + threadIdx.x; i < total; i += (long)gridDim.x * LNT) {
    const long p = i % HW;
    const int v = (i / HW) % 2, n = i / (2 * HW);
    const float u = unc.plane(n, v)[p * unc.sp], e = err.plane(n, v)[p * err.sp];
    const float r = loss_type == 0 ? sgnf(u - e)
                                   : loss_type == 1 ? (1.f - e / u) / u : 0.5f * (e * expf(u) + 1.f);
    gu[i] = r * gk;
  }
}

inline int lt_grid(long total) {
  const long b = (total + LNT - 1) / LNT;
  return (int)(b < 1 ? 1 : b > LMAXB ? LMAXB : b);
}

// LDS bytes a scatter workgroup may take (the default dynamic limit)
constexpr long SCATTER_LDS = 65536;

}  // namespace

extern "C" {

long um_lossterm_ws(int N, int H, int W) {
  long tiles = (long)N * ceil_div(H, LTY) * ceil_div(W, LTX);
  return 8 * (tiles > LMAXB ? tiles : LMAXB);
}

int um_warp_bwd_img_max_cw(void) { return (int)(SCATTER_LDS / 4); }

int um_image_error_k(const float* img, const float* rec, int N, int H, int W, float alpha,
                     float c1, float c2, float* out, double* ws, float* mean_out,
                     hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && H >= 3 && W >= 3, "um_image_error_k: %dx%dx%d (H, W >= 3)", N, H, W);
  UM_CHECK_ARG((ws != nullptr) == (mean_out != nullptr),
               "um_image_error_k: ws and mean_out go together");
  const int tx = ceil_div(W, LTX), ty = ceil_div(H, LTY);
  hipLaunchKernelGGL(lt_image_error_kernel, dim3(N * tx * ty), dim3(LNT), 0, st, img, rec, N, H,
                     W, alpha, c1, c2, out, ws, tx, ty);
  UM_LAUNCH_CHECK();
  if (ws != nullptr) {
    hipLaunchKernelGGL(lt_finish_kernel, dim3(1), dim3(LNT), 0, st, ws, N * tx * ty,
                       1.0 / ((double)N * H * W), mean_out);
    UM_LAUNCH_CHECK();
  }
  return UM_OK;
}

int um_image_error_bwd(const float* img, const float* rec, int N, int H, int W, float alpha,
                       float c1, float c2, int wrt, const float* g, const float* g_mean,
                       float* grad, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && H >= 3 && W >= 3, "um_image_error_bwd: %dx%dx%d (H, W >= 3)", N, H, W);
  UM_CHECK_ARG(wrt == 0 || wrt == 1, "um_image_error_bwd: wrt %d (0 recon, 1 images)", wrt);
  UM_CHECK_ARG(g != nullptr || g_mean != nullptr, "um_image_error_bwd: no upstream gradient");
  const int tx = ceil_div(W, LTX), ty = ceil_div(H, LTY);
  hipLaunchKernelGGL(lt_image_error_bwd_kernel, dim3(N * tx * ty, 6), dim3(LNT), 0, st,
                     wrt == 0 ? rec : img, wrt == 0 ? img : rec, N, H, W, alpha, c1, c2, g, g_mean,
                     (float)(1.0 / ((double)N * H * W)), grad, tx, ty);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_warp_bwd_img(const float* gout, int N, int C, int H, int W, const float* disp,
                    long disp_sn, long disp_sp, float sign, float* gimg, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1 && N <= 65535, "um_warp_bwd_img: %dx%dx%dx%d",
               N, C, H, W);
  UM_CHECK_ARG((long)C * W * 4 <= SCATTER_LDS,
               "um_warp_bwd_img: C*W = %ld row accumulators exceed the LDS limit of %ld floats "
               "(C*W <= %ld)", (long)C * W, SCATTER_LDS / 4, SCATTER_LDS / 4);
  hipLaunchKernelGGL(lt_warp_bwd_img_kernel, dim3(H, N), dim3(LNT), (size_t)C * W * 4, st, gout, C,
                     H, W, disp, disp_sn, disp_sp, sign, gimg);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

#define LT_GEOM(name, minhw)                                                               \
  UM_CHECK_ARG(N >= 1 && H >= (minhw) && W >= (minhw), name ": %dx%dx%d (H, W >= %d)", N, H, W, \
               (minhw))

int um_consistency_fwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                       long i_sn, long i_sc, long i_sp, int N, int H, int W, double* ws,
                       float* out, hipStream_t st) {
  LT_GEOM("um_consistency_fwd", 2);
  const int nb = lt_grid(2L * N * H * W);
  hipLaunchKernelGGL(lt_consistency_fwd_kernel, dim3(nb), dim3(LNT), 0, st,
                     SView{disp, d_sn, d_sc, d_sp}, SView{images, i_sn, i_sc, i_sp}, N, H, W, ws);
  UM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lt_finish_kernel, dim3(1), dim3(LNT), 0, st, ws, nb,
                     1.0 / ((double)N * H * W), out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_consistency_bwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                       long i_sn, long i_sc, long i_sp, int N, int H, int W, const float* g,
                       float* gdisp, float* gimages, float* scratch, int alias,
                       hipStream_t st) {
  LT_GEOM("um_consistency_bwd", 2);
  UM_CHECK_ARG(g != nullptr && (gdisp != nullptr || gimages != nullptr),
               "um_consistency_bwd: null gradient");
  UM_CHECK_ARG(gimages == nullptr || scratch != nullptr,
               "um_consistency_bwd: the image gradient needs the [N][2][H][W] scratch");
  UM_CHECK_ARG(!alias || (gdisp != nullptr && gimages != nullptr),
               "um_consistency_bwd: alias needs gdisp (the direct part) and gimages (the sum)");
  UM_CHECK_ARG((long)W * 4 <= SCATTER_LDS && H <= 65535 && N <= 65535,
               "um_consistency_bwd: W = %d exceeds the scatter's LDS limit of %ld floats", W,
               SCATTER_LDS / 4);
  const SView dv{disp, d_sn, d_sc, d_sp}, iv{images, i_sn, i_sc, i_sp};
  hipLaunchKernelGGL(lt_consistency_adj_kernel, dim3(lt_grid(2L * N * H * W)), dim3(LNT), 0, st,
                     dv, iv, N, H, W, g, gdisp, gimages != nullptr ? scratch : nullptr);
  UM_LAUNCH_CHECK();
  if (gimages != nullptr) {
    hipLaunchKernelGGL(lt_consistency_scatter_kernel, dim3(H, 2, N), dim3(LNT), (size_t)W * 4, st,
                       scratch, dv, H, W, alias ? gdisp : nullptr, gimages);
    UM_LAUNCH_CHECK();
  }
  return UM_OK;
}

int um_smoothness_fwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                      int N, int H, int W, double* ws, float* out, hipStream_t st) {
  LT_GEOM("um_smoothness_fwd", 2);
  const int nb = lt_grid(2L * N * H * W);
  hipLaunchKernelGGL(lt_smoothness_fwd_kernel, dim3(nb), dim3(LNT), 0, st,
                     SView{disp, d_sn, d_sc, d_sp}, images, N, H, W, ws);
  UM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lt_finish_kernel, dim3(1), dim3(LNT), 0, st, ws, nb,
                     1.0 / ((double)N * H * W), out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_smoothness_bwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                      int N, int H, int W, const float* g, float* gdisp, hipStream_t st) {
  LT_GEOM("um_smoothness_bwd", 2);
  hipLaunchKernelGGL(lt_smoothness_bwd_kernel, dim3(lt_grid(2L * N * H * W)), dim3(LNT), 0, st,
                     SView{disp, d_sn, d_sc, d_sp}, images, N, H, W, g, gdisp);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_nll_fwd(const float* unc, long u_sn, long u_sc, long u_sp, const float* err, long e_sn,
               long e_sc, long e_sp, int N, int H, int W, int loss_type, double* ws, float* out,
               hipStream_t st) {
  LT_GEOM("um_nll_fwd", 1);
  UM_CHECK_ARG(loss_type >= 0 && loss_type <= 2, "um_nll_fwd: loss_type %d", loss_type);
  const int nb = lt_grid(2L * N * H * W);
  hipLaunchKernelGGL(lt_nll_fwd_kernel, dim3(nb), dim3(LNT), 0, st, SView{unc, u_sn, u_sc, u_sp},
                     SView{err, e_sn, e_sc, e_sp}, N, H, W, loss_type, ws);
  UM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lt_finish_kernel, dim3(1), dim3(LNT), 0, st, ws, nb,
                     1.0 / (2.0 * N * H * W), out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_nll_bwd(const float* unc, long u_sn, long u_sc, long u_sp, const float* err, long e_sn,
               long e_sc, long e_sp, int N, int H, int W, int loss_type, const float* g,
               float* gunc, hipStream_t st) {
  LT_GEOM("um_nll_bwd", 1);
  UM_CHECK_ARG(loss_type >= 0 && loss_type <= 2, "um_nll_bwd: loss_type %d", loss_type);
  hipLaunchKernelGGL(lt_nll_bwd_kernel, dim3(lt_grid(2L * N * H * W)), dim3(LNT), 0, st,
                     SView{unc, u_sn, u_sc, u_sp}, SView{err, e_sn, e_sc, e_sp}, N, H, W,
                     loss_type, g, gunc);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
