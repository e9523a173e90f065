// Evaluation metrics (reference train/evaluate.py:66-196 and
// train/sparsification.py:8-61), off the training hot path:
//
//   um_ssim_gauss       torchmetrics structural_similarity_index_measure as the
//                       reference calls it (gaussian window, sigma 1.5 -> 11
//                       taps, data_range 1, k1 0.01, k2 0.03): per-image mean
//                       of the SSIM map over the interior (the torchmetrics
//                       crop of its reflect padding = every full window).
//   um_avgpool_valid    nn.AvgPool2d(k, stride=1) (no padding)
//   um_spars_sort       per (image, view) segment: sort the predicted error
//                       descending and carry the oracle error along
//                       (argsort + gather, sparsification.py:18-19), hipCUB
//                       segmented radix sort
//   um_spars_curve      the 100-step sparsification curve: mean of the
//                       oracle error left after removing the first
//                       int(step/steps * L) sorted pixels, over its full mean,
//                       averaged over the segments (sparsification.py:21-36)
//
// and the fused per-batch form of the same metrics for the captured
// evaluation engine (umamd/evalengine.py):
//
//   um_eval_maps        both reconstructions (train/utils.py:65-109), their
//                       gaussian SSIM sums (evaluate.py:142-146) and the
//                       image error map (evaluate.py:151 -> loss.py:96-131)
//                       in one launch + a finish launch
//   um_eval_pool        the 11x11 average pools of sparsification.py:14-16
//                       for the error, uncertainty and random maps in one
//                       separable launch, written as sort-ready segments
//   um_eval_accum       ause / aurg (sparsification.py:43-61) of the three
//                       curves, added into the running sums of
//                       evaluate.py:160-176 on the device
#include <hipcub/hipcub.hpp>

#include "common.h"
#include "lossdev.h"

namespace {

// -------------------------------------------------------- gaussian SSIM ----
constexpr int SK = 11, SR = 5;           // 11-tap window (sigma 1.5)
constexpr int STY = 16, STX = 64;        // output tile
constexpr int SRY = STY + 2 * SR, SRX = STX + 2 * SR;

struct SsimArgs {
  const float* x;  // preds  [N][C][H][W]
  const float* y;  // target
  int N, C, H, W;
  float c1, c2;
  float g[SK];      // normalised 1-D gaussian
  double* parts;    // [N][tiles] partial sums of the SSIM map
  int tiles_x, tiles_y;
};

__global__ void __launch_bounds__(256) ssim_gauss_kernel(SsimArgs a) {
  __shared__ float sx[SRY][SRX], sy[SRY][SRX];
  __shared__ float hq[5][SRY][STX];  // horizontal pass of x, y, xx, yy, xy
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int per = a.tiles_x * a.tiles_y;
  const int n = blockIdx.x / per, t = blockIdx.x - n * per;
  // output coordinates are in the valid region: pixel (oy, ox) is the window
  // centred at image (oy + SR, ox + SR)
  const int oy0 = (t / a.tiles_x) * STY, ox0 = (t % a.tiles_x) * STX;
  const int OH = a.H - 2 * SR, OW = a.W - 2 * SR;
  double acc = 0.0;
  for (int c = 0; c < a.C; ++c) {
    const float* X = a.x + ((long)n * a.C + c) * a.H * a.W;
    const float* Y = a.y + ((long)n * a.C + c) * a.H * a.W;
    for (int i = tid; i < SRY * SRX; i += 256) {
      const int r = i / SRX, q = i % SRX;
      const int yy = min(oy0 + r, a.H - 1), xx = min(ox0 + q, a.W - 1);
      sx[r][q] = X[(long)yy * a.W + xx];
      sy[r][q] = Y[(long)yy * a.W + xx];
    }
    __syncthreads();
    for (int i = tid; i < SRY * STX; i += 256) {
      const int r = i / STX, q = i % STX;
      float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < SK; ++k) {
        const float xv = sx[r][q + k], yv = sy[r][q + k], w = a.g[k];
        v[0] += w * xv;
        v[1] += w * yv;
        v[2] += w * xv * xv;
        v[3] += w * yv * yv;
        v[4] += w * xv * yv;
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) hq[k][r][q] = v[k];
    }
    __syncthreads();
    for (int i = tid; i < STY * STX; i += 256) {
      const int r = i / STX, q = i % STX;
      if (oy0 + r >= OH || ox0 + q >= OW) continue;
      float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < SK; ++k)
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j] += a.g[k] * hq[j][r + k][q];
      const float mx2 = v[0] * v[0], my2 = v[1] * v[1], mxy = v[0] * v[1];
      const float sxx = v[2] - mx2, syy = v[3] - my2, sxy = v[4] - mxy;
      acc += (double)(((2.f * mxy + a.c1) * (2.f * sxy + a.c2)) /
                      ((mx2 + my2 + a.c1) * (sxx + syy + a.c2)));
    }
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) a.parts[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[n] = sum of the image's tile partials / (C * OH * OW)
__global__ void ssim_finish_kernel(const double* parts, int N, int tiles, double count,
                                   float* out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += parts[(long)n * tiles + t];
  out[n] = (float)(s / count);
}

// ------------------------------------------------------- average pooling ---
__global__ void avgpool_valid_kernel(const float* __restrict__ x, int NC, int H, int W, int k,
                                     float* __restrict__ out) {
  const int OH = H - k + 1, OW = W - k + 1;
  const long total = (long)NC * OH * OW;
  const float inv = 1.f / (float)(k * k);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int ox = i % OW;
    const int oy = (i / OW) % OH;
    const long pl = i / ((long)OW * OH);
    const float* p = x + pl * H * W + (long)oy * W + ox;
    float s = 0.f;
    for (int u = 0; u < k; ++u)
      for (int v = 0; v < k; ++v) s += p[(long)u * W + v];
    out[i] = s * inv;
  }
}

// -------------------------------------------------- sparsification curve --
__global__ void seg_offsets_kernel(int* offs, int nseg, int L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nseg) offs[i] = i * L;
}

// one workgroup per segment: normalised[seg][k] = mean(sorted[cut_k:]) / mean(all)
__global__ void __launch_bounds__(256) spars_curve_kernel(const float* __restrict__ sorted, int L,
                                                          int steps, double* __restrict__ norm) {
  extern __shared__ double isum[];  // [steps]
  const float* v = sorted + (long)blockIdx.x * L;
  auto cut = [&](int k) { return (int)((double)k / (double)steps * (double)L); };
  for (int k = threadIdx.x; k < steps; k += blockDim.x) {
    const int c0 = cut(k), c1 = k + 1 < steps ? cut(k + 1) : L;
    double s = 0.0;
    for (int i = c0; i < c1; ++i) s += (double)v[i];
    isum[k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double suffix = 0.0;
    for (int k = steps - 1; k >= 0; --k) {
      suffix += isum[k];
      isum[k] = suffix;
    }
    const double mean = isum[0] / (double)L;
    for (int k = 0; k < steps; ++k)
      norm[(long)blockIdx.x * steps + k] = (isum[k] / (double)(L - cut(k))) / mean;
  }
}

__global__ void spars_mean_kernel(const double* norm, int nseg, int steps, float* curve) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= steps) return;
  double s = 0.0;
  for (int g = 0; g < nseg; ++g) s += norm[(long)g * steps + k];
  curve[k] = (float)(s / (double)nseg);
}

// ------------------------------------------------------ fused eval maps ----
// The reconstruction and the grid-to-pixel upsample are the loss kernels' own
// helpers (lossdev.h: warp_at, sample, up_tap, dssim_up).
constexpr int MTY = 16, MTX = 64;                    // pixel tile of one workgroup
constexpr int MRY = MTY + 2 * SR, MRX = MTX + 2 * SR;  // staged: tile + gaussian halo
constexpr int MGY = Tile<MTY, MTX>::GY, MGX = Tile<MTY, MTX>::GX;  // 3x3-SSIM grid points
constexpr int MG0 = SR - 2;  // staged row / column of grid point 0 (pixel tile origin - 2)

// SSIM of the 3x3 window whose top-left is staged (r, q) (train/loss.py:43-74).
// The same arithmetic as ssim_of(win_stats()) of lossdev.h, written out here:
// which multiply-adds the compiler fuses depends on the shape of the code
// around them, that call gives other last bits in this kernel than this form,
// and the error map is kept bit-stable.
__device__ __forceinline__ float ssim3(const float (*I)[MRX], const float (*R)[MRX], int r,
                                       int q) {
  constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f, k9 = 1.f / 9.f;
  float sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const float xv = I[r + u][q + w], yv = R[r + u][q + w];
      sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv; sxy += xv * yv;
    }
  const float mx = sx * k9, my = sy * k9;
  const float vx = sxx * k9 - mx * mx, vy = syy * k9 - my * my, vxy = sxy * k9 - mx * my;
  return ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
}

struct MapsArgs {
  const float* left;   // [N][3][H][W]
  const float* right;
  const float* pred;   // element (n, y, x, ch) at pred[n*psn + (y*W + x)*psp + ch]
  long psn, psp;
  int N, H, W, tiles_x, tiles_y;
  float c1, c2;
  float g[SK];
  float* recon;   // [N][6][H][W] or null
  float* err;     // [N][2][H][W]
  double* parts;  // [2][N][tiles] partial sums of the gaussian SSIM map
};

// One workgroup per (image, view, 16x64 pixel tile).  Per channel it stages
// the view and its reconstruction over the tile + 5-pixel halo, then
//   * the gaussian SSIM of every full 11x11 window centred in the tile
//     (separable, as ssim_gauss_kernel), summed in f64 into parts;
//   * the 3x3 SSIM dissimilarity on the tile's grid points, summed over the
//     channels in LDS (as lt_image_error_kernel of lossterms.hip);
// and finally upsamples the dissimilarity grid to the tile's pixels.
__global__ void __launch_bounds__(256) eval_maps_kernel(MapsArgs a) {
  __shared__ float sI[MRY][MRX], sR[MRY][MRX];
  __shared__ float hq[5][MRY][MTX];
  __shared__ float sD[MGY][MGX];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const long HW = (long)H * W;
  const int per = a.tiles_x * a.tiles_y;
  const int nv = blockIdx.x / per, t = blockIdx.x - nv * per;
  const int n = nv >> 1, v = nv & 1;
  const int ty0 = (t / a.tiles_x) * MTY, tx0 = (t % a.tiles_x) * MTX;
  const int gh = H - 2, gw = W - 2;
  // left view: the right image sampled at x - d_L; right view: left at x + d_R
  const float* view = (v == 0 ? a.left : a.right) + (long)n * 3 * HW;
  const float* opp = (v == 0 ? a.right : a.left) + (long)n * 3 * HW;
  const float* disp = a.pred + n * a.psn + v;
  const float sign = v == 0 ? -1.f : 1.f;
  for (int i = tid; i < MGY * MGX; i += 256) (&sD[0][0])[i] = 0.f;
  double acc = 0.0;
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < MRY * MRX; i += 256) {
      const int r = i / MRX, q = i - r * MRX;
      const int y = ty0 - SR + r, x = tx0 - SR + q;
      float iv = 0.f, rv = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const long o = (long)y * W + x;
        iv = view[c * HW + o];
        rv = sample(opp + c * HW, warp_at(x, y, sign * disp[o * a.psp], W, H), H, W, 1, nullptr);
        if (a.recon != nullptr && r >= SR && r < SR + MTY && q >= SR && q < SR + MTX)
          a.recon[((long)n * 6 + v * 3 + c) * HW + o] = rv;
      }
      sI[r][q] = iv;
      sR[r][q] = rv;
    }
    __syncthreads();
    // horizontal gaussian pass of recon (x), view (y), xx, yy, xy
    for (int i = tid; i < MRY * MTX; i += 256) {
      const int r = i / MTX, q = i % MTX;
      float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < SK; ++k) {
        const float xv = sR[r][q + k], yv = sI[r][q + k], w = a.g[k];
        h[0] += w * xv;
        h[1] += w * yv;
        h[2] += w * xv * xv;
        h[3] += w * yv * yv;
        h[4] += w * xv * yv;
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) hq[k][r][q] = h[k];
    }
    // 3x3 dissimilarity of this channel on the grid points (each entry of sD
    // belongs to one thread for the whole kernel)
    for (int i = tid; i < MGY * MGX; i += 256) {
      const int r = i / MGX, q = i - r * MGX;
      const int gy = ty0 - 2 + r, gx = tx0 - 2 + q;
      if (gy >= 0 && gy < gh && gx >= 0 && gx < gw) {
        const float ss = ssim3(sI, sR, r + MG0, q + MG0);
        sD[r][q] += fminf(fmaxf((1.f - ss) * 0.5f, 0.f), 1.f);
      }
    }
    __syncthreads();
    // vertical pass: the window centred at pixel (ty0 + r, tx0 + q)
    for (int i = tid; i < MTY * MTX; i += 256) {
      const int r = i / MTX, q = i % MTX;
      const int cy = ty0 + r, cx = tx0 + q;
      if (cy < SR || cy >= H - SR || cx < SR || cx >= W - SR) continue;
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < SK; ++k)
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] += a.g[k] * hq[j][r + k][q];
      const float mx2 = m[0] * m[0], my2 = m[1] * m[1], mxy = m[0] * m[1];
      const float sxx = m[2] - mx2, syy = m[3] - my2, sxy = m[4] - mxy;
      acc += (double)(((2.f * mxy + a.c1) * (2.f * sxy + a.c2)) /
                      ((mx2 + my2 + a.c1) * (sxx + syy + a.c2)));
    }
    __syncthreads();
  }
  for (int i = tid; i < MGY * MGX; i += 256) (&sD[0][0])[i] /= 3.f;
  __syncthreads();
  for (int i = tid; i < MTY * MTX; i += 256) {
    const int ly = i / MTX, lx = i % MTX;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    a.err[((long)n * 2 + v) * HW + (long)y * W + x] =
        dssim_up<MGX>(sD, up_tap(y, H, ty0 - 2), up_tap(x, W, tx0 - 2));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    a.parts[((long)v * a.N + n) * per + t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// acc[v] += sum over the batch of the per-image means = (sum of the view's
// partials) / (3 * OH * OW): one workgroup per view, fixed summation order
__global__ void __launch_bounds__(256) eval_maps_finish_kernel(const double* parts, int per_view,
                                                               double count, double* acc) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < per_view; i += 256) s += parts[(long)blockIdx.x * per_view + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) acc[blockIdx.x] += ((red[0] + red[1]) + (red[2] + red[3])) / count;
}

// ------------------------------------------------- fused separable pools ---
struct PoolArgs {
  const float* src[3];  // plane (n, v) of map m at src[m] + n*sn[m] + v*sv[m], pixel stride sp[m]
  long sn[3], sv[3], sp[3];
  float* out[3];        // [2N][OH*OW]
  int H, W, tiles_x;
};

// One workgroup per (map, plane, 16x64 output tile): tile + 10 rows/columns
// staged in LDS, 11 row sums, then 11 column sums, * 1/121.  Every wave reads
// 64 consecutive floats of one LDS row in both passes (no bank conflict).
__global__ void __launch_bounds__(256) eval_pool_kernel(PoolArgs a) {
  __shared__ float s[MRY][MRX];
  __shared__ float rs[MRY][MTX];
  const int tid = threadIdx.x;
  const int m = blockIdx.z, p = blockIdx.y, t = blockIdx.x;
  // wave-uniform selects (indexing the by-value argument would go to scratch)
  const float* src = m == 0 ? a.src[0] : m == 1 ? a.src[1] : a.src[2];
  const long sn = m == 0 ? a.sn[0] : m == 1 ? a.sn[1] : a.sn[2];
  const long sv = m == 0 ? a.sv[0] : m == 1 ? a.sv[1] : a.sv[2];
  const long sp = m == 0 ? a.sp[0] : m == 1 ? a.sp[1] : a.sp[2];
  float* out = m == 0 ? a.out[0] : m == 1 ? a.out[1] : a.out[2];
  const int H = a.H, W = a.W, OH = H - SK + 1, OW = W - SK + 1;
  const int oy0 = (t / a.tiles_x) * MTY, ox0 = (t % a.tiles_x) * MTX;
  const float* plane = src + (p >> 1) * sn + (p & 1) * sv;
  for (int i = tid; i < MRY * MRX; i += 256) {
    const int r = i / MRX, q = i - r * MRX;
    const int y = min(oy0 + r, H - 1), x = min(ox0 + q, W - 1);
    s[r][q] = plane[((long)y * W + x) * sp];
  }
  __syncthreads();
  for (int i = tid; i < MRY * MTX; i += 256) {
    const int r = i / MTX, q = i % MTX;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < SK; ++k) v += s[r][q + k];
    rs[r][q] = v;
  }
  __syncthreads();
  for (int i = tid; i < MTY * MTX; i += 256) {
    const int r = i / MTX, q = i % MTX;
    const int oy = oy0 + r, ox = ox0 + q;
    if (oy >= OH || ox >= OW) continue;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < SK; ++k) v += rs[r + k][q];
    out[(long)p * OH * OW + (long)oy * OW + ox] = v * (1.f / (float)(SK * SK));
  }
}

// acc[2] += sum(pred - oracle) / steps, acc[3] += sum(random - pred) / steps,
// acc[4] += 1 (one wave)
__global__ void __launch_bounds__(64) eval_accum_kernel(const float* __restrict__ oracle,
                                                        const float* __restrict__ pred,
                                                        const float* __restrict__ random,
                                                        int steps, double* acc) {
  double au = 0.0, ag = 0.0;
  for (int k = threadIdx.x; k < steps; k += 64) {
    au += (double)(pred[k] - oracle[k]);
    ag += (double)(random[k] - pred[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    au += __shfl_xor(au, o, 64);
    ag += __shfl_xor(ag, o, 64);
  }
  if (threadIdx.x == 0) {
    acc[2] += au / (double)steps;
    acc[3] += ag / (double)steps;
    acc[4] += 1.0;
  }
}

// torchmetrics _gaussian: arange((1-k)/2, (1+k)/2) in f32, exp(-(d/s)^2/2), / sum
void gauss_window(float sigma, float* g) {
  float gs = 0.f;
  for (int k = 0; k < SK; ++k) {
    const float d = (float)(k - SR) / sigma;
    g[k] = expf(-(d * d) / 2.f);
    gs += g[k];
  }
  for (int k = 0; k < SK; ++k) g[k] /= gs;
}

}  // namespace

extern "C" {

long um_ssim_ws(int N, int H, int W) {
  const int OH = H - 2 * SR, OW = W - 2 * SR;
  if (OH <= 0 || OW <= 0) return 0;
  return (long)N * ceil_div(OH, STY) * ceil_div(OW, STX) * sizeof(double);
}

int um_ssim_gauss(const float* x, const float* y, int N, int C, int H, int W, float data_range,
                  float sigma, double* ws, float* out, hipStream_t st) {
  UM_CHECK_ARG((int)(3.5f * sigma + 0.5f) * 2 + 1 == SK,
               "um_ssim_gauss: sigma %g gives a window other than %d taps", sigma, SK);
  UM_CHECK_ARG(H > 2 * SR && W > 2 * SR, "um_ssim_gauss: image %dx%d smaller than the window",
               H, W);
  SsimArgs a{};
  a.x = x; a.y = y; a.N = N; a.C = C; a.H = H; a.W = W;
  a.c1 = (0.01f * data_range) * (0.01f * data_range);
  a.c2 = (0.03f * data_range) * (0.03f * data_range);
  gauss_window(sigma, a.g);
  a.tiles_y = ceil_div(H - 2 * SR, STY);
  a.tiles_x = ceil_div(W - 2 * SR, STX);
  a.parts = ws;
  const int tiles = a.tiles_x * a.tiles_y;
  hipLaunchKernelGGL(ssim_gauss_kernel, dim3(N * tiles), dim3(256), 0, st, a);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(ceil_div(N, 64)), dim3(64), 0, st, ws, N, tiles,
                     (double)C * (H - 2 * SR) * (W - 2 * SR), out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_avgpool_valid(const float* x, int NC, int H, int W, int k, float* out, hipStream_t st) {
  UM_CHECK_ARG(k >= 1 && k <= H && k <= W, "um_avgpool_valid: window %d vs %dx%d", k, H, W);
  const long total = (long)NC * (H - k + 1) * (W - k + 1);
  long b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  hipLaunchKernelGGL(avgpool_valid_kernel, dim3((int)std::max(b, 1l)), dim3(256), 0, st, x, NC, H,
                     W, k, out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

// scratch bytes of um_spars_sort (segment offsets + hipCUB temporary storage)
long um_spars_sort_ws(int nseg, int L) {
  size_t bytes = 0;
  hipcub::DeviceSegmentedRadixSort::SortPairsDescending(
      nullptr, bytes, (const float*)nullptr, (float*)nullptr, (const float*)nullptr,
      (float*)nullptr, nseg * L, nseg, (const int*)nullptr, (const int*)nullptr);
  return (long)bytes + (long)(nseg + 1) * sizeof(int) + 256;
}

int um_spars_sort(const float* keys, const float* vals, int nseg, int L, float* keys_out,
                  float* vals_out, void* ws, long ws_bytes, hipStream_t st) {
  int* offs = reinterpret_cast<int*>(ws);
  char* tmp = reinterpret_cast<char*>(ws) + (((nseg + 1) * sizeof(int) + 255) / 256) * 256;
  size_t bytes = (size_t)(ws_bytes - (tmp - reinterpret_cast<char*>(ws)));
  hipLaunchKernelGGL(seg_offsets_kernel, dim3(ceil_div(nseg + 1, 256)), dim3(256), 0, st, offs,
                     nseg, L);
  const hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairsDescending(
      tmp, bytes, keys, keys_out, vals, vals_out, nseg * L, nseg, offs, offs + 1, 0,
      sizeof(float) * 8, st);
  UM_CHECK_ARG(e == hipSuccess, "um_spars_sort: hipcub %s", hipGetErrorString(e));
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_spars_curve(const float* sorted_vals, int nseg, int L, int steps, double* ws,
                   float* curve, hipStream_t st) {
  UM_CHECK_ARG(steps >= 1 && steps <= 4096 && L >= 1, "um_spars_curve: steps %d, L %d", steps, L);
  hipLaunchKernelGGL(spars_curve_kernel, dim3(nseg), dim3(256), steps * sizeof(double), st,
                     sorted_vals, L, steps, ws);
  hipLaunchKernelGGL(spars_mean_kernel, dim3(ceil_div(steps, 128)), dim3(128), 0, st, ws, nseg,
                     steps, curve);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

long um_eval_ws(int N, int H, int W) {
  if (N <= 0 || H <= 2 * SR || W <= 2 * SR) return 0;
  return 2l * N * ceil_div(H, MTY) * ceil_div(W, MTX) * sizeof(double);
}

int um_eval_maps(const float* left, const float* right, const float* pred, long pred_sn,
                 long pred_sp, int N, int H, int W, float* recon, float* err, double* ws,
                 double* acc, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && H > 2 * SR + 1 && W > 2 * SR + 1,
               "um_eval_maps: batch %d of %dx%d images (needs N >= 1, H and W >= 12)", N, H, W);
  MapsArgs a{};
  a.left = left; a.right = right; a.pred = pred; a.psn = pred_sn; a.psp = pred_sp;
  a.N = N; a.H = H; a.W = W;
  a.tiles_y = ceil_div(H, MTY);
  a.tiles_x = ceil_div(W, MTX);
  a.c1 = 0.01f * 0.01f;  // data range 1
  a.c2 = 0.03f * 0.03f;
  gauss_window(1.5f, a.g);
  a.recon = recon; a.err = err; a.parts = ws;
  const long per_view = (long)N * a.tiles_x * a.tiles_y;
  UM_CHECK_ARG(2 * per_view < (1l << 31), "um_eval_maps: %ld workgroups", 2 * per_view);
  hipLaunchKernelGGL(eval_maps_kernel, dim3((unsigned)(2 * per_view)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(eval_maps_finish_kernel, dim3(2), dim3(256), 0, st, ws, (int)per_view,
                     3.0 * (H - 2 * SR) * (W - 2 * SR), acc);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_eval_pool(const float* err, const float* pred, long pred_sn, long pred_sp,
                 const float* rnd, int N, int H, int W, int k, float* err_out, float* unc_out,
                 float* rnd_out, hipStream_t st) {
  UM_CHECK_ARG(k == SK, "um_eval_pool: window %d (only the reference's %d is built)", k, SK);
  UM_CHECK_ARG(N >= 1 && 2 * N <= 65535 && H >= SK && W >= SK,
               "um_eval_pool: batch %d of %dx%d maps", N, H, W);
  const long HW = (long)H * W;
  PoolArgs a{};
  a.src[0] = err; a.sn[0] = 2 * HW; a.sv[0] = HW; a.sp[0] = 1; a.out[0] = err_out;
  a.src[1] = pred + 2; a.sn[1] = pred_sn; a.sv[1] = 1; a.sp[1] = pred_sp; a.out[1] = unc_out;
  a.src[2] = rnd; a.sn[2] = 2 * HW; a.sv[2] = HW; a.sp[2] = 1; a.out[2] = rnd_out;
  a.H = H; a.W = W;
  a.tiles_x = ceil_div(W - SK + 1, MTX);
  const int tiles = a.tiles_x * ceil_div(H - SK + 1, MTY);
  hipLaunchKernelGGL(eval_pool_kernel, dim3(tiles, 2 * N, 3), dim3(256), 0, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_eval_accum(const float* oracle_curve, const float* pred_curve, const float* random_curve,
                  int steps, double* acc, hipStream_t st) {
  UM_CHECK_ARG(steps >= 1, "um_eval_accum: %d steps", steps);
  hipLaunchKernelGGL(eval_accum_kernel, dim3(1), dim3(64), 0, st, oracle_curve, pred_curve,
                     random_curve, steps, acc);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
