// Deployment path around the inference engine (umamd/deploy.py): a camera
// frame in, metric depth with a confidence mask out.
//
//   um_frame_prep   ResizeImage -> ToTensor (reference train/transforms.py:
//                   15-41) of ONE view in one launch, written straight into
//                   the engine's static input.  Pillow's two-pass 8-bit
//                   resampler as imageprep.hip runs it (same host-made
//                   tables, same integer arithmetic, bit-identical result),
//                   but a workgroup keeps the 8-bit intermediate of its tile
//                   in LDS instead of a global buffer.
//   um_depth_post   everything after the forward at the frame's size: the
//                   left-right consistency error (the left half of
//                   ConsistencyLoss, train/loss.py:179-185, with the warp of
//                   train/utils.py:65-103), the align_corners=True upsample
//                   (loss.py:120-121), pixels, depth and the validity mask.
#include <hip/hip_runtime.h>
#include <limits.h>

// No FMA contraction in this file's own code or in the helpers it takes from
// common.h (up_index), every fused multiply-add is written out: the aligned
// and the unaligned form of depth_post_kernel (and any later variant) then
// round alike and agree bit for bit, instead of by whichever fusion each
// instantiation happened to get.  (frame_prep_kernel is integer arithmetic.)
#pragma clang fp contract(off)

#include "common.h"

namespace {

// ---------------------------------------------------------- frame prep ----
// The arithmetic lines are this file's own copy of imageprep.hip's
// (resample_h_kernel / resample_v_kernel), kept here so that translation
// unit does not change.
constexpr int PREC = 22;  // Pillow PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ uint32_t clip8(int ss) {
  int v = ss >> PREC;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int FT_ROWS = 8, FT_COLS = 32;  // output tile of one workgroup (256 threads)
constexpr int FT_LDS = 64 * 1024;         // LDS budget of a tile's horizontal pass
constexpr int FT_MAX_ROWS = FT_LDS / (FT_COLS * 4);  // 512 source rows, one u8x4 per pixel
constexpr int FT_MAX_KS_H = 257;          // horizontal taps a thread walks (downscale <= 128x)

// source rows a tile of FT_ROWS output rows can need: the first tap of its
// last row lies at most ceil((FT_ROWS - 1) * Hs / Hd) + 1 rows after the
// first tap of its first row (Pillow truncates the window start), and a row
// has at most ks_v taps
inline long tile_src_rows(int Hs, int Hd, int ks_v) {
  return ((long)(FT_ROWS - 1) * Hs + Hd - 1) / Hd + 1 + ks_v;
}

// grid (column tiles, row tiles, N); dynamic LDS: cap_rows * FT_COLS u8x4
__global__ void __launch_bounds__(256)
frame_prep_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int Hd, int Wd,
                  const int* __restrict__ bounds_h, const int* __restrict__ kk_h, int ks_h,
                  const int* __restrict__ bounds_v, const int* __restrict__ kk_v, int ks_v,
                  int cap_rows, float* __restrict__ out) {
  extern __shared__ uint32_t tile[];  // [rows][FT_COLS] r | g << 8 | b << 16
  const int x0 = blockIdx.x * FT_COLS, y0 = blockIdx.y * FT_ROWS, n = blockIdx.z;
  const int ny = min(FT_ROWS, Hd - y0), nx = min(FT_COLS, Wd - x0);
  // the source rows the tile's vertical taps need (every index clamped, so a
  // table that does not belong to these sizes cannot reach outside a buffer)
  int r0 = INT_MAX, r1 = 0;
  for (int y = 0; y < ny; ++y) {
    const int a = bounds_v[2 * (y0 + y)], c = min(bounds_v[2 * (y0 + y) + 1], ks_v);
    r0 = min(r0, a);
    r1 = max(r1, a + c);
  }
  r0 = max(r0, 0);
  const int rows = min(min(r1, Hs) - r0, cap_rows);

  // pass 1: the horizontal pass of rows [r0, r0 + rows), columns [x0, x0 + nx)
  const uint8_t* img = src + ((long)n * Hs + r0) * Ws * 3;
  for (int i = threadIdx.x; i < rows * FT_COLS; i += blockDim.x) {
    const int r = i / FT_COLS, xx = i % FT_COLS;
    if (xx >= nx) continue;
    const int xmin = max(bounds_h[2 * (x0 + xx)], 0);
    const int xmax = min(min(bounds_h[2 * (x0 + xx) + 1], ks_h), Ws - xmin);
    const int* k = kk_h + (long)(x0 + xx) * ks_h;
    const uint8_t* row = img + (long)r * Ws * 3;
    int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < xmax; ++x) {
      const uint8_t* p = row + (xmin + x) * 3;
      const int w = k[x];
      s0 += (int)p[0] * w;
      s1 += (int)p[1] * w;
      s2 += (int)p[2] * w;
    }
    tile[i] = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16);
  }
  __syncthreads();

  // pass 2: the vertical pass out of LDS and ToTensor, one output pixel per thread
  const int yy = threadIdx.x / FT_COLS, x = threadIdx.x % FT_COLS;
  if (yy >= ny || x >= nx) return;
  const int ymin = max(bounds_v[2 * (y0 + yy)] - r0, 0);
  const int ymax = min(min(bounds_v[2 * (y0 + yy) + 1], ks_v), rows - ymin);
  const int* k = kk_v + (long)(y0 + yy) * ks_v;
  int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
  for (int y = 0; y < ymax; ++y) {
    const uint32_t p = tile[(ymin + y) * FT_COLS + x];
    const int w = k[y];
    s0 += (int)(p & 255u) * w;
    s1 += (int)((p >> 8) & 255u) * w;
    s2 += (int)((p >> 16) & 255u) * w;
  }
  // ToTensor: float(u8) / 255 (IEEE division, as torch's div)
  const long plane = (long)Hd * Wd;
  float* o = out + (long)n * 3 * plane + (long)(y0 + yy) * Wd + (x0 + x);
  o[0] = (float)clip8(s0) / 255.0f;
  o[plane] = (float)clip8(s1) / 255.0f;
  o[2 * plane] = (float)clip8(s2) / 255.0f;
}

// ---------------------------------------------------------- depth post ----
// (contraction is off, see the top of the file: the fused multiply-adds below
// are the written ones)
struct PostArgs {
  const float* pred;
  long sn, sp;
  int N, H, W, Hs, Ws;
  const float* params;
  float *disparity, *depth, *uncertainty, *lr_error;
  uint8_t* valid;
};

// torch.linspace(0, 1, n) in f32 (CPU kernel: symmetric halves), n >= 2
__device__ __forceinline__ float lin01(int i, int n) {
  const float step = 1.f / (float)(n - 1);
  return (i < n / 2) ? step * (float)i : fmaf(-step, (float)(n - 1 - i), 1.f);
}

// |d_L - reconstruct_left_image(d_L, d_R)| at model pixel (y, x): d_R sampled
// (grid_sample bilinear, zeros padding, align_corners=False) at the
// reference's linspace(0, 1) grid shifted by -d_L, which un-normalises to
// x * W / (W - 1) - 0.5 - d_L * W, y * H / (H - 1) - 0.5
__device__ __forceinline__ float lr_at(const float* img, long sp, int y, int x, int H, int W,
                                       float dl) {
  const float ix = fmaf(lin01(x, W) - dl, (float)W, -0.5f);
  const float iy = fmaf(lin01(y, H), (float)H, -0.5f);
  const float fx = floorf(ix), fy = floorf(iy);
  const float w = ix - fx, e = 1.f - w, n = iy - fy, s = 1.f - n;
  // NaN or out-of-range positions: no tap is inside (the comparisons fail)
  const bool xa = fx >= 0.f && fx <= (float)(W - 1), xb = fx >= -1.f && fx <= (float)(W - 2);
  const bool ya = fy >= 0.f && fy <= (float)(H - 1), yb = fy >= -1.f && fy <= (float)(H - 2);
  const int x0 = xa || xb ? (int)fx : 0, y0 = ya || yb ? (int)fy : 0;
  const float* p = img + 1;  // channel 1: d_R
  const float nw = (ya && xa) ? p[((long)y0 * W + x0) * sp] : 0.f;
  const float ne = (ya && xb) ? p[((long)y0 * W + x0 + 1) * sp] : 0.f;
  const float sw = (yb && xa) ? p[((long)(y0 + 1) * W + x0) * sp] : 0.f;
  const float se = (yb && xb) ? p[((long)(y0 + 1) * W + x0 + 1) * sp] : 0.f;
  return fabsf(dl - fmaf(se, n * w, fmaf(sw, n * e, fmaf(ne, s * w, nw * (s * e)))));
}

// the four model-resolution taps of an output pixel: d_L, sigma_L and the
// left-right error at (ya|yb, xa|xb); neighbouring output pixels of an
// upscale share them, so a thread keeps the last set
struct Taps {
  int n, ya, yb, xa, xb;
  float d[4], s[4], e[4];
};

__device__ __forceinline__ float lerp4(const float* v, float ly, float lx) {
  const float hy = 1.f - ly, hx = 1.f - lx;
  return fmaf(ly, fmaf(lx, v[3], hx * v[2]), hy * fmaf(lx, v[1], hx * v[0]));
}

// one thread per 4 consecutive pixels of the flat [N][Hs][Ws] outputs; VEC:
// every output pointer is aligned for one 16-byte (valid: 4-byte) store
template <bool VEC>
__global__ void __launch_bounds__(256) depth_post_kernel(PostArgs a) {
  const long total = (long)a.N * a.Hs * a.Ws;
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= total) return;
  const float fb = a.params[0], min_disp = a.params[1], max_unc = a.params[2],
              max_lr = a.params[3];
  const bool need_e = a.lr_error != nullptr || a.valid != nullptr;
  Taps t;
  t.n = -1;
  float disp[4], dep[4], unc[4], lre[4];
  uint32_t ok = 0;
  // pixel i0 = (image n, row y, column x): one 64-bit and one 32-bit division
  // per thread (N * Hs fits an int, checked on the host); the next three
  // pixels step along the row
  const long row = i0 / a.Ws;
  int x = (int)(i0 - row * a.Ws);
  int n = (int)row / a.Hs;
  int y = (int)row - n * a.Hs;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j > 0 && i0 + j < total && ++x == a.Ws) {  // a tail repeats the last pixel
      x = 0;
      if (++y == a.Hs) {
        y = 0;
        ++n;
      }
    }
    int ya, yb, xa, xb;
    float ly, lx;
    up_index(y, a.H, a.Hs, ya, yb, ly);
    up_index(x, a.W, a.Ws, xa, xb, lx);
    if (n != t.n || ya != t.ya || yb != t.yb || xa != t.xa || xb != t.xb) {
      const float* img = a.pred + (long)n * a.sn;
      const int ty[4] = {ya, ya, yb, yb}, tx[4] = {xa, xb, xa, xb};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* p = img + ((long)ty[q] * a.W + tx[q]) * a.sp;
        t.d[q] = p[0];
        t.s[q] = p[2];
        t.e[q] = need_e ? lr_at(img, a.sp, ty[q], tx[q], a.H, a.W, t.d[q]) : 0.f;
      }
      t.n = n; t.ya = ya; t.yb = yb; t.xa = xa; t.xb = xb;
    }
    disp[j] = lerp4(t.d, ly, lx) * (float)a.Ws;
    unc[j] = lerp4(t.s, ly, lx);
    lre[j] = lerp4(t.e, ly, lx) * (float)a.Ws;
    const bool far = disp[j] > min_disp;
    dep[j] = far ? fb / disp[j] : 0.f;
    ok |= (uint32_t)(far && unc[j] <= max_unc && lre[j] <= max_lr) << (8 * j);
  }
  if (VEC && i0 + 4 <= total) {
    if (a.disparity) *reinterpret_cast<float4*>(a.disparity + i0) =
        make_float4(disp[0], disp[1], disp[2], disp[3]);
    if (a.depth) *reinterpret_cast<float4*>(a.depth + i0) =
        make_float4(dep[0], dep[1], dep[2], dep[3]);
    if (a.uncertainty) *reinterpret_cast<float4*>(a.uncertainty + i0) =
        make_float4(unc[0], unc[1], unc[2], unc[3]);
    if (a.lr_error) *reinterpret_cast<float4*>(a.lr_error + i0) =
        make_float4(lre[0], lre[1], lre[2], lre[3]);
    if (a.valid) *reinterpret_cast<uint32_t*>(a.valid + i0) = ok;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (i0 + j >= total) break;
    if (a.disparity) a.disparity[i0 + j] = disp[j];
    if (a.depth) a.depth[i0 + j] = dep[j];
    if (a.uncertainty) a.uncertainty[i0 + j] = unc[j];
    if (a.lr_error) a.lr_error[i0 + j] = lre[j];
    if (a.valid) a.valid[i0 + j] = (uint8_t)((ok >> (8 * j)) & 1u);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int um_frame_prep_ok(int Hs, int Ws, int Hd, int Wd, int ks_h, int ks_v) {
  if (Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || ks_h <= 0 || ks_v <= 0) return 0;
  if (ks_h > FT_MAX_KS_H) return 0;
  return tile_src_rows(Hs, Hd, ks_v) <= FT_MAX_ROWS ? 1 : 0;
}

int um_frame_prep(int N, int Hs, int Ws, const unsigned char* src, int Hd, int Wd,
                  const int* bounds_h, const int* kk_h, int ks_h, const int* bounds_v,
                  const int* kk_v, int ks_v, float* out, hipStream_t st) {
  UM_CHECK_ARG(N > 0 && N <= 65535 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && ks_h > 0 && ks_v > 0,
               "um_frame_prep: bad sizes N=%d Hs=%d Ws=%d Hd=%d Wd=%d", N, Hs, Ws, Hd, Wd);
  UM_CHECK_ARG((long)Ws * 3 <= INT_MAX && (Hd + FT_ROWS - 1) / FT_ROWS <= 65535,
               "um_frame_prep: Ws=%d Hd=%d out of range", Ws, Hd);
  UM_CHECK_ARG(src && bounds_h && kk_h && bounds_v && kk_v && out, "um_frame_prep: null pointer");
  UM_CHECK_ARG(um_frame_prep_ok(Hs, Ws, Hd, Wd, ks_h, ks_v),
               "um_frame_prep: %dx%d -> %dx%d (ks_h=%d ks_v=%d) is past the resize limit: a "
               "tile of %d output rows may need ceil(%d*Hs/Hd) + 1 + ks_v = %ld source rows "
               "in LDS, at most %d (%d KiB), and ks_h at most %d",
               Hs, Ws, Hd, Wd, ks_h, ks_v, FT_ROWS, FT_ROWS - 1, tile_src_rows(Hs, Hd, ks_v),
               FT_MAX_ROWS, FT_LDS / 1024, FT_MAX_KS_H);
  long cap = tile_src_rows(Hs, Hd, ks_v);
  if (cap > Hs) cap = Hs;
  const dim3 grid((Wd + FT_COLS - 1) / FT_COLS, (Hd + FT_ROWS - 1) / FT_ROWS, N);
  hipLaunchKernelGGL(frame_prep_kernel, grid, dim3(256), (size_t)cap * FT_COLS * 4, st, src, Hs,
                     Ws, Hd, Wd, bounds_h, kk_h, ks_h, bounds_v, kk_v, ks_v, (int)cap, out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_depth_post(const float* pred, long sn, long sp, int N, int H, int W, int Hs, int Ws,
                  const float* params, float* disparity, float* depth, float* uncertainty,
                  float* lr_error, unsigned char* valid, hipStream_t st) {
  UM_CHECK_ARG(N > 0 && H >= 2 && W >= 2 && Hs >= 2 && Ws >= 2 && (long)N * Hs <= INT_MAX,
               "um_depth_post: bad sizes N=%d H=%d W=%d Hs=%d Ws=%d (every size >= 2)", N, H, W,
               Hs, Ws);
  UM_CHECK_ARG(H <= 32768 && W <= 32768 && sp >= 4 && sn >= (long)H * W * sp,
               "um_depth_post: strides sn=%ld sp=%ld for %dx%d (sp >= 4, sn >= H*W*sp)", sn, sp,
               H, W);
  UM_CHECK_ARG(pred && params, "um_depth_post: null pointer");
  const long total = (long)N * Hs * Ws, blocks = (total + 1023) / 1024;
  UM_CHECK_ARG(blocks <= INT_MAX, "um_depth_post: %ld output pixels", total);
  PostArgs a{pred, sn, sp, N, H, W, Hs, Ws, params, disparity, depth, uncertainty, lr_error,
             valid};
  const bool vec = aligned(disparity, 16) && aligned(depth, 16) && aligned(uncertainty, 16) &&
                   aligned(lr_error, 16) && aligned(valid, 4);
  if (vec)
    hipLaunchKernelGGL(depth_post_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(depth_post_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
