// Stage 0 of the deployment path (umamd/rectify.py, DepthPipeline(rectify=...)):
// the raw camera frame undistorted and stereo-rectified on the device, so that
// what the later stages read is the pinhole image they assume.
//
//   um_frame_rectify  src u8 [N][Hs][Ws][3] -> dst u8 [N][Hr][Wr][3] and the
//                    inside mask u8 [Hr][Wr]; the source coordinate of every
//                    output pixel comes from the calibration block (pinhole +
//                    Brown-Conrady, computed in the kernel) or from a Q5 table,
//                    the sample is an integer bilinear blend with border 0; one
//                    streaming launch, gathered taps, no LDS
//   um_valid_and     valid[n][i] = valid[n][i] && inside[i], one small launch
//                    after um_depth_post
//
// The definition (include/umamd.h "rectification") fixes every rounding, so
// tests/_rectify_ref.py restates it in numpy and the tests demand equality.
#include "common.h"

#include <limits.h>

namespace {

// Every float step below is its own f32 operation.
#pragma clang fp contract(off)

constexpr int OUT = INT_MIN;  // a coordinate that is not finite or past 2^20

__host__ __device__ inline bool aligned(const void* p, uintptr_t a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

struct RectArgs {
  const uint8_t* src;
  int Hs, Ws, Hr, Wr;
  int count;  // N * Hr * Wr
  const float* cal;
  const int* map;
  uint8_t* dst;
  uint8_t* inside;
};

// q(c) = (int)rintf(c * 32) for a finite |c| < 2^20, else OUT (NaN compares false)
__device__ __forceinline__ int q5(float c) {
  return fabsf(c) < 1048576.f ? (int)rintf(c * 32.f) : OUT;
}

// the calibration block in registers (uniform: scalar loads)
struct Cal {
  float fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, m[9];
};

__device__ __forceinline__ Cal load_cal(const float* c) {
  Cal k;
  k.fx = c[0], k.fy = c[1], k.cx = c[2], k.cy = c[3];
  k.k1 = c[4], k.k2 = c[5], k.p1 = c[6], k.p2 = c[7];
  k.k3 = c[8], k.k4 = c[9], k.k5 = c[10], k.k6 = c[11];
#pragma unroll
  for (int i = 0; i < 9; ++i) k.m[i] = c[12 + i];
  return k;
}

// the Q5 source coordinate of rectified pixel (v, u): the order of the header
__device__ __forceinline__ void analytic_q(const Cal& k, int ui, int vi, int& qx, int& qy) {
  const float u = (float)ui, v = (float)vi;
  const float X = (k.m[0] * u + k.m[1] * v) + k.m[2];
  const float Y = (k.m[3] * u + k.m[4] * v) + k.m[5];
  const float W = (k.m[6] * u + k.m[7] * v) + k.m[8];
  const float x = X / W, y = Y / W;  // IEEE division
  const float x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
  const float num = 1.f + r2 * (k.k1 + r2 * (k.k2 + r2 * k.k3));
  const float den = 1.f + r2 * (k.k4 + r2 * (k.k5 + r2 * k.k6));
  const float kr = num / den;
  const float xd = (x * kr + (2.f * k.p1) * xy) + k.p2 * (r2 + 2.f * x2);
  const float yd = (y * kr + k.p1 * (r2 + 2.f * y2)) + (2.f * k.p2) * xy;
  qx = q5(k.fx * xd + k.cx);
  qy = q5(k.fy * yd + k.cy);
}

// The blended pixel r | g << 8 | b << 16 of image `img` (its first byte) at the
// Q5 coordinate, border 0: a tap outside the image is not read.  The two
// pixels of a row are 6 contiguous bytes at any byte offset (3 * ix): a dword
// and a half-word where both rows are wholly inside, byte loads at the border.
__device__ __forceinline__ uint32_t sample(const uint8_t* img, int Hs, int Ws, int qx, int qy,
                                           bool& in) {
  in = false;
  if (qx == OUT || qy == OUT) return 0u;
  in = qx >= 0 && qx <= (Ws - 1) * 32 && qy >= 0 && qy <= (Hs - 1) * 32;
  const int ix = qx >> 5, iy = qy >> 5;  // arithmetic shifts
  if (ix < -1 || ix >= Ws || iy < -1 || iy >= Hs) return 0u;  // all four taps outside
  const int ax = qx & 31, ay = qy & 31;
  const bool c0 = ix >= 0, c1 = ix + 1 < Ws, r0 = iy >= 0, r1 = iy + 1 < Hs;
  const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay,
            w11 = ax * ay;
  const uint8_t* p = img + ((long)iy * Ws + ix) * 3;  // formed, read only where inside
  const long down = 3L * Ws;
  uint32_t out = 0u;
  if (c0 && c1 && r0 && r1) {
    // exactly the 6 bytes of each row, nothing past the taps; memcpy leaves the
    // lowering to the compiler, which emits one unaligned global_load_dword and
    // one global_load_ushort per row for gfx950 (4 loads a pixel instead of 12)
    uint32_t lo0, lo1;
    uint16_t hi0, hi1;
    __builtin_memcpy(&lo0, p, 4);
    __builtin_memcpy(&hi0, p + 4, 2);
    __builtin_memcpy(&lo1, p + down, 4);
    __builtin_memcpy(&hi1, p + down + 4, 2);
    const uint64_t t0 = lo0 | ((uint64_t)hi0 << 32), t1 = lo1 | ((uint64_t)hi1 << 32);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int p00 = (int)((t0 >> (8 * ch)) & 0xff), p01 = (int)((t0 >> (8 * ch + 24)) & 0xff);
      const int p10 = (int)((t1 >> (8 * ch)) & 0xff), p11 = (int)((t1 >> (8 * ch + 24)) & 0xff);
      out |= (uint32_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10) << (8 * ch);
    }
    return out;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int p00 = r0 && c0 ? p[ch] : 0;
    const int p01 = r0 && c1 ? p[3 + ch] : 0;
    const int p10 = r1 && c0 ? p[down + ch] : 0;
    const int p11 = r1 && c1 ? p[down + 3 + ch] : 0;
    out |= (uint32_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10) << (8 * ch);
  }
  return out;
}

// one thread per 4 consecutive pixels of the flat [N * Hr * Wr] index; VEC: dst
// is aligned for three dword stores (pixel i0 = 4 k starts at byte 12 k) and
// inside (if given) for one; TABLE: the coordinates come from a.map
template <bool TABLE, bool VEC>
__global__ void __launch_bounds__(256) rectify_kernel(RectArgs a) {
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= a.count) return;
  Cal k;
  if (!TABLE) k = load_cal(a.cal);
  const int hw = a.Hr * a.Wr;
  const int row0 = (int)(i0 / a.Wr);
  int u = (int)(i0 - (long)row0 * a.Wr);
  int n = row0 / a.Hr;
  int v = row0 - n * a.Hr;
  const int live = a.count - i0 < 4 ? (int)(a.count - i0) : 4;
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  uint32_t m = 0u;  // the four inside bytes
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < live) {
      int qx, qy;
      if (TABLE) {
        const int* e = a.map + 2 * ((long)v * a.Wr + u);
        qx = e[0], qy = e[1];
      } else {
        analytic_q(k, u, v, qx, qy);
      }
      bool in;
      c[j] = sample(a.src + (long)n * a.Hs * a.Ws * 3, a.Hs, a.Ws, qx, qy, in);
      m |= (in ? 1u : 0u) << (8 * j);
    }
    if (++u == a.Wr) {
      u = 0;
      if (++v == a.Hr) v = 0, ++n;
    }
  }
  uint8_t* op = a.dst + 3 * i0;
  if (VEC && live == 4) {
    uint32_t* o = reinterpret_cast<uint32_t*>(op);
    o[0] = c[0] | (c[1] << 24);
    o[1] = (c[1] >> 8) | (c[2] << 16);
    o[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int j = 0; j < live; ++j) {
      op[3 * j] = (uint8_t)c[j];
      op[3 * j + 1] = (uint8_t)(c[j] >> 8);
      op[3 * j + 2] = (uint8_t)(c[j] >> 16);
    }
  }
  // the mask is the first image's: written once per call
  if (a.inside && i0 < hw) {
    if (VEC && i0 + 4 <= hw) {
      *reinterpret_cast<uint32_t*>(a.inside + i0) = m;
    } else {
      for (int j = 0; j < live && i0 + j < hw; ++j) a.inside[i0 + j] = (uint8_t)(m >> (8 * j));
    }
  }
}

// valid[n][i] = valid[n][i] && inside[i] as 0 / 1; one thread per 4 bytes of
// the flat [N * HW] index; VEC: valid is dword aligned
template <bool VEC>
__global__ void __launch_bounds__(256)
valid_and_kernel(uint8_t* __restrict__ valid, const uint8_t* __restrict__ inside, long count,
                 long HW) {
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= count) return;
  const long p0 = i0 % HW;
  if (VEC && i0 + 4 <= count) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(valid + i0);
    uint32_t in = 0u;
    if (p0 + 4 <= HW && aligned(inside + p0, 4)) {
      in = *reinterpret_cast<const uint32_t*>(inside + p0);
    } else {
      long p = p0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in |= (uint32_t)inside[p] << (8 * j);
        if (++p == HW) p = 0;
      }
    }
    uint32_t o = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o |= (((w >> (8 * j)) & 0xffu) && ((in >> (8 * j)) & 0xffu) ? 1u : 0u) << (8 * j);
    *reinterpret_cast<uint32_t*>(valid + i0) = o;
    return;
  }
  long p = p0;
  for (long i = i0; i < count && i < i0 + 4; ++i) {
    valid[i] = valid[i] != 0 && inside[p] != 0 ? 1 : 0;
    if (++p == HW) p = 0;
  }
}

}  // namespace

extern "C" {

int um_frame_rectify(const unsigned char* src, int N, int Hs, int Ws, int Hr, int Wr,
                     const float* cal, const int* map, unsigned char* dst,
                     unsigned char* inside, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && Hs >= 2 && Ws >= 2 && Hr >= 2 && Wr >= 2,
               "um_frame_rectify: N=%d Hs=%d Ws=%d Hr=%d Wr=%d (N >= 1, sizes >= 2)", N, Hs, Ws,
               Hr, Wr);
  UM_CHECK_ARG(Hs <= 32767 && Ws <= 32767, "um_frame_rectify: Hs=%d Ws=%d, at most 32767", Hs, Ws);
  const long count = (long)N * Hr * Wr;
  UM_CHECK_ARG(count <= INT_MAX, "um_frame_rectify: %ld output pixels, at most %d", count, INT_MAX);
  UM_CHECK_ARG((cal != nullptr) != (map != nullptr),
               "um_frame_rectify: exactly one of cal and map must be given");
  UM_CHECK_ARG(src && dst, "um_frame_rectify: null pointer (src or dst)");
  UM_CHECK_ARG(aligned(cal, 4) && aligned(map, 4),
               "um_frame_rectify: cal / map is not 4-byte aligned");
  RectArgs a{src, Hs, Ws, Hr, Wr, (int)count, cal, map, dst, inside};
  const dim3 grid((unsigned)((count + 1023) / 1024)), block(256);
  const bool vec = aligned(dst, 4) && aligned(inside, 4);
  if (map) {
    if (vec)
      hipLaunchKernelGGL((rectify_kernel<true, true>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((rectify_kernel<true, false>), grid, block, 0, st, a);
  } else {
    if (vec)
      hipLaunchKernelGGL((rectify_kernel<false, true>), grid, block, 0, st, a);
    else
      hipLaunchKernelGGL((rectify_kernel<false, false>), grid, block, 0, st, a);
  }
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_valid_and(unsigned char* valid, const unsigned char* inside, int N, long HW,
                 hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && HW >= 1, "um_valid_and: N=%d HW=%ld", N, HW);
  UM_CHECK_ARG(valid && inside, "um_valid_and: null pointer (valid or inside)");
  UM_CHECK_ARG(HW <= LONG_MAX / N, "um_valid_and: %d x %ld masks", N, HW);
  const long count = (long)N * HW;
  const long blocks = (count + 1023) / 1024;
  UM_CHECK_ARG(blocks <= INT_MAX, "um_valid_and: %ld masks", count);
  if (aligned(valid, 4))
    hipLaunchKernelGGL(valid_and_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, valid,
                       inside, count, HW);
  else
    hipLaunchKernelGGL(valid_and_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, valid,
                       inside, count, HW);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
