// Display image of the deployment path (umamd/render.py, the optional fourth
// stage of umamd/deploy.py DepthPipeline): a float map coloured through a
// 256-entry table and blended over the camera frame, on the device.
//
//   um_value_range   min / max of a map over its valid, non-NaN pixels (the
//                    min/max scaling of get_comparison(add_scaled=True),
//                    reference train/utils.py:276-325): at most 256 workgroups
//                    write one (lo, hi) partial each into the workspace, a
//                    one-workgroup launch finishes; no atomics, no state
//   um_depth_render  to_heatmap (reference train/utils.py:177-199, matplotlib's
//                    Colormap.__call__ on an f32 array) -> save_image's
//                    x * 255 + 0.5 rounding (folded into the table) -> an
//                    integer alpha blend over the frame; 11 bytes per pixel,
//                    a streaming kernel
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

// Every float step below is its own f32 operation (the definition in
// include/umamd.h is written that way and the tests demand equality).
#pragma clang fp contract(off)

constexpr int RANGE_MAX_PARTS = 256;  // workgroups of the first range launch

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline int range_parts(long count) {
  const long blocks = (count + 1023) / 1024;
  return (int)(blocks < RANGE_MAX_PARTS ? blocks : RANGE_MAX_PARTS);
}

// ------------------------------------------------------------ value range --
__device__ __forceinline__ void range_take(float v, bool ok, float& lo, float& hi) {
  if (ok && v == v) {  // NaN takes no part; +-inf do
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
}

// (lo, hi) of the workgroup's threads -> thread 0; red: 8 floats of LDS
__device__ __forceinline__ void range_block_reduce(float& lo, float& hi, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * wave] = lo;
    red[2 * wave + 1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) {
      lo = fminf(lo, red[2 * w]);
      hi = fmaxf(hi, red[2 * w + 1]);
    }
}

// grid-strided over groups of 4 consecutive pixels; VEC: value is aligned for
// a 16-byte load and valid (if given) for a 4-byte one.  parts[2 * block]
template <bool VEC>
__global__ void __launch_bounds__(256)
range_partial_kernel(const float* __restrict__ value, const uint8_t* __restrict__ valid,
                     long count, float* __restrict__ parts) {
  __shared__ float red[8];
  float lo = INFINITY, hi = -INFINITY;
  const long groups = (count + 3) / 4, stride = (long)gridDim.x * blockDim.x;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < groups; g += stride) {
    const long i0 = 4 * g;
    if (VEC && i0 + 4 <= count) {
      const float4 v = *reinterpret_cast<const float4*>(value + i0);
      const uint32_t m = valid ? *reinterpret_cast<const uint32_t*>(valid + i0) : 0x01010101u;
      range_take(v.x, (m & 0xffu) != 0, lo, hi);
      range_take(v.y, (m & 0xff00u) != 0, lo, hi);
      range_take(v.z, (m & 0xff0000u) != 0, lo, hi);
      range_take(v.w, (m & 0xff000000u) != 0, lo, hi);
    } else {
      for (long i = i0; i < count && i < i0 + 4; ++i)
        range_take(value[i], valid ? valid[i] != 0 : true, lo, hi);
    }
  }
  range_block_reduce(lo, hi, red);
  if (threadIdx.x == 0) {
    parts[2 * blockIdx.x] = lo;
    parts[2 * blockIdx.x + 1] = hi;
  }
}

// one workgroup: the nparts (<= 256) partials -> range[2]
__global__ void __launch_bounds__(256)
range_finish_kernel(const float* __restrict__ parts, int nparts, float* __restrict__ range) {
  __shared__ float red[8];
  const bool in = (int)threadIdx.x < nparts;
  float lo = in ? parts[2 * threadIdx.x] : INFINITY;
  float hi = in ? parts[2 * threadIdx.x + 1] : -INFINITY;
  range_block_reduce(lo, hi, red);
  if (threadIdx.x == 0) {
    range[0] = lo;
    range[1] = hi;
  }
}

// ----------------------------------------------------------------- render --
struct RenderArgs {
  const float* value;
  const uint8_t* valid;
  const uint8_t* frame;
  long count;
  const uint8_t* lut;
  const float* rparams;
  const float* range;
  int inverse;
  uint8_t* rgb;
};

// q(x) = (int)(clamp(x, 0, 1) * 256 + 0.5), q(NaN) = 0: an opacity in 1/256
__device__ __forceinline__ int alpha_q(float x) {
  if (x != x) return 0;
  const float c = fminf(fmaxf(x, 0.f), 1.f);
  return (int)(c * 256.f + 0.5f);
}

// the table entry of one value, r | g << 8 | b << 16 (NaN: black)
__device__ __forceinline__ uint32_t colour_of(float v, float lo, float den, int inverse,
                                              const uint32_t* table) {
  float t = (v - lo) / den;  // IEEE division
  if (inverse) t = 1.f - t;
  const float s = t * 256.f;
  if (s != s) return 0u;
  return table[s < 0.f ? 0 : (int)fminf(s, 255.f)];
}

__device__ __forceinline__ uint32_t blend(uint32_t c, uint32_t f, int a) {
  return (c * (uint32_t)a + f * (uint32_t)(256 - a) + 128u) >> 8;
}

// one thread per 4 consecutive pixels; VEC: value is aligned for one 16-byte
// load, valid (if given) for a dword and frame (if given) / rgb for three
// dwords (pixel i0 = 4 k starts at byte 12 k)
template <bool VEC>
__global__ void __launch_bounds__(256) render_kernel(RenderArgs a) {
  __shared__ uint32_t table[256];
  {
    const uint8_t* e = a.lut + 3 * threadIdx.x;
    table[threadIdx.x] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
  }
  __syncthreads();
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= a.count) return;
  const float lo = a.range ? a.range[0] : a.rparams[0];
  const float hi = a.range ? a.range[1] : a.rparams[1];
  const float den = hi - lo;
  const int a_ok = alpha_q(a.rparams[2]), a_bad = alpha_q(a.rparams[3]);
  if (VEC && i0 + 4 <= a.count) {
    const float4 v4 = *reinterpret_cast<const float4*>(a.value + i0);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    const uint32_t m = a.valid ? *reinterpret_cast<const uint32_t*>(a.valid + i0) : 0x01010101u;
    uint32_t f[3] = {0u, 0u, 0u};
    if (a.frame) {
      const uint32_t* fp = reinterpret_cast<const uint32_t*>(a.frame + 3 * i0);
      f[0] = fp[0];
      f[1] = fp[1];
      f[2] = fp[2];
    }
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t c = colour_of(v[j], lo, den, a.inverse, table);
      const int al = ((m >> (8 * j)) & 0xffu) ? a_ok : a_bad;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int byte = 3 * j + ch;  // of the 12 bytes of the four pixels
        const uint32_t fb = (f[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
        o[byte >> 2] |= blend((c >> (8 * ch)) & 0xffu, fb, al) << (8 * (byte & 3));
      }
    }
    uint32_t* op = reinterpret_cast<uint32_t*>(a.rgb + 3 * i0);
    op[0] = o[0];
    op[1] = o[1];
    op[2] = o[2];
    return;
  }
  for (long i = i0; i < a.count && i < i0 + 4; ++i) {
    const uint32_t c = colour_of(a.value[i], lo, den, a.inverse, table);
    const int al = (a.valid ? a.valid[i] != 0 : true) ? a_ok : a_bad;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t fb = a.frame ? a.frame[3 * i + ch] : 0u;
      a.rgb[3 * i + ch] = (uint8_t)blend((c >> (8 * ch)) & 0xffu, fb, al);
    }
  }
}

}  // namespace

extern "C" {

long um_value_range_ws(long count) {
  return count > 0 ? (long)range_parts(count) * 2 * (long)sizeof(float) : 0;
}

int um_value_range(const float* value, const unsigned char* valid, long count, float* range,
                   void* ws, hipStream_t st) {
  UM_CHECK_ARG(count > 0, "um_value_range: count=%ld", count);
  UM_CHECK_ARG(value && range && ws, "um_value_range: null pointer (value, range or ws)");
  UM_CHECK_ARG(aligned(range, 4) && aligned(ws, 4) && aligned(value, 4),
               "um_value_range: a float pointer that is not 4-byte aligned");
  const int parts = range_parts(count);
  float* p = static_cast<float*>(ws);
  if (aligned(value, 16) && aligned(valid, 4))
    hipLaunchKernelGGL(range_partial_kernel<true>, dim3(parts), dim3(256), 0, st, value, valid,
                       count, p);
  else
    hipLaunchKernelGGL(range_partial_kernel<false>, dim3(parts), dim3(256), 0, st, value, valid,
                       count, p);
  UM_LAUNCH_CHECK();
  hipLaunchKernelGGL(range_finish_kernel, dim3(1), dim3(256), 0, st, p, parts, range);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_depth_render(const float* value, const unsigned char* valid, const unsigned char* frame,
                    long count, const unsigned char* lut, const float* rparams,
                    const float* range, int inverse, unsigned char* rgb, hipStream_t st) {
  UM_CHECK_ARG(count > 0, "um_depth_render: count=%ld", count);
  UM_CHECK_ARG(value && lut && rparams && rgb,
               "um_depth_render: null pointer (value, lut, rparams or rgb)");
  UM_CHECK_ARG(aligned(value, 4) && aligned(rparams, 4) && aligned(range, 4),
               "um_depth_render: a float pointer that is not 4-byte aligned");
  const long blocks = (count + 1023) / 1024;
  UM_CHECK_ARG(blocks <= INT_MAX, "um_depth_render: %ld pixels", count);
  RenderArgs a{value, valid, frame, count, lut, rparams, range, inverse, rgb};
  const bool vec = aligned(value, 16) && aligned(valid, 4) && aligned(frame, 4) && aligned(rgb, 4);
  if (vec)
    hipLaunchKernelGGL(render_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(render_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
