// Element-wise pieces of the encoder graph and layout plumbing.
//
//   um_merge_fwd / um_merge_bwd / um_merge_wgrad
//       NodeBlock's sigmoid-weighted predecessor sum, reference
//       model/layers/encoder.py:115-124.  Input i is weighted by
//       sigmoid(w[widx[i]]) where the host passes the reference's index map
//       (F3: widx = [0, 0, 1, 2, ...]).
//   um_image_to_nhwc   NCHW f32 image -> NHWC (padded channels, zero fill)
//   um_sigmoid_scale_bwd  d/dlogit of scale*sigmoid(logit) (disp head,
//       reference model/layers/decoder.py:246 with ConvLayer sigmoid)
#include "common.h"
#include "knobs.h"

namespace {

constexpr int MAX_SRC = 16;
struct MergeArgs {
  const void* src[MAX_SRC];
  void* dsrc[MAX_SRC];
  int widx[MAX_SRC];
  int acc[MAX_SRC];
  float coef[MAX_SRC];  // used when w == null (constant coefficients)
};

// merge_bwd_bn: at most 512 workgroups (each adds 2*C f64 statistics to one
// of 16 slot rows: 4096 workgroups of the 256x512 stage meant 256 adders per
// address), the grid-stride loop covers the rest
inline int merge_bn_grid(long n8) {
  long b = (n8 + 255) / 256;
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return (int)b;
}

inline int grid_for(long n) {
  long b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

template <typename T>
__global__ void merge_fwd_kernel(MergeArgs a, int nsrc, const float* __restrict__ w, long n8,
                                 T* __restrict__ dst) {
  float coef[MAX_SRC];
  for (int i = 0; i < nsrc; ++i) coef[i] = w ? sigmoidf_(w[a.widx[i]]) : a.coef[i];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    float acc[8], v[8];
    load8(reinterpret_cast<const T*>(a.src[0]) + i * 8, acc);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= coef[0];
    for (int s = 1; s < nsrc; ++s) {
      load8(reinterpret_cast<const T*>(a.src[s]) + i * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += coef[s] * v[e];
    }
    store8(dst + i * 8, acc);
  }
}

// dsrc_i (+)= coef_i * dm ; partial dot products sum(dm * src_i) per block
template <typename T>
__global__ void merge_bwd_kernel(MergeArgs a, int nsrc, const float* __restrict__ w, long n8,
                                 const T* __restrict__ dm, float* __restrict__ parts) {
  float coef[MAX_SRC], dot[MAX_SRC];
  for (int i = 0; i < nsrc; ++i) {
    coef[i] = w ? sigmoidf_(w[a.widx[i]]) : a.coef[i];
    dot[i] = 0.f;
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    float g[8], v[8], o[8];
    load8(dm + i * 8, g);
    for (int s = 0; s < nsrc; ++s) {
      if (parts) {
        load8(reinterpret_cast<const T*>(a.src[s]) + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot[s] += g[e] * v[e];
      }
      if (a.dsrc[s]) {
        T* d = reinterpret_cast<T*>(a.dsrc[s]) + i * 8;
        if (a.acc[s]) load8(d, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (a.acc[s] ? o[e] : 0.f) + coef[s] * g[e];
        store8(d, o);
      }
    }
  }
  if (parts) {
    __shared__ float red[4];
    for (int s = 0; s < nsrc; ++s) {
      float t = wave_sum(dot[s]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
      __syncthreads();
      if (threadIdx.x == 0) parts[(long)blockIdx.x * nsrc + s] = red[0] + red[1] + red[2] + red[3];
      __syncthreads();
    }
  }
}

// merge_bwd_kernel + the BN-ELU backward statistics of source `fsrc`, whose
// gradient this merge completes (its last consumer in the backward order,
// umamd.functional.GraphBlockFn): the sums bn_elu_bwd_reduce would take over
// that gradient -- sum dz and sum dz*xhat per channel, dz = da * ELU'(y*scale
// + shift), xhat = (y - mean) * invstd, over the da as stored (T-rounded) --
// go into the layer's f64 statistics slots here, so the reduce launch and its
// re-read of da are skipped.  C / 8 divides the block size: every thread of
// the grid-stride loop keeps one 8-channel group.
// NS > 0: exactly NS sources, and every load of an element group (dm, y,
// the sources, the gradients accumulated into) is issued before the first
// store: the runtime source loop otherwise serialises one load -> store
// round trip per source (the compiler cannot move a load past a store that
// may alias it), at the 2 waves per SIMD this grid leaves.
template <typename T, typename TY, int NS>
__global__ void __launch_bounds__(256) merge_bwd_bn_kernel(
    MergeArgs a, int nsrc, const float* __restrict__ w, long n8, const T* __restrict__ dm,
    float* __restrict__ parts, int fsrc, const TY* __restrict__ y, int C,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ scale, const float* __restrict__ shift, int apply_elu,
    double* __restrict__ slots, long M) {
  __shared__ float sred[4][64 * 8][2];
  float coef[MAX_SRC], dot[MAX_SRC];
  for (int i = 0; i < nsrc; ++i) {
    coef[i] = w ? sigmoidf_(w[a.widx[i]]) : a.coef[i];
    dot[i] = 0.f;
  }
  const int cg = C / 8, g = threadIdx.x % cg;
  float mu[8], is[8], sc[8], sh[8], bs[8], bx[8];
  load8(mean + g * 8, mu);
  load8(invstd + g * 8, is);
  load8(scale + g * 8, sc);
  load8(shift + g * 8, sh);
#pragma unroll
  for (int e = 0; e < 8; ++e) { bs[e] = 0.f; bx[e] = 0.f; }
  auto stats = [&](const float (&r)[8], const float (&yv)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float dz = r[e];
      if (apply_elu) {
        const float z = yv[e] * sc[e] + sh[e];
        dz = z > 0.f ? dz : dz * __expf(z);
      }
      bs[e] += dz;
      bx[e] += dz * (yv[e] - mu[e]) * is[e];
    }
  };
  if constexpr (NS > 0) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8;
         i += (long)gridDim.x * blockDim.x) {
      float gv[8], yv[8], v[NS][8], o[NS][8];
      load8(dm + i * 8, gv);
      load8(y + i * 8, yv);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (parts) load8(reinterpret_cast<const T*>(a.src[s]) + i * 8, v[s]);
        if (a.acc[s]) load8(reinterpret_cast<const T*>(a.dsrc[s]) + i * 8, o[s]);
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (parts)
#pragma unroll
          for (int e = 0; e < 8; ++e) dot[s] += gv[e] * v[s][e];
        if (a.dsrc[s]) {
          T* d = reinterpret_cast<T*>(a.dsrc[s]) + i * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[s][e] = (a.acc[s] ? o[s][e] : 0.f) + coef[s] * gv[e];
          store8(d, o[s]);
          if (s == fsrc) {
            float r[8];
            load8_rounded(o[s], r, d);
            stats(r, yv);
          }
        }
      }
    }
  } else
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    float gv[8], v[8], o[8];
    load8(dm + i * 8, gv);
    for (int s = 0; s < nsrc; ++s) {
      if (parts) {
        load8(reinterpret_cast<const T*>(a.src[s]) + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot[s] += gv[e] * v[e];
      }
      if (a.dsrc[s]) {
        T* d = reinterpret_cast<T*>(a.dsrc[s]) + i * 8;
        if (a.acc[s]) load8(d, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (a.acc[s] ? o[e] : 0.f) + coef[s] * gv[e];
        store8(d, o);
        if (s == fsrc) {
          float r[8], yv[8];
          load8_rounded(o, r, d);
          load8(y + i * 8, yv);
          stats(r, yv);
        }
      }
    }
  }
  if (parts) {
    __shared__ float red[4];
    for (int s = 0; s < nsrc; ++s) {
      float t = wave_sum(dot[s]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
      __syncthreads();
      if (threadIdx.x == 0) parts[(long)blockIdx.x * nsrc + s] = red[0] + red[1] + red[2] + red[3];
      __syncthreads();
    }
  }
  // lanes of a wave with the same channel group: lane % cg
  for (int off = cg; off < 64; off <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bs[e] += __shfl_xor(bs[e], off, 64);
      bx[e] += __shfl_xor(bx[e], off, 64);
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < cg)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sred[wave][lane * 8 + e][0] = bs[e];
      sred[wave][lane * 8 + e][1] = bx[e];
    }
  __syncthreads();
  stat_slots_count(slots, C, M);
  stat_slots_add_row(slots, blockIdx.x, C, 0, C, [&](int k) {
    const int c = k >> 1, j = k & 1;
    return sred[0][c][j] + sred[1][c][j] + sred[2][c][j] + sred[3][c][j];
  });
}

__global__ void merge_wgrad_kernel(const float* __restrict__ parts, int nparts, int nsrc,
                                   MergeArgs a, const float* __restrict__ w, float* dw,
                                   int nw, int accumulate) {
  // single block; dw[widx[i]] += sigmoid'(w) * sum_p parts[p][i]
  __shared__ double tot[MAX_SRC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < nsrc; s += 4) {
    double t = 0.0;
    for (int p = lane; p < nparts; p += 64) t += parts[(long)p * nsrc + s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if (lane == 0) tot[s] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!accumulate)
      for (int j = 0; j < nw; ++j) dw[j] = 0.f;
    for (int s = 0; s < nsrc; ++s) {
      const float sg = sigmoidf_(w[a.widx[s]]);
      dw[a.widx[s]] += (float)(tot[s] * sg * (1.0 - sg));
    }
  }
}

// Several merge-weight gradients in ONE launch (one workgroup each): the
// weight-gradient side stream's flush batches them like the conv slab
// reductions.  Descriptors by value; fields selected with unrolled uniform
// selects (no scratch copy of the argument).
struct MwDesc {
  const float* parts;
  const float* w;
  float* dw;
  int nparts, nsrc, nw, accumulate;
  int widx[UM_MWG_SRC];
};
struct MwBatch {
  int n;
  MwDesc d[UM_MWG_MAX];
};

__global__ void __launch_bounds__(256) merge_wgrad_batch_kernel(MwBatch b) {
  const int i = blockIdx.x;
#define MSEL(expr)                                          \
  ({                                                        \
    auto v_ = b.d[0].expr;                                  \
    _Pragma("unroll") for (int j = 1; j < UM_MWG_MAX; ++j)  \
      if (j == i) v_ = b.d[j].expr;                         \
    v_;                                                     \
  })
  const float* parts = MSEL(parts);
  const float* w = MSEL(w);
  float* dw = MSEL(dw);
  const int nparts = MSEL(nparts), nsrc = MSEL(nsrc), nw = MSEL(nw), acc = MSEL(accumulate);
  int widx[UM_MWG_SRC];
#pragma unroll
  for (int q = 0; q < UM_MWG_SRC; ++q) widx[q] = MSEL(widx[q]);
#undef MSEL
  __shared__ double tot[UM_MWG_SRC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s0 = 0; s0 < UM_MWG_SRC; s0 += 4) {
    const int s = s0 + wave;
    if (s < nsrc) {
      double t = 0.0;
      for (int p = lane; p < nparts; p += 64) t += parts[(long)p * nsrc + s];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
      if (lane == 0) tot[s] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // as merge_wgrad_kernel, same order
    if (!acc)
      for (int j = 0; j < nw; ++j) dw[j] = 0.f;
#pragma unroll
    for (int s = 0; s < UM_MWG_SRC; ++s) {
      if (s < nsrc) {
        const float sg = sigmoidf_(w[widx[s]]);
        dw[widx[s]] += (float)(tot[s] * sg * (1.0 - sg));
      }
    }
  }
}

template <typename T>
__global__ void image_to_nhwc_kernel(const float* __restrict__ x, int N, int C, int H, int W,
                                     int Cp, T* __restrict__ out) {
  const long total = (long)N * H * W * Cp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = i % Cp;
    const long pix = i / Cp;
    const int xw = pix % W;
    const int yh = (pix / W) % H;
    const int n = pix / ((long)W * H);
    const float v = c < C ? x[(((long)n * C + c) * H + yh) * W + xw] : 0.f;
    out[i] = from_f32<T>(v);
  }
}

// bf16 with Cp a multiple of 8: thread = (pixel, 8-channel group), the
// planar reads coalesced across the pixels, one 16-byte store
__global__ void image_to_nhwc8_kernel(const float* __restrict__ x, int N, int C, long HW, int Cp,
                                      bf16_t* __restrict__ out) {
  const int G = Cp / 8;
  const long total = (long)N * HW * G;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int g = (int)(i / ((long)N * HW));  // group-major: a wave reads consecutive pixels
    const long pix = i - (long)g * N * HW;
    const long n = pix / HW, p = pix - n * HW;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = g * 8 + e;
      v[e] = c < C ? x[(n * C + c) * HW + p] : 0.f;
    }
    store8(out + pix * Cp + g * 8, v);
  }
}

// dlogit[m][c] = dd[m][c] * d * (1 - d/scale) for c < C (SPLIT: also at
// C + c, the split-bf16 head's residual rows); the other channels of [0, ldo)
// zeroed
template <typename T, bool SPLIT>
__global__ void sigmoid_scale_bwd_kernel(long M, int C, const float* __restrict__ d, int ldd,
                                         const float* __restrict__ dd, int lddd, float scale,
                                         T* __restrict__ dlogit, int ldo) {
  const long total = M * ldo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long m = i / ldo;
    int c = i - m * ldo;
    if (SPLIT && c >= C && c < 2 * C) c -= C;
    float v = 0.f;
    if (c < C) {
      const float dv = d[m * ldd + c];
      v = dd[m * lddd + c] * dv * (1.f - dv / scale);
    }
    dlogit[i] = from_f32<T>(v);
  }
}

// the disparity heads' shape (C = 4 outputs in an 8-wide bf16 dlogit, float4-
// aligned d / dd rows): thread = pixel, two float4 loads, one 16-byte store
template <bool SPLIT>
__global__ void sigmoid_scale_bwd4_kernel(long M, const float* __restrict__ d, int ldd,
                                          const float* __restrict__ dd, int lddd, float scale,
                                          bf16_t* __restrict__ dlogit) {
  for (long m = blockIdx.x * (long)blockDim.x + threadIdx.x; m < M;
       m += (long)gridDim.x * blockDim.x) {
    const float4 dv = *reinterpret_cast<const float4*>(d + m * ldd);
    const float4 g = *reinterpret_cast<const float4*>(dd + m * lddd);
    float v[8];
    v[0] = g.x * dv.x * (1.f - dv.x / scale);
    v[1] = g.y * dv.y * (1.f - dv.y / scale);
    v[2] = g.z * dv.z * (1.f - dv.z / scale);
    v[3] = g.w * dv.w * (1.f - dv.w / scale);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 + e] = SPLIT ? v[e] : 0.f;
    store8(dlogit + m * 8, v);
  }
}

// the split-bf16 head's forward finish (um_head_split_fin)
__global__ void head_split_fin_kernel(long M, int K, const float* __restrict__ z, int ldz,
                                      const float* __restrict__ bias, float scale,
                                      float* __restrict__ d, int ldd) {
  const long total = M * K;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long m = i / K;
    const int k = i - m * K;
    const float* zr = z + m * ldz;
    d[m * ldd + k] = scale * sigmoidf_(zr[k] + zr[K + k] + (bias ? bias[k] : 0.f));
  }
}

// K = 4 with float4-aligned rows: thread = pixel
__global__ void head_split_fin4_kernel(long M, const float* __restrict__ z, int ldz,
                                       const float* __restrict__ bias, float scale,
                                       float* __restrict__ d, int ldd) {
  const float4 b = bias ? *reinterpret_cast<const float4*>(bias) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (long m = blockIdx.x * (long)blockDim.x + threadIdx.x; m < M;
       m += (long)gridDim.x * blockDim.x) {
    const float4 hi = *reinterpret_cast<const float4*>(z + m * ldz);
    const float4 lo = *reinterpret_cast<const float4*>(z + m * ldz + 4);
    *reinterpret_cast<float4*>(d + m * ldd) =
        make_float4(scale * sigmoidf_(hi.x + lo.x + b.x), scale * sigmoidf_(hi.y + lo.y + b.y),
                    scale * sigmoidf_(hi.z + lo.z + b.z), scale * sigmoidf_(hi.w + lo.w + b.w));
  }
}

__host__ inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int um_merge_fwd(int dtype, int nsrc, const void* const* srcs, const int* widx,
                 const float* w, const float* coefs, long count, void* dst, hipStream_t st) {
  UM_CHECK_ARG(nsrc >= 1 && nsrc <= MAX_SRC, "um_merge_fwd: nsrc %d", nsrc);
  UM_CHECK_ARG(count % 8 == 0, "um_merge_fwd: count %% 8");
  MergeArgs a{};
  for (int i = 0; i < nsrc; ++i) {
    a.src[i] = srcs[i];
    a.widx[i] = widx ? widx[i] : 0;
    a.coef[i] = coefs ? coefs[i] : 1.f;
  }
  const long n8 = count / 8;
  if (dtype == UM_BF16)
    hipLaunchKernelGGL(merge_fwd_kernel<bf16_t>, dim3(grid_for(n8)), dim3(256), 0, st, a, nsrc, w,
                       n8, (bf16_t*)dst);
  else
    hipLaunchKernelGGL(merge_fwd_kernel<float>, dim3(grid_for(n8)), dim3(256), 0, st, a, nsrc, w,
                       n8, (float*)dst);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_merge_parts(long count) { return grid_for(count / 8); }
int um_merge_bn_parts(long count) { return merge_bn_grid(count / 8); }

int um_merge_bwd(int dtype, int nsrc, const void* const* srcs, void* const* dsrcs,
                 const int* accumulate, const int* widx, const float* w, const float* coefs,
                 long count, const void* dm, float* parts, hipStream_t st) {
  UM_CHECK_ARG(nsrc >= 1 && nsrc <= MAX_SRC, "um_merge_bwd: nsrc %d", nsrc);
  UM_CHECK_ARG(count % 8 == 0, "um_merge_bwd: count %% 8");
  MergeArgs a{};
  for (int i = 0; i < nsrc; ++i) {
    a.src[i] = srcs ? srcs[i] : nullptr;
    a.dsrc[i] = dsrcs[i];
    a.acc[i] = accumulate[i];
    a.widx[i] = widx ? widx[i] : 0;
    a.coef[i] = coefs ? coefs[i] : 1.f;
  }
  const long n8 = count / 8;
  if (dtype == UM_BF16)
    hipLaunchKernelGGL(merge_bwd_kernel<bf16_t>, dim3(grid_for(n8)), dim3(256), 0, st, a, nsrc, w,
                       n8, (const bf16_t*)dm, parts);
  else
    hipLaunchKernelGGL(merge_bwd_kernel<float>, dim3(grid_for(n8)), dim3(256), 0, st, a, nsrc, w,
                       n8, (const float*)dm, parts);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_merge_bwd_bn(int dtype, int nsrc, const void* const* srcs, void* const* dsrcs,
                    const int* accumulate, const int* widx, const float* w, const float* coefs,
                    long count, const void* dm, float* parts, int fsrc, const void* y, int C,
                    const float* mean, const float* invstd, const float* scale,
                    const float* shift, int apply_elu, double* slots, hipStream_t st) {
  UM_CHECK_ARG(nsrc >= 1 && nsrc <= MAX_SRC && fsrc >= 0 && fsrc < nsrc, "um_merge_bwd_bn: nsrc %d fsrc %d",
               nsrc, fsrc);
  UM_CHECK_ARG(C >= 8 && C <= 512 && C % 8 == 0 && 256 % (C / 8) == 0 && count % C == 0,
               "um_merge_bwd_bn: C %d (C/8 must divide 256)", C);
  UM_CHECK_ARG(dsrcs[fsrc] != nullptr && y != nullptr && slots != nullptr, "um_merge_bwd_bn: operands");
  MergeArgs a{};
  for (int i = 0; i < nsrc; ++i) {
    a.src[i] = srcs ? srcs[i] : nullptr;
    a.dsrc[i] = dsrcs[i];
    a.acc[i] = accumulate[i];
    a.widx[i] = widx ? widx[i] : 0;
    a.coef[i] = coefs ? coefs[i] : 1.f;
  }
  const long n8 = count / 8, M = count / C;
  // sources 2-4 on the loads-first instances (tuning key merge_ns = 0: the
  // runtime source loop for all)
  const int ns_on = umamd::knobs().merge_ns;
  const int ns = ns_on && nsrc >= 2 && nsrc <= 4 ? nsrc : 0;
#define UM_MBB_NS(T_, TY_, NS_)                                                                   \
  hipLaunchKernelGGL((merge_bwd_bn_kernel<T_, TY_, NS_>), dim3(merge_bn_grid(n8)), dim3(256), 0, st, a,  \
                     nsrc, w, n8, (const T_*)dm, parts, fsrc, (const TY_*)y, C, mean, invstd, scale, \
                     shift, apply_elu, slots, M)
#define UM_MBB(T_, TY_)                      \
  do {                                       \
    if (ns == 2) UM_MBB_NS(T_, TY_, 2);      \
    else if (ns == 3) UM_MBB_NS(T_, TY_, 3); \
    else if (ns == 4) UM_MBB_NS(T_, TY_, 4); \
    else UM_MBB_NS(T_, TY_, 0);              \
  } while (0)
  if (dtype == (UM_BF16 | UM_Y_ACT)) UM_MBB(bf16_t, bf16_t);
  else if (dtype == UM_BF16) UM_MBB(bf16_t, float);
  else UM_MBB(float, float);
#undef UM_MBB
#undef UM_MBB_NS
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_merge_wgrad(const float* parts, int nparts, int nsrc, const int* widx, const float* w,
                   float* dw, int nw, int accumulate, hipStream_t st) {
  MergeArgs a{};
  for (int i = 0; i < nsrc; ++i) a.widx[i] = widx[i];
  hipLaunchKernelGGL(merge_wgrad_kernel, dim3(1), dim3(256), 0, st, parts, nparts, nsrc, a, w, dw,
                     nw, accumulate);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_merge_wgrad_batch(const um_mwg_desc* descs, int n, hipStream_t st) {
  UM_CHECK_ARG(descs != nullptr && n >= 0 && n <= UM_MWG_MAX, "um_merge_wgrad_batch: n");
  if (n == 0) return UM_OK;
  MwBatch b{};
  b.n = n;
  for (int i = 0; i < n; ++i) {
    const um_mwg_desc& e = descs[i];
    UM_CHECK_ARG(e.parts && e.w && e.dw && e.nsrc >= 1 && e.nsrc <= UM_MWG_SRC && e.nparts >= 1,
                 "um_merge_wgrad_batch: descriptor");
    MwDesc& d = b.d[i];
    d.parts = e.parts; d.w = e.w; d.dw = e.dw;
    d.nparts = e.nparts; d.nsrc = e.nsrc; d.nw = e.nw; d.accumulate = e.accumulate;
    for (int q = 0; q < UM_MWG_SRC; ++q) d.widx[q] = q < e.nsrc ? e.widx[q] : 0;
  }
  hipLaunchKernelGGL(merge_wgrad_batch_kernel, dim3(n), dim3(256), 0, st, b);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_image_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, int Cp, void* out,
                     hipStream_t st) {
  const long total = (long)N * H * W * Cp;
  if (dtype == UM_BF16 && Cp % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
    hipLaunchKernelGGL(image_to_nhwc8_kernel, dim3(grid_for(total / 8)), dim3(256), 0, st, x, N,
                       C, (long)H * W, Cp, (bf16_t*)out);
  else if (dtype == UM_BF16)
    hipLaunchKernelGGL(image_to_nhwc_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, x, N,
                       C, H, W, Cp, (bf16_t*)out);
  else
    hipLaunchKernelGGL(image_to_nhwc_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, x, N,
                       C, H, W, Cp, (float*)out);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_sigmoid_scale_bwd(int dtype, long M, int C, const float* d, int ldd, const float* dd,
                         int lddd, float scale, void* dlogit, int ldo, hipStream_t st) {
  const long total = M * ldo;
  if (dtype == UM_BF16 && C == 4 && ldo == 8 && ldd % 4 == 0 && lddd % 4 == 0 && al16(d) &&
      al16(dd) && al16(dlogit))
    hipLaunchKernelGGL((sigmoid_scale_bwd4_kernel<false>), dim3(grid_for(M)), dim3(256), 0, st, M,
                       d, ldd, dd, lddd, scale, (bf16_t*)dlogit);
  else if (dtype == UM_BF16)
    hipLaunchKernelGGL((sigmoid_scale_bwd_kernel<bf16_t, false>), dim3(grid_for(total)), dim3(256),
                       0, st, M, C, d, ldd, dd, lddd, scale, (bf16_t*)dlogit, ldo);
  else
    hipLaunchKernelGGL((sigmoid_scale_bwd_kernel<float, false>), dim3(grid_for(total)), dim3(256),
                       0, st, M, C, d, ldd, dd, lddd, scale, (float*)dlogit, ldo);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_sigmoid_scale_bwd_split(int dtype, long M, int C, const float* d, int ldd, const float* dd,
                               int lddd, float scale, void* dlogit, int ldo, hipStream_t st) {
  UM_CHECK_ARG(ldo >= 2 * C, "um_sigmoid_scale_bwd_split: ldo < 2C");
  const long total = M * ldo;
  if (dtype == UM_BF16 && C == 4 && ldo == 8 && ldd % 4 == 0 && lddd % 4 == 0 && al16(d) &&
      al16(dd) && al16(dlogit))
    hipLaunchKernelGGL((sigmoid_scale_bwd4_kernel<true>), dim3(grid_for(M)), dim3(256), 0, st, M,
                       d, ldd, dd, lddd, scale, (bf16_t*)dlogit);
  else if (dtype == UM_BF16)
    hipLaunchKernelGGL((sigmoid_scale_bwd_kernel<bf16_t, true>), dim3(grid_for(total)), dim3(256),
                       0, st, M, C, d, ldd, dd, lddd, scale, (bf16_t*)dlogit, ldo);
  else
    hipLaunchKernelGGL((sigmoid_scale_bwd_kernel<float, true>), dim3(grid_for(total)), dim3(256),
                       0, st, M, C, d, ldd, dd, lddd, scale, (float*)dlogit, ldo);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_head_split_fin(long M, int K, const float* z, int ldz, const float* bias, float scale,
                      float* d, int ldd, hipStream_t st) {
  UM_CHECK_ARG(ldz >= 2 * K && ldd >= K, "um_head_split_fin: ld");
  const long total = M * K;
  if (K == 4 && ldz % 4 == 0 && ldd % 4 == 0 && al16(z) && al16(d) && (!bias || al16(bias))) {
    hipLaunchKernelGGL(head_split_fin4_kernel, dim3(grid_for(M)), dim3(256), 0, st, M, z, ldz, bias,
                       scale, d, ldd);
    UM_LAUNCH_CHECK();
    return UM_OK;
  }
  hipLaunchKernelGGL(head_split_fin_kernel, dim3(grid_for(total)), dim3(256), 0, st, M, K, z, ldz,
                     bias, scale, d, ldd);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
