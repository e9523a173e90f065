// Refinement of the deployment path (umamd/refine.py, the optional refine
// stage of umamd/deploy.py DepthPipeline), between um_depth_post and the mask,
// display and point stages; the definition is in include/umamd.h.
//
//   um_disp_smooth  a dilated joint-bilateral filter of disparity and
//                   uncertainty: the taps weighted by distance (table S), by
//                   the colour difference to the centre in the full-resolution
//                   frame (table G) and by the confidence 1 / (sigma^2 + eps)
//                   of the tap.  A workgroup stages its tile and the halo in
//                   LDS once and reads every tap from there.
//   um_disp_fuse    a per-pixel recursive (scalar Kalman) filter of the
//                   disparity over the frames of a stream, gated, with the
//                   model's sigma as the measurement noise, then depth and the
//                   mask by um_depth_post's expressions.  Elementwise.
#include "common.h"

#include <limits.h>

namespace {

// Every float step below is its own f32 operation (the definition in
// include/umamd.h is written that way and the tests demand equality).
#pragma clang fp contract(off)

__host__ __device__ inline bool aligned(const void* p, uintptr_t a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

// neither NaN nor +-inf
__device__ __forceinline__ bool finite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

// ------------------------------------------------------------- smoothing --
constexpr int SM_TW = 64;              // tile columns: a wave owns one tile row at a time
constexpr int SM_THREADS = 256;        // 4 waves: tile rows r, r + 4, ...
constexpr int SM_G = 768;              // entries of the colour table
constexpr int SM_MAX_HALO = 16;        // R * step
constexpr int SM_LDS = 64 * 1024;      // dynamic LDS a launch may ask for
constexpr uint32_t SM_LIVE = 1u << 24; // in the packed colour: the tap takes part

// floats of LDS for a tile of th rows with this halo: four planes and G
constexpr long smooth_lds_floats(int th, int halo) {
  return 4L * (th + 2 * halo) * (SM_TW + 2 * halo) + SM_G;
}
static_assert(smooth_lds_floats(8, SM_MAX_HALO) * 4 <= SM_LDS, "the 8-row tile always fits");

// rows of a tile: 16 where the planes fit (halo <= 13), else 8
inline int smooth_tile_rows(int halo) {
  return smooth_lds_floats(16, halo) * 4 <= SM_LDS ? 16 : 8;
}

struct SmoothArgs {
  const float *disp, *unc;
  const uint8_t* frame;
  int Hs, Ws, step, th;
  int tiles_x, tiles_y;
  const float *S, *G, *fp;
  float *disp_out, *unc_out;
};

// grid: N * tiles_y * tiles_x workgroups; dynamic LDS: smooth_lds_floats
template <int R>
__global__ void __launch_bounds__(SM_THREADS) disp_smooth_kernel(SmoothArgs a) {
  extern __shared__ float lds[];
  const int halo = R * a.step;
  const int SW = SM_TW + 2 * halo, SH = a.th + 2 * halo, SP = SH * SW;
  float* sd = lds;        // disparity
  float* su = sd + SP;    // uncertainty
  float* sc = su + SP;    // confidence, computed once per staged pixel
  uint32_t* sk = reinterpret_cast<uint32_t*>(sc + SP);  // r | g << 8 | b << 16 | SM_LIVE
  float* sg = reinterpret_cast<float*>(sk + SP);        // G

  unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)a.tiles_x);
  b /= (unsigned)a.tiles_x;
  const int ty = (int)(b % (unsigned)a.tiles_y);
  const int n = (int)(b / (unsigned)a.tiles_y);
  const int x0 = tx * SM_TW, y0 = ty * a.th;
  const long image = (long)n * a.Hs * a.Ws;
  const float eps = a.fp[0];

  float S[(R + 1) * (R + 1)];
#pragma unroll
  for (int i = 0; i < (R + 1) * (R + 1); ++i) S[i] = a.S[i];

  for (int i = threadIdx.x; i < SM_G; i += SM_THREADS) sg[i] = a.G[i];
  for (int i = threadIdx.x; i < SP; i += SM_THREADS) {
    const int sy = i / SW, sx = i - sy * SW;
    const int y = y0 - halo + sy, x = x0 - halo + sx;
    float d = 0.f, u = 0.f, c = 0.f;
    uint32_t k = 0u;
    if (y >= 0 && y < a.Hs && x >= 0 && x < a.Ws) {  // outside the image: not read
      const long p = image + (long)y * a.Ws + x;
      d = a.disp[p];
      u = a.unc[p];
      const uint8_t* e = a.frame + 3 * p;
      k = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
      if (finite(d) && finite(u)) {
        const float uu = u * u;
        const float v = uu + eps;
        c = 1.f / v;
        k |= SM_LIVE;
      }
    }
    sd[i] = d;
    su[i] = u;
    sc[i] = c;
    sk[i] = k;
  }
  __syncthreads();

  const int lx = threadIdx.x & 63, x = x0 + lx;
  if (x >= a.Ws) return;
  for (int r = threadIdx.x >> 6; r < a.th; r += SM_THREADS / 64) {
    const int y = y0 + r;
    if (y >= a.Hs) break;
    const int ci = (r + halo) * SW + lx + halo;
    const uint32_t kp = sk[ci] | SM_LIVE;  // byte 3 equals a live tap's: no part in the sum
    float num = 0.f, nus = 0.f, den = 0.f;
#pragma unroll
    for (int j = -R; j <= R; ++j) {
#pragma unroll
      for (int i = -R; i <= R; ++i) {
        const int t = ci + (j * SW + i) * a.step;
        const uint32_t kt = sk[t];
        if (kt & SM_LIVE) {
          const uint32_t k = __builtin_amdgcn_sad_u8(kp, kt, 0u);  // |dr| + |dg| + |db|
          const float sgk = S[(j < 0 ? -j : j) * (R + 1) + (i < 0 ? -i : i)] * sg[k];
          const float w = sgk * sc[t];
          const float wd = w * sd[t];
          const float wu = w * su[t];
          num = num + wd;
          nus = nus + wu;
          den = den + w;
        }
      }
    }
    const bool ok = den > 0.f && finite(den);
    const long p = image + (long)y * a.Ws + x;
    a.disp_out[p] = ok ? num / den : sd[ci];
    a.unc_out[p] = ok ? nus / den : su[ci];
  }
}

// ---------------------------------------------------------------- fusion --
struct FuseArgs {
  const float *disp_in, *unc_in, *lr_error;
  long count;
  const float *params, *fp;
  float *mean, *var;
  float *disparity, *uncertainty, *depth;
  uint8_t* valid;
  float* disp_var;
};

__device__ __forceinline__ void load4(const float* p, long i0, int live, bool vec, float* o) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p + i0);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = j < live ? p[i0 + j] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* p, long i0, int live, bool vec, const float* o) {
  if (vec) {
    *reinterpret_cast<float4*>(p + i0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < live) p[i0 + j] = o[j];
  }
}

// one thread per 4 consecutive pixels; VEC: every given pointer is aligned for
// a 16-byte (valid: 4-byte) access.  A thread reads all it needs before its
// first store, so an output may be its own input.
template <bool VEC>
__global__ void __launch_bounds__(256) disp_fuse_kernel(FuseArgs a) {
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= a.count) return;
  const float fb = a.params[0], min_disp = a.params[1], max_unc = a.params[2],
              max_lr = a.params[3];
  const float na = a.fp[1], vfloor = a.fp[2], q = a.fp[3], g2 = a.fp[4];
  const long left = a.count - i0;
  const int live = left < 4 ? (int)left : 4;
  const bool vec = VEC && live == 4;
  const bool state = a.mean != nullptr;
  float d[4], s[4], l[4] = {0.f, 0.f, 0.f, 0.f}, mean[4], var[4];
  load4(a.disp_in, i0, live, vec, d);
  load4(a.unc_in, i0, live, vec, s);
  if (a.valid) load4(a.lr_error, i0, live, vec, l);
  if (state) {
    load4(a.mean, i0, live, vec, mean);
    load4(a.var, i0, live, vec, var);
  }
  float D[4], dep[4];
  uint32_t ok = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    D[j] = d[j];
    if (state) {
      const float t = na * s[j];
      const float tt = t * t;
      const float m = tt + vfloor;
      const bool fresh = finite(d[j]) && finite(m);
      const float p = var[j] + q;
      const float e = d[j] - mean[j];
      const float pm = p + m;
      const float ee = e * e;
      const float gp = g2 * pm;
      if (fresh && var[j] >= 0.f && ee <= gp) {  // keep
        const float K = p / pm;
        const float Ke = K * e;
        const float Kp = K * p;
        mean[j] = mean[j] + Ke;
        var[j] = p - Kp;
      } else if (fresh) {  // reset
        mean[j] = d[j];
        var[j] = m;
      }  // not fresh: the state stays
      D[j] = var[j] >= 0.f ? mean[j] : d[j];
    }
    const bool far = D[j] > min_disp;
    dep[j] = far ? fb / D[j] : 0.f;
    ok |= (uint32_t)(far && s[j] <= max_unc && l[j] <= max_lr) << (8 * j);
  }
  if (state) {
    store4(a.mean, i0, live, vec, mean);
    store4(a.var, i0, live, vec, var);
    if (a.disp_var) store4(a.disp_var, i0, live, vec, var);
  }
  if (a.disparity) store4(a.disparity, i0, live, vec, D);
  if (a.uncertainty) store4(a.uncertainty, i0, live, vec, s);
  if (a.depth) store4(a.depth, i0, live, vec, dep);
  if (a.valid) {
    if (vec) {
      *reinterpret_cast<uint32_t*>(a.valid + i0) = ok;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < live) a.valid[i0 + j] = (uint8_t)((ok >> (8 * j)) & 1u);
    }
  }
}

}  // namespace

extern "C" {

int um_disp_smooth(const float* disp, const float* unc, const unsigned char* frame, int N, int Hs,
                   int Ws, int R, int step, const float* S, const float* G, const float* fp,
                   float* disp_out, float* unc_out, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && Hs >= 1 && Ws >= 1 && (long)N * Hs * Ws <= INT_MAX,
               "um_disp_smooth: N=%d Hs=%d Ws=%d (each >= 1, N * Hs * Ws <= %d)", N, Hs, Ws,
               INT_MAX);
  UM_CHECK_ARG(R >= 1 && R <= 3 && step >= 1 && (long)R * step <= SM_MAX_HALO,
               "um_disp_smooth: R=%d step=%d (1 <= R <= 3, step >= 1, R * step <= %d)", R, step,
               SM_MAX_HALO);
  UM_CHECK_ARG(disp && unc && frame && S && G && fp && disp_out && unc_out,
               "um_disp_smooth: null pointer");
  UM_CHECK_ARG(aligned(disp, 4) && aligned(unc, 4) && aligned(S, 4) && aligned(G, 4) &&
                   aligned(fp, 4) && aligned(disp_out, 4) && aligned(unc_out, 4),
               "um_disp_smooth: a float pointer that is not 4-byte aligned");
  const int halo = R * step, th = smooth_tile_rows(halo);
  const int tiles_x = (Ws + SM_TW - 1) / SM_TW, tiles_y = (Hs + th - 1) / th;
  const long tiles = (long)N * tiles_y * tiles_x;  // <= N * Hs * Ws
  const size_t lds = (size_t)smooth_lds_floats(th, halo) * sizeof(float);
  SmoothArgs a{disp, unc, frame, Hs, Ws, step, th, tiles_x, tiles_y, S, G, fp, disp_out, unc_out};
  const dim3 grid((unsigned)tiles), block(SM_THREADS);
  if (R == 1)
    hipLaunchKernelGGL(disp_smooth_kernel<1>, grid, block, lds, st, a);
  else if (R == 2)
    hipLaunchKernelGGL(disp_smooth_kernel<2>, grid, block, lds, st, a);
  else
    hipLaunchKernelGGL(disp_smooth_kernel<3>, grid, block, lds, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

int um_disp_fuse(const float* disp_in, const float* unc_in, const float* lr_error, long count,
                 const float* params, const float* fp, float* mean, float* var, float* disparity,
                 float* uncertainty, float* depth, unsigned char* valid, float* disp_var,
                 hipStream_t st) {
  const long blocks = (count + 1023) / 1024;
  UM_CHECK_ARG(count >= 1 && blocks <= INT_MAX, "um_disp_fuse: count=%ld", count);
  UM_CHECK_ARG(disp_in && unc_in && params && fp,
               "um_disp_fuse: null pointer (disp_in, unc_in, params or fp)");
  UM_CHECK_ARG(lr_error || !valid, "um_disp_fuse: valid needs lr_error");
  UM_CHECK_ARG((mean == nullptr) == (var == nullptr),
               "um_disp_fuse: mean and var are given together or not at all");
  const void* fl[] = {disp_in, unc_in, lr_error, params, fp, mean, var, disparity, uncertainty,
                      depth, disp_var};
  bool a4 = true, a16 = aligned(valid, 4);
  for (const void* p : fl) a4 = a4 && aligned(p, 4);
  for (const void* p : fl)
    if (p != params && p != fp) a16 = a16 && aligned(p, 16);
  UM_CHECK_ARG(a4, "um_disp_fuse: a float pointer that is not 4-byte aligned");
  FuseArgs a{disp_in, unc_in, lr_error, count, params, fp, mean, var, disparity, uncertainty,
             depth, valid, disp_var};
  if (a16)
    hipLaunchKernelGGL(disp_fuse_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(disp_fuse_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
