// 3-D points of the deployment path (umamd/points.py, the optional point stage
// of umamd/deploy.py DepthPipeline): the pipeline's metric depth back-projected
// through the pinhole intrinsics (fx, fy, cx, cy), on the device.
//
//   um_depth_backproject  the organised map [N][Hs][Ws][3]: (X, Y, Z) where
//                    the pixel is kept, (0, 0, 0) elsewhere; 17 bytes per
//                    pixel, one streaming launch
//   um_depth_cloud   the packed cloud of the kept sites of a stride lattice,
//                    image-major then row-major, with the uncertainty and the
//                    frame's colour per point and the per-image offsets: a
//                    count per tile of CLOUD_TILE sites, a one-workgroup
//                    exclusive scan of the counts, and a pack pass whose
//                    workgroups order their own sites (thread count -> wave
//                    scan -> wave totals in LDS); no atomics, no state
#include "common.h"

#include <limits.h>

namespace {

// Every float step below is its own f32 operation (the definition in
// include/umamd.h is written that way and the tests demand equality).
#pragma clang fp contract(off)

constexpr int CLOUD_TILE = 1024;    // lattice sites of a tile: 256 threads x 4
constexpr int SCAN_THREADS = 256;   // the one workgroup of the scan launch
static_assert(SCAN_THREADS == 256 && CLOUD_TILE == 4 * 256, "block_scan sums four waves");

__host__ __device__ inline bool aligned(const void* p, uintptr_t a) {
  return ((uintptr_t)p & (a - 1)) == 0;
}

// one coordinate: ((float)i - c) * Z / f, three f32 operations, IEEE division
__device__ __forceinline__ float backproject(int i, float c, float z, float f) {
  const float d = (float)i - c;
  const float p = d * z;
  return p / f;
}

// --------------------------------------------------------- organised map --
// one thread per 4 consecutive pixels of the flat [N * Hs][Ws] map; VEC: depth
// and xyz are aligned for 16-byte accesses and valid (if given) for a dword
template <bool VEC>
__global__ void __launch_bounds__(256)
backproject_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid, long count,
                   int Hs, int Ws, const float* __restrict__ intr, float* __restrict__ xyz) {
  const long i0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (i0 >= count) return;
  const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
  const long row0 = i0 / Ws;
  int u = (int)(i0 - row0 * Ws);
  int v = (int)(row0 % Hs);
  const bool full = i0 + 4 <= count;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t m = 0x01010101u;
  if (VEC && full) {
    const float4 z4 = *reinterpret_cast<const float4*>(depth + i0);
    z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
    if (valid) m = *reinterpret_cast<const uint32_t*>(valid + i0);
  } else {
    for (int j = 0; j < 4 && i0 + j < count; ++j) {
      z[j] = depth[i0 + j];
      if (valid) m = (m & ~(0xffu << (8 * j))) | ((uint32_t)valid[i0 + j] << (8 * j));
    }
  }
  float o[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool kept = ((m >> (8 * j)) & 0xffu) != 0;
    o[3 * j] = kept ? backproject(u, cx, z[j], fx) : 0.f;
    o[3 * j + 1] = kept ? backproject(v, cy, z[j], fy) : 0.f;
    o[3 * j + 2] = kept ? z[j] : 0.f;
    if (++u == Ws) {
      u = 0;
      if (++v == Hs) v = 0;
    }
  }
  float* op = xyz + 3 * i0;
  if (VEC && full) {
    float4* o4 = reinterpret_cast<float4*>(op);
    o4[0] = make_float4(o[0], o[1], o[2], o[3]);
    o4[1] = make_float4(o[4], o[5], o[6], o[7]);
    o4[2] = make_float4(o[8], o[9], o[10], o[11]);
  } else {
    for (int j = 0; j < 4 && i0 + j < count; ++j) {
      op[3 * j] = o[3 * j];
      op[3 * j + 1] = o[3 * j + 1];
      op[3 * j + 2] = o[3 * j + 2];
    }
  }
}

// ------------------------------------------------------------ packed cloud --
struct CloudArgs {
  const float* depth;
  const uint8_t* valid;
  const float* uncertainty;
  const uint8_t* frame;
  int Hs, Ws, stride;
  int Wl;     // lattice columns
  int sites;  // lattice sites of one image, Hl * Wl
  int tpi;    // tiles per image
  const float* intr;
  int* tiles;  // the workspace: per tile its count, after the scan its first row
  float* xyzu;
  uint8_t* rgba;
  int* offsets;
};

// The four lattice sites of a thread: s0 .. s0 + 3 of image n (those below
// a.sites exist), and the pixel each one reads.
struct Sites {
  int n, s0, u[4], v[4];
  long pix[4];
  bool vec;  // S1 only: all four exist; they are pixels pix[0] .. pix[0] + 3
};

template <bool S1>
__device__ __forceinline__ Sites thread_sites(const CloudArgs& a) {
  Sites t;
  t.n = (int)(blockIdx.x / (unsigned)a.tpi);
  const long s0 = (long)(blockIdx.x % (unsigned)a.tpi) * CLOUD_TILE + 4 * (int)threadIdx.x;
  t.s0 = (int)(s0 < a.sites ? s0 : a.sites);  // past the image: no site exists
  const long image = (long)t.n * a.Hs * a.Ws;
  int lv = t.s0 / a.Wl, lu = t.s0 - lv * a.Wl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t.v[j] = S1 ? lv : lv * a.stride;
    t.u[j] = S1 ? lu : lu * a.stride;
    t.pix[j] = image + (long)t.v[j] * a.Ws + t.u[j];
    if (++lu == a.Wl) lu = 0, ++lv;
  }
  t.vec = S1 && a.sites - t.s0 >= 4;
  return t;
}

// bit j: site s0 + j exists and is kept
template <bool S1>
__device__ __forceinline__ int kept_mask(const CloudArgs& a, const Sites& t) {
  const int live = a.sites - t.s0;  // sites of this thread that exist
  if (live <= 0) return 0;
  if (!a.valid) return live >= 4 ? 0xf : (1 << live) - 1;
  int m = 0;
  if (S1 && t.vec && aligned(a.valid + t.pix[0], 4)) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(a.valid + t.pix[0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= ((w >> (8 * j)) & 0xffu) ? 1 << j : 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < live && a.valid[t.pix[j]] != 0) m |= 1 << j;
  }
  return m;
}

// inclusive scan of x over the workgroup's 256 threads; red: 4 ints of LDS;
// total: the workgroup's sum
__device__ __forceinline__ int block_scan(int x, int* red, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int r = red[w];
    before += w < wave ? r : 0;
    total += r;
  }
  return before + incl;
}

// launch 1: tiles[tile] = kept sites of the tile
template <bool S1>
__global__ void __launch_bounds__(256) cloud_count_kernel(CloudArgs a) {
  __shared__ int red[4];
  const Sites t = thread_sites<S1>(a);
  int total;
  block_scan(__popc(kept_mask<S1>(a, t)), red, total);
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

// launch 2, one workgroup: the counts become their exclusive prefix sums (in
// place), SCAN_THREADS tiles per turn of the loop with the sum so far carried
// in a register; offsets[n] is the first row of image n's first tile
__global__ void __launch_bounds__(SCAN_THREADS)
cloud_scan_kernel(int* __restrict__ tiles, int ntiles, int tpi, int N, int* __restrict__ offsets) {
  __shared__ int red[4];
  int carry = 0;
  for (long base = 0; base < ntiles; base += SCAN_THREADS) {
    const long t = base + threadIdx.x;
    const int c = t < ntiles ? tiles[t] : 0;
    int total;
    const int first = carry + block_scan(c, red, total) - c;
    if (t < ntiles) {
      tiles[t] = first;
      if (t % tpi == 0) offsets[t / tpi] = first;
    }
    carry += total;
    __syncthreads();  // red is written again in the next turn
  }
  if (threadIdx.x == 0) offsets[N] = carry;
}

// launch 3: the kept sites of a tile -> rows tiles[tile] .. of xyzu and rgba
template <bool S1>
__global__ void __launch_bounds__(256) cloud_pack_kernel(CloudArgs a) {
  __shared__ int red[4];
  const Sites t = thread_sites<S1>(a);
  const int m = kept_mask<S1>(a, t);
  const int cnt = __popc(m);
  int total;
  long row = a.tiles[blockIdx.x] + block_scan(cnt, red, total) - cnt;
  if (m == 0) return;
  const float fx = a.intr[0], fy = a.intr[1], cx = a.intr[2], cy = a.intr[3];
  float z[4], s[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t c[4] = {0u, 0u, 0u, 0u};  // r | g << 8 | b << 16
  const bool colour = a.frame && a.rgba;
  if (S1 && t.vec && aligned(a.depth + t.pix[0], 16)) {
    const float4 z4 = *reinterpret_cast<const float4*>(a.depth + t.pix[0]);
    z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = (m >> j) & 1 ? a.depth[t.pix[j]] : 0.f;
  }
  if (a.uncertainty) {
    if (S1 && t.vec && aligned(a.uncertainty + t.pix[0], 16)) {
      const float4 s4 = *reinterpret_cast<const float4*>(a.uncertainty + t.pix[0]);
      s[0] = s4.x, s[1] = s4.y, s[2] = s4.z, s[3] = s4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = (m >> j) & 1 ? a.uncertainty[t.pix[j]] : 0.f;
    }
  }
  if (colour) {
    if (S1 && t.vec && aligned(a.frame + 3 * t.pix[0], 4)) {
      // the 12 bytes of four consecutive pixels
      const uint32_t* fp = reinterpret_cast<const uint32_t*>(a.frame + 3 * t.pix[0]);
      const uint32_t f0 = fp[0], f1 = fp[1], f2 = fp[2];
      c[0] = f0 & 0xffffffu;
      c[1] = (f0 >> 24) | ((f1 & 0xffffu) << 8);
      c[2] = (f1 >> 16) | ((f2 & 0xffu) << 16);
      c[3] = f2 >> 8;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((m >> j) & 1) {
          const uint8_t* e = a.frame + 3 * t.pix[j];
          c[j] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((m >> j) & 1)) continue;
    const float x = backproject(t.u[j], cx, z[j], fx);
    const float y = backproject(t.v[j], cy, z[j], fy);
    reinterpret_cast<float4*>(a.xyzu)[row] = make_float4(x, y, z[j], s[j]);
    if (colour) reinterpret_cast<uint32_t*>(a.rgba)[row] = c[j] | 0xff000000u;
    ++row;
  }
}

// lattice of a cloud call: false if a size is bad or past the int limits
struct Lattice {
  int Hl, Wl, tpi;
  long sites, tiles;
};

inline bool lattice(int N, int Hs, int Ws, int stride, Lattice& l) {
  if (N < 1 || Hs < 1 || Ws < 1 || stride < 1) return false;
  l.Hl = (Hs - 1) / stride + 1;
  l.Wl = (Ws - 1) / stride + 1;
  l.sites = (long)l.Hl * l.Wl;
  if (l.sites > INT_MAX || (long)N * l.sites > INT_MAX || (long)N * Hs > INT_MAX) return false;
  l.tpi = (int)((l.sites + CLOUD_TILE - 1) / CLOUD_TILE);
  l.tiles = (long)N * l.tpi;
  return true;
}

}  // namespace

extern "C" {

int um_depth_backproject(const float* depth, const unsigned char* valid, int N, int Hs, int Ws,
                         const float* intr, float* xyz, hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && Hs >= 1 && Ws >= 1, "um_depth_backproject: N=%d Hs=%d Ws=%d", N, Hs, Ws);
  UM_CHECK_ARG(depth && intr && xyz, "um_depth_backproject: null pointer (depth, intr or xyz)");
  UM_CHECK_ARG(aligned(depth, 4) && aligned(intr, 4) && aligned(xyz, 4),
               "um_depth_backproject: a float pointer that is not 4-byte aligned");
  UM_CHECK_ARG((long)N * Hs <= INT_MAX, "um_depth_backproject: %ld rows, at most %d",
               (long)N * Hs, INT_MAX);
  const long count = (long)N * Hs * Ws;
  const long blocks = (count + 1023) / 1024;
  UM_CHECK_ARG(blocks <= INT_MAX, "um_depth_backproject: %ld pixels", count);
  if (aligned(depth, 16) && aligned(valid, 4) && aligned(xyz, 16))
    hipLaunchKernelGGL(backproject_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, depth,
                       valid, count, Hs, Ws, intr, xyz);
  else
    hipLaunchKernelGGL(backproject_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, depth,
                       valid, count, Hs, Ws, intr, xyz);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

long um_depth_cloud_ws(int N, int Hs, int Ws, int stride) {
  Lattice l;
  return lattice(N, Hs, Ws, stride, l) ? l.tiles * (long)sizeof(int) : 0;
}

int um_depth_cloud(const float* depth, const unsigned char* valid, const float* uncertainty,
                   const unsigned char* frame, int N, int Hs, int Ws, int stride,
                   const float* intr, void* ws, float* xyzu, unsigned char* rgba, int* offsets,
                   hipStream_t st) {
  UM_CHECK_ARG(N >= 1 && Hs >= 1 && Ws >= 1, "um_depth_cloud: N=%d Hs=%d Ws=%d", N, Hs, Ws);
  UM_CHECK_ARG(stride >= 1, "um_depth_cloud: stride=%d", stride);
  Lattice l;
  UM_CHECK_ARG(lattice(N, Hs, Ws, stride, l),
               "um_depth_cloud: %d images of %d x %d at stride %d: the capacity N * Hl * Wl and "
               "the rows N * Hs must not exceed %d", N, Hs, Ws, stride, INT_MAX);
  UM_CHECK_ARG(depth && intr && ws && xyzu && offsets,
               "um_depth_cloud: null pointer (depth, intr, ws, xyzu or offsets)");
  UM_CHECK_ARG(aligned(depth, 4) && aligned(uncertainty, 4) && aligned(intr, 4) &&
                   aligned(ws, 4) && aligned(offsets, 4),
               "um_depth_cloud: a float or int pointer that is not 4-byte aligned");
  UM_CHECK_ARG(aligned(xyzu, 16) && aligned(rgba, 4),
               "um_depth_cloud: xyzu must be 16-byte and rgba 4-byte aligned (one store per row)");
  CloudArgs a{depth, valid, uncertainty, frame, Hs, Ws, stride, l.Wl, (int)l.sites, l.tpi, intr,
              static_cast<int*>(ws), xyzu, rgba, offsets};
  const dim3 grid((unsigned)l.tiles), block(256);
  if (stride == 1)
    hipLaunchKernelGGL(cloud_count_kernel<true>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(cloud_count_kernel<false>, grid, block, 0, st, a);
  UM_LAUNCH_CHECK();
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, a.tiles, (int)l.tiles,
                     l.tpi, N, offsets);
  UM_LAUNCH_CHECK();
  if (stride == 1)
    hipLaunchKernelGGL(cloud_pack_kernel<true>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(cloud_pack_kernel<false>, grid, block, 0, st, a);
  UM_LAUNCH_CHECK();
  return UM_OK;
}

}  // extern "C"
