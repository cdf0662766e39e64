// The distance head of LPIPS (lpips 0.1.4, LPIPS(net='vgg', lpips=True, spatial=False)) on one feature level, NCHW, for
// gfx950: forward and the gradient with respect to the first feature tensor, for f32 tensors and, under bf16 autocast,
// for bf16 a, b and ga (amk_lpips_bf16_*).
//
// torch runs the head as about a dozen memory-bound ops per level (two squares, two channel sums, two square roots, two
// divisions, a difference, a square, the 1x1 convolution, the spatial mean) and autograd keeps several tensors of the
// features' size for the backward.  Here the forward reads a and b twice and writes three f32 numbers per pixel, the
// backward reads a and b once and writes ga.  No float atomics: out and ga are bitwise reproducible, and a sample's
// result does not depend on the batch it sits in (the geometry below is a function of C and HW alone).
//
// Notation, per sample n and pixel p over the C channels: na = sqrt(sum_c a_c^2), ah_c = a_c / (na + eps), likewise nb,
// bh_c; e_c = ah_c - bh_c, d = sum_c w_c e_c^2, t = sum_c w_c e_c ah_c; out_n = (1 / HW) sum_p d.  Given the cotangent g_n,
// k = 2 g_n / HW and ga_c = k (w_c e_c - ah_c t (na + eps) / na) / (na + eps).
// The one deliberate difference from autograd: a pixel with na = 0 gets ga_c = 0 for every c (autograd's sqrt'(0) * 0 is
// NaN there; the in-place ReLU in front of every level discards whatever arrives at such a pixel).
//
// rows (3, N, HW), what the forward keeps so that the backward is one sweep:
//   row 0: 1 / (na + eps), and 0 where na == 0 -- the zero norm is recognised by that 0, and the backward's final
//          multiplication by row 0 gives the ga = 0 of the rule above without a branch;
//   row 1: 1 / (nb + eps);
//   row 2: t (na + eps) / na, taken in the forward where na itself is at hand (0 where na == 0).
//
// Work split.  A workgroup of 256 threads owns a tile of one sample's pixels over all C channels.  Thread t is pixel lane
// t % PL of channel slice t / PL (PL = 256, 64, 16 or 4; CS = 256 / PL slices): it owns W consecutive pixels and walks
// the channels slice, slice + CS, ...  Each sweep's per-pixel sums are folded over the slices in a fixed order: a
// butterfly over the slices that share a wave, then the four waves in order through LDS.  With PL = 256 the tile is
// 256 W pixels and nothing is folded; with PL = 4 a workgroup holds 4 W pixels and every thread an eighth of a 512-channel
// sweep, which is what keeps 512 x 16^2 and 512 x 32^2 (a few thousand pixels per batch) from a handful of workgroups.
// PL is the largest for which a sample is at least 64 tiles (512 workgroups at batch 8, two per CU), and CS never exceeds C.
//
// A thread owns the same pixels in every plane, and plane (n, c) starts at element (n C + c) HW: when HW is a multiple
// of the 16-byte width (4 f32, 8 bf16) every plane starts aligned and W is that width; otherwise the planes' alignments
// differ from channel to channel, no pixel run is aligned in all of them, and every access is one element (W = 1; a wave
// still reads 64 consecutive elements).  So there is no head or tail: a thread's W pixels are all inside the plane or
// all outside.
//
// bf16: T = __bf16 widens a and b to f32 on the load and rounds ga once, to nearest even, on the store; w, the rows, the
// partials and out are f32, as is everything between.
#include "amk_planes.h"

// Identical inputs must give out == 0 and ga == 0 exactly: ah - bv * ib contracted to fma(-bv, ib, ah) would leave the
// rounding error of ah behind.  So no contraction in this file; the sums say fmaf where they mean it.
#pragma clang fp contract(off)

namespace amk_lpips {

using namespace amk_planes;  // BLOCK, WAVES, Width, Vec, ld, st, Sum, Chan, block_reduce
constexpr int MIN_TILES = 64;  // per sample, while a smaller PL can still give them

struct Geo {
  int N, C;
  int64_t HW;
  int W;       // pixels per thread: the 16-byte width, or 1
  int PL;      // pixel lanes per workgroup
  int CS;      // channel slices per workgroup, PL CS == BLOCK
  int64_t TP;  // pixels per tile, PL W
  int64_t tiles;  // per sample
};

// VW: elements per 16-byte access (4 for f32, 8 for bf16)
static Geo make_geo(int N, int C, int64_t HW, int VW) {
  Geo g;
  g.N = N; g.C = C; g.HW = HW;
  g.W = HW % VW == 0 ? VW : 1;
  g.PL = BLOCK;
  while (g.PL > 4 && (HW + (int64_t)g.PL * g.W - 1) / ((int64_t)g.PL * g.W) < MIN_TILES && BLOCK / (g.PL / 4) <= C)
    g.PL /= 4;
  g.CS = BLOCK / g.PL;
  g.TP = (int64_t)g.PL * g.W;
  g.tiles = (HW + g.TP - 1) / g.TP;
  return g;
}

// Sum of v over the channel slices of the workgroup, in a fixed order; every thread returns the total of its pixels.
// Slices that share a wave (PL < 64) meet in a butterfly over lane distances PL, 2 PL, .. 32 (both partners add the same
// two numbers, so they agree to the bit); the waves' sums are then added in wave order from lds (K x WAVES x 64 floats).
// PL is uniform over the workgroup.
template <int K>
__device__ __forceinline__ void slice_sum(float (&v)[K], int PL, float* lds) {
  if (PL == BLOCK) return;
  for (int o = PL; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int PW = PL < 64 ? PL : 64;
  if (lane < PW) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[(k * WAVES + wave) * 64 + lane] = v[k];
  }
  __syncthreads();
  const int l = lane & (PW - 1);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = lds[(k * WAVES) * 64 + l];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += lds[(k * WAVES + w) * 64 + l];
    v[k] = s;
  }
  __syncthreads();
}

// Sum over the workgroup's threads in a fixed order: a butterfly inside each wave, then the waves in order.
__device__ __forceinline__ float block_sum(float v, float* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = lds[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------- forward
// Workgroup n tiles + j: rows of its pixels and part[n tiles + j] = the sum of d over them.
template <class T, int W>
__global__ __launch_bounds__(BLOCK) void fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                    const float* __restrict__ w, Geo g, float eps,
                                                    float* __restrict__ rows, float* __restrict__ part) {
  __shared__ float lds[2 * W * BLOCK];
  const int n = (int)(blockIdx.x / g.tiles);
  const int64_t tile = blockIdx.x % g.tiles;
  const int l = threadIdx.x % g.PL, s = threadIdx.x / g.PL;
  const int64_t p = tile * g.TP + (int64_t)l * W;
  const bool live = p < g.HW;  // HW is a multiple of W: all W pixels or none
  const int64_t base = (int64_t)n * g.C * g.HW + p;

  float v[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; ++k) v[k] = 0.f;
  if (live) {
#pragma unroll 4
    for (int c = s; c < g.C; c += g.CS) {
      float av[W], bv[W];
      ld<W>(a + base + (int64_t)c * g.HW, av);
      ld<W>(b + base + (int64_t)c * g.HW, bv);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        v[k] = fmaf(av[k], av[k], v[k]);
        v[W + k] = fmaf(bv[k], bv[k], v[W + k]);
      }
    }
  }
  slice_sum<2 * W>(v, g.PL, lds);

  float ia[W], ib[W], r[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float na = sqrtf(v[k]), nb = sqrtf(v[W + k]);
    ia[k] = 1.f / (na + eps);
    ib[k] = 1.f / (nb + eps);
    r[k] = na > 0.f ? (na + eps) / na : 0.f;
  }

  // the second sweep re-reads the tile that was just touched
#pragma unroll
  for (int k = 0; k < 2 * W; ++k) v[k] = 0.f;
  if (live) {
#pragma unroll 4
    for (int c = s; c < g.C; c += g.CS) {
      float av[W], bv[W];
      ld<W>(a + base + (int64_t)c * g.HW, av);
      ld<W>(b + base + (int64_t)c * g.HW, bv);
      const float wc = w[c];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float ah = av[k] * ia[k];
        const float e = ah - bv[k] * ib[k];
        const float we = wc * e;
        v[k] = fmaf(we, e, v[k]);
        v[W + k] = fmaf(we, ah, v[W + k]);
      }
    }
  }
  slice_sum<2 * W>(v, g.PL, lds);

  float dsum = 0.f;
  if (live && s == 0) {
    float r0[W], r2[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      r0[k] = r[k] > 0.f ? ia[k] : 0.f;
      r2[k] = v[W + k] * r[k];
      dsum += v[k];
    }
    const int64_t nhw = (int64_t)g.N * g.HW, q = (int64_t)n * g.HW + p;
    st<W>(rows + q, r0);
    st<W>(rows + nhw + q, ib);
    st<W>(rows + 2 * nhw + q, r2);
  }
  dsum = block_sum(dsum, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = dsum;
}

// out_n = (sum of the sample's partials, in a fixed order) / HW; workgroup n.
__global__ __launch_bounds__(BLOCK) void fold_kernel(const float* __restrict__ part, Geo g, float* __restrict__ out) {
  __shared__ float lds[WAVES];
  const int n = blockIdx.x;
  float v = 0.f;
  for (int64_t j = threadIdx.x; j < g.tiles; j += BLOCK) v += part[(int64_t)n * g.tiles + j];
  v = block_sum(v, lds);
  if (threadIdx.x == 0) out[n] = v / (float)g.HW;
}

// ---------------------------------------------------------------- backward
// ga_c = k (w_c e_c - ah_c row2) row0 on the forward's tiling; every thread writes the channels of its slice.
template <class T, int W>
__global__ __launch_bounds__(BLOCK) void bwd_kernel(const float* __restrict__ gout, const T* __restrict__ a,
                                                    const T* __restrict__ b, const float* __restrict__ w,
                                                    const float* __restrict__ rows, Geo g, T* __restrict__ ga) {
  const int n = (int)(blockIdx.x / g.tiles);
  const int64_t tile = blockIdx.x % g.tiles;
  const int l = threadIdx.x % g.PL, s = threadIdx.x / g.PL;
  const int64_t p = tile * g.TP + (int64_t)l * W;
  if (p >= g.HW) return;  // no barrier below
  const int64_t base = (int64_t)n * g.C * g.HW + p;
  const int64_t nhw = (int64_t)g.N * g.HW, q = (int64_t)n * g.HW + p;
  const float k2 = 2.f * gout[n] / (float)g.HW;
  float ia[W], ib[W], tr[W];
  ld<W>(rows + q, ia);
  ld<W>(rows + nhw + q, ib);
  ld<W>(rows + 2 * nhw + q, tr);
#pragma unroll 4
  for (int c = s; c < g.C; c += g.CS) {
    float av[W], bv[W];
    ld<W>(a + base + (int64_t)c * g.HW, av);
    ld<W>(b + base + (int64_t)c * g.HW, bv);
    const float wc = w[c];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float ah = av[k] * ia[k];
      const float e = ah - bv[k] * ib[k];
      av[k] = k2 * (wc * e - ah * tr[k]) * ia[k];
    }
    st<W>(ga + base + (int64_t)c * g.HW, av);
  }
}

template <class T> struct Vec { static constexpr int W = 4; };
template <> struct Vec<__bf16> { static constexpr int W = 8; };

template <class T>
static void launch_fwd(const T* a, const T* b, const float* w, int N, int C, int64_t HW, float eps, float* out,
                       float* rows, float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, Vec<T>::W);
  const dim3 grid((unsigned)(N * g.tiles)), block(BLOCK);
  if (g.W == 1) hipLaunchKernelGGL((fwd_kernel<T, 1>), grid, block, 0, st, a, b, w, g, eps, rows, ws);
  else hipLaunchKernelGGL((fwd_kernel<T, Vec<T>::W>), grid, block, 0, st, a, b, w, g, eps, rows, ws);
  hipLaunchKernelGGL(fold_kernel, dim3(N), block, 0, st, ws, g, out);
}

template <class T>
static void launch_bwd(const float* gout, const T* a, const T* b, const float* w, const float* rows, int N, int C,
                       int64_t HW, T* ga, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, Vec<T>::W);
  const dim3 grid((unsigned)(N * g.tiles)), block(BLOCK);
  if (g.W == 1) hipLaunchKernelGGL((bwd_kernel<T, 1>), grid, block, 0, st, gout, a, b, w, rows, g, ga);
  else hipLaunchKernelGGL((bwd_kernel<T, Vec<T>::W>), grid, block, 0, st, gout, a, b, w, rows, g, ga);
}

}  // namespace amk_lpips

using namespace amk_lpips;

#define AMK_LPIPS_SHAPE(what, VW)                                                                  \
  AMK_CHECK_ARG(N > 0 && C > 0 && HW > 0, what ": non-positive size");                              \
  AMK_CHECK_SUPPORTED((int64_t)N * make_geo(N, C, HW, VW).tiles < ((int64_t)1 << 31),               \
                      what ": shape N %d C %d HW %lld needs a grid beyond 2^31", N, C, (long long)HW)

extern "C" int64_t amk_lpips_ws_floats(int N, int C, int64_t HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (int64_t)N * make_geo(N, C, HW, 4).tiles;
}

extern "C" int amk_lpips_fwd(const float* a, const float* b, const float* w, int N, int C, int64_t HW, float eps,
                             float* out, float* rows, float* ws, void* stream) {
  AMK_CHECK_ARG(a && b && w && out && rows && ws, "amk_lpips_fwd: null pointer");
  AMK_LPIPS_SHAPE("amk_lpips_fwd", 4);
  AMK_CHECK_ARG(a16(a) && a16(b) && a16(rows), "amk_lpips_fwd: a, b and rows must be 16-byte aligned");
  launch_fwd<float>(a, b, w, N, C, HW, eps, out, rows, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_lpips_fwd");
  return AMK_OK;
}

extern "C" int amk_lpips_bwd(const float* g, const float* a, const float* b, const float* w, const float* rows, int N,
                             int C, int64_t HW, float eps, float* ga, void* stream) {
  (void)eps;  // the backward reads it through the rows
  AMK_CHECK_ARG(g && a && b && w && rows && ga, "amk_lpips_bwd: null pointer");
  AMK_LPIPS_SHAPE("amk_lpips_bwd", 4);
  AMK_CHECK_ARG(a16(a) && a16(b) && a16(ga) && a16(rows), "amk_lpips_bwd: a, b, ga and rows must be 16-byte aligned");
  launch_bwd<float>(g, a, b, w, rows, N, C, HW, ga, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_lpips_bwd");
  return AMK_OK;
}

// ---------------------------------------------------------------- bf16 a, b, ga
extern "C" int64_t amk_lpips_bf16_ws_floats(int N, int C, int64_t HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (int64_t)N * make_geo(N, C, HW, 8).tiles;
}

extern "C" int amk_lpips_bf16_fwd(const void* a, const void* b, const float* w, int N, int C, int64_t HW, float eps,
                                  float* out, float* rows, float* ws, void* stream) {
  AMK_CHECK_ARG(a && b && w && out && rows && ws, "amk_lpips_bf16_fwd: null pointer");
  AMK_LPIPS_SHAPE("amk_lpips_bf16_fwd", 8);
  AMK_CHECK_ARG(a16(a) && a16(b) && a16(rows), "amk_lpips_bf16_fwd: a, b and rows must be 16-byte aligned");
  launch_fwd<__bf16>(static_cast<const __bf16*>(a), static_cast<const __bf16*>(b), w, N, C, HW, eps, out, rows, ws,
                     static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_lpips_bf16_fwd");
  return AMK_OK;
}

extern "C" int amk_lpips_bf16_bwd(const float* g, const void* a, const void* b, const float* w, const float* rows, int N,
                                  int C, int64_t HW, float eps, void* ga, void* stream) {
  (void)eps;
  AMK_CHECK_ARG(g && a && b && w && rows && ga, "amk_lpips_bf16_bwd: null pointer");
  AMK_LPIPS_SHAPE("amk_lpips_bf16_bwd", 8);
  AMK_CHECK_ARG(a16(a) && a16(b) && a16(ga) && a16(rows),
                "amk_lpips_bf16_bwd: a, b, ga and rows must be 16-byte aligned");
  launch_bwd<__bf16>(g, static_cast<const __bf16*>(a), static_cast<const __bf16*>(b), w, rows, N, C, HW,
                     static_cast<__bf16*>(ga), static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_lpips_bf16_bwd");
  return AMK_OK;
}
