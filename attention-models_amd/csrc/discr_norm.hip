// Training-mode BatchNorm2d + LeakyReLU of the PatchGAN discriminator, NCHW, for gfx950: forward, first-order
// backward and the double backward the gradient penalty needs; f32 tensors (amk_bnact_*) and, under bf16 autocast,
// bf16 x, z, gz, gx, ggx, g_gz and g_x (amk_bnact_bf16_*).
//
// ATen runs this stack as MIOpen batch-norm kernels plus separate LeakyReLU passes, and the
// double backward as ~80 small reductions and element-wise launches per layer.  Here every entry
// point is two launches: a reduction over the channel's data into per-workgroup partials, then an
// apply pass over the same tensors (which the Infinity Cache still holds) that folds the partials
// in a fixed order and writes the outputs.  No float atomics: results are bitwise reproducible.
//
// Notation (per channel c, n = N*HW): mu, var biased batch statistics, r = (var + eps)^-1/2,
// xh = (x - mu) r, y = gamma xh + beta, z = y > 0 ? y : slope y, s = dz/dy.  y is recomputed from x.
//
// Work split: a channel is cut into S segments -- runs of whole planes, or for planes larger than
// SEG pieces of one plane -- and workgroup (s, c) owns segment s of channel c in every kernel.  A
// plane (n, c) starts at element (n C + c) HW, which is only 4-byte aligned when HW is odd: each
// plane is walked as a scalar head, an aligned float4 body and a scalar tail.
//
// bf16: every kernel is a template on the element type T of the (N, C, HW) tensors.  T = __bf16 reads 8 elements per
// 16-byte access (heads of (8 - base % 8) % 8 and tails of up to 7 elements, pieces of a plane multiples of 8), widens
// them to f32 on the load and rounds each output to bf16 once, to nearest even, on the store.  Everything in between is
// the f32 arithmetic of the f32 kernels: gamma, beta, mean, rstd, the running statistics, dgamma, dbeta, the kept
// sums, gg_gamma, gg_beta, g_gamma and every partial stay f32; y is recomputed from x in every pass and s is taken from
// that f32 y, never from a rounded z.  SEG stays 4096 elements, so S, Q and the workspace are those of f32.
#include "amk_planes.h"

namespace amk_bn {

using namespace amk_planes;  // BLOCK, WAVES, Width, Vec, ld, st, Sum, Chan, block_reduce
constexpr int64_t SEG = 4096;  // target elements per workgroup segment

struct Geo {
  int N, C;
  int64_t HW;
  int PP;     // whole planes per segment (Q == 1)
  int Q;      // pieces per plane (PP == 1)
  int64_t L;  // elements per piece (Q > 1)
  int S;      // segments per channel
};

// VW: elements per 16-byte access (4 for f32, 8 for bf16); pieces are multiples of it.
static Geo make_geo(int N, int C, int64_t HW, int VW = 4) {
  Geo g;
  g.N = N; g.C = C; g.HW = HW;
  if (HW <= SEG) {
    g.PP = (int)(SEG / HW);
    if (g.PP > N) g.PP = N;
    g.Q = 1; g.L = HW;
    g.S = (N + g.PP - 1) / g.PP;
  } else {
    g.PP = 1;
    g.Q = (int)((HW + SEG - 1) / SEG);
    g.L = (((HW + g.Q - 1) / g.Q) + VW - 1) & ~(int64_t)(VW - 1);
    g.S = N * g.Q;
  }
  return g;
}

struct Seg {
  int p0, p1;
  int64_t e0, e1;
};

__device__ __forceinline__ Seg seg_of(const Geo& g, int s) {
  Seg r;
  if (g.Q == 1) {
    r.p0 = s * g.PP; r.p1 = min(g.N, r.p0 + g.PP);
    r.e0 = 0; r.e1 = g.HW;
  } else {
    r.p0 = s / g.Q; r.p1 = r.p0 + 1;
    r.e0 = min(g.HW, (int64_t)(s % g.Q) * g.L);
    r.e1 = min(g.HW, r.e0 + g.L);
  }
  return r;
}

__device__ __forceinline__ float seg_count(const Geo& g, int s) {
  const Seg r = seg_of(g, s);
  return (float)((int64_t)(r.p1 - r.p0) * (r.e1 - r.e0));
}

// Calls f(Width<VW>, off) for every aligned VW-element run (VW = 4 for f32, 8 for bf16) and f(Width<1>, off) for every
// edge element of segment s of channel c; `off` indexes the (N, C, HW) tensor of T.  Tensor bases are 16-byte aligned.
template <class T, class F>
__device__ __forceinline__ void seg_walk(const Geo& g, int c, int s, F&& f) {
  const Seg r = seg_of(g, s);
  const int64_t len = r.e1 - r.e0;
  const int t = threadIdx.x;
  for (int p = r.p0; p < r.p1; ++p) {
    const int64_t base = ((int64_t)p * g.C + c) * g.HW + r.e0;
    constexpr int VW = Vec<T>::W;
    const int head = (int)min((int64_t)((VW - (base & (VW - 1))) & (VW - 1)), len);
    const int64_t nv = (len - head) >> Vec<T>::SH;
    const int tail = (int)(len - head - VW * nv);
    for (int64_t i = t; i < nv; i += BLOCK) f(Width<VW>{}, base + head + VW * i);
    if (t < head) f(Width<1>{}, base + t);
    else if (t < head + tail) f(Width<1>{}, base + VW * nv + t);
  }
}

// Sum of the S per-segment partials part[(c S + j) K + k] in a fixed order.
template <int K>
__device__ __forceinline__ void fold_sums(const float* __restrict__ part, const Geo& g, int c, float (&v)[K],
                                          float* lds) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.f;
  for (int j = threadIdx.x; j < g.S; j += BLOCK) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += part[((int64_t)c * g.S + j) * K + k];
  }
  block_reduce<K>(v, Sum{}, lds);
}

// ---------------------------------------------------------------- forward
// part (C, S, 2): per-segment mean and M2, each from two passes over the segment (the second hits L2).
template <class T>
__global__ __launch_bounds__(BLOCK) void stats_kernel(const T* __restrict__ x, Geo g, float* __restrict__ part) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  float v[1] = {0.f};
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) v[0] += xv[k];
  });
  block_reduce<1>(v, Sum{}, lds);
  const float cnt = seg_count(g, s);
  const float mean = cnt > 0.f ? v[0] / cnt : 0.f;
  float q[1] = {0.f};
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) { const float d = xv[k] - mean; q[0] += d * d; }
  });
  block_reduce<1>(q, Sum{}, lds);
  if (threadIdx.x == 0) {
    part[((int64_t)c * g.S + s) * 2] = mean;
    part[((int64_t)c * g.S + s) * 2 + 1] = q[0];
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void fwd_apply_kernel(
    const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, Geo g,
    const float* __restrict__ part, float eps, float momentum, float slope, T* __restrict__ z,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ run_mean,
    float* __restrict__ run_var) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  float a[3] = {0.f, 0.f, 0.f};
  for (int j = threadIdx.x; j < g.S; j += BLOCK) {
    const float b[3] = {seg_count(g, j), part[((int64_t)c * g.S + j) * 2], part[((int64_t)c * g.S + j) * 2 + 1]};
    Chan{}(a, b);
  }
  block_reduce<3>(a, Chan{}, lds);
  const float n = a[0], mu = a[1], var = a[2] / n;
  const float r = rsqrtf(var + eps);
  const float scale = gamma[c] * r, shift = beta[c] - mu * scale;
  if (s == 0 && threadIdx.x == 0) {
    mean_out[c] = mu;
    rstd_out[c] = r;
    if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
    if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (a[2] / (n - 1.f));
  }
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float y = fmaf(xv[k], scale, shift);
      xv[k] = y > 0.f ? y : slope * y;
    }
    st<W>(z + off, xv);
  });
}

// Per-channel constants of the backward kernels.
struct Chn {
  float mu, r, scale, shift;
};

__device__ __forceinline__ Chn chn(const float* gamma, const float* beta, const float* mean, const float* rstd, int c) {
  Chn h;
  h.mu = mean[c]; h.r = rstd[c];
  h.scale = gamma[c] * h.r;
  h.shift = beta[c] - h.mu * h.scale;
  return h;
}

// ---------------------------------------------------------------- first-order backward
// part (C, S, 2): per-segment sums of gy and gy * xh, gy = s * gz.
template <class T>
__global__ __launch_bounds__(BLOCK) void bwd_reduce_kernel(
    const T* __restrict__ gz, const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd, Geo g, float slope,
    float* __restrict__ part) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  const Chn h = chn(gamma, beta, mean, rstd, c);
  float v[2] = {0.f, 0.f};
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float gy = fmaf(xv[k], h.scale, h.shift) > 0.f ? gv[k] : slope * gv[k];
      v[0] += gy;
      v[1] += gy * ((xv[k] - h.mu) * h.r);
    }
  });
  block_reduce<2>(v, Sum{}, lds);
  if (threadIdx.x == 0) {
    part[((int64_t)c * g.S + s) * 2] = v[0];
    part[((int64_t)c * g.S + s) * 2 + 1] = v[1];
  }
}

// gx = gamma r (gy - Sgy/n - xh Sgyx/n); sums (2, C) = (Sgy, Sgyx), dbeta = Sgy, dgamma = Sgyx.
template <class T>
__global__ __launch_bounds__(BLOCK) void bwd_apply_kernel(
    const T* __restrict__ gz, const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd, Geo g, float slope,
    const float* __restrict__ part, T* __restrict__ gx, float* __restrict__ sums, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  const Chn h = chn(gamma, beta, mean, rstd, c);
  float v[2];
  fold_sums<2>(part, g, c, v, lds);
  if (s == 0 && threadIdx.x == 0) {
    sums[c] = v[0];
    sums[g.C + c] = v[1];
    if (dbeta) dbeta[c] = v[0];
    if (dgamma) dgamma[c] = v[1];
  }
  const float inv_n = 1.f / (float)((double)g.N * (double)g.HW);
  const float A = v[0] * inv_n, B = v[1] * inv_n;
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float gy = fmaf(xv[k], h.scale, h.shift) > 0.f ? gv[k] : slope * gv[k];
      const float xh = (xv[k] - h.mu) * h.r;
      xv[k] = h.scale * (gy - A - xh * B);
    }
    st<W>(gx + off, xv);
  });
}

// ---------------------------------------------------------------- double backward
// part (C, S, 3): per-segment sums of ggx, ggx * xh, ggx * gy.
template <class T>
__global__ __launch_bounds__(BLOCK) void bwd_bwd_reduce_kernel(
    const T* __restrict__ ggx, const T* __restrict__ gz, const T* __restrict__ x,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
    const float* __restrict__ rstd, Geo g, float slope, float* __restrict__ part) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  const Chn h = chn(gamma, beta, mean, rstd, c);
  float v[3] = {0.f, 0.f, 0.f};
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W], qv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
    ld<W>(ggx + off, qv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float gy = fmaf(xv[k], h.scale, h.shift) > 0.f ? gv[k] : slope * gv[k];
      v[0] += qv[k];
      v[1] += qv[k] * ((xv[k] - h.mu) * h.r);
      v[2] += qv[k] * gy;
    }
  });
  block_reduce<3>(v, Sum{}, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) part[((int64_t)c * g.S + s) * 3 + k] = v[k];
  }
}

// A = Sgy/n, B = Sgyx/n, C = Sggx/n, D = Sggxx/n, E = Sggxgy/n:
//   g_gz = s [gamma r (ggx - C - xh D) + gg_gamma xh + gg_beta]
//   g_x  = -gamma r^2 [xh (E - AC - 3BD) + B (ggx - C) + D (gy - A)] + gg_gamma r (gy - A - xh B)
//   g_gamma = n r (E - AC - BD)
template <class T>
__global__ __launch_bounds__(BLOCK) void bwd_bwd_apply_kernel(
    const T* __restrict__ ggx, const float* __restrict__ gg_gamma, const float* __restrict__ gg_beta,
    const T* __restrict__ gz, const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ sums, Geo g, float slope, const float* __restrict__ part, T* __restrict__ g_gz,
    T* __restrict__ g_x, float* __restrict__ g_gamma) {
  __shared__ float lds[WAVES * 3];
  const int s = blockIdx.x, c = blockIdx.y;
  const Chn h = chn(gamma, beta, mean, rstd, c);
  float v[3];
  fold_sums<3>(part, g, c, v, lds);
  const float n = (float)((double)g.N * (double)g.HW), inv_n = 1.f / n;
  const float A = sums[c] * inv_n, B = sums[g.C + c] * inv_n;
  const float Cc = v[0] * inv_n, D = v[1] * inv_n, E = v[2] * inv_n;
  const float ggg = gg_gamma ? gg_gamma[c] : 0.f, ggb = gg_beta ? gg_beta[c] : 0.f;
  if (s == 0 && threadIdx.x == 0 && g_gamma) g_gamma[c] = n * h.r * (E - A * Cc - B * D);
  const float k1 = E - A * Cc - 3.f * B * D;       // coefficient of xh in g_x's bracket
  const float gr2 = h.scale * h.r;                  // gamma r^2
  const float gr = ggg * h.r;
  seg_walk<T>(g, c, s, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W], qv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
    ld<W>(ggx + off, qv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const bool pos = fmaf(xv[k], h.scale, h.shift) > 0.f;
      const float gy = pos ? gv[k] : slope * gv[k];
      const float xh = (xv[k] - h.mu) * h.r;
      const float q = qv[k] - Cc;
      const float t = h.scale * (q - xh * D) + ggg * xh + ggb;
      gv[k] = pos ? t : slope * t;
      xv[k] = gr * (gy - A - xh * B) - gr2 * (xh * k1 + B * q + D * (gy - A));
    }
    st<W>(g_gz + off, gv);
    st<W>(g_x + off, xv);
  });
}

}  // namespace amk_bn

using namespace amk_bn;

#define AMK_BN_SHAPE(what)                                                                       \
  AMK_CHECK_ARG(N > 0 && C > 0 && HW > 0, what ": non-positive size");                           \
  AMK_CHECK_SUPPORTED(C <= 65535 && (int64_t)N * HW <= ((int64_t)1 << 31),                       \
                      what ": shape N %d C %d HW %lld not supported", N, C, (long long)HW)

template <class T>
static void launch_fwd(const T* x, const float* gamma, const float* beta, int N, int C, int64_t HW, float eps,
                       float momentum, float slope, T* z, float* mean, float* rstd, float* running_mean,
                       float* running_var, float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, Vec<T>::W);
  const dim3 grid(g.S, C), block(BLOCK);
  hipLaunchKernelGGL(stats_kernel<T>, grid, block, 0, st, x, g, ws);
  hipLaunchKernelGGL(fwd_apply_kernel<T>, grid, block, 0, st, x, gamma, beta, g, ws, eps, momentum, slope, z, mean,
                     rstd, running_mean, running_var);
}

template <class T>
static void launch_bwd(const T* gz, const T* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int N, int C, int64_t HW, float slope, T* gx, float* sums, float* dgamma,
                       float* dbeta, float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, Vec<T>::W);
  const dim3 grid(g.S, C), block(BLOCK);
  hipLaunchKernelGGL(bwd_reduce_kernel<T>, grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, slope, ws);
  hipLaunchKernelGGL(bwd_apply_kernel<T>, grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, slope, ws, gx, sums,
                     dgamma, dbeta);
}

template <class T>
static void launch_bwd_bwd(const T* ggx, const float* gg_gamma, const float* gg_beta, const T* gz, const T* x,
                           const float* gamma, const float* beta, const float* mean, const float* rstd,
                           const float* sums, int N, int C, int64_t HW, float slope, T* g_gz, T* g_x, float* g_gamma,
                           float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, Vec<T>::W);
  const dim3 grid(g.S, C), block(BLOCK);
  hipLaunchKernelGGL(bwd_bwd_reduce_kernel<T>, grid, block, 0, st, ggx, gz, x, gamma, beta, mean, rstd, g, slope, ws);
  hipLaunchKernelGGL(bwd_bwd_apply_kernel<T>, grid, block, 0, st, ggx, gg_gamma, gg_beta, gz, x, gamma, beta, mean,
                     rstd, sums, g, slope, ws, g_gz, g_x, g_gamma);
}

extern "C" int64_t amk_bnact_ws_floats(int N, int C, int64_t HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (int64_t)C * make_geo(N, C, HW).S * 3;   // S does not depend on the element type
}

extern "C" int amk_bnact_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int64_t HW,
                             float eps, float momentum, float slope, float* z, float* mean, float* rstd,
                             float* running_mean, float* running_var, float* ws, void* stream) {
  AMK_CHECK_ARG(x && gamma && beta && z && mean && rstd && ws, "amk_bnact_fwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_fwd");
  AMK_CHECK_ARG(N * HW > 1, "amk_bnact_fwd: a channel needs more than one value");
  AMK_CHECK_ARG(a16(x) && a16(z), "amk_bnact_fwd: x and z must be 16-byte aligned");
  launch_fwd<float>(x, gamma, beta, N, C, HW, eps, momentum, slope, z, mean, rstd, running_mean, running_var, ws,
                    static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_fwd");
  return AMK_OK;
}

extern "C" int amk_bnact_bwd(const float* gz, const float* x, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, int N, int C, int64_t HW, float slope, float* gx,
                             float* sums, float* dgamma, float* dbeta, float* ws, void* stream) {
  AMK_CHECK_ARG(gz && x && gamma && beta && mean && rstd && gx && sums && ws, "amk_bnact_bwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_bwd");
  AMK_CHECK_ARG(a16(gz) && a16(x) && a16(gx), "amk_bnact_bwd: gz, x and gx must be 16-byte aligned");
  launch_bwd<float>(gz, x, gamma, beta, mean, rstd, N, C, HW, slope, gx, sums, dgamma, dbeta, ws,
                    static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_bwd");
  return AMK_OK;
}

extern "C" int amk_bnact_bwd_bwd(const float* ggx, const float* gg_gamma, const float* gg_beta, const float* gz,
                                 const float* x, const float* gamma, const float* beta, const float* mean,
                                 const float* rstd, const float* sums, int N, int C, int64_t HW, float slope,
                                 float* g_gz, float* g_x, float* g_gamma, float* ws, void* stream) {
  AMK_CHECK_ARG(ggx && gz && x && gamma && beta && mean && rstd && sums && g_gz && g_x && ws,
                "amk_bnact_bwd_bwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_bwd_bwd");
  AMK_CHECK_ARG(a16(ggx) && a16(gz) && a16(x) && a16(g_gz) && a16(g_x),
                "amk_bnact_bwd_bwd: ggx, gz, x, g_gz and g_x must be 16-byte aligned");
  launch_bwd_bwd<float>(ggx, gg_gamma, gg_beta, gz, x, gamma, beta, mean, rstd, sums, N, C, HW, slope, g_gz, g_x,
                        g_gamma, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_bwd_bwd");
  return AMK_OK;
}

// ---------------------------------------------------------------- bf16 x, z, gz, gx, ggx, g_gz, g_x
static const __bf16* cb(const void* p) { return static_cast<const __bf16*>(p); }
static __bf16* mb(void* p) { return static_cast<__bf16*>(p); }

extern "C" int amk_bnact_bf16_fwd(const void* x, const float* gamma, const float* beta, int N, int C, int64_t HW,
                                  float eps, float momentum, float slope, void* z, float* mean, float* rstd,
                                  float* running_mean, float* running_var, float* ws, void* stream) {
  AMK_CHECK_ARG(x && gamma && beta && z && mean && rstd && ws, "amk_bnact_bf16_fwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_bf16_fwd");
  AMK_CHECK_ARG(N * HW > 1, "amk_bnact_bf16_fwd: a channel needs more than one value");
  AMK_CHECK_ARG(a16(x) && a16(z), "amk_bnact_bf16_fwd: x and z must be 16-byte aligned");
  launch_fwd<__bf16>(cb(x), gamma, beta, N, C, HW, eps, momentum, slope, mb(z), mean, rstd, running_mean, running_var,
                     ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_bf16_fwd");
  return AMK_OK;
}

extern "C" int amk_bnact_bf16_bwd(const void* gz, const void* x, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, int N, int C, int64_t HW, float slope,
                                  void* gx, float* sums, float* dgamma, float* dbeta, float* ws, void* stream) {
  AMK_CHECK_ARG(gz && x && gamma && beta && mean && rstd && gx && sums && ws, "amk_bnact_bf16_bwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_bf16_bwd");
  AMK_CHECK_ARG(a16(gz) && a16(x) && a16(gx), "amk_bnact_bf16_bwd: gz, x and gx must be 16-byte aligned");
  launch_bwd<__bf16>(cb(gz), cb(x), gamma, beta, mean, rstd, N, C, HW, slope, mb(gx), sums, dgamma, dbeta, ws,
                     static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_bf16_bwd");
  return AMK_OK;
}

extern "C" int amk_bnact_bf16_bwd_bwd(const void* ggx, const float* gg_gamma, const float* gg_beta, const void* gz,
                                      const void* x, const float* gamma, const float* beta, const float* mean,
                                      const float* rstd, const float* sums, int N, int C, int64_t HW, float slope,
                                      void* g_gz, void* g_x, float* g_gamma, float* ws, void* stream) {
  AMK_CHECK_ARG(ggx && gz && x && gamma && beta && mean && rstd && sums && g_gz && g_x && ws,
                "amk_bnact_bf16_bwd_bwd: null pointer");
  AMK_BN_SHAPE("amk_bnact_bf16_bwd_bwd");
  AMK_CHECK_ARG(a16(ggx) && a16(gz) && a16(x) && a16(g_gz) && a16(g_x),
                "amk_bnact_bf16_bwd_bwd: ggx, gz, x, g_gz and g_x must be 16-byte aligned");
  launch_bwd_bwd<__bf16>(cb(ggx), gg_gamma, gg_beta, cb(gz), cb(x), gamma, beta, mean, rstd, sums, N, C, HW, slope,
                         mb(g_gz), mb(g_x), g_gamma, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_bnact_bf16_bwd_bwd");
  return AMK_OK;
}
