// GroupNorm(G, C, eps) + optional Swish of the conv VQGAN, NCHW, for gfx950: forward and backward, for f32 tensors and,
// under bf16 autocast, for bf16 x, z, gz and gx (amk_gnact_bf16_*).
//
// ATen runs the pair as a normalisation kernel plus two element-wise passes and keeps the normalised tensor for the
// backward.  Here the forward is two launches (per-segment statistics, then fold + apply) and the backward three
// (per-plane partial sums, fold + apply, and a small fold of the parameter gradients over the batch); y and sigma are
// recomputed from x, mean and rstd.  No float atomics: every output is bitwise reproducible, and a sample's result
// does not depend on the batch it sits in.
//
// Notation, per run (n, g) of m = cpg HW contiguous floats (cpg = C / G channels): mu, var biased statistics,
// r = (var + eps)^-1/2, xh = (x - mu) r, y = gamma_c xh + beta_c, z = act(y); act 0 = identity, act 1 = y sigma(y).
//
// Work split: a run is cpg planes (channels) of HW floats.  It is cut into S segments -- PP whole planes each, or for
// planes larger than SEG, Q pieces of one plane -- and workgroup run * S + s owns segment s of its run in every
// kernel.  A plane starts at element (n C + c) HW, 16-byte aligned only when that is a multiple of 4: each plane is
// walked as a scalar head, an aligned float4 body and a scalar tail.
//
// bf16: every kernel is a template on the element type T of x, z, gz and gx.  T = __bf16 reads 8 elements per 16-byte
// access (head and tail of up to 7 elements; a plane is aligned only when (n C + c) HW is a multiple of 8; pieces are
// multiples of 8), widens them to f32 on the load and rounds z and gx to bf16 once, to nearest even, on the store.
// Everything between is the f32 arithmetic of T = float: statistics, y, sigma, the partial sums, mean, rstd, dgamma and
// dbeta are f32, as are gamma and beta.  SEG stays 4096 elements (8 KiB of bf16): the small layers of the model
// (512 x 16^2, 256 x 32^2) are one or two segments per run, latency-bound at one workgroup per CU, and halving their
// workgroups to keep 16 KiB per segment would halve what hides that latency; at the large layers either choice fills the
// device many times over.
#include "amk_planes.h"

namespace amk_gn {

using namespace amk_planes;  // BLOCK, WAVES, Width, Vec, ld, st, Sum, Chan, block_reduce
constexpr int64_t SEG = 4096;  // target elements per workgroup segment

struct Geo {
  int N, C, G, cpg;
  int64_t HW;
  int PP;     // whole planes per segment (Q == 1)
  int Q;      // pieces per plane (PP == 1)
  int64_t L;  // elements per piece (Q > 1)
  int S;      // segments per run
};

// VW: elements per 16-byte access (4 for f32, 8 for bf16); pieces are multiples of it.
static Geo make_geo(int N, int C, int64_t HW, int G, int VW = 4) {
  Geo g;
  g.N = N; g.C = C; g.G = G; g.cpg = C / G; g.HW = HW;
  if (HW <= SEG) {
    g.PP = (int)(SEG / HW);
    if (g.PP > g.cpg) g.PP = g.cpg;
    g.Q = 1; g.L = HW;
    g.S = (g.cpg + g.PP - 1) / g.PP;
  } else {
    g.PP = 1;
    g.Q = (int)((HW + SEG - 1) / SEG);
    g.L = (((HW + g.Q - 1) / g.Q) + (VW - 1)) & ~(int64_t)(VW - 1);
    g.S = g.cpg * g.Q;
  }
  return g;
}

struct Seg {
  int p0, p1;       // planes of the run
  int q;            // piece of the plane (0 when Q == 1)
  int64_t e0, e1;   // elements of each plane
};

__device__ __forceinline__ Seg seg_of(const Geo& g, int s) {
  Seg r;
  if (g.Q == 1) {
    r.p0 = s * g.PP; r.p1 = min(g.cpg, r.p0 + g.PP);
    r.q = 0; r.e0 = 0; r.e1 = g.HW;
  } else {
    r.p0 = s / g.Q; r.p1 = r.p0 + 1;
    r.q = s % g.Q;
    r.e0 = min(g.HW, (int64_t)r.q * g.L);
    r.e1 = min(g.HW, r.e0 + g.L);
  }
  return r;
}

__device__ __forceinline__ float seg_count(const Geo& g, int s) {
  const Seg r = seg_of(g, s);
  return (float)((int64_t)(r.p1 - r.p0) * (r.e1 - r.e0));
}

// For every plane p of segment s of `run`: pre(p), then f(Width<VW>, off) for every aligned VW-element run (VW = 4 for
// f32, 8 for bf16) and f(Width<1>, off) for every edge element, then post(p, piece); `off` indexes the (N, C, HW) tensor
// of T, whose base is 16-byte aligned.  The loops' bounds are uniform over the workgroup, so pre and post may synchronise.
template <class T, class Pre, class F, class Post>
__device__ __forceinline__ void seg_walk(const Geo& g, int run, int s, Pre&& pre, F&& f, Post&& post) {
  const Seg r = seg_of(g, s);
  const int64_t len = r.e1 - r.e0;
  const int t = threadIdx.x;
  for (int p = r.p0; p < r.p1; ++p) {
    pre(p);
    const int64_t base = ((int64_t)run * g.cpg + p) * g.HW + r.e0;
    constexpr int VW = Vec<T>::W;
    const int head = (int)min((int64_t)((VW - (base & (VW - 1))) & (VW - 1)), len);
    const int64_t nv = (len - head) >> Vec<T>::SH;
    const int tail = (int)(len - head - VW * nv);
    for (int64_t i = t; i < nv; i += BLOCK) f(Width<VW>{}, base + head + VW * i);
    if (t < head) f(Width<1>{}, base + t);
    else if (t < head + tail) f(Width<1>{}, base + VW * nv + t);
    post(p, r.q);
  }
}

struct Nop {
  __device__ __forceinline__ void operator()(int) const {}
  __device__ __forceinline__ void operator()(int, int) const {}
};

// sigma(y) = 1 / (1 + e^-y) on v_exp_f32 and v_rcp_f32 (1 ulp each).  y -> -inf: e = +inf, rcp(inf) = 0;
// y -> +inf: e = 0, sigma = 1.  e is used nowhere else, so no inf * 0 can arise.
__device__ __forceinline__ float sigmoid(float y) {
  const float e = __builtin_amdgcn_exp2f(-y * AMK_LOG2E);
  return __builtin_amdgcn_rcpf(1.f + e);
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float y) {
  if constexpr (ACT == 1) return y * sigmoid(y);
  else return y;
}

// d act / d y; swish' = sigma (1 + y (1 - sigma)): at y = -200 it is 0 * -199, at y = 200 it is 1 * (1 + 200 * 0).
template <int ACT>
__device__ __forceinline__ float act_grad(float y) {
  if constexpr (ACT == 1) {
    const float sg = sigmoid(y);
    return sg * (1.f + y * (1.f - sg));
  } else {
    return 1.f;
  }
}

// ---------------------------------------------------------------- forward
// part (N G, S, 2): per-segment mean and M2, each from two passes over the segment (the second hits L2).
template <class T>
__global__ __launch_bounds__(BLOCK) void stats_kernel(const T* __restrict__ x, Geo g, float* __restrict__ part) {
  __shared__ float lds[WAVES * 3];
  const int run = blockIdx.x / g.S, s = blockIdx.x % g.S;
  float v[1] = {0.f};
  seg_walk<T>(g, run, s, Nop{}, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) v[0] += xv[k];
  }, Nop{});
  block_reduce<1>(v, Sum{}, lds);
  const float cnt = seg_count(g, s);
  const float mean = cnt > 0.f ? v[0] / cnt : 0.f;
  float q[1] = {0.f};
  seg_walk<T>(g, run, s, Nop{}, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) { const float d = xv[k] - mean; q[0] += d * d; }
  }, Nop{});
  block_reduce<1>(q, Sum{}, lds);
  if (threadIdx.x == 0) {
    part[(int64_t)blockIdx.x * 2] = mean;
    part[(int64_t)blockIdx.x * 2 + 1] = q[0];
  }
}

template <class T, int ACT>
__global__ __launch_bounds__(BLOCK) void fwd_apply_kernel(
    const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, Geo g,
    const float* __restrict__ part, float eps, T* __restrict__ z, float* __restrict__ mean_out,
    float* __restrict__ rstd_out) {
  __shared__ float lds[WAVES * 3];
  const int run = blockIdx.x / g.S, s = blockIdx.x % g.S;
  const int c0 = (run % g.G) * g.cpg;
  float a[3] = {0.f, 0.f, 0.f};
  for (int j = threadIdx.x; j < g.S; j += BLOCK) {
    const int64_t i = ((int64_t)run * g.S + j) * 2;
    const float b[3] = {seg_count(g, j), part[i], part[i + 1]};
    Chan{}(a, b);
  }
  block_reduce<3>(a, Chan{}, lds);
  const float mu = a[1], var = a[2] / a[0];
  const float r = rsqrtf(var + eps);
  if (s == 0 && threadIdx.x == 0) {
    mean_out[run] = mu;
    rstd_out[run] = r;
  }
  float scale = 0.f, shift = 0.f;
  seg_walk<T>(g, run, s, [&](int p) {
    scale = gamma[c0 + p] * r;
    shift = beta[c0 + p] - mu * scale;
  }, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W];
    ld<W>(x + off, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) xv[k] = act_fwd<ACT>(fmaf(xv[k], scale, shift));
    st<W>(z + off, xv);
  }, Nop{});
}

// ---------------------------------------------------------------- backward
// part (N C, Q, 2): per-(n, channel, piece) sums of gy and gy * xh, gy = gz act'(y).
template <class T, int ACT>
__global__ __launch_bounds__(BLOCK) void bwd_reduce_kernel(
    const T* __restrict__ gz, const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd, Geo g,
    float* __restrict__ part) {
  __shared__ float lds[WAVES * 3];
  const int run = blockIdx.x / g.S, s = blockIdx.x % g.S;
  const int c0 = (run % g.G) * g.cpg;
  const float mu = mean[run], r = rstd[run];
  float scale = 0.f, shift = 0.f;
  float v[2];
  seg_walk<T>(g, run, s, [&](int p) {
    scale = gamma[c0 + p] * r;
    shift = beta[c0 + p] - mu * scale;
    v[0] = 0.f; v[1] = 0.f;
  }, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float gy = gv[k] * act_grad<ACT>(fmaf(xv[k], scale, shift));
      v[0] += gy;
      v[1] += gy * ((xv[k] - mu) * r);
    }
  }, [&](int p, int q) {
    block_reduce<2>(v, Sum{}, lds);
    if (threadIdx.x == 0) {
      const int64_t i = (((int64_t)run * g.cpg + p) * g.Q + q) * 2;
      part[i] = v[0];
      part[i + 1] = v[1];
    }
  });
}

// gx = r (gamma_c gy - S1/m - xh S2/m), S1 = sum gamma_c gy and S2 = sum gamma_c gy xh over the run, folded from the
// run's cpg Q partials in a fixed order.
template <class T, int ACT>
__global__ __launch_bounds__(BLOCK) void bwd_apply_kernel(
    const T* __restrict__ gz, const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd, Geo g,
    const float* __restrict__ part, T* __restrict__ gx) {
  __shared__ float lds[WAVES * 3];
  const int run = blockIdx.x / g.S, s = blockIdx.x % g.S;
  const int c0 = (run % g.G) * g.cpg;
  const float mu = mean[run], r = rstd[run];
  float v[2] = {0.f, 0.f};
  for (int j = threadIdx.x; j < g.cpg * g.Q; j += BLOCK) {
    const float gm = gamma[c0 + j / g.Q];
    const int64_t i = ((int64_t)run * g.cpg * g.Q + j) * 2;
    v[0] += gm * part[i];
    v[1] += gm * part[i + 1];
  }
  block_reduce<2>(v, Sum{}, lds);
  const float inv_m = 1.f / (float)((double)g.cpg * (double)g.HW);
  const float A = v[0] * inv_m, B = v[1] * inv_m;
  float gm = 0.f, scale = 0.f, shift = 0.f;
  seg_walk<T>(g, run, s, [&](int p) {
    gm = gamma[c0 + p];
    scale = gm * r;
    shift = beta[c0 + p] - mu * scale;
  }, [&](auto w, int64_t off) {
    constexpr int W = decltype(w)::value;
    float xv[W], gv[W];
    ld<W>(x + off, xv);
    ld<W>(gz + off, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float gy = gv[k] * act_grad<ACT>(fmaf(xv[k], scale, shift));
      const float xh = (xv[k] - mu) * r;
      xv[k] = r * (gm * gy - A - xh * B);
    }
    st<W>(gx + off, xv);
  }, Nop{});
}

// dbeta_c = sum over (n, piece) of the gy partials, dgamma_c of the gy xh partials, in a fixed order; workgroup c.
__global__ __launch_bounds__(BLOCK) void param_grad_kernel(const float* __restrict__ part, Geo g,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float lds[WAVES * 3];
  const int c = blockIdx.x;
  float v[2] = {0.f, 0.f};
  for (int j = threadIdx.x; j < g.N * g.Q; j += BLOCK) {
    const int64_t i = (((int64_t)(j / g.Q) * g.C + c) * g.Q + j % g.Q) * 2;
    v[0] += part[i];
    v[1] += part[i + 1];
  }
  block_reduce<2>(v, Sum{}, lds);
  if (threadIdx.x == 0) {
    dbeta[c] = v[0];
    dgamma[c] = v[1];
  }
}

}  // namespace amk_gn

using namespace amk_gn;

// The launch grid is N G S workgroups, one dimension.
static int64_t grid_of(int N, int C, int64_t HW, int G, int VW = 4) {
  const Geo g = make_geo(N, C, HW, G, VW);
  return (int64_t)N * G * g.S;
}

#define AMK_GN_SHAPE(what, VW)                                                                      \
  AMK_CHECK_ARG(N > 0 && C > 0 && HW > 0 && G > 0, what ": non-positive size");                     \
  AMK_CHECK_ARG(act == 0 || act == 1, what ": act must be 0 (identity) or 1 (swish), got %d", act); \
  AMK_CHECK_SUPPORTED(C % G == 0, what ": G %d does not divide C %d", G, C);                        \
  AMK_CHECK_SUPPORTED(grid_of(N, C, HW, G, VW) < ((int64_t)1 << 31),                                \
                      what ": shape N %d C %d HW %lld G %d needs a grid beyond 2^31", N, C, (long long)HW, G)

template <class T>
static void launch_fwd(const T* x, const float* gamma, const float* beta, int N, int C, int64_t HW, int G, float eps,
                       int act, T* z, float* mean, float* rstd, float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, G, Vec<T>::W);
  const dim3 grid((unsigned)grid_of(N, C, HW, G, Vec<T>::W)), block(BLOCK);
  hipLaunchKernelGGL(stats_kernel<T>, grid, block, 0, st, x, g, ws);
  if (act == 1)
    hipLaunchKernelGGL((fwd_apply_kernel<T, 1>), grid, block, 0, st, x, gamma, beta, g, ws, eps, z, mean, rstd);
  else
    hipLaunchKernelGGL((fwd_apply_kernel<T, 0>), grid, block, 0, st, x, gamma, beta, g, ws, eps, z, mean, rstd);
}

template <class T>
static void launch_bwd(const T* gz, const T* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, int N, int C, int64_t HW, int G, int act, T* gx, float* dgamma, float* dbeta,
                       float* ws, hipStream_t st) {
  const Geo g = make_geo(N, C, HW, G, Vec<T>::W);
  const dim3 grid((unsigned)grid_of(N, C, HW, G, Vec<T>::W)), block(BLOCK);
  if (act == 1) {
    hipLaunchKernelGGL((bwd_reduce_kernel<T, 1>), grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, ws);
    hipLaunchKernelGGL((bwd_apply_kernel<T, 1>), grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, ws, gx);
  } else {
    hipLaunchKernelGGL((bwd_reduce_kernel<T, 0>), grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, ws);
    hipLaunchKernelGGL((bwd_apply_kernel<T, 0>), grid, block, 0, st, gz, x, gamma, beta, mean, rstd, g, ws, gx);
  }
  hipLaunchKernelGGL(param_grad_kernel, dim3(C), block, 0, st, ws, g, dgamma, dbeta);
}

extern "C" int64_t amk_gnact_ws_floats(int N, int C, int64_t HW, int G) {
  if (N <= 0 || C <= 0 || HW <= 0 || G <= 0 || C % G != 0) return 0;
  // forward: N G S pairs; backward: N C Q pairs, and S <= cpg Q
  return (int64_t)N * C * make_geo(N, C, HW, G).Q * 2;
}

extern "C" int amk_gnact_fwd(const float* x, const float* gamma, const float* beta, int N, int C, int64_t HW, int G,
                             float eps, int act, float* z, float* mean, float* rstd, float* ws, void* stream) {
  AMK_CHECK_ARG(x && gamma && beta && z && mean && rstd && ws, "amk_gnact_fwd: null pointer");
  AMK_GN_SHAPE("amk_gnact_fwd", 4);
  AMK_CHECK_ARG(a16(x) && a16(z), "amk_gnact_fwd: x and z must be 16-byte aligned");
  launch_fwd<float>(x, gamma, beta, N, C, HW, G, eps, act, z, mean, rstd, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_gnact_fwd");
  return AMK_OK;
}

extern "C" int amk_gnact_bwd(const float* gz, const float* x, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, int N, int C, int64_t HW, int G, int act,
                             float* gx, float* dgamma, float* dbeta, float* ws, void* stream) {
  AMK_CHECK_ARG(gz && x && gamma && beta && mean && rstd && gx && dgamma && dbeta && ws,
                "amk_gnact_bwd: null pointer");
  AMK_GN_SHAPE("amk_gnact_bwd", 4);
  AMK_CHECK_ARG(a16(gz) && a16(x) && a16(gx), "amk_gnact_bwd: gz, x and gx must be 16-byte aligned");
  launch_bwd<float>(gz, x, gamma, beta, mean, rstd, N, C, HW, G, act, gx, dgamma, dbeta, ws,
                    static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_gnact_bwd");
  return AMK_OK;
}

// ---------------------------------------------------------------- bf16 x, z, gz, gx
extern "C" int64_t amk_gnact_bf16_ws_floats(int N, int C, int64_t HW, int G) {
  if (N <= 0 || C <= 0 || HW <= 0 || G <= 0 || C % G != 0) return 0;
  return (int64_t)N * C * make_geo(N, C, HW, G, 8).Q * 2;
}

extern "C" int amk_gnact_bf16_fwd(const void* x, const float* gamma, const float* beta, int N, int C, int64_t HW, int G,
                                  float eps, int act, void* z, float* mean, float* rstd, float* ws, void* stream) {
  AMK_CHECK_ARG(x && gamma && beta && z && mean && rstd && ws, "amk_gnact_bf16_fwd: null pointer");
  AMK_GN_SHAPE("amk_gnact_bf16_fwd", 8);
  AMK_CHECK_ARG(a16(x) && a16(z), "amk_gnact_bf16_fwd: x and z must be 16-byte aligned");
  launch_fwd<__bf16>(static_cast<const __bf16*>(x), gamma, beta, N, C, HW, G, eps, act, static_cast<__bf16*>(z), mean,
                     rstd, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_gnact_bf16_fwd");
  return AMK_OK;
}

extern "C" int amk_gnact_bf16_bwd(const void* gz, const void* x, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, int N, int C, int64_t HW, int G, int act,
                                  void* gx, float* dgamma, float* dbeta, float* ws, void* stream) {
  AMK_CHECK_ARG(gz && x && gamma && beta && mean && rstd && gx && dgamma && dbeta && ws,
                "amk_gnact_bf16_bwd: null pointer");
  AMK_GN_SHAPE("amk_gnact_bf16_bwd", 8);
  AMK_CHECK_ARG(a16(gz) && a16(x) && a16(gx), "amk_gnact_bf16_bwd: gz, x and gx must be 16-byte aligned");
  launch_bwd<__bf16>(static_cast<const __bf16*>(gz), static_cast<const __bf16*>(x), gamma, beta, mean, rstd, N, C, HW,
                     G, act, static_cast<__bf16*>(gx), dgamma, dbeta, ws, static_cast<hipStream_t>(stream));
  AMK_CHECK_LAUNCH("amk_gnact_bf16_bwd");
  return AMK_OK;
}
