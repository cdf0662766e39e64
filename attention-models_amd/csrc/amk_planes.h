// Helpers of the kernels that walk NCHW planes in 16-byte accesses with 256-thread workgroups (discr_norm.hip,
// gn_act.hip, lpips.hip): element loads and stores of f32 and bf16 tensors by access width, and fixed-order reductions
// over a workgroup.  Each file pulls them into its own namespace with `using namespace amk_planes;`.
#pragma once
#include "amk_bf16.h"

namespace amk_planes {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;

template <int W> struct Width { static constexpr int value = W; };

// elements per 16-byte access and its log2
template <class T> struct Vec { static constexpr int W = 4, SH = 2; };
template <> struct Vec<__bf16> { static constexpr int W = 8, SH = 3; };

// W elements at p into f32 registers.  f32: one element, one 16-byte access, or two (W == 8: the f32 companions of a
// bf16 thread's 8 elements).  bf16: one element or one 16-byte access, widened on the load.
template <int W>
__device__ __forceinline__ void ld(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (W == 8) {
    const float4 t = *reinterpret_cast<const float4*>(p), u = *reinterpret_cast<const float4*>(p + 4);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    v[4] = u.x; v[5] = u.y; v[6] = u.z; v[7] = u.w;
  } else {
    static_assert(W == 1);
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void st(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (W == 8) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    static_assert(W == 1);
    *p = v[0];
  }
}

template <int W>
__device__ __forceinline__ void ld(const __bf16* p, float (&v)[W]) {
  if constexpr (W == 8) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)t[k];
  } else {
    static_assert(W == 1);
    v[0] = (float)*p;
  }
}

// the one rounding of a bf16 output: f32 -> bf16, to nearest even
template <int W>
__device__ __forceinline__ void st(__bf16* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    bf16x8 t;
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = (__bf16)v[k];
    *reinterpret_cast<bf16x8*>(p) = t;
  } else {
    static_assert(W == 1);
    *p = (__bf16)v[0];
  }
}

struct Sum {
  template <int K>
  __device__ __forceinline__ void operator()(float (&a)[K], const float (&b)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] += b[k];
  }
};

// Chan's merge of (count, mean, M2) triples
struct Chan {
  __device__ __forceinline__ void operator()(float (&a)[3], const float (&b)[3]) const {
    const float n = a[0] + b[0];
    if (b[0] == 0.f) return;
    if (a[0] == 0.f) { a[0] = b[0]; a[1] = b[1]; a[2] = b[2]; return; }
    const float d = b[1] - a[1], f = b[0] / n;
    a[1] += d * f;
    a[2] += b[2] + d * d * a[0] * f;
    a[0] = n;
  }
};

// Fixed-order block reduction: a butterfly inside each wave (lane 0's result is used), then every thread folds the
// WAVES wave results in order, so all threads return the same value.  lds: WAVES * K floats.
template <int K, class Op>
__device__ __forceinline__ void block_reduce(float (&v)[K], Op op, float* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = __shfl_xor(v[k], o, 64);
    op(v, w);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = lds[k];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    float u[K];
#pragma unroll
    for (int k = 0; k < K; ++k) u[k] = lds[w * K + k];
    op(v, u);
  }
  __syncthreads();
}

}  // namespace amk_planes
