// Shared device/host helpers for the libamk.so kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/amk.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define AMK_WAVE 64
#define AMK_LOG2E 1.4426950408889634f
#define AMK_LN2 0.6931471805599453f

// ---- host side -----------------------------------------------------------
void amk_set_error(const char* fmt, ...);

#define AMK_CHECK_ARG(cond, ...)        \
  do {                                  \
    if (!(cond)) {                      \
      amk_set_error(__VA_ARGS__);       \
      return AMK_EINVAL;                \
    }                                   \
  } while (0)

#define AMK_CHECK_SUPPORTED(cond, ...)  \
  do {                                  \
    if (!(cond)) {                      \
      amk_set_error(__VA_ARGS__);       \
      return AMK_EUNSUPPORTED;          \
    }                                   \
  } while (0)

#define AMK_CHECK_LAUNCH(what)                                              \
  do {                                                                      \
    hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) {                                                 \
      amk_set_error("%s: %s", what, hipGetErrorString(e_));                 \
      return AMK_ELAUNCH;                                                   \
    }                                                                       \
  } while (0)

// what the float4 paths ask of a pointer
static inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the shift that divides by d when d is a power of two, else -1 (the kernels then divide)
static inline int log2_of(int d) {
  int s = 0;
  while ((1 << s) < d) ++s;
  return (1 << s) == d ? s : -1;
}

// Opt-in of KERNEL to `bytes` of dynamic LDS (more than 64 KiB needs it) on the current device.  The attribute is per
// device, so there is one flag per (kernel, device ordinal): each device gets the HIP call once, on first use.
// false: no current device (or an ordinal past the table), or the device refused -- nothing is recorded, the next call asks again.
template <auto KERNEL>
static bool amk_lds_optin(int bytes) {
  static bool done[64] = {};
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  if (!done[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    done[dev] = true;
  }
  return true;
}

// ---- device side ---------------------------------------------------------
// v_mfma_f32_32x32x2_f32: exact-f32 matrix FMA, D(32x32) += A(32x2) * B(2x32).
//   lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31];
//   accumulator register r of lane l is D[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5)][l & 31].
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Row of accumulator register r for lane half hf (0/1) in the 32x32 C/D tile.
__device__ __forceinline__ constexpr int acc_row(int r, int hf) {
  return (r & 3) + 8 * (r >> 2) + 4 * hf;
}

// The 8 XCDs are dealt workgroups round-robin; remap so that logically
// consecutive ids (which share K/V panels or codebook tiles) land on one XCD's L2.
// Bijective for any grid size (cdna guide, section 5 "XCD swizzle must be bijective").
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

__device__ __forceinline__ float wave_xor32_max(float x) {
  return fmaxf(x, __shfl_xor(x, 32, 64));
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// element e of v, e a compile-time constant after unrolling
__device__ __forceinline__ float f4(const float4& v, int e) {
  return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w));
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Barrier that orders LDS only: global loads and stores in flight stay in flight.  __syncthreads() drains them, which
// would serialise the register prefetch of the step loops (and the row stores of a persistent kernel's epilogue).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
