// Single-token attention for KV-cached decoding: one query row per (batch, head) against a cache of keys and values,
// f32, with the cache append fused in (include/amk.h: amk_attn_decode).  Replaces, for one new row, the score / softmax /
// PV core of models/softmax_attention.py:62-76 as the sampling loop of models/parti.py:135-152 would call it on a cache.
//
// The MFMA tile kernels of this library are built for 32 or more query rows per workgroup; with one row they run one
// workgroup per (batch, head) and multiply 31 rows of padding.  One row against J keys is a read of the cache: 2 J D
// floats for 4 J D flops, memory bound.  So here:
//
//   * the keys are split into chunks of KEYS keys; a workgroup owns one (batch, head, chunk), 256 threads.  A group of
//     8 lanes owns a key: lane g of it holds dims [4 (g + 8 i), +4) for i < D / 32, so one 16-byte load per lane and i
//     reads 128 contiguous bytes of the row per group.  K and V go from global memory to VGPRs; nothing of the stream
//     is staged in LDS.  The 32 key groups of a workgroup take keys j0 + kg + 32 p, p < KEYS / 32.
//   * pass 1: the chunk's scores (q scale log2 e) . k, kept in registers (at most MAXP per lane), and their maximum M
//     over the workgroup.  pass 2: p = exp2(s - M), l += p, o += p v per lane; the 32 key groups' partial rows are
//     added in key-group order through LDS.  No running rescale: one exponent per key.
//   * one chunk (the whole key range fits): o = o / l is written directly.  More: each chunk leaves (M, l, o[D]) in the
//     workspace and a second launch on the same stream, attn_decode_combine_kernel with one workgroup per (batch,
//     head), adds the partials IN CHUNK ORDER, each scaled by exp2(M_s - max M).  No f32 atomics on data and no
//     hand-off between workgroups of one launch: the result does not depend on the batch size or on the run.  (An
//     in-launch reduction -- a ticket counter per (batch, head), the last arriver combining -- was built and measured
//     first and lost at every length: DESIGN.md section 4i, profiles/kbench_parti_sample_reductions.log.)
//   * the number of valid rows is read from DEVICE memory (n_dev), so that one captured launch serves every position:
//     the grid is sized from the capacity and a workgroup whose chunk lies beyond the valid keys leaves at once.
//   * append mode (k_new given): key n = *n_dev is the new row.  The key group that owns position n takes it from
//     k_new / v_new -- never from the cache -- and is the only writer of cache row n, so no workgroup of the launch
//     reads a row that another writes.
#include "amk_bf16.h"
#include "attn_common.h"

#include <stdlib.h>

namespace amk_decode {

constexpr int GROUP = 8;             // lanes per key
constexpr int KGROUPS = 256 / GROUP; // keys in flight per workgroup and pass
constexpr int MAXP = 4;              // passes: chunks of at most 128 keys
constexpr int MIN_KEYS = KGROUPS;    // the smallest chunk; the workspace is sized for it

struct Args {
  const float *q, *k_new, *v_new;
  float *k_cache, *v_cache, *o, *ws_ml, *ws_o;
  const int32_t* n_dev;
  const uint8_t* key_mask;
  int H, capacity, keys, nsplit;
  int64_t q_sb, q_sh, n_sb, n_sh, c_sb, c_st, c_sh, o_sb, o_sh;
  float qscale;
};

// o[d] = (sum_c f_c o_c[d]) / (sum_c f_c l_c), f_c = exp2(M_c - max M), chunks in order
__device__ __forceinline__ void combine_chunks(const float* wml, const float* wo, int active, int D, int d, float* op) {
  float Mt = -INFINITY;
  for (int t = 0; t < active; ++t) Mt = fmaxf(Mt, wml[2 * t]);
  float acc = 0.f, den = 0.f;
  for (int t = 0; t < active; ++t) {
    const float f = __builtin_amdgcn_exp2f(wml[2 * t] - Mt);
    acc = fmaf(f, wo[(int64_t)t * D + d], acc);
    den = fmaf(f, wml[2 * t + 1], den);
  }
  op[d] = acc / den;
}

template <int NV>
__global__ __launch_bounds__(256) void attn_decode_kernel(Args a) {
  constexpr int D = NV * 32;
  __shared__ __attribute__((aligned(16))) float red[KGROUPS * D + KGROUPS + 8];
  float* red_l = red + KGROUPS * D;   // 32 partial denominators
  float* red_x = red_l + KGROUPS;     // 4 wave maxima
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const bool append = a.k_new != nullptr;
  const int n = a.n_dev ? *a.n_dev : a.capacity;
  const int nk = append ? n + 1 : n;   // keys attended: rows 0 .. n in append mode, 0 .. n - 1 in read mode
  if (n < 0 || nk < 1 || nk > a.capacity) return;   // out of range: nothing is read or written
  const int active = (nk + a.keys - 1) / a.keys;
  if (s >= active) return;
  const int j0 = s * a.keys, j1 = min(j0 + a.keys, nk);
  const int tid = threadIdx.x, g = tid & (GROUP - 1), kg = tid / GROUP;

  float4 q4[NV];
  {
    const float* qp = a.q + b * a.q_sb + h * a.q_sh;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      q4[i] = *reinterpret_cast<const float4*>(qp + 4 * (g + GROUP * i));
      q4[i].x *= a.qscale; q4[i].y *= a.qscale; q4[i].z *= a.qscale; q4[i].w *= a.qscale;
    }
  }
  const int64_t cbase = b * a.c_sb + h * a.c_sh;
  const int64_t nbase = b * a.n_sb + h * a.n_sh;
  const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.capacity : nullptr;

  // ---- pass 1: scores
  float sc[MAXP];
  float mx = -INFINITY;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const int j = j0 + kg + KGROUPS * p;
    float dot = 0.f;
    if (j < j1) {
      const bool fresh = append && j == n;
      const float* kp = fresh ? a.k_new + nbase : a.k_cache + cbase + j * a.c_st;
      float4 k4[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) k4[i] = *reinterpret_cast<const float4*>(kp + 4 * (g + GROUP * i));
      if (fresh) {
        float* dst = a.k_cache + cbase + j * a.c_st;
#pragma unroll
        for (int i = 0; i < NV; ++i) *reinterpret_cast<float4*>(dst + 4 * (g + GROUP * i)) = k4[i];
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        dot = fmaf(q4[i].x, k4[i].x, dot); dot = fmaf(q4[i].y, k4[i].y, dot);
        dot = fmaf(q4[i].z, k4[i].z, dot); dot = fmaf(q4[i].w, k4[i].w, dot);
      }
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    if (j < j1) {
      if (km && km[j] == 0) dot = AMK_FILL_MASKED;   // masked_fill(~context_mask, -1e9)
      sc[p] = dot;
      mx = fmaxf(mx, dot);
    } else {
      sc[p] = -INFINITY;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if ((tid & 63) == 0) red_x[tid >> 6] = mx;
  __syncthreads();
  const float M = fmaxf(fmaxf(red_x[0], red_x[1]), fmaxf(red_x[2], red_x[3]));   // finite: the chunk has a key

  // ---- pass 2: p = exp2(s - M), l and o per key group
  float l = 0.f;
  float4 o4[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const int j = j0 + kg + KGROUPS * p;
    if (j < j1) {
      const bool fresh = append && j == n;
      const float* vp = fresh ? a.v_new + nbase : a.v_cache + cbase + j * a.c_st;
      float4 v4[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) v4[i] = *reinterpret_cast<const float4*>(vp + 4 * (g + GROUP * i));
      if (fresh) {
        float* dst = a.v_cache + cbase + j * a.c_st;
#pragma unroll
        for (int i = 0; i < NV; ++i) *reinterpret_cast<float4*>(dst + 4 * (g + GROUP * i)) = v4[i];
      }
      const float pj = __builtin_amdgcn_exp2f(sc[p] - M);
      l += pj;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        o4[i].x = fmaf(pj, v4[i].x, o4[i].x); o4[i].y = fmaf(pj, v4[i].y, o4[i].y);
        o4[i].z = fmaf(pj, v4[i].z, o4[i].z); o4[i].w = fmaf(pj, v4[i].w, o4[i].w);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) *reinterpret_cast<float4*>(red + kg * D + 4 * (g + GROUP * i)) = o4[i];
  if (g == 0) red_l[kg] = l;
  __syncthreads();

  // ---- the chunk's (l, o[d]): the 32 key groups in order; thread d owns dim d
  float od = 0.f, L = 0.f;
  if (tid < D) {
#pragma unroll 8
    for (int k = 0; k < KGROUPS; ++k) {
      od += red[k * D + tid];
      L += red_l[k];
    }
  }
  float* op = a.o + b * a.o_sb + h * a.o_sh;
  if (active == 1) {
    if (tid < D) op[tid] = od / L;
    return;
  }

  // ---- more chunks: leave the partial; attn_decode_combine_kernel, next on the stream, adds them in chunk order
  const int64_t unit = (int64_t)b * a.H + h;
  if (tid < D) a.ws_o[(unit * a.nsplit + s) * D + tid] = od;
  if (tid == 0) {
    float* wml = a.ws_ml + (unit * a.nsplit + s) * 2;
    wml[0] = M; wml[1] = L;
  }
}

// The second launch: one workgroup per (batch, head) adds the chunks' partials in chunk order.
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(Args a, int D) {
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const bool append = a.k_new != nullptr;
  const int n = a.n_dev ? *a.n_dev : a.capacity;
  const int nk = append ? n + 1 : n;
  if (n < 0 || nk < 1 || nk > a.capacity) return;
  const int active = (nk + a.keys - 1) / a.keys;
  if (active == 1) return;   // written by the chunk's own workgroup
  const int64_t unit = (int64_t)b * a.H + h;
  if (tid < D)
    combine_chunks(a.ws_ml + (unit * a.nsplit) * 2, a.ws_o + (unit * a.nsplit) * D, active, D, tid,
                   a.o + b * a.o_sb + h * a.o_sh);
}

// Keys per chunk.  64 by default (DESIGN.md section 4i has the timings at 32 / 64 / 128: 16 chunks of 64 keys at Parti's
// 1024 positions put 1024 workgroups on the 256 CUs); AMK_ATTN_DECODE_KEYS = 32 / 64 / 128 overrides it for measurements, read once.
static int keys_per_chunk() {
  static const int keys = [] {
    const char* e = getenv("AMK_ATTN_DECODE_KEYS");
    const int v = e ? atoi(e) : 0;
    return (v == 32 || v == 64 || v == 128) ? v : 64;
  }();
  return keys;
}

static inline int64_t round4(int64_t x) { return (x + 3) & ~(int64_t)3; }

static void launch_chunks(int nv, dim3 grid, hipStream_t st, const Args& a) {
  switch (nv) {
    case 1: hipLaunchKernelGGL(attn_decode_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(attn_decode_kernel<2>, grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(attn_decode_kernel<3>, grid, dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(attn_decode_kernel<4>, grid, dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL(attn_decode_kernel<5>, grid, dim3(256), 0, st, a); break;
    case 6: hipLaunchKernelGGL(attn_decode_kernel<6>, grid, dim3(256), 0, st, a); break;
    case 7: hipLaunchKernelGGL(attn_decode_kernel<7>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(attn_decode_kernel<8>, grid, dim3(256), 0, st, a); break;
  }
}

// ---- the same two launches on a bf16 cache (amk_attn_decode_bf16), for the decode under bf16 autocast.  Siblings of the
// f32 kernels above, which stay as they are.  q, k_new, v_new, the caches and o are bf16; everything between the load and
// the final store is the f32 arithmetic of the f32 kernels on values that happen to be bf16 (the conversion is exact):
// q is scaled in f32 after the conversion, scores, maxima, exp2, l and o stay f32, p is never rounded, and o is rounded
// once, to nearest even, where it is stored (the chunk kernel with one chunk, the combine kernel otherwise).
// Lane layout: a 16-byte load holds 8 elements, so lane g of a key's group holds dims [8 (g + 8 i), +8) for
// i < ceil(D / 64) and the group still reads 128 contiguous bytes per step.  At D % 64 == 32 the last step covers 32 dims:
// lanes 0-3 load, lanes 4-7 hold exact zeros for q, k and v there (no load, no store).  The new row goes to the cache as the
// 16-byte pieces it was loaded in, bitwise; chunking, workspace, n_dev and the order of every sum are those of the f32 kernels.

struct ArgsB {
  const __bf16 *q, *k_new, *v_new;
  __bf16 *k_cache, *v_cache, *o;
  float *ws_ml, *ws_o;
  const int32_t* n_dev;
  const uint8_t* key_mask;
  int H, capacity, keys, nsplit;
  int64_t q_sb, q_sh, n_sb, n_sh, c_sb, c_st, c_sh, o_sb, o_sh;
  float qscale;
};

template <int D32>
__global__ __launch_bounds__(256) void attn_decode_bf16_kernel(ArgsB a) {
  constexpr int D = D32 * 32;
  constexpr int NS = (D32 + 1) / 2;        // load steps of 64 dims
  constexpr bool HALF = (D32 & 1) != 0;    // the last step holds 32 dims: lanes 0-3 of a group
  __shared__ __attribute__((aligned(16))) float red[KGROUPS * D + KGROUPS + 8];
  float* red_l = red + KGROUPS * D;
  float* red_x = red_l + KGROUPS;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const bool append = a.k_new != nullptr;
  const int n = a.n_dev ? *a.n_dev : a.capacity;
  const int nk = append ? n + 1 : n;
  if (n < 0 || nk < 1 || nk > a.capacity) return;   // out of range: nothing is read or written
  const int active = (nk + a.keys - 1) / a.keys;
  if (s >= active) return;
  const int j0 = s * a.keys, j1 = min(j0 + a.keys, nk);
  const int tid = threadIdx.x, g = tid & (GROUP - 1), kg = tid / GROUP;
  bool on[NS];   // does this lane hold dims at step i
#pragma unroll
  for (int i = 0; i < NS; ++i) on[i] = !(HALF && i == NS - 1) || g < 4;

  float qf[NS][8];
  {
    const __bf16* qp = a.q + b * a.q_sb + h * a.q_sh;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      bf16x8 q8 = {};
      if (on[i]) q8 = *reinterpret_cast<const bf16x8*>(qp + 8 * (g + GROUP * i));
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[i][e] = (float)q8[e] * a.qscale;
    }
  }
  const int64_t cbase = b * a.c_sb + h * a.c_sh;
  const int64_t nbase = b * a.n_sb + h * a.n_sh;
  const uint8_t* km = a.key_mask ? a.key_mask + (int64_t)b * a.capacity : nullptr;

  // ---- pass 1: scores
  float sc[MAXP];
  float mx = -INFINITY;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const int j = j0 + kg + KGROUPS * p;
    float dot = 0.f;
    if (j < j1) {
      const bool fresh = append && j == n;
      const __bf16* kp = fresh ? a.k_new + nbase : a.k_cache + cbase + j * a.c_st;
      bf16x8 k8[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        k8[i] = bf16x8{};
        if (on[i]) k8[i] = *reinterpret_cast<const bf16x8*>(kp + 8 * (g + GROUP * i));
      }
      if (fresh) {
        __bf16* dst = a.k_cache + cbase + j * a.c_st;
#pragma unroll
        for (int i = 0; i < NS; ++i)
          if (on[i]) *reinterpret_cast<bf16x8*>(dst + 8 * (g + GROUP * i)) = k8[i];
      }
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) dot = fmaf(qf[i][e], (float)k8[i][e], dot);
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    if (j < j1) {
      if (km && km[j] == 0) dot = AMK_FILL_MASKED;
      sc[p] = dot;
      mx = fmaxf(mx, dot);
    } else {
      sc[p] = -INFINITY;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if ((tid & 63) == 0) red_x[tid >> 6] = mx;
  __syncthreads();
  const float M = fmaxf(fmaxf(red_x[0], red_x[1]), fmaxf(red_x[2], red_x[3]));   // finite: the chunk has a key

  // ---- pass 2: p = exp2(s - M) in f32, l and o per key group
  float l = 0.f;
  float of[NS][8];
#pragma unroll
  for (int i = 0; i < NS; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) of[i][e] = 0.f;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const int j = j0 + kg + KGROUPS * p;
    if (j < j1) {
      const bool fresh = append && j == n;
      const __bf16* vp = fresh ? a.v_new + nbase : a.v_cache + cbase + j * a.c_st;
      bf16x8 v8[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        v8[i] = bf16x8{};
        if (on[i]) v8[i] = *reinterpret_cast<const bf16x8*>(vp + 8 * (g + GROUP * i));
      }
      if (fresh) {
        __bf16* dst = a.v_cache + cbase + j * a.c_st;
#pragma unroll
        for (int i = 0; i < NS; ++i)
          if (on[i]) *reinterpret_cast<bf16x8*>(dst + 8 * (g + GROUP * i)) = v8[i];
      }
      const float pj = __builtin_amdgcn_exp2f(sc[p] - M);
      l += pj;
#pragma unroll
      for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) of[i][e] = fmaf(pj, (float)v8[i][e], of[i][e]);
    }
  }
#pragma unroll
  for (int i = 0; i < NS; ++i)
    if (on[i]) {
      float* rp = red + kg * D + 8 * (g + GROUP * i);
      *reinterpret_cast<float4*>(rp) = make_float4(of[i][0], of[i][1], of[i][2], of[i][3]);
      *reinterpret_cast<float4*>(rp + 4) = make_float4(of[i][4], of[i][5], of[i][6], of[i][7]);
    }
  if (g == 0) red_l[kg] = l;
  __syncthreads();

  // ---- the chunk's (l, o[d]): the 32 key groups in order; thread d owns dim d
  float od = 0.f, L = 0.f;
  if (tid < D) {
#pragma unroll 8
    for (int k = 0; k < KGROUPS; ++k) {
      od += red[k * D + tid];
      L += red_l[k];
    }
  }
  if (active == 1) {
    if (tid < D) a.o[b * a.o_sb + h * a.o_sh + tid] = (__bf16)(od / L);   // the one rounding, to nearest even
    return;
  }
  const int64_t unit = (int64_t)b * a.H + h;
  if (tid < D) a.ws_o[(unit * a.nsplit + s) * D + tid] = od;
  if (tid == 0) {
    float* wml = a.ws_ml + (unit * a.nsplit + s) * 2;
    wml[0] = M; wml[1] = L;
  }
}

__global__ __launch_bounds__(256) void attn_decode_bf16_combine_kernel(ArgsB a, int D) {
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const bool append = a.k_new != nullptr;
  const int n = a.n_dev ? *a.n_dev : a.capacity;
  const int nk = append ? n + 1 : n;
  if (n < 0 || nk < 1 || nk > a.capacity) return;
  const int active = (nk + a.keys - 1) / a.keys;
  if (active == 1) return;   // written by the chunk's own workgroup
  const int64_t unit = (int64_t)b * a.H + h;
  if (tid < D) {   // combine_chunks with the one rounding on the store
    const float* wml = a.ws_ml + (unit * a.nsplit) * 2;
    const float* wo = a.ws_o + (unit * a.nsplit) * D;
    float Mt = -INFINITY;
    for (int t = 0; t < active; ++t) Mt = fmaxf(Mt, wml[2 * t]);
    float acc = 0.f, den = 0.f;
    for (int t = 0; t < active; ++t) {
      const float f = __builtin_amdgcn_exp2f(wml[2 * t] - Mt);
      acc = fmaf(f, wo[(int64_t)t * D + tid], acc);
      den = fmaf(f, wml[2 * t + 1], den);
    }
    a.o[b * a.o_sb + h * a.o_sh + tid] = (__bf16)(acc / den);
  }
}

static void launch_chunks_bf16(int d32, dim3 grid, hipStream_t st, const ArgsB& a) {
  switch (d32) {
    case 1: hipLaunchKernelGGL(attn_decode_bf16_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(attn_decode_bf16_kernel<2>, grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(attn_decode_bf16_kernel<3>, grid, dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(attn_decode_bf16_kernel<4>, grid, dim3(256), 0, st, a); break;
    case 5: hipLaunchKernelGGL(attn_decode_bf16_kernel<5>, grid, dim3(256), 0, st, a); break;
    case 6: hipLaunchKernelGGL(attn_decode_bf16_kernel<6>, grid, dim3(256), 0, st, a); break;
    case 7: hipLaunchKernelGGL(attn_decode_bf16_kernel<7>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(attn_decode_bf16_kernel<8>, grid, dim3(256), 0, st, a); break;
  }
}

}  // namespace amk_decode

using namespace amk_decode;

extern "C" int64_t amk_attn_decode_ws_floats(int B, int H, int D, int capacity) {
  if (B <= 0 || H <= 0 || D <= 0 || capacity <= 0) return 0;
  const int64_t units = (int64_t)B * H, smax = (capacity + MIN_KEYS - 1) / MIN_KEYS;
  return round4(units * smax * 2) + units * smax * D;
}

extern "C" int amk_attn_decode(const float* q, const float* k_new, const float* v_new, float* k_cache, float* v_cache,
                               float* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                               int B, int H, int D, int capacity,
                               int64_t q_sb, int64_t q_sh, int64_t new_sb, int64_t new_sh,
                               int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_sh,
                               float scale, void* stream) {
  AMK_CHECK_ARG(q && k_cache && v_cache && o && ws, "amk_attn_decode: null pointer");
  AMK_CHECK_ARG((k_new != nullptr) == (v_new != nullptr), "amk_attn_decode: k_new and v_new go together");
  AMK_CHECK_ARG(!k_new || n_dev, "amk_attn_decode: append mode needs the device-resident length n_dev");
  AMK_CHECK_ARG(B > 0 && H > 0 && D > 0 && capacity > 0, "amk_attn_decode: bad sizes B=%d H=%d D=%d capacity=%d", B, H, D, capacity);
  AMK_CHECK_SUPPORTED(D % 32 == 0 && D <= 256, "amk_attn_decode: head dim %d (a multiple of 32 from 32 to 256)", D);
  AMK_CHECK_SUPPORTED(H <= 65535 && B <= 65535, "amk_attn_decode: B=%d, H=%d beyond the grid", B, H);
  AMK_CHECK_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new) |
                  reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) | reinterpret_cast<uintptr_t>(o) |
                  reinterpret_cast<uintptr_t>(ws)) & 15) == 0 && (reinterpret_cast<uintptr_t>(n_dev) & 3) == 0,
                "amk_attn_decode: pointers must be 16-byte aligned (n_dev: 4)");
  AMK_CHECK_ARG(((q_sb | q_sh | new_sb | new_sh | c_sb | c_st | c_sh | o_sb | o_sh) & 3) == 0,
                "amk_attn_decode: strides must be multiples of 4 elements");
  const int keys = keys_per_chunk();
  const int nsplit = (capacity + keys - 1) / keys;
  const int64_t units = (int64_t)B * H;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Args a;
  a.q = q; a.k_new = k_new; a.v_new = v_new; a.k_cache = k_cache; a.v_cache = v_cache; a.o = o;
  a.ws_ml = ws;
  a.ws_o = a.ws_ml + round4(units * ((capacity + MIN_KEYS - 1) / MIN_KEYS) * 2);
  a.n_dev = n_dev; a.key_mask = key_mask;
  a.H = H; a.capacity = capacity; a.keys = keys; a.nsplit = nsplit;
  a.q_sb = q_sb; a.q_sh = q_sh; a.n_sb = new_sb; a.n_sh = new_sh; a.c_sb = c_sb; a.c_st = c_st; a.c_sh = c_sh;
  a.o_sb = o_sb; a.o_sh = o_sh;
  a.qscale = scale * AMK_LOG2E;
  launch_chunks(D / 32, dim3((unsigned)nsplit, (unsigned)H, (unsigned)B), st, a);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)H, (unsigned)B), dim3(256), 0, st, a, D);
  AMK_CHECK_LAUNCH("amk_attn_decode");
  return AMK_OK;
}

extern "C" int amk_attn_decode_bf16(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                    void* o, float* ws, const int32_t* n_dev, const uint8_t* key_mask,
                                    int B, int H, int D, int capacity,
                                    int64_t q_sb, int64_t q_sh, int64_t new_sb, int64_t new_sh,
                                    int64_t c_sb, int64_t c_st, int64_t c_sh, int64_t o_sb, int64_t o_sh,
                                    float scale, void* stream) {
  AMK_CHECK_ARG(q && k_cache && v_cache && o && ws, "amk_attn_decode_bf16: null pointer");
  AMK_CHECK_ARG((k_new != nullptr) == (v_new != nullptr), "amk_attn_decode_bf16: k_new and v_new go together");
  AMK_CHECK_ARG(!k_new || n_dev, "amk_attn_decode_bf16: append mode needs the device-resident length n_dev");
  AMK_CHECK_ARG(B > 0 && H > 0 && D > 0 && capacity > 0, "amk_attn_decode_bf16: bad sizes B=%d H=%d D=%d capacity=%d", B, H, D, capacity);
  AMK_CHECK_SUPPORTED(D % 32 == 0 && D <= 256, "amk_attn_decode_bf16: head dim %d (a multiple of 32 from 32 to 256)", D);
  AMK_CHECK_SUPPORTED(H <= 65535 && B <= 65535, "amk_attn_decode_bf16: B=%d, H=%d beyond the grid", B, H);
  AMK_CHECK_ARG(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new) |
                  reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) | reinterpret_cast<uintptr_t>(o) |
                  reinterpret_cast<uintptr_t>(ws)) & 15) == 0 && (reinterpret_cast<uintptr_t>(n_dev) & 3) == 0,
                "amk_attn_decode_bf16: pointers must be 16-byte aligned (n_dev: 4)");
  AMK_CHECK_ARG(((q_sb | q_sh | new_sb | new_sh | c_sb | c_st | c_sh | o_sb | o_sh) & 7) == 0,
                "amk_attn_decode_bf16: strides must be multiples of 8 elements");
  const int keys = keys_per_chunk();
  const int nsplit = (capacity + keys - 1) / keys;
  const int64_t units = (int64_t)B * H;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ArgsB a;
  a.q = static_cast<const __bf16*>(q); a.k_new = static_cast<const __bf16*>(k_new); a.v_new = static_cast<const __bf16*>(v_new);
  a.k_cache = static_cast<__bf16*>(k_cache); a.v_cache = static_cast<__bf16*>(v_cache); a.o = static_cast<__bf16*>(o);
  a.ws_ml = ws;
  a.ws_o = a.ws_ml + round4(units * ((capacity + MIN_KEYS - 1) / MIN_KEYS) * 2);
  a.n_dev = n_dev; a.key_mask = key_mask;
  a.H = H; a.capacity = capacity; a.keys = keys; a.nsplit = nsplit;
  a.q_sb = q_sb; a.q_sh = q_sh; a.n_sb = new_sb; a.n_sh = new_sh; a.c_sb = c_sb; a.c_st = c_st; a.c_sh = c_sh;
  a.o_sb = o_sb; a.o_sh = o_sh;
  a.qscale = scale * AMK_LOG2E;
  launch_chunks_bf16(D / 32, dim3((unsigned)nsplit, (unsigned)H, (unsigned)B), st, a);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_decode_bf16_combine_kernel, dim3((unsigned)H, (unsigned)B), dim3(256), 0, st, a, D);
  AMK_CHECK_LAUNCH("amk_attn_decode_bf16");
  return AMK_OK;
}
