// AgentAttention core for gfx950.
//
// Replaces models/agent_attention.py:55-73 of the reference: adaptive-avg-pool of q into p
// agent tokens per head, agent aggregation softmax((A*scale) K^T) V, agent broadcast
// softmax((q*scale) A^T) V_agent, plus a depthwise 3x3 convolution of v over the
// (head, token) plane.  With p <= 16 agents the work is O(T*p*d) per head -- HBM/VALU bound,
// nowhere near a GEMM.  The sequence is cut into 128-token chunks and every kernel runs one
// workgroup per (batch, head, chunk) -- B*h*ceil(T/128) workgroups, so a (2, 1024) call still
// spreads over 96 CUs and a (64, 1024) call over-subscribes the chip 12x -- with the sums over
// tokens (agent aggregation, dV_agent, dA, conv weight gradients) written as per-chunk partials
// and folded by tiny combine kernels in fixed chunk order (deterministic, no atomics):
//     forward : pool -> s1_partial -> s1_combine -> s2
//     backward: s2_bwd -> mid -> s1_bwd -> pool_bwd
// Every global access is a coalesced b128 with 16 lanes per 256-byte row.  Two thread mappings
// per chunk:
//     phase A  2 threads <-> token: the chunk's q/k/v/dO rows are staged in an LDS tile (row
//                                 stride 68 floats); each thread takes 32 channels of its token
//                                 against the agents (broadcast from LDS), the pair adds up with
//                                 one DPP swap; the p-wide softmaxes; dq / dk rows leave through
//                                 the same tile
//     phase B  16 lanes <-> row  : sums over tokens, the depthwise convolution (its 3x3 halo
//                                 comes from L2), O / dv stores; sums fold over the 4 row
//                                 groups of a wave by DPP and over the 4 waves through LDS
// bias1 / bias2 are scalars added to every score of a softmax row: the softmax is invariant
// to them, so they do not enter the arithmetic and their gradient is exactly 0.
//
// The description above is the head dim 64 build.  Every kernel is templated on the head dim D (32, 64, 128) through
// Cfg<D>; a row is always D / 4 lanes of 4 channels:
//     D = 32 : 128-token chunks, 2 threads <-> token (16 channels each),  8 lanes <-> row, 32 rows per pass
//     D = 64 : 128-token chunks, 2 threads <-> token (32 channels each), 16 lanes <-> row, 16 rows per pass
//     D = 128:  64-token chunks, 4 threads <-> token (32 channels each), 32 lanes <-> row,  8 rows per pass
// D = 128 halves the chunk so that the staged tile (64 x 132 floats) and a thread's share of a token (32 channels)
// stay what they are at D = 64: same registers, static LDS under 64 KB, no scratch.  The streaming backward (below)
// exists for D = 64 only.
//
// Two element types.  The kernels that touch q, k, v, o, dO, dq, dk, dv live in agent_kernels.h, which this file includes
// once with E = float (agent_*_kernel, amk_agent_attn_fwd / _bwd) and once with E = __bf16 (agent_*_bf16_kernel,
// amk_agent_attn_bf16_fwd / _bwd, for torch.autocast(bfloat16)): there a lane's 4 channels are one 8-byte access, widened
// exactly on the load and rounded to nearest even once on the store, and everything between is the f32 arithmetic above
// in the same order, so the bf16 outputs are the f32 outputs rounded once.  dq is written by two kernels (stage-2 part,
// then the pooled dA / len): its first part crosses in f32 through the workspace (BwdParams::dqf).  The kernels that see
// only f32 workspaces (agent_s1_combine_kernel, agent_mid_kernel, agent_conv_reduce_kernel) are here and serve both.
#include "amk_common.h"
#include <stdlib.h>

namespace amk_agent {

constexpr int MAXP = 16;
constexpr int NT = 256;      // threads per workgroup
template <int D>
struct Cfg {
  static_assert(D == 32 || D == 64 || D == 128, "head dims 32, 64, 128");
  static constexpr int CH = D == 128 ? 64 : 128;   // tokens per chunk
  static constexpr int TS = D + 4;                 // LDS row stride of the staged tile (conflict-free b128 row reads)
  static constexpr int PSTR = D + 2;               // forward partial record per (chunk, agent): D sums, chunk max, chunk row sum
  static constexpr int TPT = NT / CH;              // phase A: threads per token
  static constexpr int TCH = D / TPT;              // phase A: channels per thread
  static constexpr int LPR = D / 4;                // phase B: lanes per row
  static constexpr int RPP = NT / LPR;             // phase B: rows per pass of the workgroup
  static constexpr int NPIECE = CH / RPP;          // phase B: rows per lane group in a chunk
  static constexpr int LPR_LOG = D == 32 ? 3 : D == 64 ? 4 : 5, TPT_LOG = TPT == 2 ? 1 : 2;
  static_assert((1 << LPR_LOG) == LPR && (1 << TPT_LOG) == TPT, "");
  static_assert(4 * MAXP * D <= CH * TS, "the cross-wave reduction reuses the tile");
};
// Loops of one wave over a row of D channels take channels c = lane + 64 k, k < ceil(D / 64); only at D = 32 do
// lanes fall past the row, so the guard is written `D >= 64 || c < D` (at D = 64 it is the constant true and the
// loop is the single `c = lane` of the D = 64 build).

struct Strides { int64_t sb, st, sh; };

// q, k, v, o, d_o, dq, dk, dv are views of the kernel's element type E (float, or __bf16 under bf16 autocast); strides
// count elements.  Everything else is f32 on both paths.
struct Params {
  const void *q, *k, *v;           // (B,h,T,d) views of E
  const float *convw, *convb;      // (d,1,3,3), (d)
  void* o;                         // (B,h,T,d) view of E
  float *agents, *vagent, *stats1; // (B,h,p,d), (B,h,p,d), (B,h,p,2) saved for backward
  float* part;                     // (B,h,NC,p,PSTR) stage-1 partials
  int B, H, T, P, NC;
  Strides qs, ks, vs, os;
  float scale;
};

struct BwdParams {
  const void *q, *k, *v, *d_o;     // views of E
  const float *convw;
  const float *agents, *vagent, *stats1;
  void *dq, *dk, *dv;              // (B,h,T,d) views of E, fully overwritten
  float *pva, *pa2, *pa1;          // (B,h,NC,p,d) per-chunk partials: dV_agent, dA (stage 2), dA (stage 1)
  float *dva, *da2, *delta1;       // (B,h,p,d), (B,h,p,d), (B,h,p) folded by the mid kernel
  float *dconvw_part, *dconvb_part;// (B*h*NC, 9, d), (B*h*NC, d) partial sums
  int B, H, T, P, NC;
  Strides qs, ks, vs, dos, dqs, dks, dvs;
  float scale;
  float* dqf;                      // E = __bf16: contiguous (B,h,T,d) floats, the stage-2 part of dq on its way to the pool
                                   // backward, which adds the pooled term in f32 and rounds dq once
};

__device__ __forceinline__ float4 splat4(float x) { return make_float4(x, x, x, x); }
// Global rows through buffer descriptors with the validity folded into the OFFSET (an invalid row gets an offset past
// the descriptor's range: the load returns zeros, the store is dropped).  `cond ? *ptr : 0` compiles to a branch
// around the load, and behind such a branch every wait drains everything in flight: a tile's eight row requests
// became eight serial round trips (5.5 us to stage 32 KB; tools/scratch/stamps_agent.py).
constexpr unsigned PAST = 0x80000000u;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slab(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7ffffffe, 0x00020000);
}
// The element type E of q, k, v, o, dO, dq, dk, dv: a lane's 4 channels are one b128 (float) or one b64 (__bf16) access.
// bf16 widens exactly on the load and is rounded to nearest even once, on the store; everything in between is the
// f32 arithmetic of the float build, in the same order.
__device__ __forceinline__ float4 widen4(u32x2 w) {
  return make_float4(__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
                     __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u));
}
__device__ __forceinline__ unsigned rne16(float x) {   // the bf16 bits of x, round to nearest even (integer arithmetic:
  const unsigned u = __builtin_bit_cast(unsigned, x);  // independent of the denormal mode); NaN -> the quiet NaN 0x7fc0
  return (u & 0x7fffffffu) > 0x7f800000u ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ u32x2 narrow4(float4 v) {
  u32x2 w;
  w.x = rne16(v.x) | (rne16(v.y) << 16); w.y = rne16(v.z) | (rne16(v.w) << 16);
  return w;
}
template <class E>
__device__ __forceinline__ float4 bld4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  if constexpr (sizeof(E) == 4) return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
  else return widen4(__builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0)));
}
template <class E>
__device__ __forceinline__ void bst4(__amdgpu_buffer_rsrc_t r, unsigned off, float4 v) {
  if constexpr (sizeof(E) == 4) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)off, 0, 0);
  else __builtin_amdgcn_raw_buffer_store_b64(narrow4(v), r, (int)off, 0, 0);
}
// 4 channels through a plain pointer (the pooling kernels)
template <class E>
__device__ __forceinline__ float4 gld4(const E* p) {
  if constexpr (sizeof(E) == 4) return *reinterpret_cast<const float4*>(p);
  else return widen4(*reinterpret_cast<const u32x2*>(p));
}
template <class E>
__device__ __forceinline__ void gst4(E* p, float4 v) {
  if constexpr (sizeof(E) == 4) *reinterpret_cast<float4*>(p) = v;
  else *reinterpret_cast<u32x2*>(p) = narrow4(v);
}
// byte offset of row t (channels c4..) in a (T, D) view with row stride st, or PAST
template <class E>
__device__ __forceinline__ unsigned row_off(int t, int T, int64_t st, int c4) {
  return (t >= 0 && t < T) ? (unsigned)(((int64_t)t * st + c4) * (int)sizeof(E)) : PAST;
}
__device__ __forceinline__ void fma4(float4& a, float s, const float4& x) {
  a.x += s * x.x; a.y += s * x.y; a.z += s * x.z; a.w += s * x.w;
}
__device__ __forceinline__ void mad4(float4& a, const float4& w, const float4& x) {
  a.x += w.x * x.x; a.y += w.y * x.y; a.z += w.z * x.z; a.w += w.w * x.w;
}
__host__ __device__ __forceinline__ int bin_lo(int i, int T, int P) { return (int)(((int64_t)i * T) / P); }
__host__ __device__ __forceinline__ int bin_hi(int i, int T, int P) { return (int)((((int64_t)(i + 1)) * T + P - 1) / P); }

// Workgroup-cooperative: rows [t0, t0+CH) of a (T, D) view -> tile[CH][TS]; rows >= T are zero.
// D / 4 lanes per row (16 per 256-byte row at D = 64), RPP rows per pass: coalesced b128 loads, conflict-free LDS writes.
template <int D, class E>
__device__ __forceinline__ void stage_rows(float* tile, const E* base, int64_t st, int t0, int T, int tid) {
  using C = Cfg<D>;
  const int c4 = (tid & (C::LPR - 1)) * 4;
  const __amdgpu_buffer_rsrc_t rs = slab(base);
  float4 pc[C::NPIECE];
#pragma unroll
  for (int j = 0; j < C::NPIECE; ++j) pc[j] = bld4<E>(rs, row_off<E>(t0 + C::RPP * j + (tid >> C::LPR_LOG), T, st, c4));   // all in flight
#pragma unroll
  for (int j = 0; j < C::NPIECE; ++j) st4(tile + (C::RPP * j + (tid >> C::LPR_LOG)) * C::TS + c4, pc[j]);
}
// the same in two halves: request the pieces (registers), put them into the tile later -- the second tile of a kernel
// is in flight while the first one is worked on
template <int D, class E>
__device__ __forceinline__ void fetch_rows(float4 (&pc)[Cfg<D>::NPIECE], const E* base, int64_t st, int t0, int T, int tid) {
  using C = Cfg<D>;
  const int c4 = (tid & (C::LPR - 1)) * 4;
  const __amdgpu_buffer_rsrc_t rs = slab(base);
#pragma unroll
  for (int j = 0; j < C::NPIECE; ++j) pc[j] = bld4<E>(rs, row_off<E>(t0 + C::RPP * j + (tid >> C::LPR_LOG), T, st, c4));
}
template <int D>
__device__ __forceinline__ void put_rows(float* tile, const float4 (&pc)[Cfg<D>::NPIECE], int tid) {
  using C = Cfg<D>;
  const int c4 = (tid & (C::LPR - 1)) * 4;
#pragma unroll
  for (int j = 0; j < C::NPIECE; ++j) st4(tile + (C::RPP * j + (tid >> C::LPR_LOG)) * C::TS + c4, pc[j]);
}
// tile[CH][TS] -> rows [t0, min(t0+CH, T)) of a (T, D) view
template <int D, class E>
__device__ __forceinline__ void unstage_rows(const float* tile, E* base, int64_t st, int t0, int T, int tid) {
  using C = Cfg<D>;
  const int c4 = (tid & (C::LPR - 1)) * 4;
  const __amdgpu_buffer_rsrc_t rs = slab(base);
#pragma unroll
  for (int r0 = 0; r0 < C::CH; r0 += C::RPP) {
    const int r = r0 + (tid >> C::LPR_LOG);
    bst4<E>(rs, row_off<E>(t0 + r, T, st, c4), ld4(tile + r * C::TS + c4));
  }
}
// a value moved inside a row of 16 lanes by a DPP pattern (one VALU modifier; __shfl_xor compiles to ds_bpermute_b32, an
// LDS-crossbar round trip)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
// phase A: thread (tok, part) owns channels [TCH*part, TCH*part+TCH) of token tok
template <int D>
__device__ __forceinline__ void load_half(const float* tile, int tok, int half, float (&r)[Cfg<D>::TCH]) {
  constexpr int HALF = Cfg<D>::TCH;
  const float* src = tile + tok * Cfg<D>::TS + HALF * half;
#pragma unroll
  for (int j = 0; j < HALF / 4; ++j) {
    const float4 t = ld4(src + 4 * j);
    r[4 * j] = t.x; r[4 * j + 1] = t.y; r[4 * j + 2] = t.z; r[4 * j + 3] = t.w;
  }
}
// <thread's part of the row, a[TCH*part ...]> summed over the parts of the token (lanes 2k, 2k+1; or 4k .. 4k+3)
template <int D>
__device__ __forceinline__ float dot_half(const float (&r)[Cfg<D>::TCH], const float* a, int half) {
  constexpr int HALF = Cfg<D>::TCH;
  const float* src = a + HALF * half;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < HALF / 4; ++j) {
    const float4 t = ld4(src + 4 * j);
    s += r[4 * j] * t.x + r[4 * j + 1] * t.y + r[4 * j + 2] * t.z + r[4 * j + 3] * t.w;
  }
  s = s + dpp_mov<0xB1>(s);   // quad_perm [1, 0, 3, 2]: the other half of the token (pair)
  if (Cfg<D>::TPT == 4) s = s + dpp_mov<0x4E>(s);   // quad_perm [2, 3, 0, 1]: the other pair of the quad
  return s;
}
// sum over the row groups of a wave (phase B: the lane bits above the row's D / 4 lanes select the token)
template <int D>
__device__ __forceinline__ float4 fold_subs(float4 a) {
  if (D == 32) {
    a.x += __shfl_xor(a.x, 8, 64); a.y += __shfl_xor(a.y, 8, 64); a.z += __shfl_xor(a.z, 8, 64); a.w += __shfl_xor(a.w, 8, 64);
  }
  if (D <= 64) {
    a.x += __shfl_xor(a.x, 16, 64); a.y += __shfl_xor(a.y, 16, 64); a.z += __shfl_xor(a.z, 16, 64); a.w += __shfl_xor(a.w, 16, 64);
  }
  a.x += __shfl_xor(a.x, 32, 64); a.y += __shfl_xor(a.y, 32, 64); a.z += __shfl_xor(a.z, 32, 64); a.w += __shfl_xor(a.w, 32, 64);
  return a;
}
// sum of the four waves' entries red[(w*MAXP + i)*D + c]
template <int D>
__device__ __forceinline__ float fold4(const float* red, int i, int c) {
  return red[(0 * MAXP + i) * D + c] + red[(1 * MAXP + i) * D + c] + red[(2 * MAXP + i) * D + c] +
         red[(3 * MAXP + i) * D + c];
}

#ifdef AMK_AGENT_STAMPS   // diagnostic build (tools/scratch/stamps_agent.py): per-workgroup time stamps of s2_bwd
__device__ unsigned long long* g_stamps = nullptr;
#define AG_STAMP(i) do { if (threadIdx.x == 0 && g_stamps) g_stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define AG_STAMP(i) do { } while (0)
#endif

// blockIdx -> (b, h, chunk); chunk fastest so neighbouring workgroups share the conv halo rows in L2
struct Where { int b, h, ch, t0; int64_t bh; };
template <int CH>
__device__ __forceinline__ Where where(int H, int NC) {
  Where w;
  w.ch = blockIdx.x % NC;
  const int bh = blockIdx.x / NC;
  w.h = bh % H; w.b = bh / H; w.bh = bh; w.t0 = w.ch * CH;
  return w;
}

// (forward 0, 1 and 3 -- pool, s1_partial, s2 -- are in agent_kernels.h; so are backward 0, 2, 3 and the streaming forms)
// forward 2: fold the chunk partials (fixed chunk order): V_agent and the (max, sum) stats.
// One workgroup per (b, h), one wave per agent.  The chunk stats sit one per lane (64 chunks per
// pass) so their loads and exponentials are independent instead of a serial chain.
template <int D>
__global__ __launch_bounds__(256) void agent_s1_combine_kernel(Params p) {
  constexpr int PSTR = Cfg<D>::PSTR, CPL = (D + 63) / 64;   // channels per lane
  __shared__ float a_s[4][64], l_s[4][64];  // per wave: rescale factor and row sum of 64 chunks
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = blockIdx.x;
  for (int i = wave; i < p.P; i += 4) {
    const float* rec0 = p.part + (bh * p.NC * p.P + i) * PSTR;
    const int64_t cstr = (int64_t)p.P * PSTR;
    float M = -INFINITY;
    for (int c = lane; c < p.NC; c += 64) M = fmaxf(M, rec0[c * cstr + D]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    float L = 0.f, s[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) s[k] = 0.f;
    for (int c0 = 0; c0 < p.NC; c0 += 64) {
      const int cmine = c0 + lane;
      a_s[wave][lane] = cmine < p.NC ? expf(rec0[cmine * cstr + D] - M) : 0.f;
      l_s[wave][lane] = cmine < p.NC ? rec0[cmine * cstr + D + 1] : 0.f;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int n = min(64, p.NC - c0);
#pragma unroll 4
      for (int c = 0; c < n; ++c) {  // ascending chunk order; a wave reads only what it wrote
        const float a = a_s[wave][c];
        L += a * l_s[wave][c];
#pragma unroll
        for (int k = 0; k < CPL; ++k)
          if ((D >= 64 || lane + 64 * k < D)) s[k] += a * rec0[(c0 + c) * cstr + lane + 64 * k];
      }
      __builtin_amdgcn_wave_barrier();
    }
    const int64_t row = bh * p.P + i;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if ((D >= 64 || lane + 64 * k < D)) p.vagent[row * D + lane + 64 * k] = s[k] / L;
    if (lane == 0) { p.stats1[row * 2] = M; p.stats1[row * 2 + 1] = L; }
  }
}

// depthwise 3x3 over the (head, token) plane at (hh, t), channels c4..c4+3, zero padded.
// wq[j] holds weight tap j of the four channels.  FLIP: transposed convolution (backward).
template <bool FLIP>
__device__ __forceinline__ void conv4(float4& acc, const float* xb, const Strides& xs, int H, int T, int hh, int t, int c4,
                                      const float4 (&wq)[9]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int h2 = FLIP ? hh - (a - 1) : hh + (a - 1);
    if (h2 < 0 || h2 >= H) continue;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int t2 = FLIP ? t - (b - 1) : t + (b - 1);
      if (t2 < 0 || t2 >= T) continue;
      mad4(acc, wq[a * 3 + b], ld4(xb + (int64_t)h2 * xs.sh + (int64_t)t2 * xs.st + c4));
    }
  }
}
__device__ __forceinline__ void load_taps(const float* convw, int c4, float4 (&wq)[9]) {
#pragma unroll
  for (int j = 0; j < 9; ++j)
    wq[j] = make_float4(convw[(c4 + 0) * 9 + j], convw[(c4 + 1) * 9 + j], convw[(c4 + 2) * 9 + j], convw[(c4 + 3) * 9 + j]);
}

// The stage-2 part of dq goes to the float tensor dq itself, or (E = __bf16) in f32 to the contiguous workspace dqf.
// dq_part: the (T, D) float view of this (b, h); dq_part_st: its row stride.
template <int D, class E>
__device__ __forceinline__ float* dq_part(const BwdParams& p, const Where& w) {
  if constexpr (sizeof(E) == 4) return static_cast<float*>(p.dq) + (int64_t)w.b * p.dqs.sb + (int64_t)w.h * p.dqs.sh;
  else return p.dqf + w.bh * p.T * D;
}
template <int D, class E>
__device__ __forceinline__ int64_t dq_part_st(const BwdParams& p) {
  if constexpr (sizeof(E) == 4) return p.dqs.st;
  else return D;
}
// where the pool backward reads that part of row `row` = (b h) T + t back: from dq itself (dst), or from dqf
template <int D, class E>
__device__ __forceinline__ const float* dq_part_row(const BwdParams& p, const E* dst, int64_t row, int c4) {
  if constexpr (sizeof(E) == 4) return dst;
  else return p.dqf + row * D + c4;
}

// backward 1: fold the stage-2 partials in chunk order: dV_agent, dA (stage 2), delta1 = <dV_agent, V_agent>.
// One workgroup per (b, h).
template <int D>
__global__ __launch_bounds__(256) void agent_mid_kernel(BwdParams p) {
  constexpr int CPL = (D + 63) / 64;   // channels per lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = blockIdx.x;
  for (int i = wave; i < p.P; i += 4) {
    float sva[CPL], sa2[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) { sva[k] = 0.f; sa2[k] = 0.f; }
#pragma unroll 4
    for (int c = 0; c < p.NC; ++c) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        if ((D >= 64 || lane + 64 * k < D)) {
          const int64_t o = (((bh * p.NC + c) * p.P) + i) * D + lane + 64 * k;
          sva[k] += p.pva[o];
          sa2[k] += p.pa2[o];
        }
      }
    }
    const int64_t row = bh * p.P + i;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if ((D >= 64 || lane + 64 * k < D)) {
        p.dva[row * D + lane + 64 * k] = sva[k];
        p.da2[row * D + lane + 64 * k] = sa2[k];
        const float t = sva[k] * p.vagent[row * D + lane + 64 * k];
        s = k == 0 ? t : s + t;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) p.delta1[row] = s;
  }
}

// ---------------------------------------------------------------------------------------
// Streaming forms of the two chunk kernels of the backward (P <= 8 agents per head).  The kernels above stage a
// chunk's rows in LDS and run two thread mappings over them (2 threads <-> token for the p-wide arithmetic, 16 lanes <->
// row for the sums): five barrier-separated phases per workgroup, the agents re-read from LDS for every token, and
// -- every workgroup of the chip being in the same phase at the same time -- HBM idle during the arithmetic.  Here
// ONE mapping serves everything: 16 lanes per row (4 channels each), a 16-lane group takes CH / 16 consecutive rows
// from load to store; the agents' channels of a lane sit in registers, a row's p scores are 4-channel partial dots
// folded over the 16 lanes by four DPP steps, and nothing goes through LDS but the final fold of the per-group sums.
// The convolution's weight / bias gradient moves to the stage-1 kernel, which holds the dO window anyway:
//   dw[a][b] = sum g[h][t] v[h+a-1][t+b-1] = sum v[h'][t'] g[h'-(a-1)][t'-(b-1)]   (h' = h+a-1, t' = t+b-1).
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
// sum over the 16 lanes of a row group, every lane ends with it: four DPP moves inside the row (quad swaps, then the
// mirrored half-row and row: after the quad steps all four lanes of a quad agree, so a mirror is as good as an xor) --
// __shfl_xor compiles to ds_bpermute_b32, an LDS-crossbar round trip per step, 48 of them per token row here
__device__ __forceinline__ float fold16(float x) {
  x += dpp_mov<0xB1>(x);    // quad_perm [1, 0, 3, 2]
  x += dpp_mov<0x4E>(x);    // quad_perm [2, 3, 0, 1]
  x += dpp_mov<0x141>(x);   // row_half_mirror
  x += dpp_mov<0x140>(x);   // row_mirror
  return x;
}

constexpr int PB = 64;   // tokens per workgroup of the pool backward

// every kernel that touches a tensor of E, once per element type (agent_kernels.h)
#define AGENT_E float
#define AGENT_KERNEL(n) agent_##n##_kernel
#include "agent_kernels.h"
#undef AGENT_E
#undef AGENT_KERNEL
#define AGENT_E __bf16
#define AGENT_KERNEL(n) agent_##n##_bf16_kernel
#include "agent_kernels.h"
#undef AGENT_E
#undef AGENT_KERNEL

}  // namespace amk_agent

using namespace amk_agent;

// strides count elements: a row of a lane's 4 channels starts on a 16-byte boundary (4 floats, 8 bf16)
static bool sok(const Strides& s, int64_t m) { return s.sb % m == 0 && s.st % m == 0 && s.sh % m == 0; }
// the kernels address one batch entry's (h, T, d) slab through a 32-bit byte offset (offsets from 2^31 on mean "past the end")
static bool span_ok(const Strides& s, int H, int T, int D, int esz) {
  return s.st >= 0 && s.sh >= 0 && ((int64_t)(H - 1) * s.sh + (int64_t)(T - 1) * s.st + D) * esz < 0x7ffffffell;
}
static bool dh_ok(int Dh) { return Dh == 32 || Dh == 64 || Dh == 128; }
static int chunk_len(int Dh) { return Dh == 128 ? Cfg<128>::CH : Dh == 32 ? Cfg<32>::CH : Cfg<64>::CH; }
static int nchunks(int T, int Dh) { return (T + chunk_len(Dh) - 1) / chunk_len(Dh); }

// kernels are instantiated for up to 8 and up to 16 agents per head (register arrays sized to that)
#define AMK_AGENT_LAUNCH(KERNEL, P_, ...)                                    \
  do {                                                                       \
    if ((P_) <= 8) hipLaunchKernelGGL((KERNEL<D, 8>), __VA_ARGS__);          \
    else hipLaunchKernelGGL((KERNEL<D, 16>), __VA_ARGS__);                   \
  } while (0)
// BF: the __bf16 wrappers (agent_<NAME>_bf16_kernel) instead of the float ones (agent_<NAME>_kernel)
#define AMK_AGENT_LAUNCH_E(NAME, P_, ...)                                                \
  do {                                                                                   \
    if constexpr (BF) AMK_AGENT_LAUNCH(agent_##NAME##_bf16_kernel, P_, __VA_ARGS__);     \
    else AMK_AGENT_LAUNCH(agent_##NAME##_kernel, P_, __VA_ARGS__);                       \
  } while (0)

extern "C" int amk_agent_num_chunks(int T) { return T > 0 ? nchunks(T, 64) : 0; }
extern "C" int amk_agent_num_chunks_dh(int T, int Dh) { return T > 0 && dh_ok(Dh) ? nchunks(T, Dh) : 0; }

extern "C" int64_t amk_agent_ws_floats_dh(int B, int H, int T, int P, int Dh, int backward) {
  if (B <= 0 || H <= 0 || T <= 0 || P <= 0 || !dh_ok(Dh)) return 0;
  const int64_t cells = (int64_t)B * H * nchunks(T, Dh) * P, rows = (int64_t)B * H * P;
  return backward ? 3 * cells * Dh + 2 * rows * Dh + rows : cells * (Dh + 2);
}
extern "C" int64_t amk_agent_ws_floats(int B, int H, int T, int P, int backward) { return amk_agent_ws_floats_dh(B, H, T, P, 64, backward); }
// the bf16 backward keeps the stage-2 part of dq in f32 behind the f32 path's workspace: (B, h, T, d) floats more
extern "C" int64_t amk_agent_bf16_ws_floats(int B, int H, int T, int P, int Dh, int backward) {
  const int64_t n = amk_agent_ws_floats_dh(B, H, T, P, Dh, backward);
  return n && backward ? n + (int64_t)B * H * T * Dh : n;
}

template <int D, bool BF>
static void agent_fwd_launch(const Params& p, hipStream_t st) {
  const unsigned cells = (unsigned)((int64_t)p.B * p.H * p.NC);
  if constexpr (BF) hipLaunchKernelGGL(agent_pool_bf16_kernel<D>, dim3((unsigned)(p.B * p.H * p.P)), dim3(NT), 0, st, p);
  else hipLaunchKernelGGL(agent_pool_kernel<D>, dim3((unsigned)(p.B * p.H * p.P)), dim3(NT), 0, st, p);
  AMK_AGENT_LAUNCH_E(s1_partial, p.P, dim3(cells), dim3(NT), 0, st, p);
  hipLaunchKernelGGL(agent_s1_combine_kernel<D>, dim3((unsigned)(p.B * p.H)), dim3(256), 0, st, p);
  AMK_AGENT_LAUNCH_E(s2, p.P, dim3(cells), dim3(NT), 0, st, p);
}

// both element types: BF = false is amk_agent_attn_fwd (float, strides multiples of 4), BF = true amk_agent_attn_bf16_fwd
// (__bf16, strides multiples of 8)
template <bool BF>
static int agent_fwd_host(const char* name, const void* q, const void* k, const void* v, const float* conv_w, const float* conv_b,
                          void* o, float* agents, float* vagent, float* stats1, float* ws, int B, int H, int T, int Dh, int P,
                          const Strides& qs, const Strides& ks, const Strides& vs, const Strides& os, float scale, void* stream) {
  constexpr int ESZ = BF ? 2 : 4, SM = 16 / ESZ;
  AMK_CHECK_ARG(q && k && v && conv_w && conv_b && o && agents && vagent && stats1 && ws, "%s: null pointer", name);
  AMK_CHECK_ARG(B > 0 && H > 0 && T > 0 && P > 0, "%s: non-positive size", name);
  AMK_CHECK_SUPPORTED(dh_ok(Dh), "%s: head dim %d not supported (32, 64 or 128)", name, Dh);
  AMK_CHECK_SUPPORTED(P <= MAXP && P <= T, "%s: agents per head %d > %d or > T", name, P, MAXP);
  Params p;
  p.q = q; p.k = k; p.v = v; p.convw = conv_w; p.convb = conv_b; p.o = o;
  p.agents = agents; p.vagent = vagent; p.stats1 = stats1; p.part = ws;
  p.B = B; p.H = H; p.T = T; p.P = P; p.NC = nchunks(T, Dh);
  p.qs = qs; p.ks = ks; p.vs = vs; p.os = os;
  p.scale = scale;
  AMK_CHECK_ARG(a16(q) && a16(k) && a16(v) && a16(o) && sok(p.qs, SM) && sok(p.ks, SM) && sok(p.vs, SM) && sok(p.os, SM),
                "%s: pointers must be 16-byte aligned and strides multiples of %d", name, SM);
  const int64_t cells = (int64_t)B * H * p.NC;
  AMK_CHECK_SUPPORTED(cells * P < (1ll << 31), "%s: B*h*chunks*p exceeds the grid limit", name);
  AMK_CHECK_SUPPORTED(span_ok(p.qs, H, T, Dh, ESZ) && span_ok(p.ks, H, T, Dh, ESZ) && span_ok(p.vs, H, T, Dh, ESZ) &&
                          span_ok(p.os, H, T, Dh, ESZ),
                      "%s: one batch entry of a tensor must span less than 2 GiB with non-negative strides", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (Dh == 32) agent_fwd_launch<32, BF>(p, st);
  else if (Dh == 128) agent_fwd_launch<128, BF>(p, st);
  else agent_fwd_launch<64, BF>(p, st);
  AMK_CHECK_LAUNCH(name);
  return AMK_OK;
}

extern "C" int amk_agent_attn_fwd(const float* q, const float* k, const float* v, const float* conv_w, const float* conv_b,
                                  float* o, float* agents, float* vagent, float* stats1, float* ws,
                                  int B, int H, int T, int Dh, int P,
                                  int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                  int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                  float scale, void* stream) {
  return agent_fwd_host<false>("amk_agent_attn_fwd", q, k, v, conv_w, conv_b, o, agents, vagent, stats1, ws, B, H, T, Dh, P,
                               {q_sb, q_st, q_sh}, {k_sb, k_st, k_sh}, {v_sb, v_st, v_sh}, {o_sb, o_st, o_sh}, scale, stream);
}
extern "C" int amk_agent_attn_bf16_fwd(const void* q, const void* k, const void* v, const float* conv_w, const float* conv_b,
                                       void* o, float* agents, float* vagent, float* stats1, float* ws,
                                       int B, int H, int T, int Dh, int P,
                                       int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                       int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t o_sb, int64_t o_st, int64_t o_sh,
                                       float scale, void* stream) {
  return agent_fwd_host<true>("amk_agent_attn_bf16_fwd", q, k, v, conv_w, conv_b, o, agents, vagent, stats1, ws, B, H, T, Dh, P,
                              {q_sb, q_st, q_sh}, {k_sb, k_st, k_sh}, {v_sb, v_st, v_sh}, {o_sb, o_st, o_sh}, scale, stream);
}

// the LDS-staged chunk kernels for every head dim; the streaming forms (head dim 64, P <= 8) unless AMK_AGENT_STREAM=0
template <int D, bool BF>
static void agent_bwd_launch(const BwdParams& p, hipStream_t st, bool streaming) {
  const unsigned cells = (unsigned)((int64_t)p.B * p.H * p.NC);
  const int P = p.P;
#define AMK_AGENT_STREAM_LAUNCH_(KERNEL)                                                               \
  do {                                                                                                  \
    if (P <= 4) hipLaunchKernelGGL(KERNEL<4>, dim3(cells), dim3(NT), 0, st, p);                        \
    else if (P <= 6) hipLaunchKernelGGL(KERNEL<6>, dim3(cells), dim3(NT), 0, st, p);                   \
    else hipLaunchKernelGGL(KERNEL<8>, dim3(cells), dim3(NT), 0, st, p);                               \
  } while (0)
#define AMK_AGENT_STREAM_LAUNCH(NAME)                                                    \
  do {                                                                                   \
    if constexpr (BF) AMK_AGENT_STREAM_LAUNCH_(agent_##NAME##_stream_bf16_kernel);       \
    else AMK_AGENT_STREAM_LAUNCH_(agent_##NAME##_stream_kernel);                         \
  } while (0)
  if (D == 64 && streaming) AMK_AGENT_STREAM_LAUNCH(s2_bwd);
  else AMK_AGENT_LAUNCH_E(s2_bwd, P, dim3(cells), dim3(NT), 0, st, p);
  hipLaunchKernelGGL(agent_mid_kernel<D>, dim3((unsigned)(p.B * p.H)), dim3(256), 0, st, p);
  if (D == 64 && streaming) AMK_AGENT_STREAM_LAUNCH(s1_bwd);
  else AMK_AGENT_LAUNCH_E(s1_bwd, P, dim3(cells), dim3(NT), 0, st, p);
#undef AMK_AGENT_STREAM_LAUNCH
#undef AMK_AGENT_STREAM_LAUNCH_
  const int64_t pblk = (int64_t)p.B * p.H * ((p.T + PB - 1) / PB);
  if constexpr (BF) hipLaunchKernelGGL(agent_pool_bwd_bf16_kernel<D>, dim3((unsigned)pblk), dim3(NT), 0, st, p);
  else hipLaunchKernelGGL(agent_pool_bwd_kernel<D>, dim3((unsigned)pblk), dim3(NT), 0, st, p);
}

struct BwdStrides { Strides q, k, v, d_o, dq, dk, dv; };

template <bool BF>
static int agent_bwd_host(const char* name, const void* q, const void* k, const void* v, const float* conv_w, const void* d_o,
                          const float* agents, const float* vagent, const float* stats1, void* dq, void* dk, void* dv,
                          float* ws, float* dconvw_part, float* dconvb_part, int B, int H, int T, int Dh, int P,
                          const BwdStrides& s, float scale, void* stream) {
  constexpr int ESZ = BF ? 2 : 4, SM = 16 / ESZ;
  AMK_CHECK_ARG(q && k && v && conv_w && d_o && agents && vagent && stats1 && dq && dk && dv && ws && dconvw_part &&
                    dconvb_part, "%s: null pointer", name);
  AMK_CHECK_ARG(B > 0 && H > 0 && T > 0 && P > 0, "%s: non-positive size", name);
  AMK_CHECK_SUPPORTED(dh_ok(Dh) && P <= MAXP && P <= T, "%s: unsupported d=%d (32, 64 or 128) / p=%d", name, Dh, P);
  BwdParams p;
  p.q = q; p.k = k; p.v = v; p.d_o = d_o; p.convw = conv_w; p.agents = agents; p.vagent = vagent; p.stats1 = stats1;
  p.dq = dq; p.dk = dk; p.dv = dv; p.dconvw_part = dconvw_part; p.dconvb_part = dconvb_part;
  p.B = B; p.H = H; p.T = T; p.P = P; p.NC = nchunks(T, Dh);
  const int64_t cells = (int64_t)B * H * p.NC, rows = (int64_t)B * H * P;
  // bf16: the f32 stage-2 part of dq comes first (its rows move as float4s: 16-byte aligned when ws is)
  p.dqf = BF ? ws : nullptr;
  p.pva = BF ? ws + (int64_t)B * H * T * Dh : ws; p.pa2 = p.pva + cells * P * Dh; p.pa1 = p.pa2 + cells * P * Dh;
  p.dva = p.pa1 + cells * P * Dh; p.da2 = p.dva + rows * Dh; p.delta1 = p.da2 + rows * Dh;
  p.qs = s.q; p.ks = s.k; p.vs = s.v; p.dos = s.d_o; p.dqs = s.dq; p.dks = s.dk; p.dvs = s.dv;
  p.scale = scale;
  AMK_CHECK_ARG(a16(q) && a16(k) && a16(v) && a16(d_o) && a16(dq) && a16(dk) && a16(dv) && (!BF || a16(ws)) && sok(p.qs, SM) && sok(p.ks, SM) &&
                    sok(p.vs, SM) && sok(p.dos, SM) && sok(p.dqs, SM) && sok(p.dks, SM) && sok(p.dvs, SM),
                "%s: pointers must be 16-byte aligned and strides multiples of %d", name, SM);
  const int64_t pblk = (int64_t)B * H * ((T + PB - 1) / PB);
  AMK_CHECK_SUPPORTED(pblk < (1ll << 31), "%s: B*h*T exceeds the grid limit", name);
  AMK_CHECK_SUPPORTED(span_ok(p.qs, H, T, Dh, ESZ) && span_ok(p.ks, H, T, Dh, ESZ) && span_ok(p.vs, H, T, Dh, ESZ) &&
                          span_ok(p.dos, H, T, Dh, ESZ) && span_ok(p.dqs, H, T, Dh, ESZ) && span_ok(p.dks, H, T, Dh, ESZ) &&
                          span_ok(p.dvs, H, T, Dh, ESZ),
                      "%s: one batch entry of a tensor must span less than 2 GiB with non-negative strides", name);
  AMK_CHECK_SUPPORTED(!BF || (int64_t)T * Dh * 4 < 0x7ffffffell, "%s: one head of the f32 dq workspace must span less than 2 GiB", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // AMK_AGENT_STREAM=0: the LDS-staged chunk kernels also for P <= 8 (head dim 64); read per call, like AMK_MOE_NARROW
  const char* e = getenv("AMK_AGENT_STREAM");
  const bool streaming = (e ? atoi(e) : 1) && P <= 8;
  if (Dh == 32) agent_bwd_launch<32, BF>(p, st, streaming);
  else if (Dh == 128) agent_bwd_launch<128, BF>(p, st, streaming);
  else agent_bwd_launch<64, BF>(p, st, streaming);
  AMK_CHECK_LAUNCH(name);
  return AMK_OK;
}

extern "C" int amk_agent_attn_bwd(const float* q, const float* k, const float* v, const float* conv_w, const float* d_o,
                                  const float* agents, const float* vagent, const float* stats1,
                                  float* dq, float* dk, float* dv, float* ws, float* dconvw_part, float* dconvb_part,
                                  int B, int H, int T, int Dh, int P,
                                  int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                  int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t do_sb, int64_t do_st, int64_t do_sh,
                                  int64_t dq_sb, int64_t dq_st, int64_t dq_sh, int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                                  int64_t dv_sb, int64_t dv_st, int64_t dv_sh, float scale, void* stream) {
  return agent_bwd_host<false>("amk_agent_attn_bwd", q, k, v, conv_w, d_o, agents, vagent, stats1, dq, dk, dv, ws, dconvw_part,
                               dconvb_part, B, H, T, Dh, P,
                               {{q_sb, q_st, q_sh}, {k_sb, k_st, k_sh}, {v_sb, v_st, v_sh}, {do_sb, do_st, do_sh},
                                {dq_sb, dq_st, dq_sh}, {dk_sb, dk_st, dk_sh}, {dv_sb, dv_st, dv_sh}}, scale, stream);
}
extern "C" int amk_agent_attn_bf16_bwd(const void* q, const void* k, const void* v, const float* conv_w, const void* d_o,
                                       const float* agents, const float* vagent, const float* stats1,
                                       void* dq, void* dk, void* dv, float* ws, float* dconvw_part, float* dconvb_part,
                                       int B, int H, int T, int Dh, int P,
                                       int64_t q_sb, int64_t q_st, int64_t q_sh, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                       int64_t v_sb, int64_t v_st, int64_t v_sh, int64_t do_sb, int64_t do_st, int64_t do_sh,
                                       int64_t dq_sb, int64_t dq_st, int64_t dq_sh, int64_t dk_sb, int64_t dk_st, int64_t dk_sh,
                                       int64_t dv_sb, int64_t dv_st, int64_t dv_sh, float scale, void* stream) {
  return agent_bwd_host<true>("amk_agent_attn_bf16_bwd", q, k, v, conv_w, d_o, agents, vagent, stats1, dq, dk, dv, ws, dconvw_part,
                              dconvb_part, B, H, T, Dh, P,
                              {{q_sb, q_st, q_sh}, {k_sb, k_st, k_sh}, {v_sb, v_st, v_sh}, {do_sb, do_st, do_sh},
                               {dq_sb, dq_st, dq_sh}, {dk_sb, dk_st, dk_sh}, {dv_sb, dv_st, dv_sh}}, scale, stream);
}

// dconvw[c][a*3+b] = sum over the rows of dconvw_part[row][a*3+b][c]; dconvb[c] = sum of dconvb_part[row][c]: one launch,
// a fixed order, the weight gradient written in the parameter's own (d, 1, 3, 3) layout -- instead of two library
// reductions and a transposing copy.  A workgroup takes one tap (or the bias) and 16 channels: 64 strided row walks of
// float4s in flight side by side, folded through LDS in a fixed order.
template <int D>
__global__ __launch_bounds__(256) void agent_conv_reduce_kernel(const float* __restrict__ wpart, const float* __restrict__ bpart,
                                                                int64_t rows, float* __restrict__ dconvw, float* __restrict__ dconvb) {
  __shared__ float red[64][17];
  const int r = blockIdx.x;                       // 0..8: weight tap, 9: bias
  const int c4i = threadIdx.x & 3, part = threadIdx.x >> 2, c0 = blockIdx.y * 16;
  const float* src = (r < 9 ? wpart + (int64_t)r * D : bpart) + c0 + c4i * 4;
  const int64_t stride = r < 9 ? 9 * D : D;
  float4 acc = amk_agent::splat4(0.f);
  for (int64_t i = part; i < rows; i += 64) {
    const float4 v = ld4(src + i * stride);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[part][c4i * 4 + 0] = acc.x; red[part][c4i * 4 + 1] = acc.y; red[part][c4i * 4 + 2] = acc.z; red[part][c4i * 4 + 3] = acc.w;
  __syncthreads();
  if (threadIdx.x < 16) {
    float t = 0.f;
    for (int j = 0; j < 64; ++j) t += red[j][threadIdx.x];
    const int c = c0 + threadIdx.x;
    if (r < 9) dconvw[c * 9 + r] = t;
    else dconvb[c] = t;
  }
}

extern "C" int amk_agent_conv_grad_reduce(const float* dconvw_part, const float* dconvb_part, int64_t rows, int Dh,
                                          float* dconvw, float* dconvb, void* stream) {
  AMK_CHECK_ARG(dconvw_part && dconvb_part && dconvw && dconvb && rows > 0, "amk_agent_conv_grad_reduce: null pointer or no rows");
  AMK_CHECK_SUPPORTED(dh_ok(Dh), "amk_agent_conv_grad_reduce: head dim %d not supported (32, 64 or 128)", Dh);
  AMK_CHECK_ARG((reinterpret_cast<uintptr_t>(dconvw_part) & 15) == 0 && (reinterpret_cast<uintptr_t>(dconvb_part) & 15) == 0,
                "amk_agent_conv_grad_reduce: partials must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (Dh == 32) hipLaunchKernelGGL(agent_conv_reduce_kernel<32>, dim3(10, 32 / 16), dim3(256), 0, st, dconvw_part, dconvb_part, rows, dconvw, dconvb);
  else if (Dh == 128) hipLaunchKernelGGL(agent_conv_reduce_kernel<128>, dim3(10, 128 / 16), dim3(256), 0, st, dconvw_part, dconvb_part, rows, dconvw, dconvb);
  else hipLaunchKernelGGL(agent_conv_reduce_kernel<64>, dim3(10, 64 / 16), dim3(256), 0, st, dconvw_part, dconvb_part, rows, dconvw, dconvb);
  AMK_CHECK_LAUNCH("amk_agent_conv_grad_reduce");
  return AMK_OK;
}

// diagnostic (not part of the ABI): resident workgroups per CU the runtime computes for the chunk kernels (head dim 64)
extern "C" int amk_debug_agent_occupancy(int which) {
  int n = -1;
  hipError_t e;
  if (which == 0) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, amk_agent::agent_s1_partial_kernel<64, 8>, amk_agent::NT, 0);
  else if (which == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, amk_agent::agent_s2_kernel<64, 8>, amk_agent::NT, 0);
  else if (which == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, amk_agent::agent_s2_bwd_kernel<64, 8>, amk_agent::NT, 0);
  else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, amk_agent::agent_s1_bwd_kernel<64, 8>, amk_agent::NT, 0);
  return e == hipSuccess ? n : -(int)e;
}

#ifdef AMK_AGENT_STAMPS
extern "C" int amk_debug_agent_set_stamps(void* buf) {
  unsigned long long* b = static_cast<unsigned long long*>(buf);
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(amk_agent::g_stamps), &b, sizeof(b));
}
#endif
