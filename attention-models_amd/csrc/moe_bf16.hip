// The routed expert products of MoELayer under bf16 autocast (reference: the per-expert nn.Linear of models/moe.py:23-38
// inside accelerator.autocast(), trainers/vit.py:67): the three grouped GEMMs of csrc/moe.hip on v_mfma_f32_32x32x16_bf16,
// on the same (offsets, perm) lists that amk_moe_route writes and with the same a_div / g_div / x_div addressing.
// Operands bf16, accumulation f32, outputs f32 (Y feeds amk_moe_combine and amk_moe_gate_grad unchanged, dW and db are
// parameter gradients): nothing is rounded to bf16 on the way out.  No atomics, no workspace, one launch per entry
// point, nothing allocated or synchronised: bitwise reproducible and capturable.
//   nt  Y[p, :] = A[p / a_div, :] W[e]^T + bias[e]      unit = (expert, 256 outputs, 64 pairs); four waves, each all
//   nn  Y[p, :] = scale[p] (G[p / a_div, :] W[e])       64 pairs x 64 outputs (2 x 2 accumulators); contraction in
//       steps of 32.  The pair rows are gathered through perm into a [64][32] row-read image (16-byte chunks at
//       chunk ^ ((row >> 2) & 3): writes and ds_read_b128 conflict-free, as the NT kernel of gemm_bf16.hip); pairs
//       past the expert's count are staged as exact zeros.  nt: W[e] rows likewise, [256][32].  nn: the contraction
//       index is the row of W[e] as stored, so the [32][256] image (row stride 288: 144 dwords = 16 mod 64) is read with
//       ds_read_b64_tr_b16.  A pair's row is the same chain wherever the pair sits in its expert: the tile only decides
//       which accumulator register holds it.
//   wgrad  dW[e] = sum_p scale[p] G[p / g_div, :]^T (x) X[p / x_div, :], db[e] = sum_p scale[p] G[...]
//       unit = (expert, 128 n, 128 k); four waves as 2 x 2 of 64 x 64; the expert's pairs in steps of 32, both
//       operands staged as gathered -- [32 pairs][128] bf16, row stride 160 -- and read with ds_read_b64_tr_b16 (the
//       weight-gradient kernel of gemm_bf16.hip).  scale[p] G is rounded to bf16 once, at the LDS store; db is the
//       column sums of those staged values in f32 (k tile 0 only).  One workgroup owns a whole output tile: no split,
//       no partial sums; an expert without pairs writes exact zeros.
// Every operand piece goes through a range-checked buffer descriptor with its validity folded into the offset (absent
// pairs, rows and columns past the end, the tail of the contraction: an offset past the range reads zeros), so the
// tile loops have no branch around a memory instruction.  One register set is in flight beside the two LDS stages;
// 45 KB of static LDS and at most 128 VGPRs keep two to three workgroups on a CU, which is what hides the loads.
#include "amk_common.h"

namespace amk_moe16 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr unsigned PAST = 0x80000000u;   // beyond every descriptor's range (the host keeps all buffers below 2 GiB)
constexpr int TR = 64;                   // pairs per nt / nn tile
constexpr int BN = 256;                  // outputs per nt / nn tile
constexpr int BK = 32;                   // contraction step
constexpr int WSTR = BN + 32;            // nn: bf16 per row of the [32][256] weight image
constexpr int GSTR = 128 + 32;           // wgrad: bf16 per row of the [32][128] operand images

struct Params {
  const __bf16 *A, *X, *W;   // A: nt / nn input rows, wgrad G; X: wgrad only
  const float *bias, *scale;
  float *Y, *dbias;          // Y: (P, N) nt, (P, Kd) nn, dW (E, N, Kd) wgrad
  const int32_t *offsets, *perm;
  int E, N, Kd, ncol, ntk;
  int a_div, x_div, a_shift, x_shift;
  int64_t lda, ldx;
  unsigned a_bytes, x_bytes, s_bytes;
};

__device__ __forceinline__ void lds_barrier() {   // orders LDS only: global loads in flight stay in flight
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ bf16x4 tr_read(const __bf16* p) {
  const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  return __builtin_bit_cast(bf16x4, v);
}
// 32x32x16 operand whose contraction index is the ROW of the LDS image: lane (col = c0 + (l & 31), half) gets rows
// r0 + 8 half + (0..7)
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* img, int r0, int c0, int lane) {
  const int hf = lane >> 5, grp = (lane >> 4) & 1, q = (lane & 15) >> 2, pp = lane & 3;
  const __bf16* a = img + (r0 + 8 * hf + q) * STRIDE + c0 + 16 * grp + 4 * pp;
  const bf16x4 lo = tr_read(a), hi = tr_read(a + 4 * STRIDE);
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = lo[i]; r[4 + i] = hi[i]; }
  return r;
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int div_by(int p, int d, int sh) { return sh >= 0 ? p >> sh : p / d; }

// This workgroup's unit = (expert, output tile, 64-pair row tile), in the order [expert][output tile][row tile]: the row
// tiles that read one weight panel are neighbours, and the ids are remapped over the ACTUAL number of units (the grid is
// an upper bound, the surplus workgroups leave) so that neighbours run behind one L2.  Every wave decodes by itself:
// lane j holds expert j's tile count, one scan, one ballot.
__device__ __forceinline__ bool find_unit(const int32_t* offsets, int E, int ncol, int bid, int& e, int& ct, int& m0, int& cnt) {
  const int lane = threadIdx.x & 63;
  int total = 0;
  for (int base = 0; base < E; base += 64) {
    const int j = base + lane;
    const int c = j < E ? offsets[j + 1] - offsets[j] : 0;
    total += wave_sum((c + TR - 1) / TR);
  }
  total *= ncol;
  if (bid >= total) return false;
  int u = xcd_remap(bid, total);
  for (int base = 0; base < E; base += 64) {
    const int j = base + lane;
    const int c = j < E ? offsets[j + 1] - offsets[j] : 0;
    const int parts = (c + TR - 1) / TR;
    const int incl = wave_incl_scan(parts * ncol, lane);
    const int tot = __builtin_amdgcn_readlane(incl, 63);
    if (u < tot) {
      const int f = __builtin_ctzll(__ballot(incl > u));   // first expert whose running unit count passes u
      e = base + f;
      cnt = __shfl(c, f, 64);
      const int parts_e = __shfl(parts, f, 64);
      u -= __shfl(incl, f, 64) - parts_e * ncol;
      ct = u / parts_e;
      m0 = (u - ct * parts_e) * TR;
      return true;
    }
    u -= tot;
  }
  return false;
}

// nt (NN false): Y[p, n0 + c] = sum_k A[p / a_div, k] W[e, n0 + c, k] + bias[e, n0 + c], contraction length L = Kd
// nn (NN true):  Y[p, n0 + c] = scale[p] sum_n G[p / a_div, n] W[e, n, n0 + c],          contraction length L = N
template <bool NN>
__global__ __launch_bounds__(256, 2) void grouped_bf16_kernel(Params g) {
  constexpr int AT = TR * BK;                                 // elements of the pair image
  constexpr int STAGE = AT + (NN ? BK * WSTR : BN * BK);      // elements of one stage {pair image, weight image}
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  __shared__ int prow[TR];
  __shared__ float srow[TR];
  int e, ct, m0, cnt;
  if (!find_unit(g.offsets, g.E, g.ncol, blockIdx.x, e, ct, m0, cnt)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int OUT = NN ? g.Kd : g.N, L = NN ? g.N : g.Kd;      // output row length, contraction length
  const int n0 = ct * BN;
  if (tid < TR) {
    const int p = (m0 + tid < cnt) ? g.perm[g.offsets[e] + m0 + tid] : -1;
    prow[tid] = p;
    srow[tid] = (NN && g.scale && p >= 0) ? g.scale[p] : 1.f;
  }
  __syncthreads();
  const __bf16* We = g.W + (int64_t)e * g.N * g.Kd;
  const __amdgpu_buffer_rsrc_t a_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)g.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)We, 0, (int)((int64_t)g.N * g.Kd * 2), 0x00020000);
  // staging.  Pair image and the nt weight image: pieces (row ar + 64 i, 8 contraction elements at 8 ach).  The nn weight
  // image: pieces (contraction row sr + 8 i, 8 outputs at 8 cg).
  const int ar = tid >> 2, ach = tid & 3;
  const int cg = tid & 31, sr = tid >> 5;
  unsigned aoff, woff[4];
  {
    const int p = prow[ar];
    aoff = p >= 0 ? (unsigned)(((int64_t)div_by(p, g.a_div, g.a_shift) * g.lda + 8 * ach) * 2) : PAST;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (NN) {
      const int col = n0 + 8 * cg;
      woff[i] = col < OUT ? (unsigned)(((int64_t)(sr + 8 * i) * g.Kd + col) * 2) : PAST;
    } else {
      const int n = n0 + ar + 64 * i;
      woff[i] = n < OUT ? (unsigned)(((int64_t)n * g.Kd + 8 * ach) * 2) : PAST;
    }
  }
  const unsigned wstep = NN ? (unsigned)(BK * g.Kd * 2) : (unsigned)(BK * 2);
  struct Stg { float4 a, w[4]; };
  auto gload = [&](Stg& s, int t) {   // (steps past the contraction: every piece reads zeros)
    const bool kin = BK * t + 8 * ach < L;   // (L a multiple of 8: a piece is in or out)
    s.a = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, (int)((kin && aoff != PAST) ? aoff + (unsigned)t * (BK * 2) : PAST), 0, 0));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool win = woff[i] != PAST && (NN ? BK * t + sr + 8 * i < L : kin);
      s.w[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(w_rs, (int)(win ? woff[i] + (unsigned)t * wstep : PAST), 0, 0));
    }
  };
  const int swz = 8 * (ach ^ ((ar >> 2) & 3));   // (rows ar + 64 i: the same swizzle)
  auto lstore = [&](__bf16* stage, const Stg& s) {
    *reinterpret_cast<float4*>(&stage[ar * BK + swz]) = s.a;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (NN) *reinterpret_cast<float4*>(&stage[AT + (sr + 8 * i) * WSTR + 8 * cg]) = s.w[i];
      else *reinterpret_cast<float4*>(&stage[AT + (ar + 64 * i) * BK + swz]) = s.w[i];
    }
  };
  f32x16 acc[2][2];   // [pair block][output block]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  const int nk = (L + BK - 1) / BK;
  Stg st;
  gload(st, 0);
  lstore(smem, st);
  gload(st, 1);
  lds_barrier();
  for (int t = 0; t < nk; ++t) {
    const __bf16* cur = smem + (t & 1) * STAGE;
    lstore(smem + ((t + 1) & 1) * STAGE, st);   // tile t + 1 -> the other stage; then fetch tile t + 2
    gload(st, t + 2);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      const int sw = 8 * ((2 * s + hf) ^ ((ln >> 2) & 3));   // (row offsets are multiples of 32: the swizzle of ln)
      bf16x8 af[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const bf16x8*>(&cur[(32 * i + ln) * BK + sw]);
        wf[i] = NN ? tr_frag<WSTR>(cur + AT, 16 * s, 64 * wave + 32 * i, lane)
                   : *reinterpret_cast<const bf16x8*>(&cur[AT + (64 * wave + 32 * i + ln) * BK + sw]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], wf[j], acc[i][j], 0, 0, 0);
    }
    lds_barrier();
  }
  // acc[i][j][r] = Y[prow[32 i + acc_row(r, hf)]][n0 + 64 wave + 32 j + ln]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + 64 * wave + 32 * j + ln;
    if (n < OUT) {
      const float bv = (!NN && g.bias) ? g.bias[(int64_t)e * g.N + n] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * i + acc_row(r, hf);
          const int p = prow[row];
          if (p >= 0) g.Y[(int64_t)p * OUT + n] = NN ? acc[i][j][r] * srow[row] : acc[i][j][r] + bv;
        }
    }
  }
}

// dW[e, n0 + a, k0 + b] = sum over the expert's pairs of bf16(scale[p] G[p / g_div, n0 + a]) X[p / x_div, k0 + b]
template <bool HAS_SCALE>
__global__ __launch_bounds__(256, 2) void grouped_wgrad_bf16_kernel(Params g) {
  constexpr int BP = 32, TN = 128, IMG = BP * GSTR, STAGE = 2 * IMG;   // {G image, X image}
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int wn = wave >> 1, wk = wave & 1;
  const int ntn = (g.N + TN - 1) / TN;
  const int total = g.E * ntn * g.ntk;
  const int u = xcd_remap(blockIdx.x, total);
  // unit order (expert, n tile, k tile): the k tiles that read the same G panel are neighbours
  const int tk = u % g.ntk, rest = u / g.ntk;
  const int e = rest / ntn, tn = rest - e * ntn;
  const int n0 = tn * TN, k0 = tk * TN;
  const int beg = g.offsets[e], cnt = g.offsets[e + 1] - beg;
  const int nk = (cnt + BP - 1) / BP;
  const __amdgpu_buffer_rsrc_t p_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(g.perm + beg), 0, cnt * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t g_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)g.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.X, 0, (int)g.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.scale, 0, HAS_SCALE ? (int)g.s_bytes : 0, 0x00020000);
  // staging: thread -> column group (8 columns) of both images, pair rows sr and sr + 16 of the step
  const int cg = tid & 15, sr = tid >> 4;
  const bool gok = n0 + 8 * cg < g.N, xok = k0 + 8 * cg < g.Kd;   // (N and Kd multiples of 8: a piece is in or out)
  struct Stg { float4 gv[2], xv[2]; float sc[2]; };
  int pn[2];
  auto pload = [&](int t) {   // (rows past the expert's count: past the descriptor's range, 0 -- and never used)
#pragma unroll
    for (int i = 0; i < 2; ++i) pn[i] = __builtin_amdgcn_raw_buffer_load_b32(p_rs, (BP * t + sr + 16 * i) * 4, 0, 0);
  };
  auto gload = [&](Stg& s, int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool in = BP * t + sr + 16 * i < cnt;
      const unsigned go = (unsigned)(((int64_t)div_by(pn[i], g.a_div, g.a_shift) * g.lda + n0 + 8 * cg) * 2);
      const unsigned xo = (unsigned)(((int64_t)div_by(pn[i], g.x_div, g.x_shift) * g.ldx + k0 + 8 * cg) * 2);
      s.gv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(g_rs, (int)((in && gok) ? go : PAST), 0, 0));
      s.xv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)((in && xok) ? xo : PAST), 0, 0));
      if (HAS_SCALE) s.sc[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(s_rs, (int)(in ? (unsigned)pn[i] * 4u : PAST), 0, 0));
    }
  };
  const bool do_bias = g.dbias != nullptr && tk == 0;
  float bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;
  auto lstore = [&](__bf16* stage, const Stg& s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x8 v = __builtin_bit_cast(bf16x8, s.gv[i]);
      if (HAS_SCALE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)((float)v[j] * s.sc[i]);   // the one bf16 rounding of scale x G
      }
      *reinterpret_cast<bf16x8*>(&stage[(sr + 16 * i) * GSTR + 8 * cg]) = v;
      if (do_bias) {   // (absent pairs carry zeros)
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += (float)v[j];
      }
      *reinterpret_cast<float4*>(&stage[IMG + (sr + 16 * i) * GSTR + 8 * cg]) = s.xv[i];
    }
  };
  f32x16 acc[2][2];   // [n block][k block]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  Stg st;
  pload(0);
  gload(st, 0);
  pload(1);
  lstore(smem, st);
  gload(st, 1);
  pload(2);
  lds_barrier();
  for (int t = 0; t < nk; ++t) {
    const __bf16* cur = smem + (t & 1) * STAGE;
    lstore(smem + ((t + 1) & 1) * STAGE, st);   // step t + 1 -> the other stage; fetch step t + 2, the pair ids of t + 3
    gload(st, t + 2);
    pload(t + 3);
#pragma unroll
    for (int s = 0; s < BP / 16; ++s) {
      const bf16x8 a0 = tr_frag<GSTR>(cur, 16 * s, 64 * wn, lane), a1 = tr_frag<GSTR>(cur, 16 * s, 64 * wn + 32, lane);
      const bf16x8 b0 = tr_frag<GSTR>(cur + IMG, 16 * s, 64 * wk, lane), b1 = tr_frag<GSTR>(cur + IMG, 16 * s, 64 * wk + 32, lane);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
    }
    lds_barrier();
  }
  // acc[i][j][r] = dW[e][n0 + 64 wn + 32 i + acc_row(r, hf)][k0 + 64 wk + 32 j + ln]
  float* dWe = g.Y + (int64_t)e * g.N * g.Kd;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kc = k0 + 64 * wk + 32 * j + ln;
      if (kc < g.Kd) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + 64 * wn + 32 * i + acc_row(r, hf);
          if (n < g.N) dWe[(int64_t)n * g.Kd + kc] = acc[i][j][r];
        }
      }
    }
  if (do_bias) {   // fold the 16 row groups of each column group, in row-group order
    float* red = reinterpret_cast<float*>(smem);   // (the loop, or the prologue, ended with a barrier)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[sr * TN + 8 * cg + j] = bsum[j];
    lds_barrier();
    if (tid < TN) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += red[r * TN + tid];
      if (n0 + tid < g.N) g.dbias[(int64_t)e * g.N + n0 + tid] = s;
    }
  }
}

}  // namespace amk_moe16

using namespace amk_moe16;

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int log2_of(int d) {
  int s = 0;
  while ((1 << s) < d) ++s;
  return (1 << s) == d ? s : -1;
}
constexpr int64_t TWO_GIB = 1ll << 31;

// shared checks; `width` is the row length of the gathered operand (Kd for nt, N for nn)
static int check_common(const char* who, const void* A, const void* W, const void* Y, const void* offsets, const void* perm,
                        int64_t P, int E, int N, int Kd, int a_div, int64_t lda, int width) {
  AMK_CHECK_ARG(A && W && Y && offsets && perm, "%s: null pointer", who);
  AMK_CHECK_ARG(P > 0 && E > 0 && N > 0 && Kd > 0 && a_div > 0, "%s: non-positive size P=%lld E=%d N=%d Kd=%d", who, (long long)P, E, N, Kd);
  AMK_CHECK_SUPPORTED(N % 8 == 0 && Kd % 8 == 0, "%s: N=%d and Kd=%d must be multiples of 8", who, N, Kd);
  AMK_CHECK_SUPPORTED(E <= 1024, "%s: at most 1024 experts", who);
  AMK_CHECK_ARG(al16(A) && al16(W) && al16(Y), "%s: pointers must be 16-byte aligned", who);
  AMK_CHECK_ARG(lda % 8 == 0 && lda >= width, "%s: row stride %lld must be a multiple of 8 and at least %d", who, (long long)lda, width);
  AMK_CHECK_SUPPORTED(P < TWO_GIB && (int64_t)N * Kd * 2 < TWO_GIB, "%s: too many pairs or one expert's weights beyond 2 GiB", who);
  return AMK_OK;
}

static int grouped_impl(bool nn, const char* who, const void* A, int64_t lda, int a_div, const void* W, const float* vec,
                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd, float* Y, void* stream) {
  const int width = nn ? N : Kd, out = nn ? Kd : N;
  const int rc = check_common(who, A, W, Y, offsets, perm, P, E, N, Kd, a_div, lda, width);
  if (rc) return rc;
  AMK_CHECK_ARG(al16(vec), "%s: pointers must be 16-byte aligned", who);
  const int64_t a_bytes = ((P - 1) / a_div * lda + width) * 2;
  AMK_CHECK_SUPPORTED(a_bytes < TWO_GIB && P * out * 4 < TWO_GIB, "%s: every buffer must stay below 2 GiB", who);
  Params g{};
  g.A = static_cast<const __bf16*>(A); g.W = static_cast<const __bf16*>(W); g.Y = Y; g.offsets = offsets; g.perm = perm;
  if (nn) g.scale = vec; else g.bias = vec;
  g.E = E; g.N = N; g.Kd = Kd; g.a_div = a_div; g.a_shift = log2_of(a_div); g.lda = lda; g.a_bytes = (unsigned)a_bytes;
  g.ncol = (out + BN - 1) / BN;
  const int64_t grid = ((P + TR - 1) / TR + E) * g.ncol;   // an upper bound of the units; the surplus workgroups leave at once
  AMK_CHECK_SUPPORTED(grid < TWO_GIB, "%s: grid too large", who);
  if (nn) hipLaunchKernelGGL(grouped_bf16_kernel<true>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), g);
  else hipLaunchKernelGGL(grouped_bf16_kernel<false>, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), g);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

extern "C" int amk_grouped_gemm_nt_bf16(const void* A, int64_t lda, int a_div, const void* W, const float* bias,
                                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                        float* Y, void* stream) {
  return grouped_impl(false, "amk_grouped_gemm_nt_bf16", A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd, Y, stream);
}

extern "C" int amk_grouped_gemm_nn_bf16(const void* G, int64_t ldg, int a_div, const void* W, const float* scale,
                                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                        float* Y, void* stream) {
  return grouped_impl(true, "amk_grouped_gemm_nn_bf16", G, ldg, a_div, W, scale, offsets, perm, P, E, N, Kd, Y, stream);
}

extern "C" int amk_grouped_gemm_wgrad_bf16(const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                                           const float* scale, const int32_t* offsets, const int32_t* perm,
                                           int64_t P, int E, int N, int Kd, float* dW, float* dbias, void* stream) {
  const char* who = "amk_grouped_gemm_wgrad_bf16";
  const int rc = check_common(who, G, X, dW, offsets, perm, P, E, N, Kd, g_div, ldg, N);
  if (rc) return rc;
  AMK_CHECK_ARG(x_div > 0, "%s: non-positive size x_div=%d", who, x_div);
  AMK_CHECK_ARG(al16(scale) && al16(dbias), "%s: pointers must be 16-byte aligned", who);
  AMK_CHECK_ARG(ldx % 8 == 0 && ldx >= Kd, "%s: row stride %lld must be a multiple of 8 and at least %d", who, (long long)ldx, Kd);
  const int64_t g_bytes = ((P - 1) / g_div * ldg + N) * 2, x_bytes = ((P - 1) / x_div * ldx + Kd) * 2;
  AMK_CHECK_SUPPORTED(g_bytes < TWO_GIB && x_bytes < TWO_GIB && P * 4 < TWO_GIB, "%s: every buffer must stay below 2 GiB", who);
  Params g{};
  g.A = static_cast<const __bf16*>(G); g.X = static_cast<const __bf16*>(X); g.scale = scale; g.Y = dW; g.dbias = dbias;
  g.offsets = offsets; g.perm = perm;
  g.E = E; g.N = N; g.Kd = Kd; g.a_div = g_div; g.x_div = x_div; g.a_shift = log2_of(g_div); g.x_shift = log2_of(x_div);
  g.lda = ldg; g.ldx = ldx; g.a_bytes = (unsigned)g_bytes; g.x_bytes = (unsigned)x_bytes; g.s_bytes = (unsigned)(P * 4);
  g.ntk = (Kd + 127) / 128;
  const int64_t grid = (int64_t)E * ((N + 127) / 128) * g.ntk;
  AMK_CHECK_SUPPORTED(grid < TWO_GIB, "%s: grid too large", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (scale) hipLaunchKernelGGL(grouped_wgrad_bf16_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(grouped_wgrad_bf16_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, g);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}
