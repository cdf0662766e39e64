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
// SwitchHead's experts (V experts (E, 64, dim), output experts (E, dim, 64): one side at most 64 wide) take the same
// two kernels in a narrow tile form -- amk_grouped_gemm_nt64 / nn64 / wgrad64_bf16 -- in which no wave multiplies zeros:
//   nt64 / nn64  unit = (expert, 256 pairs), all (<= 64) outputs; the four waves split the PAIRS, 64 x 64 each, and share
//       one [64][32] (nt) or [32][64] (nn, row stride 96: 48 dwords, the rows of a transposing read 16 dwords apart mod
//       64) weight image per contraction step.  The chain of a row is that of the wide form.
//   wgrad64  tiles of 64 n x 128 k (N <= 64; waves 1 x 4 of 64 x 32) or 128 n x 64 k (Kd <= 64; 4 x 1 of 32 x 64): as
//       many workgroups as the 128 x 128 form starts at these shapes, each with half the staging and half the MFMAs.
//   amk_moe_expert_sums_bf16: expert_sums_kernel of csrc/moe.hip -- the same f32 sums in the same order -- reading f32
//       or bf16 rows and rounding Z to bf16 once at the store.
// Every operand piece goes through a range-checked buffer descriptor with its validity folded into the offset (absent
// pairs, rows and columns past the end, the tail of the contraction: an offset past the range reads zeros), so the
// tile loops have no branch around a memory instruction.  One register set is in flight beside the two LDS stages;
// 45 KB of static LDS and at most 128 VGPRs keep two to three workgroups on a CU, which is what hides the loads.
#include "amk_bf16.h"

namespace amk_moe16 {

constexpr unsigned PAST = 0x80000000u;   // beyond every descriptor's range (the host keeps all buffers below 2 GiB)
constexpr int BK = 32;                   // contraction step
// nt / nn tile: 64 pairs x 256 outputs, the four waves over the outputs; NARROW: 256 pairs x 64 outputs, over the pairs
template <bool NARROW> struct Tile {
  static constexpr int TR = NARROW ? 256 : 64;   // pairs
  static constexpr int BN = NARROW ? 64 : 256;   // outputs
  static constexpr int WSTR = BN + 32;           // nn: bf16 per row of the [32][BN] weight image
};

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

__device__ __forceinline__ int div_by(int p, int d, int sh) { return sh >= 0 ? p >> sh : p / d; }

// This workgroup's unit = (expert, output tile, TR-pair row tile), in the order [expert][output tile][row tile]: the row
// tiles that read one weight panel are neighbours, and the ids are remapped over the ACTUAL number of units (the grid is
// an upper bound, the surplus workgroups leave) so that neighbours run behind one L2.  Every wave decodes by itself:
// lane j holds expert j's tile count, one scan, one ballot.
template <int TR>
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
template <bool NN, bool NARROW>
__global__ __launch_bounds__(256, 2) void grouped_bf16_kernel(Params g) {
  constexpr int TR = Tile<NARROW>::TR, BN = Tile<NARROW>::BN, WSTR = Tile<NARROW>::WSTR;
  constexpr int NA = TR / 64, NW = BN / 64;                   // 16-byte pieces per thread of the pair / weight image
  constexpr int WCG = BN / 8, WRS = 256 / WCG;                // nn weight image: column groups, rows per pass
  constexpr int AT = TR * BK;                                 // elements of the pair image
  constexpr int STAGE = AT + (NN ? BK * WSTR : BN * BK);      // elements of one stage {pair image, weight image}
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  __shared__ int prow[TR];
  __shared__ float srow[TR];
  int e, ct, m0, cnt;
  if (!find_unit<TR>(g.offsets, g.E, g.ncol, blockIdx.x, e, ct, m0, cnt)) return;
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
  // image: pieces (contraction row sr + WRS i, 8 outputs at 8 cg).
  const int ar = tid >> 2, ach = tid & 3;
  const int cg = tid % WCG, sr = tid / WCG;
  unsigned aoff[NA], woff[NW];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int p = prow[ar + 64 * i];
    aoff[i] = p >= 0 ? (unsigned)(((int64_t)div_by(p, g.a_div, g.a_shift) * g.lda + 8 * ach) * 2) : PAST;
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    if (NN) {
      const int col = n0 + 8 * cg;
      woff[i] = col < OUT ? (unsigned)(((int64_t)(sr + WRS * i) * g.Kd + col) * 2) : PAST;
    } else {
      const int n = n0 + ar + 64 * i;
      woff[i] = n < OUT ? (unsigned)(((int64_t)n * g.Kd + 8 * ach) * 2) : PAST;
    }
  }
  const unsigned wstep = NN ? (unsigned)(BK * g.Kd * 2) : (unsigned)(BK * 2);
  struct Stg { float4 a[NA], w[NW]; };
  auto gload = [&](Stg& s, int t) {   // (steps past the contraction: every piece reads zeros)
    const bool kin = BK * t + 8 * ach < L;   // (L a multiple of 8: a piece is in or out)
#pragma unroll
    for (int i = 0; i < NA; ++i)
      s.a[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(a_rs, (int)((kin && aoff[i] != PAST) ? aoff[i] + (unsigned)t * (BK * 2) : PAST), 0, 0));
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const bool win = woff[i] != PAST && (NN ? BK * t + sr + WRS * i < L : kin);
      s.w[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(w_rs, (int)(win ? woff[i] + (unsigned)t * wstep : PAST), 0, 0));
    }
  };
  const int swz = 8 * (ach ^ ((ar >> 2) & 3));   // (rows ar + 64 i: the same swizzle)
  auto lstore = [&](__bf16* stage, const Stg& s) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<float4*>(&stage[(ar + 64 * i) * BK + swz]) = s.a[i];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      if (NN) *reinterpret_cast<float4*>(&stage[AT + (sr + WRS * i) * WSTR + 8 * cg]) = s.w[i];
      else *reinterpret_cast<float4*>(&stage[AT + (ar + 64 * i) * BK + swz]) = s.w[i];
    }
  };
  const int pb = NARROW ? 64 * wave : 0, ob = NARROW ? 0 : 64 * wave;   // this wave's 64 pairs x 64 outputs of the tile
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
        af[i] = *reinterpret_cast<const bf16x8*>(&cur[(pb + 32 * i + ln) * BK + sw]);
        wf[i] = NN ? tr_frag<WSTR>(cur + AT, 16 * s, ob + 32 * i, lane)
                   : *reinterpret_cast<const bf16x8*>(&cur[AT + (ob + 32 * i + ln) * BK + sw]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], wf[j], acc[i][j], 0, 0, 0);
    }
    lds_barrier();
  }
  // acc[i][j][r] = Y[prow[pb + 32 i + acc_row(r, hf)]][n0 + ob + 32 j + ln]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + ob + 32 * j + ln;
    if (n < OUT) {
      const float bv = (!NN && g.bias) ? g.bias[(int64_t)e * g.N + n] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = pb + 32 * i + acc_row(r, hf);
          const int p = prow[row];
          if (p >= 0) g.Y[(int64_t)p * OUT + n] = NN ? acc[i][j][r] * srow[row] : acc[i][j][r] + bv;
        }
    }
  }
}

// dW[e, n0 + a, k0 + b] = sum over the expert's pairs of bf16(scale[p] G[p / g_div, n0 + a]) X[p / x_div, k0 + b]
// Tile TN x TK of dW[e], the four waves as WN x (4 / WN): 128 x 128 as 2 x 2 (the wide form), 64 x 128 as 1 x 4 and
// 128 x 64 as 4 x 1 (the narrow forms).
template <int TN, int TK, int WN, bool HAS_SCALE>
__global__ __launch_bounds__(256, 2) void grouped_wgrad_bf16_kernel(Params g) {
  constexpr int BP = 32, GSTR = TN + 32, XSTR = TK + 32, IMG = BP * GSTR, STAGE = IMG + BP * XSTR;   // {G image, X image}
  constexpr int WK = 4 / WN, WTN = TN / WN, WTK = TK / WK, BI = WTN / 32, BJ = WTK / 32;             // wave tile, its blocks
  constexpr int NG = TN / 64, NX = TK / 64;                        // 16-byte pieces per thread of the G / X image
  constexpr int GCG = TN / 8, GRS = 256 / GCG, XCG = TK / 8, XRS = 256 / XCG;   // column groups, pair rows per pass
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, hf = lane >> 5;
  const int wn = wave / WK, wk = wave % WK;
  const int ntn = (g.N + TN - 1) / TN;
  const int total = g.E * ntn * g.ntk;
  const int u = xcd_remap(blockIdx.x, total);
  // unit order (expert, n tile, k tile): the k tiles that read the same G panel are neighbours
  const int tk = u % g.ntk, rest = u / g.ntk;
  const int e = rest / ntn, tn = rest - e * ntn;
  const int n0 = tn * TN, k0 = tk * TK;
  const int beg = g.offsets[e], cnt = g.offsets[e + 1] - beg;
  const int nk = (cnt + BP - 1) / BP;
  const __amdgpu_buffer_rsrc_t p_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(g.perm + beg), 0, cnt * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t g_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)g.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.X, 0, (int)g.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t s_rs = __builtin_amdgcn_make_buffer_rsrc((void*)g.scale, 0, HAS_SCALE ? (int)g.s_bytes : 0, 0x00020000);
  // staging: thread -> column group (8 columns) of each image, pair rows gr + GRS i (G) and xr + XRS i (X) of the step
  const int gc = tid % GCG, gr = tid / GCG, xc = tid % XCG, xr = tid / XCG;
  const bool gok = n0 + 8 * gc < g.N, xok = k0 + 8 * xc < g.Kd;   // (N and Kd multiples of 8: a piece is in or out)
  struct Stg { float4 gv[NG], xv[NX]; float sc[NG]; };
  int pg[NG], px[NX];
  auto pload = [&](int t) {   // (rows past the expert's count: past the descriptor's range, 0 -- and never used)
#pragma unroll
    for (int i = 0; i < NG; ++i) pg[i] = __builtin_amdgcn_raw_buffer_load_b32(p_rs, (BP * t + gr + GRS * i) * 4, 0, 0);
#pragma unroll
    for (int i = 0; i < NX; ++i) px[i] = __builtin_amdgcn_raw_buffer_load_b32(p_rs, (BP * t + xr + XRS * i) * 4, 0, 0);
  };
  auto gload = [&](Stg& s, int t) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const bool in = BP * t + gr + GRS * i < cnt;
      const unsigned go = (unsigned)(((int64_t)div_by(pg[i], g.a_div, g.a_shift) * g.lda + n0 + 8 * gc) * 2);
      s.gv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(g_rs, (int)((in && gok) ? go : PAST), 0, 0));
      if (HAS_SCALE) s.sc[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(s_rs, (int)(in ? (unsigned)pg[i] * 4u : PAST), 0, 0));
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const bool in = BP * t + xr + XRS * i < cnt;
      const unsigned xo = (unsigned)(((int64_t)div_by(px[i], g.x_div, g.x_shift) * g.ldx + k0 + 8 * xc) * 2);
      s.xv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(x_rs, (int)((in && xok) ? xo : PAST), 0, 0));
    }
  };
  const bool do_bias = g.dbias != nullptr && tk == 0;
  float bsum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum[j] = 0.f;
  auto lstore = [&](__bf16* stage, const Stg& s) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      bf16x8 v = __builtin_bit_cast(bf16x8, s.gv[i]);
      if (HAS_SCALE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)((float)v[j] * s.sc[i]);   // the one bf16 rounding of scale x G
      }
      *reinterpret_cast<bf16x8*>(&stage[(gr + GRS * i) * GSTR + 8 * gc]) = v;
      if (do_bias) {   // (absent pairs carry zeros)
#pragma unroll
        for (int j = 0; j < 8; ++j) bsum[j] += (float)v[j];
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) *reinterpret_cast<float4*>(&stage[IMG + (xr + XRS * i) * XSTR + 8 * xc]) = s.xv[i];
  };
  f32x16 acc[BI][BJ];   // [n block][k block]
#pragma unroll
  for (int i = 0; i < BI; ++i)
#pragma unroll
    for (int j = 0; j < BJ; ++j) acc[i][j] = zero16();
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
      bf16x8 a[BI], b[BJ];
#pragma unroll
      for (int i = 0; i < BI; ++i) a[i] = tr_frag<GSTR>(cur, 16 * s, WTN * wn + 32 * i, lane);
#pragma unroll
      for (int j = 0; j < BJ; ++j) b[j] = tr_frag<XSTR>(cur + IMG, 16 * s, WTK * wk + 32 * j, lane);
#pragma unroll
      for (int i = 0; i < BI; ++i)
#pragma unroll
        for (int j = 0; j < BJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    lds_barrier();
  }
  // acc[i][j][r] = dW[e][n0 + WTN wn + 32 i + acc_row(r, hf)][k0 + WTK wk + 32 j + ln]
  float* dWe = g.Y + (int64_t)e * g.N * g.Kd;
#pragma unroll
  for (int i = 0; i < BI; ++i)
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int kc = k0 + WTK * wk + 32 * j + ln;
      if (kc < g.Kd) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + WTN * wn + 32 * i + acc_row(r, hf);
          if (n < g.N) dWe[(int64_t)n * g.Kd + kc] = acc[i][j][r];
        }
      }
    }
  if (do_bias) {   // fold the GRS row groups of each column group, in row-group order
    float* red = reinterpret_cast<float*>(smem);   // (the loop, or the prologue, ended with a barrier)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[gr * TN + 8 * gc + j] = bsum[j];
    lds_barrier();
    if (tid < TN) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < GRS; ++r) s += red[r * TN + tid];
      if (n0 + tid < g.N) g.dbias[(int64_t)e * g.N + n0 + tid] = s;
    }
  }
}

// Z[g, e, :] = bf16(sum over the fan pairs of row g that chose expert e of scale[p] A[p / a_div, :]): expert_sums_kernel
// of csrc/moe.hip (one workgroup per row, the row's pairs sorted by expert, each output walking its expert's pairs in
// ascending order with the same f32 multiply-add) on 8 columns per thread, A in f32 or bf16, one rounding at the store.
template <bool A16>
__global__ __launch_bounds__(256) void expert_sums_bf16_kernel(const void* __restrict__ A, int64_t lda, int a_div,
                                                               const int64_t* __restrict__ ids, const float* __restrict__ scale,
                                                               int fan, int E, int d, __bf16* __restrict__ Z) {
  extern __shared__ int es_lds[];
  int* sid = es_lds;                                       // [fan] expert of pair j
  float* ssc = reinterpret_cast<float*>(es_lds + fan);     // [fan] its scale
  int* order = es_lds + 2 * fan;                           // [fan] the pairs sorted by expert (stable: ascending j)
  int* start = es_lds + 3 * fan;                           // [E + 1] first entry of an expert in `order`
  const int64_t g = blockIdx.x, p0 = g * fan;
  for (int j = threadIdx.x; j < fan; j += 256) {
    sid[j] = (int)ids[p0 + j];
    ssc[j] = scale ? scale[p0 + j] : 1.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += 256) {
    int first = 0, mine = 0;
    for (int j = 0; j < fan; ++j) { first += sid[j] < e; mine += sid[j] == e; }
    start[e] = first;
    if (e == E - 1) start[E] = first + mine;
    for (int j = 0; j < fan; ++j)
      if (sid[j] == e) order[first++] = j;
  }
  __syncthreads();
  const int dv = d >> 3, nv = E * dv;
  for (int idx = threadIdx.x; idx < nv; idx += 256) {
    const int e = idx / dv, c = (idx - e * dv) * 8;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    for (int i = start[e]; i < start[e + 1]; ++i) {
      const int j = order[i];
      const float w = ssc[j];
      const int64_t at = ((p0 + j) / a_div) * lda + c;
      float a[8];
      if (A16) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(static_cast<const __bf16*>(A) + at);
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = (float)v[q];
      } else {
        const float4 lo = *reinterpret_cast<const float4*>(static_cast<const float*>(A) + at);
        const float4 hi = *reinterpret_cast<const float4*>(static_cast<const float*>(A) + at + 4);
        a[0] = lo.x; a[1] = lo.y; a[2] = lo.z; a[3] = lo.w; a[4] = hi.x; a[5] = hi.y; a[6] = hi.z; a[7] = hi.w;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += w * a[q];
    }
    bf16x8 z;
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = (__bf16)acc[q];
    *reinterpret_cast<bf16x8*>(Z + g * (int64_t)E * d + (int64_t)idx * 8) = z;
  }
}

}  // namespace amk_moe16

using namespace amk_moe16;

constexpr int64_t TWO_GIB = 1ll << 31;

// shared checks; `width` is the row length of the gathered operand (Kd for nt, N for nn)
static int check_common(const char* who, const void* A, const void* W, const void* Y, const void* offsets, const void* perm,
                        int64_t P, int E, int N, int Kd, int a_div, int64_t lda, int width) {
  AMK_CHECK_ARG(A && W && Y && offsets && perm, "%s: null pointer", who);
  AMK_CHECK_ARG(P > 0 && E > 0 && N > 0 && Kd > 0 && a_div > 0, "%s: non-positive size P=%lld E=%d N=%d Kd=%d", who, (long long)P, E, N, Kd);
  AMK_CHECK_SUPPORTED(N % 8 == 0 && Kd % 8 == 0, "%s: N=%d and Kd=%d must be multiples of 8", who, N, Kd);
  AMK_CHECK_SUPPORTED(E <= 1024, "%s: at most 1024 experts", who);
  AMK_CHECK_ARG(a16(A) && a16(W) && a16(Y), "%s: pointers must be 16-byte aligned", who);
  AMK_CHECK_ARG(lda % 8 == 0 && lda >= width, "%s: row stride %lld must be a multiple of 8 and at least %d", who, (long long)lda, width);
  AMK_CHECK_SUPPORTED(P < TWO_GIB && (int64_t)N * Kd * 2 < TWO_GIB, "%s: too many pairs or one expert's weights beyond 2 GiB", who);
  return AMK_OK;
}

static int grouped_impl(bool nn, bool narrow, const char* who, const void* A, int64_t lda, int a_div, const void* W, const float* vec,
                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd, float* Y, void* stream) {
  const int width = nn ? N : Kd, out = nn ? Kd : N;
  const int rc = check_common(who, A, W, Y, offsets, perm, P, E, N, Kd, a_div, lda, width);
  if (rc) return rc;
  AMK_CHECK_SUPPORTED(!narrow || out <= 64, "%s: at most 64 outputs (%s=%d); the wide entry point takes more", who, nn ? "Kd" : "N", out);
  AMK_CHECK_ARG(a16(vec), "%s: pointers must be 16-byte aligned", who);
  const int64_t a_bytes = ((P - 1) / a_div * lda + width) * 2;
  AMK_CHECK_SUPPORTED(a_bytes < TWO_GIB && P * out * 4 < TWO_GIB, "%s: every buffer must stay below 2 GiB", who);
  Params g{};
  g.A = static_cast<const __bf16*>(A); g.W = static_cast<const __bf16*>(W); g.Y = Y; g.offsets = offsets; g.perm = perm;
  if (nn) g.scale = vec; else g.bias = vec;
  g.E = E; g.N = N; g.Kd = Kd; g.a_div = a_div; g.a_shift = log2_of(a_div); g.lda = lda; g.a_bytes = (unsigned)a_bytes;
  const int TR = narrow ? Tile<true>::TR : Tile<false>::TR, BN = narrow ? Tile<true>::BN : Tile<false>::BN;
  g.ncol = (out + BN - 1) / BN;
  const int64_t grid = ((P + TR - 1) / TR + E) * g.ncol;   // an upper bound of the units; the surplus workgroups leave at once
  AMK_CHECK_SUPPORTED(grid < TWO_GIB, "%s: grid too large", who);
  const dim3 gd((unsigned)grid), bd(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (narrow) {
    if (nn) hipLaunchKernelGGL((grouped_bf16_kernel<true, true>), gd, bd, 0, st, g);
    else hipLaunchKernelGGL((grouped_bf16_kernel<false, true>), gd, bd, 0, st, g);
  } else {
    if (nn) hipLaunchKernelGGL((grouped_bf16_kernel<true, false>), gd, bd, 0, st, g);
    else hipLaunchKernelGGL((grouped_bf16_kernel<false, false>), gd, bd, 0, st, g);
  }
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

extern "C" int amk_grouped_gemm_nt_bf16(const void* A, int64_t lda, int a_div, const void* W, const float* bias,
                                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                        float* Y, void* stream) {
  return grouped_impl(false, false, "amk_grouped_gemm_nt_bf16", A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd, Y, stream);
}

extern "C" int amk_grouped_gemm_nn_bf16(const void* G, int64_t ldg, int a_div, const void* W, const float* scale,
                                        const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                        float* Y, void* stream) {
  return grouped_impl(true, false, "amk_grouped_gemm_nn_bf16", G, ldg, a_div, W, scale, offsets, perm, P, E, N, Kd, Y, stream);
}

// narrow: tiles of 64 x 128 (N <= 64) or 128 x 64 (Kd <= 64) instead of 128 x 128
static int wgrad_impl(bool narrow, const char* who, const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                      const float* scale, const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                      float* dW, float* dbias, void* stream) {
  const int rc = check_common(who, G, X, dW, offsets, perm, P, E, N, Kd, g_div, ldg, N);
  if (rc) return rc;
  AMK_CHECK_SUPPORTED(!narrow || N <= 64 || Kd <= 64, "%s: N=%d or Kd=%d must be at most 64; the wide entry point takes both wider", who, N, Kd);
  const int tile = !narrow ? 0 : N <= 64 ? 1 : 2;
  AMK_CHECK_ARG(x_div > 0, "%s: non-positive size x_div=%d", who, x_div);
  AMK_CHECK_ARG(a16(scale) && a16(dbias), "%s: pointers must be 16-byte aligned", who);
  AMK_CHECK_ARG(ldx % 8 == 0 && ldx >= Kd, "%s: row stride %lld must be a multiple of 8 and at least %d", who, (long long)ldx, Kd);
  const int64_t g_bytes = ((P - 1) / g_div * ldg + N) * 2, x_bytes = ((P - 1) / x_div * ldx + Kd) * 2;
  AMK_CHECK_SUPPORTED(g_bytes < TWO_GIB && x_bytes < TWO_GIB && P * 4 < TWO_GIB, "%s: every buffer must stay below 2 GiB", who);
  Params g{};
  g.A = static_cast<const __bf16*>(G); g.X = static_cast<const __bf16*>(X); g.scale = scale; g.Y = dW; g.dbias = dbias;
  g.offsets = offsets; g.perm = perm;
  g.E = E; g.N = N; g.Kd = Kd; g.a_div = g_div; g.x_div = x_div; g.a_shift = log2_of(g_div); g.x_shift = log2_of(x_div);
  g.lda = ldg; g.ldx = ldx; g.a_bytes = (unsigned)g_bytes; g.x_bytes = (unsigned)x_bytes; g.s_bytes = (unsigned)(P * 4);
  const int TN = tile == 1 ? 64 : 128, TK = tile == 2 ? 64 : 128;
  g.ntk = (Kd + TK - 1) / TK;
  const int64_t grid = (int64_t)E * ((N + TN - 1) / TN) * g.ntk;
  AMK_CHECK_SUPPORTED(grid < TWO_GIB, "%s: grid too large", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 gd((unsigned)grid), bd(256);
  if (tile == 0) {
    if (scale) hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<128, 128, 2, true>), gd, bd, 0, st, g);
    else hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<128, 128, 2, false>), gd, bd, 0, st, g);
  } else if (tile == 1) {
    if (scale) hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<64, 128, 1, true>), gd, bd, 0, st, g);
    else hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<64, 128, 1, false>), gd, bd, 0, st, g);
  } else {
    if (scale) hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<128, 64, 4, true>), gd, bd, 0, st, g);
    else hipLaunchKernelGGL((grouped_wgrad_bf16_kernel<128, 64, 4, false>), gd, bd, 0, st, g);
  }
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}

extern "C" int amk_grouped_gemm_wgrad_bf16(const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                                           const float* scale, const int32_t* offsets, const int32_t* perm,
                                           int64_t P, int E, int N, int Kd, float* dW, float* dbias, void* stream) {
  return wgrad_impl(false, "amk_grouped_gemm_wgrad_bf16", G, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, E, N, Kd, dW, dbias, stream);
}

// ---- the narrow forms (SwitchHead's experts: one side of W[e] at most 64 wide)
extern "C" int amk_grouped_gemm_nt64_bf16(const void* A, int64_t lda, int a_div, const void* W, const float* bias,
                                          const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                          float* Y, void* stream) {
  return grouped_impl(false, true, "amk_grouped_gemm_nt64_bf16", A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd, Y, stream);
}

extern "C" int amk_grouped_gemm_nn64_bf16(const void* G, int64_t ldg, int a_div, const void* W, const float* scale,
                                          const int32_t* offsets, const int32_t* perm, int64_t P, int E, int N, int Kd,
                                          float* Y, void* stream) {
  return grouped_impl(true, true, "amk_grouped_gemm_nn64_bf16", G, ldg, a_div, W, scale, offsets, perm, P, E, N, Kd, Y, stream);
}

extern "C" int amk_grouped_gemm_wgrad64_bf16(const void* G, int64_t ldg, int g_div, const void* X, int64_t ldx, int x_div,
                                             const float* scale, const int32_t* offsets, const int32_t* perm,
                                             int64_t P, int E, int N, int Kd, float* dW, void* stream) {
  return wgrad_impl(true, "amk_grouped_gemm_wgrad64_bf16", G, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, E, N, Kd, dW, nullptr, stream);
}

extern "C" int amk_moe_expert_sums_bf16(const void* A, int a_is_bf16, int64_t lda, int a_div, const int64_t* ids, const float* scale,
                                        int64_t G, int fan, int E, int d, void* Z, void* stream) {
  const char* who = "amk_moe_expert_sums_bf16";
  AMK_CHECK_ARG(A && ids && Z, "%s: null pointer", who);
  AMK_CHECK_ARG(G > 0 && fan > 0 && E > 0 && d > 0 && a_div > 0, "%s: non-positive size G=%lld fan=%d E=%d d=%d", who, (long long)G, fan, E, d);
  AMK_CHECK_SUPPORTED(d % 8 == 0, "%s: d=%d must be multiples of 8", who, d);
  AMK_CHECK_SUPPORTED(E <= 1024 && fan <= 4096, "%s: at most 1024 experts and 4096 pairs per row", who);
  AMK_CHECK_ARG(a16(A) && a16(Z) && a16(scale), "%s: pointers must be 16-byte aligned", who);
  AMK_CHECK_ARG(lda % 8 == 0 && lda >= d, "%s: row stride %lld must be a multiple of 8 and at least %d", who, (long long)lda, d);
  AMK_CHECK_SUPPORTED(G < TWO_GIB, "%s: grid too large", who);
  const size_t lds = ((size_t)fan * 3 + E + 1) * 4;
  hipStream_t st = static_cast<hipStream_t>(stream);
  __bf16* z = static_cast<__bf16*>(Z);
  if (a_is_bf16) hipLaunchKernelGGL(expert_sums_bf16_kernel<true>, dim3((unsigned)G), dim3(256), lds, st, A, lda, a_div, ids, scale, fan, E, d, z);
  else hipLaunchKernelGGL(expert_sums_bf16_kernel<false>, dim3((unsigned)G), dim3(256), lds, st, A, lda, a_div, ids, scale, fan, E, d, z);
  AMK_CHECK_LAUNCH(who);
  return AMK_OK;
}
