// Masked-token loss head under bf16 autocast for gfx950: logits + cross-entropy on the valid rows only, bf16 operands on
// v_mfma_f32_32x32x16_bf16, every softmax quantity in f32.
//
// The semantics, the launches and the row-on-the-lane structure are those of csrc/ce_head.hip (read that file's header
// first); what differs is the operand type and how the tiles reach the matrix unit:
//
//   ce_compact / ce_finalize : the f32 head's kernels themselves, through csrc/ce_head_common.h (they never touch x or w).
//   ce_fwd    : z^T (128 words x 32 rows per wave) = w_tile (A operand) x x[rows]^T (B operand).  Both operands have the
//               contraction index contiguous in memory: staged as stored, [128 rows][32 k] bf16 per step with the four
//               16-byte chunks of a row XOR-swizzled (as the NT tiles of csrc/gemm_bf16.hip), fragments by ds_read_b128.
//               The logits stay in the f32 accumulators: running (max, sum of exp), the target logit, one partial per
//               (row, slice) -- never rounded to bf16, never written.
//   ce_bwd_g  : the same tile again; g = (exp(z - lse) - [v == t]) * (d_loss / count) in f32, rounded ONCE to bf16 into
//               the workspace G (compacted row i at stride ldg = V rounded up to 128; columns V .. ldg are zeros).
//   ce_bwd_dx : dx[rows[i], :] = sum_v G[i, v] w[v, :], f32 accumulation over ascending v, one rounding to bf16.  G has
//               the contraction index contiguous (ds_read_b128); w has it as the memory row: staged as stored,
//               [32 v][128 k] at a row stride of 160, fragments by ds_read_b64_tr_b16 (tr_frag of amk_bf16.h).
//   ce_bwd_dw : dw[v, :] = sum_i G[i, v] x[rows[i], :], f32 accumulation over ascending i, written as f32 (what the
//               gradient buckets hold).  Both operands have the contraction index as the memory row: both transposing.
//   ce_zero_rows : dx rows whose target is ignore_index or outside [0, V) are written as zeros.
// Every grid is sized from M; a row tile that starts at or past count exits before any load.  No atomics.
//
// With a bias (amk_ce_head_bias_bf16_fwd / _bwd: the HAS_BIAS instantiations of ce_fwd and ce_bwd_g; the biasless ones are
// the code they were): the f32 accumulator of the logits tile is PRELOADED with the F32 bias b[v0 + 32 b + acc_row(r, hf)]
// instead of being cleared -- the bias is the first term of the f32 MFMA chain and is never rounded to bf16.  A word at or
// past the end of the slice is not loaded and preloads 0: nothing at or past b[V] is read.
//   ce_bwd_db : db[v] = sum_i G[i, v] over the compacted rows, the once-rounded bf16 G that dw reads, accumulated in f32.
//               A workgroup of 1024 threads owns 64 columns: thread (column pair c = tid & 31, group q = tid >> 5) adds
//               rows q, q + 32, q + 64, ... in ascending order (ceil(count / 32) terms per column), the 32 group sums of a
//               column fold as a binary tree in LDS (q += q + 16, then 8, 4, 2, 1).  count == 0 writes zeros.  No
//               workspace beyond G.
//
// The tile loops hold no branch around a memory instruction: a piece outside the problem is loaded from a clamped
// address and replaced by zeros with a select.  One LDS-only barrier per step: the global prefetch stays in flight.
#include "ce_head_common.h"
#include "amk_bf16.h"

namespace amk_ce16 {

using namespace amk_ce_common;   // TR, TA, the limits, slices, the host drivers

constexpr int BK = 32;       // contraction depth per LDS stage (two MFMA steps of 16)
constexpr int FSTR = 32;     // bf16 per LDS row of a [128 rows][32 k] tile (chunk c of row r sits at c ^ ((r >> 2) & 3))
constexpr int STR = 160;     // bf16 per LDS row of a [32 k][128 columns] tile (80 dwords = 16 mod 64: conflict-free
                             // transposing reads)
constexpr int FT = BK * STR; // elements of one operand tile buffer (>= 128 * FSTR)
constexpr int STAGE = 2 * FT;
static_assert(FT >= 128 * FSTR, "the two tile shapes share one buffer");

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// 16 bytes from p when ok, else zeros; the load itself is unconditional (from `safe`, always readable)
__device__ __forceinline__ float4 ld16(const __bf16* p, const __bf16* safe, bool ok) {
  const float4 v = *reinterpret_cast<const float4*>(ok ? p : safe);
  return ok ? v : zero4();
}

// 32x32x16 operand whose contraction index is contiguous in the LDS row: lane (row = r0 + (l & 31), half) gets
// k = 16 s + 8 half + (0..7)   (r0 a multiple of 16: the swizzle is the lane's)
__device__ __forceinline__ bf16x8 k_frag(const __bf16* img, int r0, int s, int ln, int hf) {
  return *reinterpret_cast<const bf16x8*>(&img[(r0 + ln) * FSTR + 8 * ((2 * s + hf) ^ ((ln >> 2) & 3))]);
}

struct Stage { float4 a[2], b[2]; };

// [128 rows][32 k] tile: thread f covers rows (f >> 2) and (f >> 2) + 64, k = 8 (f & 3) .. + 7
__device__ __forceinline__ void store_t(__bf16* T, const float4 (&v)[2]) {
  const int ar = threadIdx.x >> 2, ach = threadIdx.x & 3;
  const int sw = 8 * (ach ^ ((ar >> 2) & 3));   // (rows ar and ar + 64: the same swizzle)
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&T[(ar + 64 * i) * FSTR + sw]) = v[i];
}
// [32 k][128 columns] tile: thread f covers rows (f >> 4) and (f >> 4) + 16, columns 8 (f & 15) .. + 7
__device__ __forceinline__ void store_d(__bf16* T, const float4 (&v)[2]) {
  const int sr = threadIdx.x >> 4, cg = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&T[(sr + 16 * i) * STR + 8 * cg]) = v[i];
}

// The staged product over nk steps of BK: step t + 1 is written to the other LDS stage and step t + 2 is requested from
// memory before step t is multiplied.  load(g, t) must give zeros for a step past the contraction.
template <class Load, class Store, class Mma>
__device__ __forceinline__ void product(int nk, __bf16* smem, Load load, Store store, Mma mma) {
  Stage g;
  load(g, 0);
  store(smem, g);
  load(g, 1);
  lds_barrier();
  for (int t = 0; t < nk; ++t) {
    store(smem + ((t + 1) & 1) * STAGE, g);
    load(g, t + 2);
    mma(smem + (t & 1) * STAGE);
    lds_barrier();
  }
}

__device__ __forceinline__ void clear(f32x16 (&acc)[4]) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
}

// acc[b][r] = bias[v0 + 32 b + acc_row(r, hf)]: the bias is the first term of the logits' MFMA chain.  A whole tile inside
// the slice (a workgroup-uniform test) takes sixteen 16-byte loads (registers 4 g .. 4 g + 3 of a block are four
// consecutive words; bias is 16-byte aligned and v0 a multiple of 128); the slice's last, partial tile loads word by word
// under a predicate (a word at or past vend is not loaded and keeps 0): nothing at or past bias[vend] is read.
__device__ __forceinline__ void preload_bias(const float* __restrict__ bias, int v0, int vend, int hf, f32x16 (&acc)[4]) {
  if (v0 + TA <= vend) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 q = *reinterpret_cast<const float4*>(bias + v0 + 32 * b + 8 * g + 4 * hf);
        acc[b][4 * g] = q.x; acc[b][4 * g + 1] = q.y; acc[b][4 * g + 2] = q.z; acc[b][4 * g + 3] = q.w;
      }
  } else {
    const float* bp = bias + v0 + 4 * hf;   // one base, constant offsets: the loads are predicated, not clamped
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = 32 * b + 8 * (r >> 2) + (r & 3);   // acc_row(r, hf) - 4 hf
        float bv = 0.f;
        if (v0 + 4 * hf + o < vend) bv = bp[o];
        acc[b][r] = bv;
      }
  }
}

// ---------------------------------------------------------------------------------------
// The logits tile shared by ce_fwd and ce_bwd_g: z^T for words [v0, v0 + 128) x the workgroup's 128 compacted rows.
template <bool HAS_BIAS>
__device__ __forceinline__ void logits_tile(const __bf16* __restrict__ x, int64_t ldx, const __bf16* __restrict__ w, int64_t ldw,
                                            int K, int v0, int vend, const int* srow, __bf16* smem, f32x16 (&acc)[4],
                                            const float* __restrict__ bias) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, hf = lane >> 5;
  const int ar = tid >> 2, ach = tid & 3;
  const __bf16 *wp[2], *xp[2];
  bool wok[2], xok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = ar + 64 * i, r = srow[c];
    wok[i] = v0 + c < vend;
    xok[i] = r >= 0;
    wp[i] = w + (int64_t)(wok[i] ? v0 + c : 0) * ldw + 8 * ach;
    xp[i] = x + (int64_t)(xok[i] ? r : 0) * ldx + 8 * ach;
  }
  if constexpr (HAS_BIAS) {
    preload_bias(bias, v0, vend, hf, acc);
  } else {
    clear(acc);
  }
  product((K + BK - 1) / BK, smem,
          [&](Stage& g, int t) {
            const bool kin = BK * t + 8 * ach < K;   // (K a multiple of 8: a piece is in or out)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              g.a[i] = ld16(wp[i] + BK * t, w, kin && wok[i]);
              g.b[i] = ld16(xp[i] + BK * t, x, kin && xok[i]);
            }
          },
          [&](__bf16* st, const Stage& g) { store_t(st, g.a); store_t(st + FT, g.b); },
          [&](const __bf16* cur) {
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
              const bf16x8 b = k_frag(cur + FT, 32 * wave, s, ln, hf);
#pragma unroll
              for (int blk = 0; blk < 4; ++blk)
                acc[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag(cur, 32 * blk, s, ln, hf), b, acc[blk], 0, 0, 0);
            }
          });
}

template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const __bf16* __restrict__ x, int64_t ldx, const __bf16* __restrict__ w,
                                                     int64_t ldw, const int64_t* __restrict__ target, int V, int K,
                                                     int nsplit, int vper, const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ count, float* __restrict__ pm,
                                                     float* __restrict__ ps, float* __restrict__ pz,
                                                     const float* __restrict__ bias) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  __shared__ int srow[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int split = blockIdx.x % nsplit;
  const int r0 = (blockIdx.x / nsplit) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  if (tid < TR) srow[tid] = r0 + tid < cnt ? rows[r0 + tid] : -1;
  __syncthreads();
  const int i = r0 + 32 * wave + ln;
  const int src = srow[32 * wave + ln];
  const int64_t t = src >= 0 ? target[src] : -1;

  const int vbeg = split * vper, vend = min(V, vbeg + vper);
  float m = -INFINITY, s = 0.f, zt = 0.f;
  bool found = false;
  f32x16 acc[4];
  for (int v0 = vbeg; v0 < vend; v0 += TA) {
    logits_tile<HAS_BIAS>(x, ldx, w, ldw, K, v0, vend, srow, smem, acc, bias);
    float tmax = -INFINITY;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int v = v0 + 32 * b + acc_row(r, hf);
        const float z = v < vend ? acc[b][r] : -INFINITY;
        acc[b][r] = z;
        tmax = fmaxf(tmax, z);
        if (v == t) { zt = z; found = true; }
      }
    const float mn = fmaxf(m, tmax);
    if (mn > -INFINITY) {   // (a lane half none of whose words is in the tile keeps (-inf, 0))
      float add = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __expf(acc[b][r] - mn);
      s = s * __expf(m - mn) + add;
      m = mn;
    }
  }
  // the two half-waves of a row hold interleaved words: half 0's sum first
  const float om = __shfl_xor(m, 32, 64), os = __shfl_xor(s, 32, 64), oz = __shfl_xor(zt, 32, 64);
  const bool of = __shfl_xor((int)found, 32, 64) != 0;
  if (hf == 0 && src >= 0) {
    const float mm = fmaxf(m, om);
    const float s0 = m > -INFINITY ? s * __expf(m - mm) : 0.f;
    const float s1 = om > -INFINITY ? os * __expf(om - mm) : 0.f;
    const int64_t o = (int64_t)i * nsplit + split;
    pm[o] = mm;
    ps[o] = s0 + s1;
    pz[o] = found ? zt : (of ? oz : 0.f);
  }
}

// ---------------------------------------------------------------------------------------
template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void ce_bwd_g_kernel(const __bf16* __restrict__ x, int64_t ldx, const __bf16* __restrict__ w,
                                                       int64_t ldw, const int64_t* __restrict__ target, int V, int K, int nvt,
                                                       const float* __restrict__ d_loss, const float* __restrict__ lse,
                                                       const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                       __bf16* __restrict__ G, int64_t ldg, const float* __restrict__ bias) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  __shared__ int srow[TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int v0 = (blockIdx.x % nvt) * TA;
  const int r0 = (blockIdx.x / nvt) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  if (tid < TR) srow[tid] = r0 + tid < cnt ? rows[r0 + tid] : -1;
  __syncthreads();
  f32x16 acc[4];
  logits_tile<HAS_BIAS>(x, ldx, w, ldw, K, v0, V, srow, smem, acc, bias);
  const int i = r0 + 32 * wave + ln;
  const int src = srow[32 * wave + ln];
  if (src < 0) return;
  const int64_t t = target[src];
  const bool oor = t < 0 || t >= V;
  const float l = lse[i];
  const float sc = d_loss[0] / (float)cnt;
  __bf16* gp = G + (int64_t)i * ldg;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int v = v0 + 32 * b + 8 * g + 4 * hf;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __expf(acc[b][4 * g + e] - l);
        const float gv = (p - (v + e == t ? 1.f : 0.f)) * sc;
        o[e] = (__bf16)((v + e < V && !oor) ? gv : 0.f);
      }
      *reinterpret_cast<bf16x4*>(gp + v) = o;
    }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_bwd_dx_kernel(const __bf16* __restrict__ G, int64_t ldg, const __bf16* __restrict__ w,
                                                        int64_t ldw, const int64_t* __restrict__ target, int V, int K, int nkt,
                                                        const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                        __bf16* __restrict__ dx, int64_t lddx) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int kt0 = (blockIdx.x % nkt) * TA;
  const int r0 = (blockIdx.x / nkt) * TR;
  const int cnt = count[0];
  if (r0 >= cnt) return;
  const int ar = tid >> 2, ach = tid & 3;   // G: compacted rows r0 + ar (+ 64), v = 8 ach .. + 7 of the step
  const int sr = tid >> 4, cg = tid & 15;   // w: rows v = sr (+ 16) of the step, columns kt0 + 8 cg .. + 7
  const __bf16* gp[2];
  bool gok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    gok[i] = r0 + ar + 64 * i < cnt;
    gp[i] = G + (int64_t)(gok[i] ? r0 + ar + 64 * i : 0) * ldg + 8 * ach;
  }
  const bool cok = kt0 + 8 * cg < K;
  const __bf16* wc = w + (cok ? kt0 + 8 * cg : 0);
  f32x16 acc[4];
  clear(acc);
  product((V + BK - 1) / BK, smem,
          [&](Stage& g, int t) {
            const bool vin = BK * t + 8 * ach < ldg;   // (columns V .. ldg of G are zeros)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int v = BK * t + sr + 16 * i;
              const bool wok = cok && v < V;
              g.a[i] = ld16(wc + (int64_t)(wok ? v : 0) * ldw, w, wok);
              g.b[i] = ld16(gp[i] + BK * t, w, vin && gok[i]);
            }
          },
          [&](__bf16* st, const Stage& g) { store_d(st, g.a); store_t(st + FT, g.b); },
          [&](const __bf16* cur) {
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
              const bf16x8 b = k_frag(cur + FT, 32 * wave, s, ln, hf);
#pragma unroll
              for (int blk = 0; blk < 4; ++blk)
                acc[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<STR>(cur, 16 * s, 32 * blk, lane), b, acc[blk], 0, 0, 0);
            }
          });
  const int i = r0 + 32 * wave + ln;
  if (i >= cnt) return;
  const int src = rows[i];
  const int64_t t = target[src];
  if (t < 0 || t >= V) return;   // ce_zero_rows writes that row
  __bf16* dp = dx + (int64_t)src * lddx;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = kt0 + 32 * b + 8 * g + 4 * hf;
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (__bf16)acc[b][4 * g + e];
      if (k < K) *reinterpret_cast<bf16x4*>(dp + k) = o;   // (K a multiple of 8: four columns are in or out)
    }
}

__global__ __launch_bounds__(256) void ce_zero_rows_kernel(const int64_t* __restrict__ target, int64_t ignore_index, int64_t M,
                                                           int V, int K, __bf16* __restrict__ dx, int64_t lddx) {
  const int k8 = K / 8;
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = f / k8;
  if (m >= M) return;
  const int64_t t = target[m];
  if (t == ignore_index || t < 0 || t >= V) *reinterpret_cast<float4*>(dx + m * lddx + 8 * (f % k8)) = zero4();
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_bwd_dw_kernel(const __bf16* __restrict__ G, int64_t ldg, const __bf16* __restrict__ x,
                                                        int64_t ldx, int V, int K, int nkt,
                                                        const int32_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                        float* __restrict__ dw, int64_t lddw) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 31, hf = lane >> 5;
  const int kt0 = (blockIdx.x % nkt) * TR;
  const int vt0 = (blockIdx.x / nkt) * TA;
  const int cnt = count[0];
  const int sr = tid >> 4, cg = tid & 15;   // compacted rows i = sr (+ 16) of the step; columns vt0 / kt0 + 8 cg .. + 7
  const bool cok = kt0 + 8 * cg < K;
  const __bf16* gc = G + vt0 + 8 * cg;      // (vt0 + 128 <= ldg)
  const __bf16* xc = x + (cok ? kt0 + 8 * cg : 0);
  f32x16 acc[4];
  clear(acc);
  product((cnt + BK - 1) / BK, smem,
          [&](Stage& g, int t) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int i = BK * t + sr + 16 * j;
              const bool iok = i < cnt;
              const int src = rows[iok ? i : 0];   // (M >= 1 entries; past count: -1, not used)
              g.a[j] = ld16(gc + (int64_t)(iok ? i : 0) * ldg, x, iok);
              g.b[j] = ld16(xc + (int64_t)(iok ? src : 0) * ldx, x, iok && cok);
            }
          },
          [&](__bf16* st, const Stage& g) { store_d(st, g.a); store_d(st + FT, g.b); },
          [&](const __bf16* cur) {
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
              const bf16x8 b = tr_frag<STR>(cur + FT, 16 * s, 32 * wave, lane);
#pragma unroll
              for (int blk = 0; blk < 4; ++blk)
                acc[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<STR>(cur, 16 * s, 32 * blk, lane), b, acc[blk], 0, 0, 0);
            }
          });
  const int k = kt0 + 32 * wave + ln;
  if (k >= K) return;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int v = vt0 + 32 * b + acc_row(r, hf);
      if (v < V) dw[(int64_t)v * lddw + k] = acc[b][r];
    }
}

// ---------------------------------------------------------------------------------------
// db[v] = sum_i G[i, v], i < count, in f32: see the file header for the order.
constexpr int DBC = 64;   // columns per workgroup (two per thread: one 4-byte load)
constexpr int DBQ = 32;   // row groups per column
__global__ __launch_bounds__(DBC / 2 * DBQ) void ce_bwd_db_kernel(const __bf16* __restrict__ G, int64_t ldg, int V,
                                                                  const int32_t* __restrict__ count, float* __restrict__ db) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  __shared__ float red[DBQ][DBC + 1];
  const int c = 2 * (threadIdx.x & (DBC / 2 - 1)), q = threadIdx.x / (DBC / 2);
  const int v = blockIdx.x * DBC + c;   // (v + 1 < ldg: the grid covers ldg / DBC workgroups)
  const int cnt = count[0];
  float s0 = 0.f, s1 = 0.f;
  for (int i = q; i < cnt; i += DBQ) {
    const bf16x2 g = *reinterpret_cast<const bf16x2*>(G + (int64_t)i * ldg + v);
    s0 += (float)g[0];
    s1 += (float)g[1];
  }
  red[q][c] = s0;
  red[q][c + 1] = s1;
  __syncthreads();
  for (int o = DBQ / 2; o >= 1; o >>= 1) {
    if (q < o) {
      red[q][c] += red[q + o][c];
      red[q][c + 1] += red[q + o][c + 1];
    }
    __syncthreads();
  }
  if (q == 0) {
    if (v < V) db[v] = red[0][c];
    if (v + 1 < V) db[v + 1] = red[0][c + 1];
  }
}

// this file, as the drivers of ce_head_common.h see it
struct Head {
  using T = __bf16;
  static constexpr int MULT = 8;
  static constexpr decltype(&ce_fwd_kernel<false>) fwd[2] = {ce_fwd_kernel<false>, ce_fwd_kernel<true>};
  static constexpr decltype(&ce_bwd_g_kernel<false>) bwd_g[2] = {ce_bwd_g_kernel<false>, ce_bwd_g_kernel<true>};
  static constexpr auto zero_rows = &ce_zero_rows_kernel;
  static constexpr auto bwd_dx = &ce_bwd_dx_kernel;
  static constexpr auto bwd_dw = &ce_bwd_dw_kernel;
  static constexpr auto bwd_db = &ce_bwd_db_kernel;
  static constexpr int DB_COLS = DBC, DB_THREADS = DBC / 2 * DBQ;
};

}  // namespace amk_ce16

using namespace amk_ce16;

extern "C" int64_t amk_ce_head_bf16_fwd_ws_bytes(int64_t M, int V, int K) { return ce_fwd_ws_bytes(M, V, K); }

extern "C" int64_t amk_ce_head_bf16_bwd_ws_bytes(int64_t M, int V, int K) { return ce_bwd_ws_bytes(M, V, K, sizeof(Head::T)); }

extern "C" int amk_ce_head_bf16_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                                    int64_t ignore_index, int64_t M, int V, int K, float* loss, float* lse, int32_t* rows,
                                    int32_t* count, void* ws, int64_t ws_bytes, void* stream) {
  return fwd_impl<Head>("amk_ce_head_bf16_fwd", x, ldx, w, ldw, target, ignore_index, M, V, K, loss, lse, rows, count, ws, ws_bytes,
                        stream, nullptr);
}

extern "C" int amk_ce_head_bias_bf16_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                                         const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, float* loss,
                                         float* lse, int32_t* rows, int32_t* count, void* ws, int64_t ws_bytes, void* stream) {
  AMK_CHECK_ARG(bias, "amk_ce_head_bias_bf16_fwd: null pointer (bias)");
  AMK_CHECK_ARG(a16(bias), "amk_ce_head_bias_bf16_fwd: misaligned pointer (bias: 16 bytes)");
  return fwd_impl<Head>("amk_ce_head_bias_bf16_fwd", x, ldx, w, ldw, target, ignore_index, M, V, K, loss, lse, rows, count, ws,
                        ws_bytes, stream, bias);
}

extern "C" int amk_ce_head_bf16_bwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const int64_t* target,
                                    int64_t ignore_index, int64_t M, int V, int K, const float* d_loss, const float* lse,
                                    const int32_t* rows, const int32_t* count, void* dx, int64_t lddx, float* dw, int64_t lddw,
                                    void* ws, int64_t ws_bytes, void* stream) {
  return bwd_impl<Head>("amk_ce_head_bf16_bwd", x, ldx, w, ldw, target, ignore_index, M, V, K, d_loss, lse, rows, count, dx, lddx,
                        dw, lddw, ws, ws_bytes, stream, nullptr, nullptr);
}

extern "C" int amk_ce_head_bias_bf16_bwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias,
                                         const int64_t* target, int64_t ignore_index, int64_t M, int V, int K, const float* d_loss,
                                         const float* lse, const int32_t* rows, const int32_t* count, void* dx, int64_t lddx,
                                         float* dw, int64_t lddw, float* dbias, void* ws, int64_t ws_bytes, void* stream) {
  AMK_CHECK_ARG(bias && dbias, "amk_ce_head_bias_bf16_bwd: null pointer (bias or dbias)");
  AMK_CHECK_ARG(a16(bias) && a16(dbias), "amk_ce_head_bias_bf16_bwd: misaligned pointer (bias, dbias: 16 bytes)");
  return bwd_impl<Head>("amk_ce_head_bias_bf16_bwd", x, ldx, w, ldw, target, ignore_index, M, V, K, d_loss, lse, rows, count, dx,
                        lddx, dw, lddw, ws, ws_bytes, stream, bias, dbias);
}

